"""Worker of tests/test_export_derived.py::test_capped_grids: one launch and its exports in a process of its own, because the
library reads HZ_EXPORT_BLOCKS once per process (export.hip block_cap). It checks nothing: it writes every exported vector to the
job's directory and the parent compares them with the reference it holds.

    python export_derived_worker.py <job.json>
job = {"template", "kw", "n_instances", "inputs": [input object], "which": [input of instance k], "sym": path of the .sym, "r1cs": path of its .r1cs or null,
       "exports": [[first instance, count] | "all"], "out": directory}  ->  <out>/export_<i>.npy, uint8 [count][nvars][32]"""
import json
import os
import sys

import numpy as np

try:  # torch's bundled ROCm runtime first, as tests/conftest.py does
    import torch
except Exception:  # pragma: no cover
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(path):
    from circuits_amd import ConstraintError, lib
    job = json.load(open(path))
    L = lib()
    g = L.ctx(job["template"], n_instances=job["n_instances"], **job["kw"])
    for k, w in enumerate(job["which"]):
        g.set_inputs(job["inputs"][w], instance=k)
    try:
        g.run()
    except ConstraintError:
        pass
    mp = g.import_sym(open(job["sym"]).read(), open(job["r1cs"], "rb").read() if job.get("r1cs") else None)
    nv = mp.nvars()
    for i, ex in enumerate(job["exports"]):
        first, count = (0, job["n_instances"]) if ex == "all" else ex
        out = torch.full((count * nv * 32,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        if ex == "all":
            mp.export_dev(out.data_ptr(), -1)
        else:
            L._check(L.c.hz_witness_export_range_dev(g.h, mp.h, first, count, out.data_ptr(), None))
        torch.cuda.synchronize()
        np.save(os.path.join(job["out"], "export_%d.npy" % i), out.cpu().numpy().reshape(count, nv, 32))
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
