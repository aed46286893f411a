#!/usr/bin/env python3
"""hz_ledger_apply_l2 against the native builder's walk + evaluate, on the same transfers (not part of bench.py).

One workload: the native builder's own batch of 2048 signed transfers on 2^13 accounts (state_apply_bench's recipe: senders and receivers
as synthetic_batch draws them, 20 % of the sender's balance, selector 176), nLevels + 1 = 33 siblings, 64 fee slots, one fee receiver.
  ledger         Ledger.apply_l2 per call: wall time with every output returned to the host, wall time with the outputs left on the
                 device, device time (first kernel to the last write-back) and the device time of the semantic kernels alone (first
                 kernel to the failure-word read). Every call runs on a freshly loaded ledger: the batch is valid once.
  existing path  walk_s + eval_s of hzb_batch_stats for the same transfers (tools/state_apply_bench.py's existing_path)
  hot            the same number of transfers, every one paying ONE receiver: the case that decides between a lane per account and a
                 wavefront scan in k_ledger_scan
  k = 20         the first batch's recipe on 2^20 accounts (ledger only)
Each case runs in a child process of its own under a time limit; nothing is started after a failure. Writes profiles/device_ledger.json."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import state_apply_bench as SB   # noqa: E402

SHAPE, SEED = SB.SHAPE, SB.SEED


def batch(base, pairs):
    """the transfers as hz_l2tx, valid in order (balances and nonces tracked as the builder's recipe does)"""
    from circuits_amd import builder as B
    from circuits_amd.capi import l2tx_array
    tmp, txs = {}, []
    for frm, to in pairs:
        bal, nonce = tmp[frm] if frm in tmp else (base.state(frm)["balance"], 0)
        amount_f = B.floor_fix2float(bal * 20 // 100)
        amount = B.float2fix(amount_f)
        txs.append({"fromIdx": frm, "toIdx": to, "amountF": amount_f, "nonce": nonce, "tokenID": 1, "userFee": 176})
        tmp[frm] = (bal - amount - B.compute_fee(amount, 176), nonce + 1)
        tb, tn = tmp[to] if to in tmp else (base.state(to)["balance"], 0)
        tmp[to] = (tb + amount, tn)
    return l2tx_array(txs), len(txs)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def one(case, reps):
    import random
    from circuits_amd import builder as B
    from circuits_amd import lib
    L = lib()
    if L.device_count() <= 0:
        raise SystemExit("no gfx950 device: this tool measures on the device")
    k = 20 if case == "k20" else 13
    base = B.DenseState.build(k, seed=SEED, hash_rows=lambda t, n, data: L.poseidon_batch_bytes(t, n, data))
    pairs, fee_idx = SB.transfers(base, SHAPE[0], SEED)
    if case == "hot":
        rng = random.Random(SEED)
        hot = base.first_idx + rng.randrange(base.N)
        pairs = [(f, hot) for f, _ in pairs]
    arr, m = batch(base, pairs)
    plan, idxs = [1] + [0] * (SHAPE[3] - 1), [fee_idx] + [0] * (SHAPE[3] - 1)
    cols = base.leaf_fields()
    lg = L.ledger(k, first_idx=base.first_idx)
    res = {"case": case, "k": k, "m": m, "events": int(L.ledger_plan_l2(arr, plan, idxs, k, base.first_idx)["account"].size), "n_sib": SHAPE[1] + 1, "F": SHAPE[3]}
    import numpy as np
    into = {name: np.zeros(shape, dtype=np.uint8) for name, shape in lg.shapes(m, SHAPE[3], SHAPE[1] + 1)}
    t = {"wall_host_outputs_ms": [], "wall_device_outputs_ms": [], "device_ms": [], "semantic_ms": []}
    roots = set()
    for r in range(2 * (reps + 1)):
        lg.load(*cols)
        host = r % 2 == 0
        t0 = time.perf_counter()
        lg.apply_l2(arr, plan, idxs, n_sib=SHAPE[1] + 1, outputs=host, into=into if host else None)
        wall = (time.perf_counter() - t0) * 1e3
        roots.add(lg.root())
        if r >= 2:   # the first call of each kind grows the call's buffers
            t["wall_host_outputs_ms" if host else "wall_device_outputs_ms"].append(wall)
            t["device_ms"].append(lg.device_ms())
            t["semantic_ms"].append(lg.semantic_ms())
    assert len(roots) == 1
    res.update({name: spread(xs) for name, xs in t.items()})
    lg.close()
    if case == "builder":
        g = L.ctx("rollup-main", nTx=SHAPE[0], nLevels=SHAPE[1], maxL1Tx=SHAPE[2], maxFeeTx=SHAPE[3])
        layout = g.packed_layout()
        g.close()
        res["existing"] = SB.existing_path(L, base, pairs, fee_idx, layout, max(3, reps // 3))
        res["ratio_existing_over_ledger_wall"] = res["existing"]["walk_plus_eval_ms"] / res["wall_host_outputs_ms"]["median"]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["builder", "hot", "k20"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (one child process each)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_ledger.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child is not None:
        return one(a.child, a.reps)
    results = []
    for case in a.cases:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(a.reps)], stdout=subprocess.PIPE, timeout=a.timeout)
        if p.returncode != 0:
            raise SystemExit("case %s ended with status %d: nothing more is run" % (case, p.returncode))
        results.append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    doc = {"tool": "tools/ledger_bench.py", "shape": list(SHAPE), "seed": SEED, "what": "2048 L2 transfers and one fee transaction through "
           "Ledger.apply_l2 against the native builder's walk + evaluate time for the same transfers; ms; every sample listed under all", "results": results}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
