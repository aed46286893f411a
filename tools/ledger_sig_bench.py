#!/usr/bin/env python3
"""hz_ledger_apply_l2_signed against its two baselines, measured in one run (not part of bench.py).

The workload is tools/ledger_bench.py's: 2048 signed transfers on 2^13 accounts, nLevels + 1 = 33 siblings, 64 fee slots, one fee receiver.
  signed     Ledger.apply_l2_signed per call on a freshly loaded ledger: wall time with every output returned to the host, device time,
             and the device time of the two signature kernels alone (hz_ledger_sig_ms)
  unsigned   the parent path: Ledger.apply_l2 for the same transfers, alternating with the signed calls
  verify     Ledger.verify_l2 alone: wall time and hz_ledger_sig_ms
  host       the stand-alone host build of the same routines (tests/native/ledger_sig_check.cpp --bench, g++ -O3) verifying the same 2048
             signatures on --threads threads
The feature earns its place if (signed - unsigned) wall time is below the host figure. Writes profiles/device_ledger_signed.json with
every sample listed."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import state_apply_bench as SB   # noqa: E402

SHAPE, SEED, CHAIN_ID = SB.SHAPE, SB.SEED, 1


def signed_transfers(base, pairs):
    """ledger_bench.batch's transfers as dictionaries, each signed with its sender's key"""
    from circuits_amd import builder as B
    keys = base.keys()
    tmp, txs = {}, []
    for frm, to in pairs:
        bal, nonce = tmp[frm] if frm in tmp else (base.state(frm)["balance"], 0)
        amount_f = B.floor_fix2float(bal * 20 // 100)
        amount = B.float2fix(amount_f)
        t = {"fromIdx": frm, "toIdx": to, "amountF": amount_f, "nonce": nonce, "tokenID": 1, "userFee": 176}
        t.update(keys[int(base.key_idx[frm - base.first_idx])].sign_msg(B.build_hash_sig(t, CHAIN_ID)))
        txs.append(t)
        tmp[frm] = (bal - amount - B.compute_fee(amount, 176), nonce + 1)
        tb, tn = tmp[to] if to in tmp else (base.state(to)["balance"], 0)
        tmp[to] = (tb + amount, tn)
    return txs


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def host_baseline(base, txs, threads, reps):
    src = os.path.join(ROOT, "tests", "native", "ledger_sig_check.cpp")
    lines = []
    for t in txs:
        s = base.state(t["fromIdx"])
        f = [CHAIN_ID, 1, t["fromIdx"], t["toIdx"], t["amountF"], t["nonce"], t["tokenID"], t["userFee"], 0, 0, 0, 0, t["s"], t["r8x"], t["r8y"], s["ay"], s["sign"],
             0, 0, 0, 0]   # every signature is valid; --bench compares the verdict only
        lines.append(" ".join("%x" % v for v in f))
    text = "\n".join(lines) + "\n"
    out = []
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "ledger_sig_check")
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-Wno-unknown-pragmas", "-pthread", src, "-o", exe])
        for _ in range(reps):
            r = subprocess.run([exe, "--bench", str(threads)], input=text, capture_output=True, text=True, timeout=600)
            if r.returncode != 0 or "mismatches=0" not in r.stdout:
                raise SystemExit("host baseline failed: " + r.stdout + r.stderr)
            out.append(float(r.stdout.split("bench_ms=")[1].split()[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_ledger_signed.json"))
    a = ap.parse_args()
    import numpy as np
    from circuits_amd import builder as B
    from circuits_amd import lib
    from circuits_amd.capi import LEDGER_SIG_ARRAYS
    L = lib()
    if L.device_count() <= 0:
        raise SystemExit("no gfx950 device: this tool measures on the device")
    k = 13
    base = B.DenseState.build(k, seed=SEED, hash_rows=lambda t, n, data: L.poseidon_batch_bytes(t, n, data))
    pairs, fee_idx = SB.transfers(base, SHAPE[0], SEED)
    txs = signed_transfers(base, pairs)
    m, n_sib, F = len(txs), SHAPE[1] + 1, SHAPE[3]
    plan, idxs = [1] + [0] * (F - 1), [fee_idx] + [0] * (F - 1)
    cols = base.leaf_fields()
    lg = L.ledger(k, first_idx=base.first_idx)
    into = {name: np.zeros(shape, dtype=np.uint8) for name, shape in lg.shapes(m, F, n_sib)}
    into.update({name: np.zeros((m, 32), dtype=np.uint8) for name in LEDGER_SIG_ARRAYS})
    t = {"signed_wall_ms": [], "signed_device_ms": [], "signed_sig_ms": [], "unsigned_wall_ms": [], "unsigned_device_ms": [], "verify_wall_ms": [], "verify_sig_ms": []}
    roots = set()
    for r in range(a.reps + 1):   # the first round grows the call's buffers and builds the fixed-base table
        lg.load(*cols)
        t0 = time.perf_counter()
        verdict = lg.verify_l2(txs, CHAIN_ID, 1)
        wall_v = (time.perf_counter() - t0) * 1e3
        assert not verdict.any()
        sig_v = lg.sig_ms()
        t0 = time.perf_counter()
        lg.apply_l2_signed(txs, plan, idxs, CHAIN_ID, 1, n_sib=n_sib, into=into)
        wall_s = (time.perf_counter() - t0) * 1e3
        dev_s, sig_s = lg.device_ms(), lg.sig_ms()
        roots.add(lg.root())
        lg.load(*cols)
        t0 = time.perf_counter()
        lg.apply_l2(txs, plan, idxs, n_sib=n_sib, into={n: into[n] for n, _ in lg.shapes(m, F, n_sib)})
        wall_u = (time.perf_counter() - t0) * 1e3
        dev_u = lg.device_ms()
        roots.add(lg.root())
        if r:
            for name, v in (("signed_wall_ms", wall_s), ("signed_device_ms", dev_s), ("signed_sig_ms", sig_s), ("unsigned_wall_ms", wall_u), ("unsigned_device_ms", dev_u),
                            ("verify_wall_ms", wall_v), ("verify_sig_ms", sig_v)):
                t[name].append(v)
    assert len(roots) == 1
    lg.close()
    res = {name: spread(xs) for name, xs in t.items()}
    res["host_verify_ms"] = spread(host_baseline(base, txs, a.threads, max(3, a.reps // 3)))
    res["signed_minus_unsigned_wall_ms"] = res["signed_wall_ms"]["median"] - res["unsigned_wall_ms"]["median"]
    res["earns_its_place"] = res["signed_minus_unsigned_wall_ms"] < res["host_verify_ms"]["median"]
    doc = {"tool": "tools/ledger_sig_bench.py", "shape": list(SHAPE), "seed": SEED, "k": k, "m": m, "n_sib": n_sib, "F": F, "host_threads": a.threads,
           "what": "2048 signed L2 transfers through Ledger.apply_l2_signed against Ledger.apply_l2 for the same transfers and against the host build of the "
                   "same verification routine; ms; every sample listed under all", "results": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({name: (v["median"] if isinstance(v, dict) else v) for name, v in res.items()}))


if __name__ == "__main__":
    main()
