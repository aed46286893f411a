#!/usr/bin/env python3
"""hz_ledger_apply_l2_addr against the same transfers with explicit indices, and against the native builder's walk + evaluate with its own
lookup (not part of bench.py).

DESIGN 8c's workload -- 2048 transfers drawn as synthetic_batch draws them, 20 % of the sender's balance, selector 176, nLevels + 1 = 33
siblings, 64 fee slots, one fee receiver -- with two transfers in three naming their receiver by its address (toIdx = 0). A DenseState
holds eight addresses, so every address has many holders and the lowest one receives: balances follow the RESOLVED receivers.
  addr           Ledger.apply_l2_addr per call, receivers found on the device: wall time with every output returned to the host, device
                 time (first kernel to the last write-back; the lookup lies before it) and resolve_ms, the two lookup kernels alone
  indices        the same transfers with the resolved receivers as explicit indices through Ledger.apply_l2 in the same run: the path
                 that existed before; the difference is what the lookup and its round trip cost
  existing path  walk_s + eval_s of hzb_batch_stats for the to-address batch, HZB_TX_HAS_AUX_TO unset so that the builder searches
Every call runs on a freshly loaded ledger: the batch is valid once. Each case (k = 13, k = 20) runs in a child process of its own under
a time limit; nothing is started after a failure. Writes profiles/device_ledger_addr.json."""
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
    """-> (to-address transaction dictionaries, the same with the resolved receivers as indices), valid in order"""
    from circuits_amd import builder as B
    lowest = {}
    for i in range(base.first_idx, base.first_idx + base.N):
        lowest.setdefault(base.state(i)["ethAddr"], i)
    tmp, by_addr, by_idx = {}, [], []
    for n, (frm, to) in enumerate(pairs):
        bal, nonce = tmp[frm] if frm in tmp else (base.state(frm)["balance"], 0)
        amount_f = B.floor_fix2float(bal * 20 // 100)
        amount = B.float2fix(amount_f)
        t = {"fromIdx": frm, "toIdx": to, "amountF": amount_f, "nonce": nonce, "tokenID": 1, "userFee": 176}
        if n % 3:
            eth = base.state(to)["ethAddr"]
            to = lowest[eth]
            by_addr.append(dict(t, toIdx=0, toEthAddr=eth))
        else:
            by_addr.append(t)
        by_idx.append(dict(t, toIdx=to))
        tmp[frm] = (bal - amount - B.compute_fee(amount, 176), nonce + 1)
        tb, tn = tmp[to] if to in tmp else (base.state(to)["balance"], 0)
        tmp[to] = (tb + amount, tn)
    return by_addr, by_idx


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def existing_path(L, base, txs, fee_idx, layout, reps):
    """the native builder on the to-address batch: it looks every receiver up itself (a walk over all leaves per transaction)"""
    import numpy as np
    from circuits_amd import native_builder as NB
    signer = [a.k.to_bytes(32, "little") for a in base.keys()]
    arr = np.zeros(len(txs), dtype=NB.tx_dtype())
    for i, t in enumerate(txs):
        arr["from_idx"][i], arr["to_idx"][i], arr["amount_f"][i], arr["nonce"][i] = t["fromIdx"], t["toIdx"], t["amountF"], t["nonce"]
        arr["user_fee"][i], arr["flags"][i] = 176, NB.HAS_NONCE | NB.HAS_SIGNER   # no HAS_AUX_TO: the builder searches
    arr["token_id"] = 1
    arr["to_eth_addr"] = np.frombuffer(b"".join(int(t.get("toEthAddr", 0)).to_bytes(32, "little") for t in txs), dtype="V32")
    arr["signer_key"] = np.frombuffer(b"".join(signer[int(base.key_idx[t["fromIdx"] - base.first_idx])] for t in txs), dtype="V32")
    runs = []
    for _ in range(reps + 1):
        db = NB.NativeRollupDB(chain_id=1, device=0, base=base)
        bb = db.build_batch(*SHAPE)
        bb.add_txs(arr)
        bb.add_token(1)
        bb.add_fee_idx(fee_idx)
        t0 = time.perf_counter()
        bb.build(layout)
        wall = time.perf_counter() - t0
        s = bb.stats()
        runs.append({"build_wall_ms": wall * 1e3, "walk_ms": s["walk_s"] * 1e3, "eval_ms": s["eval_s"] * 1e3})
        bb.close()
        db.close()
    runs = runs[1:]
    out = {k: spread([r[k] for r in runs]) for k in runs[0]}
    out["walk_plus_eval_ms"] = statistics.median(r["walk_ms"] + r["eval_ms"] for r in runs)
    return out


def one(case, reps):
    import numpy as np
    from circuits_amd import builder as B
    from circuits_amd import lib
    from circuits_amd.capi import l2sig_array, l2tx_array
    L = lib()
    if L.device_count() <= 0:
        raise SystemExit("no gfx950 device: this tool measures on the device")
    k = int(case.lstrip("k"))
    base = B.DenseState.build(k, seed=SEED, hash_rows=lambda t, n, data: L.poseidon_batch_bytes(t, n, data))
    pairs, fee_idx = SB.transfers(base, SHAPE[0], SEED)
    by_addr, by_idx = batch(base, pairs)
    m, n_sib = len(by_addr), SHAPE[1] + 1
    plan, idxs = [1] + [0] * (SHAPE[3] - 1), [fee_idx] + [0] * (SHAPE[3] - 1)
    cols = base.leaf_fields()
    lg = L.ledger(k, first_idx=base.first_idx)
    res = {"case": case, "k": k, "m": m, "to_address": sum(1 for t in by_addr if t["toIdx"] == 0), "n_sib": n_sib, "F": SHAPE[3]}
    into = {name: np.zeros(shape, dtype=np.uint8) for name, shape in lg.shapes(m, SHAPE[3], n_sib)}
    into["auxToIdx"] = np.zeros((m, 32), dtype=np.uint8)
    idx_arr, addr_arr, addr_sigs = l2tx_array(by_idx), l2tx_array(by_addr), l2sig_array(by_addr)   # both paths take prebuilt arrays
    t = {"addr_wall_ms": [], "addr_device_ms": [], "resolve_ms": [], "indices_wall_ms": [], "indices_device_ms": []}
    roots = set()
    for r in range(2 * (reps + 1)):
        lg.load(*cols)
        addr = r % 2 == 0
        t0 = time.perf_counter()
        if addr:
            lg.apply_l2_addr(addr_arr, plan, idxs, 1, 1, n_sib=n_sib, into=into, sigs=addr_sigs)
        else:
            lg.apply_l2(idx_arr, plan, idxs, n_sib=n_sib, into=into)
        wall = (time.perf_counter() - t0) * 1e3
        roots.add(lg.root())
        if r >= 2:   # the first call of each kind grows the call's buffers
            t["addr_wall_ms" if addr else "indices_wall_ms"].append(wall)
            t["addr_device_ms" if addr else "indices_device_ms"].append(lg.device_ms())
            if addr:
                t["resolve_ms"].append(lg.resolve_ms())
    assert len(roots) == 1   # both paths leave the same state
    res.update({name: spread(xs) for name, xs in t.items()})
    lg.close()
    if case == "k13":
        g = L.ctx("rollup-main", nTx=SHAPE[0], nLevels=SHAPE[1], maxL1Tx=SHAPE[2], maxFeeTx=SHAPE[3])
        layout = g.packed_layout()
        g.close()
        res["existing"] = existing_path(L, base, by_addr, fee_idx, layout, max(3, reps // 3))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["k13", "k20"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (one child process each)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_ledger_addr.json"))
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
    doc = {"tool": "tools/ledger_addr_bench.py", "shape": list(SHAPE), "seed": SEED, "what": "2048 L2 transfers, two in three to an address, and one fee "
           "transaction through Ledger.apply_l2_addr, against the same transfers by index through Ledger.apply_l2 and the native builder's walk + "
           "evaluate with its own lookup; ms; every sample listed under all", "results": results}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
