#!/usr/bin/env python3
"""hz_ledger_apply_batch with an L1 run in front, against hz_ledger_apply_l2 over the same number of L2 transfers (not part of bench.py).

DESIGN 8c's workload -- 2^13 accounts, transfers drawn as synthetic_batch draws them, 20 % of the sender's balance, selector 176,
nLevels + 1 = 33 siblings, 64 fee slots, one fee receiver -- as 256 L1 + 1792 L2 transactions: the first 256 pairs become L1
transactions (one in four a plain deposit, one a depositTransfer, two forceTransfers; every sixteenth asks for twice the sender's
balance and is nullified by underflow), the rest stay L2 transfers on the balances the L1 run leaves.
  batch          Ledger.apply_batch per call: wall time with every output returned to the host, device time (first kernel to the last
                 write-back) and l1_ms, the L1 kernel alone
  l2             Ledger.apply_l2 over all 2048 pairs as L2 transfers on the same accounts, alternating with `batch` in the same run
  hot            Ledger.apply_batch with 256 L1 forceTransfers back and forth on ONE pair of accounts (every step of the serial phase
                 reads what the step before it wrote) and no L2 transaction: l1_ms is the worst case of the serial phase
  hot512         the same with 512 transfers (HZ_LEDGER_MAX_L1): the slope between the two, (l1_ms(512) - l1_ms(256)) / 256, is the cost of
                 one step of the serial phase without the launch, the events and the two parallel phases
Every call runs on a freshly loaded ledger: the batch is valid once. The case runs in a child process under a time limit. Writes
profiles/device_ledger_l1.json."""
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
N_L1 = SHAPE[2]


def batches(base, pairs):
    """-> (L1 dictionaries, L2 dictionaries after them, all pairs as L2 dictionaries), each valid in order"""
    from circuits_amd import builder as B

    def l2_run(pairs, tmp):
        out = []
        for frm, to in pairs:
            bal, nonce = tmp[frm] if frm in tmp else (base.state(frm)["balance"], 0)
            amount_f = B.floor_fix2float(bal * 20 // 100)
            amount = B.float2fix(amount_f)
            out.append({"fromIdx": frm, "toIdx": to, "amountF": amount_f, "nonce": nonce, "tokenID": 1, "userFee": 176})
            tmp[frm] = (bal - amount - B.compute_fee(amount, 176), nonce + 1)
            tb, tn = tmp[to] if to in tmp else (base.state(to)["balance"], 0)
            tmp[to] = (tb + amount, tn)
        return out
    tmp, l1 = {}, []
    for n, (frm, to) in enumerate(pairs[:N_L1]):
        bal = tmp[frm][0] if frm in tmp else base.state(frm)["balance"]
        load_f = B.floor_fix2float(bal // 10) if n % 4 < 2 else 0
        amount_f = 0 if n % 4 == 0 else B.floor_fix2float(2 * bal + 10 if n % 16 == 15 else bal * 20 // 100)
        load, amount = B.float2fix(load_f), B.float2fix(amount_f)
        l1.append({"fromIdx": frm, "toIdx": to if amount else 0, "amountF": amount_f, "loadAmountF": load_f, "tokenID": 1, "fromEthAddr": base.state(frm)["ethAddr"]})
        eff = amount if bal + load - amount >= 0 else 0
        tmp[frm] = (bal + load - eff, 0)
        if amount:
            tb = tmp[to][0] if to in tmp else base.state(to)["balance"]
            tmp[to] = (tb + eff, 0)
    return l1, l2_run(pairs[N_L1:], tmp), l2_run(pairs, {})


def hot_batch(base, pairs, n=N_L1):
    """n forceTransfers back and forth between the first pair's accounts, a tenth of the sender's balance each"""
    from circuits_amd import builder as B
    a, b = pairs[0][0], pairs[0][1] if pairs[0][1] != pairs[0][0] else pairs[1][0]
    bal, out = {a: base.state(a)["balance"], b: base.state(b)["balance"]}, []
    for i in range(n):
        frm, to = (a, b) if i % 2 == 0 else (b, a)
        amount_f = B.floor_fix2float(bal[frm] // 10)
        out.append({"fromIdx": frm, "toIdx": to, "amountF": amount_f, "loadAmountF": 0, "tokenID": 1, "fromEthAddr": base.state(frm)["ethAddr"]})
        bal[frm] -= B.float2fix(amount_f)
        bal[to] += B.float2fix(amount_f)
    return out


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def one(reps):
    import numpy as np
    from circuits_amd import builder as B
    from circuits_amd import lib
    from circuits_amd.capi import l1tx_array, l2sig_array, l2tx_array
    L = lib()
    if L.device_count() <= 0:
        raise SystemExit("no gfx950 device: this tool measures on the device")
    k = 13
    base = B.DenseState.build(k, seed=SEED, hash_rows=lambda t, n, data: L.poseidon_batch_bytes(t, n, data))
    pairs, fee_idx = SB.transfers(base, SHAPE[0], SEED)
    l1, l2, all_l2 = batches(base, pairs)
    hot, hot512 = hot_batch(base, pairs), hot_batch(base, pairs, 512)
    n_sib, F = SHAPE[1] + 1, SHAPE[3]
    plan, idxs = [1] + [0] * (F - 1), [fee_idx] + [0] * (F - 1)
    cols = base.leaf_fields()
    lg = L.ledger(k, first_idx=base.first_idx)
    res = {"k": k, "n_l1": len(l1), "m": len(l2), "n_sib": n_sib, "F": F}
    into = {name: np.zeros(shape, dtype=np.uint8) for name, shape in lg.shapes(SHAPE[0], F, n_sib)}
    into["auxToIdx"], into["l1_flags"] = np.zeros((SHAPE[0], 32), dtype=np.uint8), np.zeros(len(l1), dtype=np.uint8)
    hot_into = {name: np.zeros(shape, dtype=np.uint8) for name, shape in lg.shapes(len(hot), F, n_sib)}
    hot_into["auxToIdx"], hot_into["l1_flags"] = np.zeros((len(hot), 32), dtype=np.uint8), np.zeros(len(hot), dtype=np.uint8)
    hot512_into = {name: np.zeros(shape, dtype=np.uint8) for name, shape in lg.shapes(len(hot512), F, n_sib)}
    hot512_into["auxToIdx"], hot512_into["l1_flags"] = np.zeros((len(hot512), 32), dtype=np.uint8), np.zeros(len(hot512), dtype=np.uint8)
    l1_arr, l2_arr, l2_sigs, all_arr, hot_arr = l1tx_array(l1), l2tx_array(l2), l2sig_array(l2), l2tx_array(all_l2), l1tx_array(hot)
    hot512_arr = l1tx_array(hot512)
    t = {name: [] for name in ("batch_wall_ms", "batch_device_ms", "batch_l1_ms", "l2_wall_ms", "l2_device_ms", "hot_wall_ms", "hot_device_ms", "hot_l1_ms",
                               "hot512_wall_ms", "hot512_device_ms", "hot512_l1_ms")}
    kinds = ("batch", "l2", "hot", "hot512")
    for r in range(len(kinds) * (reps + 1)):
        lg.load(*cols)
        kind = kinds[r % len(kinds)]
        t0 = time.perf_counter()
        if kind == "batch":
            lg.apply_batch(l1_arr, l2_arr, plan, idxs, 1, 1, n_sib=n_sib, into=into, sigs=l2_sigs)
        elif kind == "l2":
            lg.apply_l2(all_arr, plan, idxs, n_sib=n_sib, into=into)
        elif kind == "hot":
            lg.apply_batch(hot_arr, [], plan, idxs, 1, 1, n_sib=n_sib, into=hot_into, sigs=False)
        else:
            lg.apply_batch(hot512_arr, [], plan, idxs, 1, 1, n_sib=n_sib, into=hot512_into, sigs=False)
        wall = (time.perf_counter() - t0) * 1e3
        if r >= len(kinds):   # the first call of each kind grows the call's buffers
            t[kind + "_wall_ms"].append(wall)
            t[kind + "_device_ms"].append(lg.device_ms())
            if kind != "l2":
                t[kind + "_l1_ms"].append(lg.l1_ms())
        if kind == "batch":
            res["nullified"] = int((into["l1_flags"] >> 1).sum())
    res.update({name: spread(xs) for name, xs in t.items()})
    res["l1_step_us"] = (res["hot512_l1_ms"]["median"] - res["hot_l1_ms"]["median"]) / (len(hot512) - len(hot)) * 1e3
    res["l1_share_of_device_time"] = res["batch_l1_ms"]["median"] / res["batch_device_ms"]["median"]
    lg.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=300, help="seconds for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_ledger_l1.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return one(a.reps)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], stdout=subprocess.PIPE, timeout=a.timeout)
    if p.returncode != 0:
        raise SystemExit("the measurement ended with status %d" % p.returncode)
    result = json.loads(p.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(result), flush=True)
    doc = {"tool": "tools/ledger_l1_bench.py", "shape": list(SHAPE), "seed": SEED, "what": "256 L1 + 1792 L2 transactions and one fee transaction through "
           "Ledger.apply_batch, against 2048 L2 transfers on the same accounts through Ledger.apply_l2, alternating in one run, and 256 L1 "
           "and 512 forceTransfers on one pair of accounts; ms; every sample listed under all", "results": [result]}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
