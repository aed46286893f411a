#!/usr/bin/env python3
"""hz_ledger_apply_batch_atomic against hz_ledger_apply_batch_creates over the same rows without links (not part of bench.py).

DESIGN 8h's recipe on a state of 2^13 accounts -- 256 createAccountDeposit rows in front of 1792 L2 transfers between existing accounts
(20 % of the sender's balance, selector 176), nLevels + 1 = 33 siblings, 64 fee slots, one fee receiver, on a growing ledger -- with every
L2 signature verified on the device (HZ_LEDGER_VERIFY_SIGS) and, for the atomic call, the transfers linked in pairs: transaction 2j
requires the next (rqOffset 1), transaction 2j + 1 the previous (rqOffset 7), each signed over its partner's link fields.
  atomic         GrowingLedger.apply_batch_atomic per call: wall time with every output returned to the host, device_ms, semantic_ms,
                 sig_ms (the two signature kernels; the message kernel hashes the rq fields) and rq_ms (k_ledger_rq)
  creates        GrowingLedger.apply_batch_creates over the same rows, signed without links, alternating with `atomic` in the same run
The expectation, stated before the measurement: sig_ms does not move (Poseidon's width is the same, three inputs are no longer zero) and
rq_ms is a few microseconds (three 32-byte compares a lane). Every ledger call runs on a freshly loaded ledger: the batch is valid once.
The case runs in a child process under a time limit. Writes profiles/device_ledger_atomic.json with every sample."""
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
import ledger_create_bench as CB  # noqa: E402
import sparse_tree_bench as TB    # noqa: E402
import state_apply_bench as SB    # noqa: E402

SHAPE, SEED = SB.SHAPE, SB.SEED
N_L1 = SHAPE[2]
RQ_FIELDS = ("rqTxCompressedDataV2", "rqToEthAddr", "rqToBjjAy")


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def one(reps):
    import numpy as np
    from circuits_amd import builder as B
    from circuits_amd import lib
    from circuits_amd.capi import LEDGER_CREATE_ARRAYS, LEDGER_EXIT_ARRAYS, LEDGER_SIG_ARRAYS, from_bjj_array, l1tx_array, l2rq_array, l2sig_array, l2tx_array
    L = lib()
    if L.device_count() <= 0:
        raise SystemExit("no gfx950 device: this tool measures on the device")
    k = 13
    hash_rows = lambda t, n, data: L.poseidon_batch_bytes(t, n, data)   # noqa: E731
    base = B.DenseState.build(k, seed=SEED, hash_rows=hash_rows)
    pairs, fee_idx = SB.transfers(base, SHAPE[0], SEED)
    creates = CB.create_rows(TB.l1_create_txs(N_L1, np.random.default_rng(SEED)))
    tmp, l2 = {}, []
    for frm, to in pairs[N_L1:]:   # 1792 transfers drawn on the base's balances, as tools/ledger_create_bench.py draws them
        bal, nonce = tmp[frm] if frm in tmp else (base.state(frm)["balance"], 0)
        amount_f = B.floor_fix2float(bal * 20 // 100)
        amount = B.float2fix(amount_f)
        l2.append({"fromIdx": frm, "toIdx": to, "amountF": amount_f, "nonce": nonce, "tokenID": 1, "userFee": 176})
        tmp[frm] = (bal - amount - B.compute_fee(amount, 176), nonce + 1)
        tb, tn = tmp[to] if to in tmp else (base.state(to)["balance"], 0)
        tmp[to] = (tb + amount, tn)
    keys = base.keys()
    linked = [dict(t) for t in l2]
    for i, t in enumerate(linked):   # pairs: (0, 1), (2, 3), ...; an odd last transaction stays alone
        j = i + 1 if i % 2 == 0 else i - 1
        if j < len(linked):
            t["rqOffset"] = 1 if j > i else 7
            t.update(zip(RQ_FIELDS, (B.build_tx_compressed_data_v2(l2[j]), 0, 0)))
    t0 = time.perf_counter()
    for txs in (l2, linked):
        for t in txs:
            t.update(keys[int(base.key_idx[t["fromIdx"] - base.first_idx])].sign_msg(B.build_hash_sig(t, 1)))
    sign_s = time.perf_counter() - t0
    n_sib, F = SHAPE[1] + 1, SHAPE[3]
    plan, idxs = [1] + [0] * (F - 1), [fee_idx] + [0] * (F - 1)
    cols = base.leaf_fields()
    m = len(l2)
    R = N_L1 + m
    grow = L.ledger_growing(base.N + N_L1, first_idx=base.first_idx, n_sib_max=n_sib)
    into = {name: np.zeros(shape, dtype=np.uint8) for name, shape in grow.shapes(R, F, n_sib)}
    into["auxToIdx"], into["l1_flags"] = np.zeros((R, 32), dtype=np.uint8), np.zeros(N_L1, dtype=np.uint8)
    into.update({name: np.zeros((1 if name == "new_exit_root" else R, 32), dtype=np.uint8) for name in LEDGER_EXIT_ARRAYS})
    into.update({name: np.zeros((1 if name == "new_last_idx" else R, 32), dtype=np.uint8) for name in LEDGER_CREATE_ARRAYS})
    into.update({name: np.zeros((m, 32), dtype=np.uint8) for name in LEDGER_SIG_ARRAYS})
    l2_arr, create_l1, create_keys = l2tx_array(l2), l1tx_array(creates), from_bjj_array(creates)
    sigs = {"creates": l2sig_array(l2), "atomic": l2sig_array(linked)}
    rq = l2rq_array(linked)
    res = {"k": k, "n_l1": N_L1, "m": m, "linked": sum(1 for t in linked if t.get("rqOffset")), "n_sib": n_sib, "F": F, "host_signing_s": sign_s}
    kinds = ("atomic", "creates")
    t = {kind + "_" + name: [] for kind in kinds for name in ("wall_ms", "device_ms", "semantic_ms", "sig_ms")}
    t["atomic_rq_ms"] = []
    roots = {}
    for r in range(len(kinds) * (reps + 1)):
        kind = kinds[r % len(kinds)]
        grow.load_accounts(*cols)
        t0 = time.perf_counter()
        if kind == "atomic":
            grow.apply_batch_atomic(create_l1, l2_arr, plan, idxs, 1, 1, n_sib=n_sib, verify=True, into=into, sigs=sigs[kind], from_bjj=create_keys, rq=rq)
        else:
            grow.apply_batch_creates(create_l1, l2_arr, plan, idxs, 1, 1, n_sib=n_sib, verify=True, into=into, sigs=sigs[kind], from_bjj=create_keys)
        wall = (time.perf_counter() - t0) * 1e3
        roots[kind] = grow.root()
        if r < len(kinds):   # the first call of each kind grows the call's buffers and builds the fixed-base table
            continue
        t[kind + "_wall_ms"].append(wall)
        t[kind + "_device_ms"].append(grow.device_ms())
        t[kind + "_semantic_ms"].append(grow.semantic_ms())
        t[kind + "_sig_ms"].append(grow.sig_ms())
        if kind == "atomic":
            t["atomic_rq_ms"].append(grow.rq_ms())
    res.update({name: spread(xs) for name, xs in t.items()})
    res["same_root"] = roots["atomic"] == roots["creates"]
    res["atomic_minus_creates_wall_ms"] = res["atomic_wall_ms"]["median"] - res["creates_wall_ms"]["median"]
    res["atomic_minus_creates_sig_ms"] = res["atomic_sig_ms"]["median"] - res["creates_sig_ms"]["median"]
    # the expectation's outcome by rules that stand here, not chosen after a look at the figures: "does not move" is a difference of medians within the spread (max - min) of
    # the unlinked call's own samples; "a few microseconds" is a median below 20 us, events around one small kernel included
    own = res["creates_sig_ms"]["max"] - res["creates_sig_ms"]["min"]
    res["expectation"] = {"sig_ms_did_not_move": abs(res["atomic_minus_creates_sig_ms"]) <= own, "creates_sig_ms_spread": own,
                          "rq_ms_is_a_few_microseconds": res["atomic_rq_ms"]["median"] < 0.020, "rq_us_median": res["atomic_rq_ms"]["median"] * 1e3}
    grow.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=420, help="seconds for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_ledger_atomic.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return one(a.reps)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], stdout=subprocess.PIPE, timeout=a.timeout)
    if p.returncode != 0:
        raise SystemExit("the measurement ended with status %d" % p.returncode)
    result = json.loads(p.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(result), flush=True)
    doc = {"tool": "tools/ledger_atomic_bench.py", "shape": list(SHAPE), "seed": SEED, "what": "256 createAccountDeposit + 1792 L2 transfers on 2^13 accounts on a "
           "growing ledger, every signature verified on the device: GrowingLedger.apply_batch_atomic with the transfers linked in pairs (rqOffset 1 and 7) "
           "against GrowingLedger.apply_batch_creates over the same rows signed without links, alternating in one run; ms; every sample listed under all",
           "expectation": "stated beforehand: sig_ms does not move (same Poseidon width), rq_ms is a few microseconds (three 32-byte compares per lane)",
           "outcome": result["expectation"], "results": [result]}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
