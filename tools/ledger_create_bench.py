#!/usr/bin/env python3
"""hz_ledger_apply_batch_creates on a growing ledger against the calls it replaces (not part of bench.py).

The headline recipe on a state of 2^13 accounts: 256 createAccountDeposit rows in front of 1792 L2 transfers between existing accounts
(20 % of the sender's balance, selector 176), nLevels + 1 = 33 siblings, 64 fee slots, one fee receiver. No signature is verified here, as
in DESIGN 8f's measurement.
  creates        GrowingLedger.apply_batch_creates per call: wall time with every output returned to the host, device_ms, semantic_ms and
                 create_ms (k_ledger_create + k_ledger_create_pack)
  dense     (a)  Ledger.apply_batch on a dense ledger over the same rows with every create replaced by a deposit of the same load on an
                 existing account, alternating with `creates` in the same run
  native    (b)  the same batch (creates included) through the native builder: its walk + evaluate time, as tools/sparse_tree_bench.py reads it
  load           hz_ledger_load_accounts against hz_ledger_load for the same 2^13 accounts (--big: 2^16 as well)
Every ledger call runs on a freshly loaded ledger: the batch is valid once. The case runs in a child process under a time limit. Writes
profiles/device_ledger_create.json with every sample."""
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
import sparse_tree_bench as TB    # noqa: E402
import state_apply_bench as SB    # noqa: E402

SHAPE, SEED = SB.SHAPE, SB.SEED
N_L1 = SHAPE[2]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def create_rows(arr):
    """tools/sparse_tree_bench.py's create-account deposits (hzb_tx records) as the ledger's L1 dictionaries"""
    return [{"onChain": 1, "fromIdx": 0, "toIdx": 0, "amountF": 0, "loadAmountF": int(r["load_amount_f"]), "tokenID": int(r["token_id"]),
             "fromEthAddr": int.from_bytes(bytes(r["from_eth_addr"]), "little"), "fromBjjCompressed": int.from_bytes(bytes(r["from_bjj_compressed"]), "little")}
            for r in arr]


def time_loads(L, base, capacity, reps):
    """hz_ledger_load_accounts on a growing ledger and hz_ledger_load on a dense one, the same accounts: wall ms"""
    cols = base.leaf_fields()
    grow, dense = L.ledger_growing(capacity, first_idx=base.first_idx, n_sib_max=SHAPE[1] + 1), L.ledger(base.k, first_idx=base.first_idx)
    t = {"load_accounts_wall_ms": [], "load_wall_ms": []}
    for r in range(reps + 1):
        t0 = time.perf_counter()
        grow.load_accounts(*cols)
        t1 = time.perf_counter()
        dense.load(*cols)
        t2 = time.perf_counter()
        if r:
            t["load_accounts_wall_ms"].append((t1 - t0) * 1e3)
            t["load_wall_ms"].append((t2 - t1) * 1e3)
    same_root = grow.root() == dense.root()
    grow.close()
    dense.close()
    return dict({name: spread(xs) for name, xs in t.items()}, same_root=same_root)


def one(reps, big):
    import numpy as np
    from circuits_amd import builder as B
    from circuits_amd import lib
    from circuits_amd.capi import LEDGER_CREATE_ARRAYS, LEDGER_EXIT_ARRAYS, from_bjj_array, l1tx_array, l2sig_array, l2tx_array
    L = lib()
    if L.device_count() <= 0:
        raise SystemExit("no gfx950 device: this tool measures on the device")
    k = 13
    hash_rows = lambda t, n, data: L.poseidon_batch_bytes(t, n, data)   # noqa: E731
    base = B.DenseState.build(k, seed=SEED, hash_rows=hash_rows)
    pairs, fee_idx = SB.transfers(base, SHAPE[0], SEED)
    rng = np.random.default_rng(SEED)
    create_arr = TB.l1_create_txs(N_L1, rng)
    creates = create_rows(create_arr)
    deposits = [{"onChain": 1, "fromIdx": frm, "toIdx": 0, "amountF": 0, "loadAmountF": c["loadAmountF"], "tokenID": 1, "fromEthAddr": base.state(frm)["ethAddr"]}
                for (frm, _), c in zip(pairs[:N_L1], creates)]
    # 1792 transfers drawn on the base's balances, which both batches here leave at least as high
    tmp, l2 = {}, []
    for frm, to in pairs[N_L1:]:
        bal, nonce = tmp[frm] if frm in tmp else (base.state(frm)["balance"], 0)
        amount_f = B.floor_fix2float(bal * 20 // 100)
        amount = B.float2fix(amount_f)
        l2.append({"fromIdx": frm, "toIdx": to, "amountF": amount_f, "nonce": nonce, "tokenID": 1, "userFee": 176})
        tmp[frm] = (bal - amount - B.compute_fee(amount, 176), nonce + 1)
        tb, tn = tmp[to] if to in tmp else (base.state(to)["balance"], 0)
        tmp[to] = (tb + amount, tn)
    n_sib, F = SHAPE[1] + 1, SHAPE[3]
    plan, idxs = [1] + [0] * (F - 1), [fee_idx] + [0] * (F - 1)
    cols = base.leaf_fields()
    R = N_L1 + len(l2)
    grow, dense = L.ledger_growing(base.N + N_L1, first_idx=base.first_idx, n_sib_max=n_sib), L.ledger(k, first_idx=base.first_idx)
    into = {name: np.zeros(shape, dtype=np.uint8) for name, shape in dense.shapes(R, F, n_sib)}
    into["auxToIdx"], into["l1_flags"] = np.zeros((R, 32), dtype=np.uint8), np.zeros(N_L1, dtype=np.uint8)
    dense_into = dict(into)
    into.update({name: np.zeros((1 if name == "new_exit_root" else R, 32), dtype=np.uint8) for name in LEDGER_EXIT_ARRAYS})
    into.update({name: np.zeros((1 if name == "new_last_idx" else R, 32), dtype=np.uint8) for name in LEDGER_CREATE_ARRAYS})
    dep_arr, l2_arr, l2_sigs = l1tx_array(deposits), l2tx_array(l2), l2sig_array(l2)
    create_l1, create_keys = l1tx_array(creates), from_bjj_array(creates)
    res = {"k": k, "n_l1": N_L1, "m": len(l2), "n_sib": n_sib, "F": F, "capacity": base.N + N_L1}
    names = ("creates_wall_ms", "creates_device_ms", "creates_semantic_ms", "creates_create_ms", "dense_wall_ms", "dense_device_ms", "dense_semantic_ms")
    t = {name: [] for name in names}
    kinds = ("creates", "dense")
    for r in range(len(kinds) * (reps + 1)):
        kind = kinds[r % len(kinds)]
        if kind == "creates":
            grow.load_accounts(*cols)
            t0 = time.perf_counter()
            grow.apply_batch_creates(create_l1, l2_arr, plan, idxs, 1, 1, n_sib=n_sib, into=into, sigs=l2_sigs, from_bjj=create_keys)
            lg = grow
        else:
            dense.load(*cols)
            t0 = time.perf_counter()
            dense.apply_batch(dep_arr, l2_arr, plan, idxs, 1, 1, n_sib=n_sib, into=dense_into, sigs=l2_sigs)
            lg = dense
        wall = (time.perf_counter() - t0) * 1e3
        if r < len(kinds):   # the first call of each kind grows the call's buffers
            continue
        t[kind + "_wall_ms"].append(wall)
        t[kind + "_device_ms"].append(lg.device_ms())
        t[kind + "_semantic_ms"].append(lg.semantic_ms())
        if kind == "creates":
            t["creates_create_ms"].append(grow.create_ms())
            res["size_after"], res["last_idx_after"] = int(grow.size()), int(grow.last_idx())
    res.update({name: spread(xs) for name, xs in t.items()})
    res["creates_minus_dense_wall_ms"] = res["creates_wall_ms"]["median"] - res["dense_wall_ms"]["median"]
    grow.close()
    dense.close()
    # (b): the same batch through the native builder
    arr = np.concatenate([create_arr, TB.l2_txs(base, pairs[N_L1:])])
    res["native"] = TB.existing_path(L, base, arr, SHAPE, fee_idx, min(reps, 5))
    res["native_over_creates_wall"] = res["native"]["walk_plus_eval_ms"] / res["creates_wall_ms"]["median"]
    res["load_2_13"] = time_loads(L, base, base.N + N_L1, reps)
    if big:
        res["load_2_16"] = time_loads(L, B.DenseState.build(16, seed=SEED, hash_rows=hash_rows), (1 << 16) + N_L1, 3)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--big", action="store_true", help="the load of 2^16 accounts as well")
    ap.add_argument("--timeout", type=int, default=420, help="seconds for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_ledger_create.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return one(a.reps, a.big)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)] + (["--big"] if a.big else []), stdout=subprocess.PIPE,
                       timeout=a.timeout)
    if p.returncode != 0:
        raise SystemExit("the measurement ended with status %d" % p.returncode)
    result = json.loads(p.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(result), flush=True)
    doc = {"tool": "tools/ledger_create_bench.py", "shape": list(SHAPE), "seed": SEED, "what": "256 createAccountDeposit + 1792 L2 transfers on 2^13 accounts "
           "through GrowingLedger.apply_batch_creates, against (a) the same rows with deposits on existing accounts through Ledger.apply_batch on a "
           "dense ledger, alternating in one run, and (b) the native builder's walk + evaluate for the same batch; the load of the accounts through "
           "hz_ledger_load_accounts against hz_ledger_load; ms; every sample listed under all", "results": [result]}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
