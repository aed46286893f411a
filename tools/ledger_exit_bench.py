#!/usr/bin/env python3
"""hz_ledger_apply_batch_exits against the calls it replaces (not part of bench.py).

DESIGN 8b's first workload -- 2048 L2 exits of 2048 distinct senders on a state of 2^13 accounts, 20 % of the sender's balance,
selector 176, nLevels + 1 = 33 siblings, 64 fee slots, one fee receiver: 2048 inserts into the empty exit tree and 2048 updates of the
senders' state leaves, in ONE call that also computes the amounts, fees, balances and nonces.
  exits          Ledger.apply_batch_exits per call: wall time with every output returned to the host, device_ms (first kernel to the last
                 write-back), semantic_ms (first kernel to the failure-word read) and exit_ms (the exit kernels plus the exit tree's update,
                 which runs on its own stream beside the state tree's)
  l2        (a)  Ledger.apply_l2 over 2048 transfers of the same senders on the same accounts, alternating with `exits` in the same run
  two_trees (b)  tools/sparse_tree_bench.py's two separate calls in the same run: SparseTree.apply of 2048 inserts into an empty tree, then
                 of 2048 updates on a tree that holds the 2^13 accounts, with drawn leaf fields (the trees alone: no amounts, no balances)
  mixed          a second workload: 256 L1 transactions (32 of them forceExits) and 1792 L2 transactions (256 of them exits) through
                 Ledger.apply_batch_exits
Every ledger call runs on a freshly loaded ledger: the batch is valid once. The case runs in a child process under a time limit. Writes
profiles/device_ledger_exit.json with every sample."""
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
import ledger_l1_bench as LB      # noqa: E402
import sparse_tree_bench as TB    # noqa: E402
import state_apply_bench as SB    # noqa: E402

SHAPE, SEED = SB.SHAPE, SB.SEED
EXIT_IDX = 1


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def exit_rows(base, senders, to=None):
    """one L2 row per sender, 20 % of its balance, selector 176: an exit, or a transfer to to[i]"""
    from circuits_amd import builder as B
    return [{"fromIdx": s, "toIdx": EXIT_IDX if to is None else to[i], "amountF": B.floor_fix2float(base.state(s)["balance"] * 20 // 100), "nonce": 0,
             "tokenID": 1, "userFee": 176} for i, s in enumerate(senders)]


def mixed(base, pairs):
    """ledger_l1_bench's 256 L1 + 1792 L2 batch with every eighth L1 row a forceExit and every seventh L2 row an exit: what the row takes
    out of its sender is the same, so the batch stays valid; only the receivers of those rows get less"""
    l1, l2, _ = LB.batches(base, pairs)
    for n, t in enumerate(l1):
        if n % 8 == 5:
            t["toIdx"] = EXIT_IDX
    nx = 0
    for n, t in enumerate(l2):
        if n % 7 == 3 and nx < 256:
            t["toIdx"], nx = EXIT_IDX, nx + 1
    # a receiver that no longer gets its amount may fall short later: keep the rows whose sender still covers them
    from circuits_amd import builder as B
    bal = {}
    get = lambda a: bal[a] if a in bal else base.state(a)["balance"]   # noqa: E731
    for t in l1:
        load, amount = B.float2fix(t["loadAmountF"]), B.float2fix(t["amountF"])
        eff = amount if get(t["fromIdx"]) + load - amount >= 0 else 0
        bal[t["fromIdx"]] = get(t["fromIdx"]) + load - eff
        if amount and t["toIdx"] != EXIT_IDX:
            bal[t["toIdx"]] = get(t["toIdx"]) + eff
    nonce = {}
    for t in l2:
        frm = t["fromIdx"]
        t["amountF"] = B.floor_fix2float(get(frm) * 20 // 100)
        amount = B.float2fix(t["amountF"])
        t["nonce"] = nonce.get(frm, 0)
        nonce[frm] = t["nonce"] + 1
        bal[frm] = get(frm) - amount - B.compute_fee(amount, 176)
        if t["toIdx"] != EXIT_IDX:
            bal[t["toIdx"]] = get(t["toIdx"]) + amount
    return l1, l2


def one(reps):
    import numpy as np
    from circuits_amd import builder as B
    from circuits_amd import lib
    from circuits_amd.capi import LEDGER_EXIT_ARRAYS, l1tx_array, l2sig_array, l2tx_array
    L = lib()
    if L.device_count() <= 0:
        raise SystemExit("no gfx950 device: this tool measures on the device")
    k, m = 13, 2048
    base = B.DenseState.build(k, seed=SEED, hash_rows=lambda t, n, data: L.poseidon_batch_bytes(t, n, data))
    rng = np.random.default_rng(SEED)
    first = base.first_idx
    senders = [first + int(x) for x in rng.choice(base.N, size=m, replace=False)]
    receivers = [first + int(x) for x in rng.integers(0, base.N, size=m)]
    pairs, fee_idx = SB.transfers(base, SHAPE[0], SEED)
    n_sib, F = SHAPE[1] + 1, SHAPE[3]
    plan, idxs = [1] + [0] * (F - 1), [fee_idx] + [0] * (F - 1)
    exits, transfers = exit_rows(base, senders), exit_rows(base, senders, receivers)
    mix_l1, mix_l2 = mixed(base, pairs)
    cols = base.leaf_fields()
    lg = L.ledger(k, first_idx=first)
    res = {"k": k, "m": m, "n_sib": n_sib, "F": F, "mixed_n_l1": len(mix_l1), "mixed_m": len(mix_l2),
           "mixed_force_exits": sum(t["toIdx"] == EXIT_IDX for t in mix_l1), "mixed_l2_exits": sum(t["toIdx"] == EXIT_IDX for t in mix_l2)}

    def outputs(rows, n_l1):
        into = {name: np.zeros(shape, dtype=np.uint8) for name, shape in lg.shapes(rows, F, n_sib)}
        into["auxToIdx"], into["l1_flags"] = np.zeros((rows, 32), dtype=np.uint8), np.zeros(n_l1, dtype=np.uint8)
        into.update({name: np.zeros((1 if name == "new_exit_root" else rows, 32), dtype=np.uint8) for name in LEDGER_EXIT_ARRAYS})
        return into
    into, mix_into = outputs(m, 0), outputs(len(mix_l1) + len(mix_l2), len(mix_l1))
    l2_into = {name: into[name] for name, _ in lg.shapes(m, F, n_sib)}
    exit_arr, tr_arr = l2tx_array(exits), l2tx_array(transfers)
    mix_l1_arr, mix_l2_arr, mix_sigs = l1tx_array(mix_l1), l2tx_array(mix_l2), l2sig_array(mix_l2)
    # (b): the two separate tree calls, as tools/sparse_tree_bench.py makes them
    state_tree, exit_tree = L.smt(n_sib), L.smt(n_sib)
    TB.timed(state_tree, np.arange(first, first + base.N, dtype=np.uint64), np.stack(cols, axis=1))
    keys = np.array(senders, dtype=np.uint64)
    f_exit, f_state = TB.draw_fields(m, rng), TB.draw_fields(m, rng)
    names = ("exits_wall_ms", "exits_device_ms", "exits_semantic_ms", "exits_exit_ms", "l2_wall_ms", "l2_device_ms", "l2_semantic_ms", "two_trees_wall_ms",
             "two_trees_device_ms", "mixed_wall_ms", "mixed_device_ms", "mixed_semantic_ms", "mixed_exit_ms", "mixed_l1_ms")
    t = {name: [] for name in names}
    kinds = ("exits", "l2", "two_trees", "mixed")
    for r in range(len(kinds) * (reps + 1)):
        kind = kinds[r % len(kinds)]
        if kind != "two_trees":
            lg.load(*cols)
        else:
            exit_tree.reset()
        t0 = time.perf_counter()
        if kind == "exits":
            lg.apply_batch_exits([], exit_arr, plan, idxs, 1, 1, n_sib=n_sib, into=into, sigs=False)
        elif kind == "l2":
            lg.apply_l2(tr_arr, plan, idxs, n_sib=n_sib, into=l2_into)
        elif kind == "mixed":
            lg.apply_batch_exits(mix_l1_arr, mix_l2_arr, plan, idxs, 1, 1, n_sib=n_sib, into=mix_into, sigs=mix_sigs)
        else:
            exit_tree.apply(keys, f_exit, n_sib=n_sib)
            dev = exit_tree.device_ms()
            state_tree.apply(keys, f_state, n_sib=n_sib)
            dev += state_tree.device_ms()
        wall = (time.perf_counter() - t0) * 1e3
        if r < len(kinds):   # the first call of each kind grows the call's buffers
            continue
        t[kind + "_wall_ms"].append(wall)
        if kind == "two_trees":
            t["two_trees_device_ms"].append(dev)
            continue
        t[kind + "_device_ms"].append(lg.device_ms())
        t[kind + "_semantic_ms"].append(lg.semantic_ms())
        if kind != "l2":
            t[kind + "_exit_ms"].append(lg.exit_ms())
        if kind == "mixed":
            t["mixed_l1_ms"].append(lg.l1_ms())
            res["mixed_nullified"] = int((mix_into["l1_flags"] >> 1).sum())
            res["mixed_exit_leaves"] = int(lg.exit_tree().size())
        if kind == "exits":
            res["exit_leaves"] = int(lg.exit_tree().size())
    res.update({name: spread(xs) for name, xs in t.items()})
    res["exits_over_two_trees_wall"] = res["exits_wall_ms"]["median"] / res["two_trees_wall_ms"]["median"]
    res["exits_over_l2_wall"] = res["exits_wall_ms"]["median"] / res["l2_wall_ms"]["median"]
    lg.close()
    state_tree.close()
    exit_tree.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=300, help="seconds for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_ledger_exit.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return one(a.reps)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], stdout=subprocess.PIPE, timeout=a.timeout)
    if p.returncode != 0:
        raise SystemExit("the measurement ended with status %d" % p.returncode)
    result = json.loads(p.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(result), flush=True)
    doc = {"tool": "tools/ledger_exit_bench.py", "shape": list(SHAPE), "seed": SEED, "what": "2048 L2 exits of distinct senders through "
           "Ledger.apply_batch_exits, against (a) 2048 L2 transfers of the same senders through Ledger.apply_l2 and (b) the two separate "
           "SparseTree.apply calls of tools/sparse_tree_bench.py, alternating in one run; and 256 L1 (32 forceExits) + 1792 L2 (256 exits) "
           "through Ledger.apply_batch_exits; ms; every sample listed under all", "results": [result]}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
