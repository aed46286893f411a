#!/usr/bin/env python3
"""hz_smt (the sparse device-resident Merkle tree) against the existing batch-builder path, on the same tree operations (not part of
bench.py); medians over --reps, ms. n_sib = 33 (nLevels + 1 of the headline circuit), all seven outputs returned.

  exit_inserts_2048   2048 L2 exits of 2048 distinct senders on a state of 2^13 accounts: 2048 INSERTS into the empty exit tree, and
                      2048 updates of the senders' state leaves.
  state_mix_8192      256 create-account deposits (idx = lastIdx + 1 ..) and 2048 L2 transfers on a state of 2^13 accounts: 256
                      INSERTS into the state tree followed by 4096 updates (sender, receiver, sender, receiver, ...).
  device path    SparseTree.apply of those operations: wall time of the Python wrapper's call and device time (hz_smt_device_ms). The
                 exit workload is two calls, one per tree; the inserts alone are reported beside their sum.
  existing path  the same transactions as ONE batch of the native builder (hzb_* over the DenseState base, hz_poseidon_dag installed):
                 its walk + evaluate time (hzb_batch_stats), as tools/state_apply_bench.py reads it. That batch does more than the two
                 trees -- it hashes the signatures' messages, packs the circuit inputs, serves the fee transaction (signing is reported,
                 not counted) --, and the leaf FIELDS of the device path are drawn, not the transactions' balances: the cost of a hash
                 does not depend on them.
Also: builder.ExitTreeFixture(2048) through the Python builder's walk + hz_poseidon_dag (device=0) and through sparse_tree=.
Writes profiles/device_sparse_tree.json."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_LEVELS = 32
N_SIB = N_LEVELS + 1
K = 13
SEED = 0x48455A31


def draw_fields(n, rng):
    import numpy as np
    f = rng.integers(0, 256, size=(n, 4, 32), dtype=np.uint8)
    f[:, :, 24:] = 0   # every field below 2^192
    return f


def timed(tree, keys, fields):
    t0 = time.perf_counter()
    tree.apply(keys, fields, n_sib=N_SIB)
    return (time.perf_counter() - t0) * 1e3, tree.device_ms()


def med(rows):
    return {"wall_ms": statistics.median(r[0] for r in rows), "device_ms": statistics.median(r[1] for r in rows),
            "wall_ms_all": [r[0] for r in rows], "device_ms_all": [r[1] for r in rows]}


def l2_txs(base, pairs):
    """signed L2 transactions (from, to) of 20 % of the sender's balance, as synthetic_batch's recipe makes them -> hzb_tx records"""
    import numpy as np
    from circuits_amd import builder as B
    from circuits_amd import native_builder as NB
    signer = [a.k.to_bytes(32, "little") for a in base.keys()]
    arr = np.zeros(len(pairs), dtype=NB.tx_dtype())
    tmp, keys = {}, []
    for i, (frm, to) in enumerate(pairs):
        bal, nonce = tmp[frm] if frm in tmp else (base.state(frm)["balance"], 0)
        amount_f = B.floor_fix2float(bal * 20 // 100)
        amount = B.float2fix(amount_f)
        arr["from_idx"][i], arr["to_idx"][i], arr["amount_f"][i], arr["nonce"][i] = frm, to, amount_f, nonce
        arr["user_fee"][i], arr["flags"][i] = 176, NB.HAS_NONCE | NB.HAS_SIGNER
        keys.append(signer[int(base.key_idx[frm - base.first_idx])])
        nb = bal - amount - B.compute_fee(amount, 176)
        tmp[frm] = (nb, nonce + 1)
        if to == B.EXIT_IDX:
            continue
        if to != frm:
            tb, tn = tmp[to] if to in tmp else (base.state(to)["balance"], 0)
            tmp[to] = (tb + amount, tn)
        else:
            tmp[frm] = (nb + amount, nonce + 1)
    arr["token_id"] = 1
    arr["signer_key"] = np.frombuffer(b"".join(keys), dtype="V32")
    return arr


def l1_create_txs(n, rng):
    """create-account deposits (fromIdx 0: the account gets idx = lastIdx + 1) -> hzb_tx records"""
    import numpy as np
    from circuits_amd import builder as B
    from circuits_amd import native_builder as NB
    accounts = [B.Account(SEED * 1000 + 100 + i) for i in range(8)]
    arr = np.zeros(n, dtype=NB.tx_dtype())
    pick = [accounts[int(q)] for q in rng.integers(0, len(accounts), size=n)]
    arr["on_chain"] = 1
    arr["token_id"] = 1
    arr["load_amount_f"] = [B.floor_fix2float(int(x)) for x in rng.integers(1, 1 << 62, size=n)]
    arr["from_bjj_compressed"] = np.frombuffer(b"".join(a.bjj_compressed.to_bytes(32, "little") for a in pick), dtype="V32")
    arr["from_eth_addr"] = np.frombuffer(b"".join(a.eth_addr.to_bytes(32, "little") for a in pick), dtype="V32")
    return arr


def existing_path(L, base, arr, shape, fee_idx, reps):
    """the batch through the native builder: medians of its own clocks over `reps` builds after one that warms the evaluator's buffers"""
    from circuits_amd import native_builder as NB
    g = L.ctx("rollup-main", nTx=shape[0], nLevels=shape[1], maxL1Tx=shape[2], maxFeeTx=shape[3])
    layout = NB.layout_tables(g.packed_layout())
    g.close()
    runs, facts = [], {}
    for _ in range(reps + 1):
        db = NB.NativeRollupDB(chain_id=1, device=0, base=base)
        bb = db.build_batch(*shape)
        bb.add_txs(arr)
        bb.add_token(1)
        bb.add_fee_idx(fee_idx)
        t0 = time.perf_counter()
        bb.build(layout)
        wall = time.perf_counter() - t0
        s = bb.stats()
        runs.append({"build_wall_ms": wall * 1e3, "walk_ms": s["walk_s"] * 1e3, "eval_ms": s["eval_s"] * 1e3, "sign_ms": s["sign_s"] * 1e3,
                     "dag_device_ms": s["device_ms"], "jobs": s["jobs"], "segments": s["segments"]})
        facts = {"last_idx_after": bb.roots()[2]}
        bb.close()
        db.close()
    runs = runs[1:]
    out = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    out["walk_plus_eval_ms"] = out["walk_ms"] + out["eval_ms"]
    out.update(facts)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_sparse_tree.json"))
    a = ap.parse_args()
    import numpy as np
    from circuits_amd import builder as B
    from circuits_amd import lib
    L = lib()
    if L.device_count() <= 0:
        raise SystemExit("no gfx950 device: this tool measures on the device")
    rng = np.random.default_rng(SEED)
    base = B.DenseState.build(K, seed=SEED, hash_rows=lambda t, n, data: L.poseidon_batch_bytes(t, n, data))
    n0, first = base.N, base.first_idx
    state, exits = L.smt(N_SIB), L.smt(N_SIB)
    base_keys = np.arange(first, first + n0, dtype=np.uint64)
    base_fields = np.stack(base.leaf_fields(), axis=1)
    doc = {"tool": "tools/sparse_tree_bench.py", "n_sib": N_SIB, "state_accounts": n0, "seed": SEED, "reps": a.reps,
           "what": "SparseTree.apply against the native builder's walk + evaluate time for the same transactions; medians, ms"}
    build = timed(state, base_keys, base_fields)
    doc["state_tree_build"] = {"m": n0, "wall_ms": build[0], "device_ms": build[1], "root_matches_dense_state": state.root() == base.root}

    # ---- 2048 exits of distinct senders: 2048 exit-tree inserts + 2048 state-tree updates
    senders = [first + int(x) for x in rng.choice(n0, size=2048, replace=False)]
    keys = np.array(senders, dtype=np.uint64)
    f_exit, f_state = draw_fields(2048, rng), draw_fields(2048, rng)
    ins, upd = [], []
    for _ in range(a.reps + 2):
        exits.reset()
        ins.append(timed(exits, keys, f_exit))
        upd.append(timed(state, keys, f_state))   # (updates: the same call again is the same work)
    both = [(i[0] + u[0], i[1] + u[1]) for i, u in zip(ins, upd)]
    w1 = {"m": 2048, "exit_inserts": med(ins[2:]), "state_updates": med(upd[2:]), "apply": med(both[2:])}
    shape = (2048, N_LEVELS, 256, 64)
    w1["existing"] = existing_path(L, base, l2_txs(base, [(s, B.EXIT_IDX) for s in senders]), shape, senders[0], max(3, a.reps // 2))
    w1["ratio_existing_over_apply_wall"] = w1["existing"]["walk_plus_eval_ms"] / w1["apply"]["wall_ms"]
    fx = {"python_walk_dag": [], "sparse_tree": []}
    for r in range(3):
        t0 = time.perf_counter()
        host_fx = B.ExitTreeFixture(2048, device=0)
        fx["python_walk_dag"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        dev_fx = B.ExitTreeFixture(2048, sparse_tree=exits)
        fx["sparse_tree"].append((time.perf_counter() - t0) * 1e3)
        w1["fixture_roots_equal"] = host_fx.exit_tree.root == dev_fx.exit_tree.root
    w1["exit_tree_fixture_wall_ms"] = {k: statistics.median(v[1:]) for k, v in fx.items()}
    doc["exit_inserts_2048"] = w1
    print(json.dumps(w1), flush=True)

    # ---- 256 create-account deposits + 2048 transfers: 256 inserts + 4096 updates on the state tree
    pairs = [(first + int(x), first + int(y)) for x, y in rng.integers(0, n0, size=(2048, 2))]
    new_keys = np.arange(first + n0, first + n0 + 256, dtype=np.uint64)
    mix_keys = np.concatenate([new_keys, np.array([x for p in pairs for x in p], dtype=np.uint64)])
    mix_fields = draw_fields(mix_keys.size, rng)
    mix = []
    for _ in range(a.reps + 2):
        state.reset()
        timed(state, base_keys, base_fields)
        mix.append(timed(state, mix_keys, mix_fields))
    w2 = {"keys_before": n0, "m": int(mix_keys.size), "inserts": 256, "updates": 4096, "size_after": state.size(), "apply": med(mix[2:])}
    arr = np.concatenate([l1_create_txs(256, rng), l2_txs(base, pairs)])
    w2["existing"] = existing_path(L, base, arr, (2304, N_LEVELS, 256, 64), pairs[0][0], max(3, a.reps // 2))
    w2["existing_created_the_256_accounts"] = w2["existing"]["last_idx_after"] == first + n0 + 255
    w2["ratio_existing_over_apply_wall"] = w2["existing"]["walk_plus_eval_ms"] / w2["apply"]["wall_ms"]
    doc["state_mix_8192"] = w2
    print(json.dumps(w2), flush=True)
    state.close()
    exits.close()
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
