#!/usr/bin/env python3
"""hz_state_apply against the existing batch-builder path, on the same updates (not part of bench.py).

For k = 13 and k = 20: a DenseState of 2^k accounts; 2048 L2 transfers drawn as synthetic_batch draws senders and receivers, i.e.
m = 4096 ordered leaf updates (sender, receiver, sender, receiver, ...).
  device path    State.apply of those 4096 updates on the device-resident tree: wall time per call (the Python wrapper's call, outputs
                 included: 17 siblings, old value, old / new root per update) and device time per call (hz_state_device_ms)
  existing path  the same transfers through the native builder (hzb_db over the DenseState base, hz_poseidon_dag installed): its walk +
                 evaluate time (hzb_batch_stats). That batch does more than the account tree -- it signs, hashes the signatures'
                 messages, packs the circuit inputs and serves the fee transaction --, which the stats keep apart where they can
                 (sign_s is reported, not counted); the leaf FIELDS of the device path are drawn, not the transfers' balances: the
                 cost of a hash does not depend on them.
Each k runs in a child process of its own under a time limit; nothing is started after a failure. Writes profiles/device_state_apply.json."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE = (2048, 32, 256, 64)   # the headline batch; no L1 transaction is added, so all 2048 slots are L2 transfers
SEED = 0x48455A31


def transfers(base, n_tx, seed):
    """(from, to) pairs as synthetic_batch's recipe draws them"""
    import random
    rng = random.Random(seed)
    return [(base.first_idx + rng.randrange(base.N), base.first_idx + rng.randrange(base.N)) for _ in range(n_tx)], base.first_idx + rng.randrange(base.N)


def existing_path(L, base, pairs, fee_idx, layout, reps):
    import numpy as np
    from circuits_amd import builder as B
    from circuits_amd import native_builder as NB
    n_tx = len(pairs)
    signer = [a.k.to_bytes(32, "little") for a in base.keys()]
    arr = np.zeros(n_tx, dtype=NB.tx_dtype())
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
        if to != frm:
            tb, tn = tmp[to] if to in tmp else (base.state(to)["balance"], 0)
            tmp[to] = (tb + amount, tn)
        else:
            tmp[frm] = (nb + amount, nonce + 1)
    arr["token_id"] = 1
    arr["signer_key"] = np.frombuffer(b"".join(keys), dtype="V32")
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
        runs.append({"build_wall_ms": wall * 1e3, "walk_ms": s["walk_s"] * 1e3, "eval_ms": s["eval_s"] * 1e3, "sign_ms": s["sign_s"] * 1e3,
                     "dag_device_ms": s["device_ms"], "jobs": s["jobs"], "segments": s["segments"]})
        bb.close()
        db.close()
    runs = runs[1:]   # the first build warms the evaluator's resident buffers
    out = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    out["walk_plus_eval_ms"] = out["walk_ms"] + out["eval_ms"]
    return out


def one(k, reps):
    import numpy as np
    from circuits_amd import builder as B
    from circuits_amd import lib
    L = lib()
    if L.device_count() <= 0:
        raise SystemExit("no gfx950 device: this tool measures on the device")
    t0 = time.perf_counter()
    base = B.DenseState.build(k, seed=SEED, hash_rows=lambda t, n, data: L.poseidon_batch_bytes(t, n, data))
    build_s = time.perf_counter() - t0
    pairs, fee_idx = transfers(base, SHAPE[0], SEED)
    idx = [x for p in pairs for x in p]
    rng = np.random.default_rng(SEED)
    cols = base.leaf_fields()
    acc = np.array(idx) - base.first_idx
    fields = np.stack([cols[0][acc], rng.integers(0, 256, size=(len(idx), 32), dtype=np.uint8), cols[2][acc], cols[3][acc]], axis=1)
    fields[:, 1, 24:] = 0   # balances below 2^192
    t0 = time.perf_counter()
    st = base.to_device(L)
    load_wall = time.perf_counter() - t0
    res = {"k": k, "m": len(idx), "distinct_accounts": len(set(idx)), "dense_state_build_s": build_s, "load_wall_ms": load_wall * 1e3,
           "load_device_ms": st.device_ms(), "root_matches_dense_state": st.root() == base.root}
    wall, dev = [], []
    for r in range(reps + 2):
        t0 = time.perf_counter()
        st.apply(idx, fields, n_sib=SHAPE[1] + 1)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(st.device_ms())
    res["apply"] = {"wall_ms": statistics.median(wall[2:]), "device_ms": statistics.median(dev[2:]), "wall_ms_all": wall, "device_ms_all": dev}
    st.close()
    g = L.ctx("rollup-main", nTx=SHAPE[0], nLevels=SHAPE[1], maxL1Tx=SHAPE[2], maxFeeTx=SHAPE[3])
    layout = g.packed_layout()
    g.close()
    res["existing"] = existing_path(L, base, pairs, fee_idx, layout, max(3, reps // 3))
    res["ratio_existing_over_apply_wall"] = res["existing"]["walk_plus_eval_ms"] / res["apply"]["wall_ms"]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="*", default=[13, 20])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per k (one child process each)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_state_apply.json"))
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child is not None:
        return one(a.child, a.reps)
    results = []
    for k in a.k:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(k), "--reps", str(a.reps)], stdout=subprocess.PIPE, timeout=a.timeout)
        if p.returncode != 0:
            raise SystemExit("k = %d ended with status %d: nothing more is run" % (k, p.returncode))
        results.append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    doc = {"tool": "tools/state_apply_bench.py", "shape": list(SHAPE), "seed": SEED, "what": "4096 ordered leaf updates (2048 transfers): State.apply "
           "against the native builder's walk + evaluate time for the same transfers; medians, ms", "results": results}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
