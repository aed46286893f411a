#!/usr/bin/env python3
"""Exit trees of earlier batches kept on the ledger, and Withdraw's inputs in bulk (not part of bench.py).

8g's workload -- 2048 L2 exits of 2048 distinct senders on a state of 2^13 accounts, 20 % of the sender's balance, selector 176, nLevels + 1 =
33 siblings -- as 16 batches of 128 exits on one ledger, each kept after it is applied (Ledger.exit_keep).
  keep           per batch: the wall time of Ledger.apply_batch_exits (no output returned to the host) and, right behind it, the wall and
                 device time of Ledger.exit_keep
  rows           Ledger.withdraw_rows of n = 2^16 and 2^20 queries spread over the 16 kept batches (every query a kept leaf, drawn with
                 repetition): withdraw_ms (the two kernels), the wall time with every output copied into host arrays, and with the device
                 arrays alone
  proofs         the only path there was, in the same process: SparseTree.proofs (hz_smt_proofs: a host walk, a gather, a download) plus
                 Ledger.exit_accounts on the LIVE tree -- the last batch's -- for 2^16 keys of that batch, wall time
  withdraw_fed   Withdraw(32) witnesses per second, a context of 2^16 instances, 16 launches a step: before every launch the context's
                 eight inputs are set from Ledger.withdraw_rows_dev of a fresh withdraw_rows call (set_input_dev, instance -1); beside it
                 the same context stepping on inputs left in place, as bench.py's config 5 does, and that line of profiles/r06_bench_line.json
The three expectations of the feature's issue are carried as rules; the tool prints whether each held. The case runs once, in a child
process under a time limit. Writes profiles/device_exit_archive.json with every sample."""
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
import state_apply_bench as SB    # noqa: E402

SHAPE, SEED = SB.SHAPE, SB.SEED
EXIT_IDX = 1
BATCHES, PER_BATCH = 16, 128


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def one(reps):
    import numpy as np
    import torch
    from circuits_amd import builder as B
    from circuits_amd import lib
    from circuits_amd.capi import WITHDRAW_ARRAYS, WITHDRAW_SIGNALS, l2tx_array
    L = lib()
    if L.device_count() <= 0:
        raise SystemExit("no gfx950 device: this tool measures on the device")
    k, m = 13, BATCHES * PER_BATCH
    n_levels = SHAPE[1]
    n_sib = n_levels + 1
    base = B.DenseState.build(k, seed=SEED, hash_rows=lambda t, n, data: L.poseidon_batch_bytes(t, n, data))
    rng = np.random.default_rng(SEED)
    first = base.first_idx
    senders = [first + int(x) for x in rng.choice(base.N, size=m, replace=False)]
    rows = [{"fromIdx": s, "toIdx": EXIT_IDX, "amountF": B.floor_fix2float(base.state(s)["balance"] * 20 // 100), "nonce": 0, "tokenID": 1, "userFee": 176}
            for s in senders]
    lg = L.ledger(k, first_idx=first)
    lg.load(*base.leaf_fields())
    res = {"k": k, "batches": BATCHES, "exits_per_batch": PER_BATCH, "n_sib": n_sib}
    t = {"apply_wall_ms": [], "keep_wall_ms": [], "keep_device_ms": []}
    for b in range(BATCHES):
        arr = l2tx_array(rows[b * PER_BATCH:(b + 1) * PER_BATCH])
        t0 = time.perf_counter()
        lg.apply_batch_exits([], arr, [1], [0], 1, b + 1, n_sib=n_sib, outputs=False, sigs=False)
        t1 = time.perf_counter()
        lg.exit_keep(b + 1)
        t2 = time.perf_counter()
        t["apply_wall_ms"].append((t1 - t0) * 1e3)
        t["keep_wall_ms"].append((t2 - t1) * 1e3)
        t["keep_device_ms"].append(lg.exit_keep_ms())
    res["archive"] = lg.exit_archive_stats()
    assert res["archive"]["snapshots"] == BATCHES and lg.exit_tree().size() == PER_BATCH

    def queries(n):
        pick = rng.integers(0, m, size=n)
        return (pick // PER_BATCH + 1).astype(np.uint32), np.array(senders, dtype=np.uint64)[pick]

    for n, tag in ((1 << 16, "64k"), (1 << 20, "1m")):
        bn, idx = queries(n)
        into = {name: np.zeros((n, 32), dtype=np.uint8) for name in WITHDRAW_ARRAYS[:7]}
        into["siblings_state"] = np.zeros((n, n_sib, 32), dtype=np.uint8)
        into["status"] = np.zeros(n, dtype=np.uint8)
        lg.withdraw_rows(bn, idx, n_levels, into=into)   # the first call grows the buffers
        assert not into["status"].any()
        dev_ms, host_wall, dev_wall = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            lg.withdraw_rows(bn, idx, n_levels, into=into)
            host_wall.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            lg.withdraw_rows(bn, idx, n_levels, outputs=False)
            dev_wall.append((time.perf_counter() - t0) * 1e3)
            dev_ms.append(lg.withdraw_ms())
        t.update({"rows_%s_device_ms" % tag: dev_ms, "rows_%s_wall_host_outputs_ms" % tag: host_wall, "rows_%s_wall_device_outputs_ms" % tag: dev_wall})

    # the path there was: the live tree is the last batch's
    n = 1 << 16
    last = np.array(senders[(BATCHES - 1) * PER_BATCH:], dtype=np.uint64)
    keys = last[rng.integers(0, PER_BATCH, size=n)]
    tree = lg.exit_tree()
    tree.proofs(keys, n_sib=n_sib)
    lg.exit_accounts(keys)
    t["proofs_64k_wall_ms"] = []
    for _ in range(reps):
        t0 = time.perf_counter()
        p = tree.proofs(keys, n_sib=n_sib)
        f = lg.exit_accounts(keys)
        t["proofs_64k_wall_ms"].append((time.perf_counter() - t0) * 1e3)
    got = lg.withdraw_rows(np.full(n, BATCHES, dtype=np.uint32), keys, n_levels)
    assert p["found"].all() and got["siblings_state"].tobytes() == p["siblings"].tobytes() and got["balance"].tobytes() == f[:, 1].tobytes()

    # Withdraw(32) fed from the archive
    N, launches = 1 << 16, 16
    c = L.ctx("withdraw", nLevels=n_levels, n_instances=N)
    stream = torch.cuda.Stream()
    fed_in = torch.cuda.Event()

    def feed():
        bn, idx = queries(N)
        lg.withdraw_rows(bn, idx, n_levels, outputs=False)
        dev = lg.withdraw_rows_dev()
        for name, signal in WITHDRAW_SIGNALS.items():
            c.set_input_dev(signal, dev[name], N * (n_sib if name == "siblings_state" else 1), instance=-1, stream=stream.cuda_stream)
        fed_in.record(stream)

    def step(fed):
        for _ in range(launches):
            if fed:
                feed()
            c.enqueue(stream.cuda_stream)
            if fed:
                fed_in.synchronize()   # the next withdraw_rows reuses the arrays the copies read; the witness kernels run on beside it
        c.check()

    step(True)
    t["withdraw_fed_per_s"], t["withdraw_in_place_per_s"] = [], []
    for r in range(2 * reps):
        fed = r % 2 == 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(fed)
        torch.cuda.synchronize()
        t["withdraw_fed_per_s" if fed else "withdraw_in_place_per_s"].append(launches * N / (time.perf_counter() - t0))
    res.update({name: spread(xs) for name, xs in t.items()})
    try:
        line = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_line.json")))
        res["r06_withdraw_per_s"] = line["withdraw"]["value"]
    except (OSError, KeyError, ValueError):
        res["r06_withdraw_per_s"] = None
    # the expectations, as rules
    res["rules"] = {
        "rows_device_outputs_64k_no_slower_than_proofs_path": {
            "rows_wall_ms": res["rows_64k_wall_device_outputs_ms"]["median"], "proofs_wall_ms": res["proofs_64k_wall_ms"]["median"],
            "held": res["rows_64k_wall_device_outputs_ms"]["median"] <= res["proofs_64k_wall_ms"]["median"]},
        "a_keep_costs_a_small_part_of_its_apply": {
            "keep_over_apply_wall": res["keep_wall_ms"]["median"] / res["apply_wall_ms"]["median"],
            "held": res["keep_wall_ms"]["median"] <= 0.25 * res["apply_wall_ms"]["median"]},
        "fed_withdraw_rate_within_the_spread_of_the_rate_on_inputs_in_place": {
            "fed_per_s": res["withdraw_fed_per_s"]["median"], "in_place_per_s": res["withdraw_in_place_per_s"]["median"],
            "in_place_min_per_s": res["withdraw_in_place_per_s"]["min"], "r06_per_s": res["r06_withdraw_per_s"],
            "held": res["withdraw_fed_per_s"]["median"] >= res["withdraw_in_place_per_s"]["min"]}}
    lg.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_exit_archive.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return one(a.reps)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], stdout=subprocess.PIPE, timeout=a.timeout)
    if p.returncode != 0:
        raise SystemExit("the measurement ended with status %d" % p.returncode)
    result = json.loads(p.stdout.decode().strip().splitlines()[-1])
    for name, rule in result["rules"].items():
        print("%s: %s  %s" % (name, "held" if rule["held"] else "DID NOT HOLD", {k2: v for k2, v in rule.items() if k2 != "held"}), flush=True)
    doc = {"tool": "tools/exit_archive_bench.py", "shape": list(SHAPE), "seed": SEED, "what": "2048 L2 exits of distinct senders on 2^13 accounts as 16 "
           "batches of 128 through Ledger.apply_batch_exits, each kept (Ledger.exit_keep); Ledger.withdraw_rows of 2^16 and 2^20 queries over the 16 "
           "kept batches; SparseTree.proofs + Ledger.exit_accounts on the live tree for 2^16 keys; Withdraw(32) at 16 launches of 2^16 instances fed "
           "from Ledger.withdraw_rows_dev, and on inputs left in place; ms and witnesses/s; every sample listed under all; rules: the issue's three "
           "expectations, none a merge condition", "results": [result]}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
