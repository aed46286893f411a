#!/usr/bin/env python3
"""From an applied batch to a context that can run: the host route against hz_ledger_main_inputs (not part of bench.py).

DESIGN 8h's recipe at the headline shape (2048, 32, 256, 64): a growing ledger of 2^13 accounts, 256 createAccountDeposit rows in front of
1792 signed L2 transfers (20 % of the sender's balance, selector 176), every signature verified on the device, one fee receiver. Two routes
alternate in one run, each on a freshly loaded ledger, each ending when the context's inputs lie on the device:
  host     today's route, its code unchanged: builder.ledger_atomic_batch_inputs(host_outputs=False) over the transaction dictionaries, then
           Ctx.set_inputs for the transaction-only signals and Ctx.set_input_dev for every signal the ledger left on the device
  packed   capi.Ledger.apply_resident over prebuilt ctypes rows, capi.Ledger.main_inputs (k_ledger_main_inputs writes the packed input
           buffer in device memory), Ctx.stage device to device
Recorded per route: the wall time, the apply call's share of it, and for `packed` main_inputs_ms and the bytes written; after the last
repetition of each route the context runs and main.hashGlobalInputs is read: the two must be equal.
The expectation, stated before the measurement: the median wall time of `packed` is below that of `host`, by medians of three. Nobody has
measured either route; no ratio is stated in advance. The case runs in a child process under a time limit. Writes
profiles/device_ledger_feed.json with every sample, the outcome included when it is a miss."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ledger_create_bench as CB  # noqa: E402
import sparse_tree_bench as TB    # noqa: E402
import state_apply_bench as SB    # noqa: E402

SHAPE, SEED = SB.SHAPE, SB.SEED
N_L1 = SHAPE[2]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def one(reps):
    import numpy as np
    import torch
    from circuits_amd import builder as B
    from circuits_amd import lib
    from circuits_amd.capi import from_bjj_array, l1tx_array, l2sig_array, l2tx_array
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
    for t in l2:
        t.update(keys[int(base.key_idx[t["fromIdx"] - base.first_idx])].sign_msg(B.build_hash_sig(t, 1)))
    n_sib, F = SHAPE[1] + 1, SHAPE[3]
    plan, idxs = [1] + [0] * (F - 1), [fee_idx] + [0] * (F - 1)
    cols = base.leaf_fields()
    last = base.first_idx + base.N - 1
    grow = L.ledger_growing(base.N + N_L1, first_idx=base.first_idx, n_sib_max=n_sib)
    g = L.ctx("rollup-main", nTx=SHAPE[0], nLevels=SHAPE[1], maxL1Tx=SHAPE[2], maxFeeTx=SHAPE[3])
    nbytes = g.packed_layout()[0]
    l2_arr, create_l1, create_keys, sigs = l2tx_array(l2), l1tx_array(creates), from_bjj_array(creates), l2sig_array(l2)
    apply_s = [0.0]
    inner = grow.apply_batch_atomic

    def timed_apply(*a, **kw):   # the apply's share of the host route, measured around the call the builder makes
        t0 = time.perf_counter()
        try:
            return inner(*a, **kw)
        finally:
            apply_s[0] = time.perf_counter() - t0
    grow.apply_batch_atomic = timed_apply
    routes = ("host", "packed")
    t = {r + "_" + name: [] for r in routes for name in ("wall_ms", "apply_ms")}
    t["packed_main_inputs_ms"] = []
    hashes, roots = {}, {}
    for r in range(len(routes) * (reps + 1)):
        route = routes[r % len(routes)]
        grow.load_accounts(*cols)
        like = types.SimpleNamespace(last_idx=last, num_batch=0)
        g.clear_inputs()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if route == "host":
            inp, dev = B.ledger_atomic_batch_inputs(grow, like, creates, l2, *SHAPE, [1], [fee_idx], 1, host_outputs=False, verify=True)[:2]
            g.set_inputs(inp)
            for name, (ptr, count) in dev.items():
                g.set_input_dev(name, ptr, count)
            applied = apply_s[0]
        else:
            t1 = time.perf_counter()
            grow.apply_resident(create_l1, l2_arr, plan, idxs, 1, 1, n_sib=n_sib, verify=True, atomic=True, sigs=sigs, from_bjj=create_keys)
            applied = time.perf_counter() - t1
            addr, _, buf = grow.main_inputs(g, last)
            g.stage(0, addr, nbytes)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        roots[route] = grow.root()
        if r >= len(routes) * reps:   # the last repetition of each route: the circuit itself on what the route left
            g.run()
            hashes[route] = g.get("main.hashGlobalInputs")
        if r < len(routes):   # the first call of each route grows the call's buffers and builds the fixed-base table
            continue
        t[route + "_wall_ms"].append(wall)
        t[route + "_apply_ms"].append(applied * 1e3)
        if route == "packed":
            t["packed_main_inputs_ms"].append(grow.main_inputs_ms())
    res = {"k": k, "n_l1": N_L1, "m": len(l2), "n_sib": n_sib, "F": F, "packed_bytes": nbytes}
    res.update({name: spread(xs) for name, xs in t.items()})
    res["same_root"] = roots["host"] == roots["packed"]
    res["hash_global_inputs"] = {r: "%x" % hashes[r] for r in routes}
    res["same_hash_global_inputs"] = hashes["host"] == hashes["packed"]
    for r in routes:
        res[r + "_beside_apply_ms"] = res[r + "_wall_ms"]["median"] - res[r + "_apply_ms"]["median"]
    res["expectation"] = {"packed_wall_below_host_wall": res["packed_wall_ms"]["median"] < res["host_wall_ms"]["median"],
                          "host_over_packed_wall": res["host_wall_ms"]["median"] / res["packed_wall_ms"]["median"]}
    grow.close()
    g.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=420, help="seconds for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_ledger_feed.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return one(a.reps)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], stdout=subprocess.PIPE, timeout=a.timeout)
    if p.returncode != 0:
        raise SystemExit("the measurement ended with status %d" % p.returncode)
    result = json.loads(p.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(result), flush=True)
    doc = {"tool": "tools/ledger_feed_bench.py", "shape": list(SHAPE), "seed": SEED, "what": "256 createAccountDeposit + 1792 signed L2 transfers on 2^13 accounts on a "
           "growing ledger, verified on the device, from the request to a RollupMain context whose inputs lie on the device: the host route "
           "(builder.ledger_atomic_batch_inputs(host_outputs=False), Ctx.set_inputs, Ctx.set_input_dev per signal) against the packed route (apply_resident over prebuilt "
           "rows, hz_ledger_main_inputs, hz_inputs_stage), alternating in one run on freshly loaded ledgers; ms; every sample listed under all",
           "expectation": "stated beforehand: the packed route's median wall time is below the host route's, by medians of %d; no ratio stated" % a.reps,
           "outcome": result["expectation"], "results": [result]}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
