#!/usr/bin/env python3
"""hz_ledger_rollback against the only way back there was -- a reload of the whole state -- and against the apply it undoes; the price of the
journal on an apply; and the apply calls with the journal off on this tree against a parent build (not part of bench.py). DESIGN.md 8m.

Cases, at the sizes 8c and 8h use (state_apply_bench's recipe: 20 % of the sender's balance, selector 176, 33 siblings, 64 fee slots):
  dense13 / dense20   2048 L2 transfers through Ledger.apply_l2 on 2^13 / 2^20 dense accounts
  grow13              256 createAccountDeposit rows + 1792 transfers through GrowingLedger.apply_batch_creates on a growing ledger of 2^13
Per case, in one child process, outputs left on the device, after one round that grows every buffer:
  (a) reload           hz_ledger_load / _load_accounts of the state: wall
      apply_on         the batch with a journal of depth 8: wall, device_ms, journal_ms, the record's bytes
      rollback_1       hz_ledger_rollback of that one batch: wall, rollback_ms; the root is the loaded state's again
      rollback_8       eight consecutive batches (the recipe carried on over balances and nonces) undone in one call: wall, rollback_ms
  (c) apply_off        the same batch with the journal off, alternating with apply_on: the price of the feature, reported, not gated
THE EXPECTATION, written before the first run: the rollback of one batch costs less wall time than the apply it undoes -- it hashes
nothing, uploads nothing and makes one synchronise. Judged by the rule that stands here: median(rollback_1 wall) < median(apply_on wall);
HELD or MISSED per case. Nothing is fixed in advance about the reload: it is reported as a ratio.
  (b) --ab PARENT      PARENT holds a parent build (its circuits_amd package with its libraries). The journal-off apply of each case,
      this tree against the parent, alternating child processes in one call; every median of this tree must lie within the parent's own
      spread (min .. max over its samples of the same run). Writes profiles/ledger_rollback_ab.json.
Every child runs under a time limit; nothing is started after a failure. Writes profiles/device_ledger_rollback.json with every sample."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
CASES = {"dense13": 13, "dense20": 20, "grow13": 13}
DEPTH, EIGHT = 8, 8


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def setup(case, n_batches, package_root):
    """-> (L, ledger factory, load, [apply(ledger) per batch]): the recipe's batches, valid in order on the loaded state"""
    sys.path.insert(0, TOOLS)
    import numpy as np
    import ledger_create_bench as CB
    import sparse_tree_bench as TB
    import state_apply_bench as SB
    sys.path.insert(0, package_root)   # last, so in front: the recipes above put this tree on the path themselves
    from circuits_amd import builder as B
    from circuits_amd import lib
    from circuits_amd.capi import from_bjj_array, l1tx_array, l2sig_array, l2tx_array
    L = lib()
    if L.device_count() <= 0:
        raise SystemExit("no gfx950 device: this tool measures on the device")
    SHAPE, SEED = SB.SHAPE, SB.SEED
    k, grow = CASES[case], case.startswith("grow")
    n_l1 = SHAPE[2] if grow else 0
    base = B.DenseState.build(k, seed=SEED, hash_rows=lambda t, n, data: L.poseidon_batch_bytes(t, n, data))
    pairs, fee_idx = SB.transfers(base, SHAPE[0], SEED)
    more = SB.transfers(base, SHAPE[0] * (n_batches - 1), SEED + 1)[0] if n_batches > 1 else []
    n_sib, F = SHAPE[1] + 1, SHAPE[3]
    plan, idxs = [1] + [0] * (F - 1), [fee_idx] + [0] * (F - 1)
    rng = np.random.default_rng(SEED)
    tmp, applies = {}, []
    for b in range(n_batches):
        rows = (pairs if b == 0 else more[(b - 1) * SHAPE[0]:b * SHAPE[0]])[n_l1:]
        l2 = []
        for frm, to in rows:
            bal, nonce = tmp[frm] if frm in tmp else (base.state(frm)["balance"], 0)
            amount_f = B.floor_fix2float(bal * 20 // 100)
            amount = B.float2fix(amount_f)
            l2.append({"fromIdx": frm, "toIdx": to, "amountF": amount_f, "nonce": nonce, "tokenID": 1, "userFee": 176})
            tmp[frm] = (bal - amount - B.compute_fee(amount, 176), nonce + 1)
            tb, tn = tmp[to] if to in tmp else (base.state(to)["balance"], 0)
            tmp[to] = (tb + amount, tn)
        arr = l2tx_array(l2)
        if grow:
            creates = CB.create_rows(TB.l1_create_txs(n_l1, rng))
            l1, keys, sigs = l1tx_array(creates), from_bjj_array(creates), l2sig_array(l2)
            applies.append(lambda lg, l1=l1, keys=keys, arr=arr, sigs=sigs: lg.apply_batch_creates(l1, arr, plan, idxs, 1, 1, n_sib=n_sib, outputs=False, sigs=sigs, from_bjj=keys))
        else:
            applies.append(lambda lg, arr=arr: lg.apply_l2(arr, plan, idxs, n_sib=n_sib, outputs=False))
    cols = base.leaf_fields()
    if grow:
        make = lambda: L.ledger_growing(base.N + n_l1 * n_batches, first_idx=base.first_idx, n_sib_max=n_sib)   # noqa: E731
        load = lambda lg: lg.load_accounts(*cols)                                                               # noqa: E731
    else:
        make = lambda: L.ledger(k, first_idx=base.first_idx)   # noqa: E731
        load = lambda lg: lg.load(*cols)                       # noqa: E731
    return L, make, load, applies


def timed(f, *args):
    t0 = time.perf_counter()
    f(*args)
    return (time.perf_counter() - t0) * 1e3


def measure(case, reps):
    L, make, load, applies = setup(case, EIGHT, ROOT)
    on, off = make(), make()
    on.journal(DEPTH)
    names = ("reload_wall_ms", "apply_on_wall_ms", "apply_on_device_ms", "journal_ms", "apply_off_wall_ms", "apply_off_device_ms", "rollback_1_wall_ms", "rollback_1_ms",
             "rollback_8_wall_ms", "rollback_8_ms", "apply_8_wall_ms")
    t = {name: [] for name in names}
    res = {"case": case, "k": CASES[case], "depth": DEPTH}
    for r in range(reps + 1):
        s = {}
        s["reload_wall_ms"] = timed(load, on)
        root0 = on.root()
        s["apply_on_wall_ms"] = timed(applies[0], on)
        s["apply_on_device_ms"], s["journal_ms"] = on.device_ms(), on.journal_ms()
        res["record_bytes"] = on.journal_stats()["bytes_used"]
        s["rollback_1_wall_ms"] = timed(on.rollback, 0)
        s["rollback_1_ms"] = on.rollback_ms()
        assert on.root() == root0 and on.applied() == 0
        load(off)
        s["apply_off_wall_ms"] = timed(applies[0], off)
        s["apply_off_device_ms"] = off.device_ms()
        root1 = off.root()
        s["apply_8_wall_ms"] = sum(timed(a, on) for a in applies)
        res["eight_records_bytes"] = on.journal_stats()["bytes_used"]
        s["rollback_8_wall_ms"] = timed(on.rollback, 0)
        s["rollback_8_ms"] = on.rollback_ms()
        assert on.root() == root0 and on.applied() == 0
        applies[0](on)
        assert on.root() == root1   # the rolled-back ledger takes the batch as the freshly loaded one does
        if r:   # the first round grows the call's buffers and the journal's slabs
            for name in names:
                t[name].append(s[name])
    res["journal_stats"] = on.journal_stats()
    res.update({name: spread(xs) for name, xs in t.items()})
    med = lambda name: res[name]["median"]   # noqa: E731
    res["expectation"] = {"rule": "median(rollback_1 wall) < median(apply_on wall)", "rollback_1_wall_ms": med("rollback_1_wall_ms"),
                          "apply_on_wall_ms": med("apply_on_wall_ms"), "outcome": "HELD" if med("rollback_1_wall_ms") < med("apply_on_wall_ms") else "MISSED"}
    res["reload_over_rollback_1_wall"] = med("reload_wall_ms") / med("rollback_1_wall_ms")
    res["reload_over_rollback_8_wall"] = med("reload_wall_ms") / med("rollback_8_wall_ms")
    res["journal_price_wall_ms"] = med("apply_on_wall_ms") - med("apply_off_wall_ms")
    on.close()
    off.close()
    print(json.dumps(res))


def apply_off(case, reps, package_root):
    """the journal-off apply alone, through whichever package lies at package_root: nothing here names the journal"""
    L, make, load, applies = setup(case, 1, package_root)
    lg = make()
    wall, dev, sem = [], [], []
    for r in range(reps + 1):
        load(lg)
        w = timed(applies[0], lg)
        if r:
            wall.append(w)
            dev.append(lg.device_ms())
            sem.append(lg.semantic_ms())
    lg.close()
    print(json.dumps({"case": case, "wall_ms": wall, "device_ms": dev, "semantic_ms": sem, "version": L.version().decode() if isinstance(L.version(), bytes) else L.version()}))


def child(args, timeout):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, timeout=timeout)
    if p.returncode != 0:
        raise SystemExit("%s ended with status %d: nothing more is run" % (" ".join(args), p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_ledger_rollback.json"))
    ap.add_argument("--ab", default=None, help="a directory that holds a parent build's circuits_amd package: measure (b) instead")
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "ledger_rollback_ab.json"))
    ap.add_argument("--rounds", type=int, default=3, help="(b): child processes per side and case")
    ap.add_argument("--child", default=None)
    ap.add_argument("--package", default=ROOT)
    a = ap.parse_args()
    if a.child == "measure":
        return measure(a.cases[0], a.reps)
    if a.child == "off":
        return apply_off(a.cases[0], a.reps, a.package)
    if a.ab:
        results = []
        for case in a.cases:
            side = {"parent": {"wall_ms": [], "device_ms": [], "semantic_ms": []}, "branch": {"wall_ms": [], "device_ms": [], "semantic_ms": []}}
            for _ in range(a.rounds):
                for name, root in (("parent", os.path.abspath(a.ab)), ("branch", ROOT)):
                    got = child(["--child", "off", "--cases", case, "--reps", str(a.reps), "--package", root], a.timeout)
                    for key in side[name]:
                        side[name][key] += got[key]
            row = {"case": case}
            for key in ("wall_ms", "device_ms", "semantic_ms"):
                p, b = spread(side["parent"][key]), spread(side["branch"][key])
                row[key] = {"parent": p, "branch": b, "branch_median_within_parent_spread": p["min"] <= b["median"] <= p["max"]}
            row["within"] = all(row[key]["branch_median_within_parent_spread"] for key in ("wall_ms", "device_ms", "semantic_ms"))
            results.append(row)
            print(json.dumps(row), flush=True)
        doc = {"tool": "tools/ledger_rollback_bench.py --ab", "what": "the apply of each case with the journal off (the default), a parent build against this tree, "
               "alternating child processes in one call; the requirement: every median of this tree lies within the parent's own spread of the same run; ms; every "
               "sample listed under all", "rounds": a.rounds, "reps": a.reps, "results": results, "outcome": "WITHIN" if all(r["within"] for r in results) else "OUTSIDE"}
        with open(a.ab_out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return
    results = []
    for case in a.cases:
        results.append(child(["--child", "measure", "--cases", case, "--reps", str(a.reps)], a.timeout))
        print(json.dumps(results[-1]), flush=True)
    doc = {"tool": "tools/ledger_rollback_bench.py", "what": "hz_ledger_rollback of one batch and of eight against a reload of the state and against the apply it undoes, and "
           "the apply with a journal of depth 8 against the journal off, on 2048 transfers over 2^13 and 2^20 dense accounts and on 256 creates + 1792 transfers over a "
           "growing ledger of 2^13; outputs left on the device; ms; every sample listed under all",
           "expectation": "stated beforehand: median(rollback_1 wall) < median(apply_on wall) -- one batch's rollback costs less than the apply it undoes",
           "outcome": {r["case"]: r["expectation"]["outcome"] for r in results}, "results": results}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
