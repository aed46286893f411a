"""Exits on the device-resident ledger (hz_ledger_apply_batch_exits) without a device: the scheme model (exit scan included)
against BatchBuilder operation by operation, on seeded batches that hold every row kind and on the named edges; the host planner
(hz_ledger_plan_exits) against a plain Python restatement, and its exit-tree part against the builder's own newExit / isOld0_2 / oldKey2;
the HZ_HD routines of csrc/ledger_exit.h built for the host under the address and undefined-behaviour sanitizers; the build's resource
remarks and the exported symbols.
The model tests hold the model against the existing BatchBuilder: they validate the reference the GPU tests use. What the device
computes is guarded by tests/test_ledger_exit.py."""
import ctypes
import os
import subprocess
import sys

import pytest

import ledger_addr_common as A
import ledger_common as C
import ledger_exit_common as X
import ledger_l1_common as L1
from circuits_amd import HzError
from circuits_amd import builder as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hz_ledger_apply_batch_exits", "hz_ledger_exit_outputs_dev", "hz_ledger_exit_tree", "hz_ledger_exit_accounts", "hz_ledger_plan_exits",
               "hz_ledger_exit_ms"]


def _model_vs_builder(st, l1_txs, l2_txs, plan, idxs, n_tx=None):
    """-> the built BatchBuilder, after the model has been compared with it: every leaf field of every row, the fees, the flags, newExit,
    the accounts and the exit leaves afterwards"""
    db, bb = X.builder_batch(st, l1_txs, l2_txs, plan, idxs, 8, n_tx=n_tx)
    inp = bb.get_input()
    pad = [{} for _ in range((n_tx or 0) - len(l1_txs) - len(l2_txs))]
    eff = [dict(t, toIdx=A.brute_force(st, t)) if A.is_to_addr(t) and L1.has_amount(t) else t for t in l2_txs]   # the model is given receivers
    res = X.scheme_model(st.state, l1_txs, eff + pad, plan, idxs)
    assert res[0] == "ok", res
    for name, vals in res[1].items():
        assert vals == inp[name], name
    assert res[2][:-1] == inp["imAccFeeOut"] and res[3] == inp["imFinalAccFee"]
    assert res[4] == L1.builder_flags(bb, len(l1_txs))
    for a, leaf in res[5].items():
        assert leaf == db.leaves[a], a
    assert res[6] == inp["newExit"]
    assert res[7] == bb.exit_leaves
    return bb


def test_scheme_model_matches_the_builder_and_every_row_kind_occurs():
    seen = set()
    for k, st, l1_txs, l2_txs in X.seeded_batches():
        assert 16 <= st.N <= 64 and len(l1_txs) <= 8 and len(l2_txs) <= 10
        bb = _model_vs_builder(st, l1_txs, l2_txs, [1, 2, 0, 0], L1.fee_accounts(st), n_tx=len(l1_txs) + len(l2_txs) + 1)
        seen |= X.kinds_of(bb, l1_txs, l2_txs)
    assert seen == set(X.KINDS), sorted(set(X.KINDS) - seen)


def test_named_edges_match_the_builder():
    sp = X.exit_state(6)
    f0 = sp.first_idx
    edges = X.edge_batches(sp)
    assert set(edges) == set(X.EDGES)
    # newExit, isOld0_2, oldKey2 per row; isAmountNullified of the L1 rows
    expect = {"first_exit_into_empty_tree": ([1], [1], [0], []), "second_key_meets_a_leaf": ([1, 1], [1, 0], [0, f0 + 1], []),
              "keys_sharing_low_bits": ([1, 1], [1, 0], [0, f0 + 1], []), "same_account_twice": ([1, 0, 0], [1, 0, 0], [0, 0, 0], []),
              "zero_amount_exit": ([0, 0], [0, 0], [0, 0], [0]), "exit_whole_balance_with_fee": ([1], [1], [0], []),
              "transfer_in_then_exit_funded_by_it": ([0, 1], [0, 1], [0, 0], []), "exit_then_transfer_same_sender": ([1, 0], [1, 0], [0, 0], []),
              "force_exit_nullified_by_eth_addr": ([1], [1], [0], [1]), "force_exit_nullified_by_token": ([1], [1], [0], [1]),
              "force_exit_nullified_by_underflow": ([1], [1], [0], [1]), "force_exit_then_l2_exit_same_idx": ([1, 0], [1, 0], [0, 0], [0]),
              "nullified_force_exit_then_l2_exit": ([1, 0], [1, 0], [0, 0], [1])}
    for name, (l1_txs, l2_txs) in edges.items():
        bb = _model_vs_builder(sp, l1_txs, l2_txs, [1, 2], [f0 + 40, 0])
        inp = bb.get_input()
        got = (inp["newExit"], inp["isOld0_2"], inp["oldKey2"], [m["isAmountNullified"] for m in bb.tx_meta[:len(l1_txs)]])
        assert got == expect[name], (name, got)
        a = f0 + 1
        if name == "keys_sharing_low_bits":      # the pair hangs at depth 6 below what was a leaf at the root: the old leaf is oldKey2 / oldValue2, no sibling
            assert not any(inp["siblings2"][1]) and inp["oldValue2"][1] == B.hash_state(bb.exit_leaves[a]) and (f0 + 1) ^ (f0 + 33) == 1 << 5
        if name == "same_account_twice":         # the before-leaf is the first exit's and the balance accumulates
            first, second = L1.amount_of(l2_txs[0]), L1.amount_of(l2_txs[2])
            assert inp["balance2"][2] == first and inp["tokenID2"][2] == 1 and inp["ay2"][2] == sp.state(a)["ay"] and inp["nonce2"][2] == 0
            assert bb.exit_leaves[a]["balance"] == first + second
        if name == "zero_amount_exit":           # no exit-tree operation: tokenID2 = token_id for L2, all zero for L1
            assert bb.new_exit_root == 0 and inp["tokenID2"] == [0, 1] and not any(inp["siblings2"][0]) and not any(inp["siblings2"][1])
        if name == "exit_whole_balance_with_fee":
            assert bb.db.leaves[f0 + 6]["balance"] == 0 and bb.exit_leaves[f0 + 6]["balance"] == X.WHOLE
        if name.startswith("force_exit_nullified"):   # an insert with balance 0
            assert bb.exit_leaves[a]["balance"] == 0 and bb.new_exit_root != 0 and all(inp[f + "2"][0] == 0 for f in C.LEAF)
        if name == "nullified_force_exit_then_l2_exit":   # an update from 0
            assert inp["balance2"][1] == 0 and inp["tokenID2"][1] == 1 and bb.exit_leaves[a]["balance"] == L1.amount_of(l2_txs[0])
    # an L2 exit above the balance: the builder raises, the model refuses it at its row with reason 3
    over = [C.tx(f0 + 3, f0 + 4, 5, nonce=0), X.x2(f0 + 1, L1.float_floor(2 * sp.state(f0 + 1)["balance"]), nonce=0)]
    assert X.scheme_model(sp.state, [], over, [1], [0])[:3] == ("refused", 1, 3)
    with pytest.raises(ValueError):
        X.builder_batch(sp, [], over, [1], [0], 8)


def test_reason_5_on_an_exit_leaf_needs_more_than_a_batch_can_hold():
    """An exit leaf starts at 0 in every batch and grows by float40 amounts: below 2^138 each, at most 65536 a call. So its balance stays
    below 2^154, and reason 5 on an exit leaf (a new exit balance of 2^192 or more) cannot be reached through hz_ledger_apply_batch_exits --
    an account cannot 'exit all of' a balance of 2^192 - 1 in one row either, since no float40 is that large. The check stays in the scan,
    and the model and the host program take it at the boundary on values passed in"""
    assert X.MAX_AMOUNT < 1 << 138 and 65536 * X.MAX_AMOUNT < 1 << 154 < 1 << 192
    assert B.float2fix(((1 << 35) - 1) | (31 << 35)) == X.MAX_AMOUNT
    p = {"exit_row": [3, 7], "exit_key": [300, 300], "exit_perm": [0, 1]}
    leaf = {"tokenID": 1, "nonce": 9, "sign": 1, "balance": 5, "ay": 77, "ethAddr": 88}
    assert X.exit_scan(lambda a: leaf, p, [(1 << 192) - 1, 0])[2] is None
    before, after, fail = X.exit_scan(lambda a: leaf, p, [(1 << 192) - 1, 1])
    assert fail == (7, 5) and before[0] is None and before[1]["balance"] == (1 << 192) - 1 and after[0]["nonce"] == 0


def test_host_planner_equals_the_plain_python_one():
    from circuits_amd import lib
    from circuits_amd.capi import lib_path
    if not os.path.exists(lib_path()):
        pytest.skip("the library was not built in this tree")
    hz = lib()
    sp = X.exit_state(6)
    batches = [(st, a, b, k) for k, st, a, b in X.seeded_batches()] + [(sp, a, b, 6) for a, b in X.edge_batches(sp).values()]
    per_row = ("ev_sender", "ev_receiver", "last_event", "ev_exit", "last_exit")
    for st, l1_txs, l2_txs, k in batches:
        plan, idxs = [1, 2, 0], L1.fee_accounts(st)[:3]
        l2 = [dict(t, toIdx=A.brute_force(st, t)) if A.is_to_addr(t) else t for t in l2_txs] + [{}]   # the planner is given receivers
        got = hz.ledger_plan_exits(l1_txs, l2, plan, idxs, k, first_idx=st.first_idx)
        exp = X.plan_model(l1_txs, l2, plan, idxs)
        for name in per_row + ("account", "exit_row", "exit_key", "exit_prev", "exit_perm"):
            assert got[name].tolist() == exp[name], name
        tree = X.tree_plan_model(exp["exit_key"])
        assert got["exit_insert"].tolist() == [t[0] for t in tree] == [int(p < 0) for p in exp["exit_prev"]]
        assert got["exit_is_old0"].tolist() == [t[1] for t in tree] and got["exit_old_key"].tolist() == [t[2] for t in tree]
        # the exit tree's plan is what the builder's own tree reports, row by row
        db, bb = X.builder_batch(st, l1_txs, l2, plan, idxs, 8)
        inp = bb.get_input()
        for x, row in enumerate(exp["exit_row"]):
            assert inp["newExit"][row] == tree[x][0] and inp["isOld0_2"][row] == tree[x][1]
            assert inp["oldKey2"][row] == (tree[x][2] if tree[x][0] and not tree[x][1] else 0)
        # without an exit row the state events are hz_ledger_plan_batch's
        plain_l1, plain_l2 = [t for t in l1_txs if not X.is_exit(t)], [t for t in l2 if not X.is_exit(t)]
        a, b = hz.ledger_plan_exits(plain_l1, plain_l2, plan, idxs, k, first_idx=st.first_idx), hz.ledger_plan_batch(plain_l1, plain_l2, plan, idxs, k, first_idx=st.first_idx)
        assert all(a[name].tolist() == b[name].tolist() for name in ("ev_sender", "ev_receiver", "last_event", "account")) and a["exit_row"].size == 0
        assert a["ev_exit"].tolist() == [-1] * len(a["ev_exit"]) == a["last_exit"].tolist()
    # the leaf pair of f0 + 1 and f0 + 33 hangs at depth 6: n_sib = 6 cannot express it, 7 can. An argument error, from the planner
    f0 = sp.first_idx
    pair = [X.x2(f0 + 1, 5, nonce=0), X.x2(f0 + 33, 5, nonce=0)]
    assert [t[3] for t in X.tree_plan_model([f0 + 1, f0 + 33])] == [0, 6]
    assert hz.ledger_plan_exits([], pair, [1], [0], 6, n_sib=7, first_idx=f0)["exit_old_key"].tolist() == [f0 + 1, f0 + 1]
    with pytest.raises(HzError) as e:
        hz.ledger_plan_exits([], pair, [1], [0], 6, n_sib=6, first_idx=f0)
    assert e.value.status == 1 and "depth >= n_sib = 6" in str(e.value), str(e.value)
    # the existing planners keep refusing an exit
    for call in (lambda: hz.ledger_plan_l2(pair, [1], [0], 6, first_idx=f0), lambda: hz.ledger_plan_batch([], pair, [1], [0], 6, first_idx=f0),
                 lambda: hz.ledger_plan_batch([X.fx(sp, f0 + 1, 5)], [], [1], [0], 6, first_idx=f0)):
        with pytest.raises(HzError) as e:
            call()
        assert e.value.status == 1 and "not supported yet" in str(e.value), str(e.value)


def test_host_build_of_the_exit_routines_agrees_with_the_model(tmp_path):
    """csrc/ledger_exit.h (the exit leaf's e0, the leaf-2 rows, the step on the balance, which operations report an old leaf) as a
    stand-alone host program under -fsanitize=address,undefined: the exit keys of the named edges and the seeded batches with the amounts
    the model gives them, and balances on both sides of 2^192"""
    sp = X.exit_state(6)
    groups = []
    for st, l1_txs, l2_txs in [(sp, a, b) for a, b in X.edge_batches(sp).values()] + [(st, a, b) for _, st, a, b in X.seeded_batches()]:
        p = X.plan_model(l1_txs, l2_txs, [1], [0])
        _, _, eff3s = X.l1_run(st.state, l1_txs, p)
        by_key = {}
        for x, row in enumerate(p["exit_row"]):
            t = (list(l1_txs) + list(l2_txs))[row]
            by_key.setdefault(p["exit_key"][x], []).append(eff3s[row] if row < len(l1_txs) else L1.amount_of(t))
        for key, amounts in by_key.items():
            s = st.state(key)
            groups.append((s["tokenID"] | s["nonce"] << 32 | s["sign"] << 72, amounts))
    assert len(groups) > 20 and any(len(a) > 1 for _, a in groups) and any(0 in a for _, a in groups)
    top = (1 << 192) - 1
    groups += [(0xFFFFFFFF | ((1 << 40) - 1) << 32 | 1 << 72, [top, 0, 1, X.MAX_AMOUNT]), (7 | 5 << 32, [X.MAX_AMOUNT] * 3 + [top - 3 * X.MAX_AMOUNT, 1]),
               (1 << 72, [1 << 192]), (0, [0, 0])]
    text = X.check_lines(groups)
    n = len(text.splitlines())
    assert " 0\n" in text and " 1\n" in text
    src = os.path.join(os.path.dirname(__file__), "native", "ledger_exit_check.cpp")
    exe = str(tmp_path / "ledger_exit_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and "cases=%d mismatches=0" % n in r.stdout, r.stdout + r.stderr
    # the program does judge: one expectation changed is one mismatch
    lines = text.splitlines()
    at = next(i for i, ln in enumerate(lines) if ln.startswith("o "))
    lines[at] = lines[at][:-1] + ("0" if lines[at].endswith("1") else "1")
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 1 and "mismatches=1" in r.stdout, r.stdout + r.stderr


def test_exit_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as RU
    path = os.path.join(RU.BUILD, "ledger.ru.txt")
    if not os.path.exists(path):
        pytest.skip("the library was not built in this tree (no build/ledger.ru.txt)")
    rows = {r["name"]: r for r in RU.table([path])}
    for name in ("hz::k_ledger_exit_scan", "hz::k_ledger_exit_pack", "hz::k_ledger_exit_gather", "hz::k_ledger_l1", "hz::k_ledger_tx"):
        assert name in rows, sorted(rows)
        assert rows[name]["scratch"] == 0, (name, rows[name])
    assert rows["hz::k_ledger_l1"]["lds"] == 55808   # a forceExit needs no slot: DESIGN 8f's layout as it was


def test_new_symbols_are_declared_and_exported():
    from circuits_amd.capi import EXPORTS, LEDGER_EXIT_ARRAYS, lib_path
    assert all(s in EXPORTS for s in NEW_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    assert all(s + "(" in header for s in NEW_SYMBOLS) and "#define HZ_LEDGER_EXIT_ARRAYS 6" in header and "} hz_ledger_exit_out;" in header
    assert LEDGER_EXIT_ARRAYS == X.EXIT_ARRAYS and "L2 exits" not in header.split("OUT OF SCOPE: L1 transactions")[1].split("*/")[0]
    if not os.path.exists(lib_path()):
        pytest.skip("the library was not built in this tree")
    c = ctypes.CDLL(lib_path())
    assert [s for s in NEW_SYMBOLS if not hasattr(c, s)] == []
