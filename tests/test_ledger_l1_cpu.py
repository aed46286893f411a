"""L1 transactions on the device-resident ledger (hz_ledger_apply_batch) without a device: the scheme model against
BatchBuilder field by field on batches that, by the builder alone, hold every nullifier cause and the underflow chain; the host planner
against the model's events and slots; the HZ_HD routines of csrc/ledger_l1.h built for the host under the address and
undefined-behaviour sanitizers against that model; the build's resource remarks and the exported symbols.
The first two tests hold the model against the existing BatchBuilder: they validate the reference the other tests use and pass without
the library's L1 code. What the device computes is guarded by tests/test_ledger_l1.py, and the shared HZ_HD routines by the host program
here."""
import ctypes
import os
import subprocess
import sys

import pytest

import ledger_addr_common as A
import ledger_common as C
import ledger_l1_common as L1
from circuits_amd import builder as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hz_ledger_apply_batch", "hz_ledger_plan_batch", "hz_ledger_l1_flags_dev", "hz_ledger_l1_ms"]


def _model_vs_builder(st, l1_txs, l2_txs, plan, idxs, n_tx=None):
    """-> the built BatchBuilder, after the model has been compared with it field by field"""
    db, bb = L1.builder_batch(st, l1_txs, l2_txs, plan, idxs, 8, n_tx=n_tx)
    inp = bb.get_input()
    pad = [{} for _ in range((n_tx or 0) - len(l1_txs) - len(l2_txs))]
    res = L1.scheme_model(st.state, l1_txs, list(l2_txs) + pad, plan, idxs)
    assert res[0] == "ok", res
    for name, vals in res[1].items():
        assert vals == inp[name], name
    assert res[2][:-1] == inp["imAccFeeOut"] and res[3] == inp["imFinalAccFee"]
    assert res[4] == L1.builder_flags(bb, len(l1_txs))
    assert [(f >> 1) & 1 for f in res[4]] == [m["isAmountNullified"] for m in bb.tx_meta[:len(l1_txs)]]
    for a, leaf in res[5].items():
        assert leaf == db.leaves[a], a
    return bb


def test_scheme_model_matches_the_builder_and_every_cause_occurs():
    seen = set()
    for k, st, l1_txs, l2_txs in L1.seeded_batches():
        assert 16 <= st.N <= 64 and len(l1_txs) <= 8 and len(l2_txs) <= 8
        bb = _model_vs_builder(st, l1_txs, l2_txs, [1, 2, 0, 0], L1.fee_accounts(st), n_tx=len(l1_txs) + len(l2_txs) + 1)
        seen |= L1.builder_causes(bb, len(l1_txs))
    assert seen == set(L1.CAUSES), sorted(set(L1.CAUSES) - seen)


def test_named_edges_match_the_builder():
    sp = A.special_state(6)
    f0 = sp.first_idx
    expect = {   # isAmountNullified of the L1 run, then nullifyLoadAmount
        "underflow_chain": ([1, 1, 0], [0, 0, 0]), "deposit_transfer_spends_its_load": ([0], [0]), "load_nullified_then_underflow": ([0, 1], [1, 0]),
        "self_transfer": ([0, 1], [0, 0]), "from_eth_addr_mismatch": ([1, 0], [0, 0]), "receiver_token_mismatch": ([1], [0]),
        "zero_amount_deposit": ([0, 0], [0, 0]), "one_account_pair": ([0, 0, 1, 0, 1, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0, 0]),
        "l2_funded_by_l1_deposit": ([0], [0])}
    edges = L1.edge_batches(sp)
    assert set(edges) == set(expect)
    for name, (l1_txs, l2_txs) in edges.items():
        bb = _model_vs_builder(sp, l1_txs, l2_txs, [1, 2], [f0 + 40, 0])
        flags = L1.builder_flags(bb, len(l1_txs))
        assert ([(f >> 1) & 1 for f in flags], [f & 1 for f in flags]) == expect[name], name
        inp = bb.get_input()
        if name == "receiver_token_mismatch":   # the receiver row is there, with the balance it keeps
            assert inp["tokenID2"][0] == 2 and inp["balance2"][0] == sp.state(f0 + 9)["balance"] and any(inp["siblings2"][0])
        if name == "zero_amount_deposit":
            assert all(inp[f + "2"][i] == 0 for f in C.LEAF for i in (0, 1)) and not any(inp["siblings2"][0])
        if name == "underflow_chain":
            assert "chain" in L1.builder_causes(bb, 3)
    # an L2 transfer that counted on a nullified L1 transfer: the builder raises, the model refuses it at its own row with reason 3
    l1_txs, l2_txs = L1.refused_after_nullified(sp)
    assert L1.scheme_model(sp.state, l1_txs, l2_txs, [1], [0])[:3] == ("refused", 2, 3)
    with pytest.raises(ValueError):
        L1.builder_batch(sp, l1_txs, l2_txs, [1], [0], 8)
    # reason 5 through loadAmount, at the L1 row that brings a balance to 2^192 (a float40 is below 2^138: it takes a balance that is nearly there)
    rs = L1.rich_state(6)
    res = L1.scheme_model(rs.state, [L1.own(rs, f0 + 3, f0 + 1, 10), L1.own(rs, f0 + 1, 0, 0, load=5000)], [], [1], [0])
    assert res[:3] == ("refused", 1, 5)
    assert L1.scheme_model(rs.state, [L1.own(rs, f0 + 1, f0 + 3, 5000, load=5000)], [], [1], [0])[0] == "ok"


def test_host_planner_equals_the_models_events_and_slots():
    from circuits_amd import lib
    from circuits_amd.capi import lib_path
    if not os.path.exists(lib_path()):
        pytest.skip("the library was not built in this tree")
    hz = lib()
    sp = A.special_state(6)
    batches = [(st, a, b, k) for k, st, a, b in L1.seeded_batches()] + [(sp, a, b, 6) for a, b in L1.edge_batches(sp).values()]
    for st, l1_txs, l2_txs, k in batches:
        plan, idxs = [1, 2, 0], [st.first_idx + 2, 0, st.first_idx + 3]
        got = hz.ledger_plan_batch(l1_txs, l2_txs + [{}], plan, idxs, k, first_idx=st.first_idx)
        exp = L1.plan_model(l1_txs, l2_txs + [{}], plan, idxs)
        for name in ("ev_sender", "ev_receiver", "fee_slot", "last_event", "account", "prev_same", "l1_slot_sender", "l1_slot_receiver", "slot_account"):
            assert got[name].tolist() == exp[name], name
    # without an L1 run it is hz_ledger_plan_l2
    _, st, _, l2_txs = L1.seeded_batches()[0]
    a, b = hz.ledger_plan_batch([], l2_txs, [1], [0], 4, first_idx=st.first_idx), hz.ledger_plan_l2(l2_txs, [1], [0], 4, first_idx=st.first_idx)
    assert all(a[name].tolist() == b[name].tolist() for name in b) and a["slot_account"].size == 0


def test_host_build_of_the_l1_routines_agrees_with_the_model(tmp_path):
    """csrc/ledger_l1.h (float40, static nullifiers, the step of the recurrence, the sender's delta) as a stand-alone host program under
    -fsanitize=address,undefined, on the named edges, the seeded batches and amounts at the ends of the float40 range"""
    sp = A.special_state(6)
    f0 = sp.first_idx
    cases = [(sp.state, l1_txs) for l1_txs, _ in L1.edge_batches(sp).values()] + [(st.state, l1_txs) for _, st, l1_txs, _ in L1.seeded_batches()]
    top = ((1 << 35) - 1) | (31 << 35)
    ends = [dict(L1.own(sp, f0 + 1, f0 + 3), amountF=1, loadAmountF=top), dict(L1.own(sp, f0 + 1, f0 + 3), amountF=top, loadAmountF=1 | (31 << 35)),
            dict(L1.own(sp, f0 + 3, f0 + 1), amountF=top), dict(L1.own(sp, f0 + 1, f0 + 1), amountF=31 << 35, loadAmountF=31 << 35),
            dict(L1.own(sp, f0 + 5, f0 + 3), amountF=7)]    # f0 + 5 holds the "any" address: 160 set bits
    assert sp.state(f0 + 5)["ethAddr"] == A.ANY
    cases.append((sp.state, ends))
    text = L1.check_lines(cases)
    n = sum(1 for ln in text.splitlines() if ln[0] in "te")
    src = os.path.join(os.path.dirname(__file__), "native", "ledger_l1_check.cpp")
    exe = str(tmp_path / "ledger_l1_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and "cases=%d mismatches=0" % n in r.stdout, r.stdout + r.stderr
    # the program does judge: one expectation changed is one mismatch
    lines = text.splitlines()
    at = next(i for i, ln in enumerate(lines) if ln.startswith("e "))
    lines[at] += "1"
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 1 and "mismatches=1" in r.stdout, r.stdout + r.stderr


def test_l1_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as RU
    path = os.path.join(RU.BUILD, "ledger.ru.txt")
    sig = os.path.join(RU.BUILD, "ledger_sig.ru.txt")
    if not os.path.exists(path) or not os.path.exists(sig):
        pytest.skip("the library was not built in this tree (no build/ledger.ru.txt)")
    rows = {r["name"]: r for r in RU.table([path, sig])}
    for name in ("hz::k_ledger_l1", "hz::k_ledger_tx", "hz::k_ledger_scan", "hz::k_ledger_pack", "hz::k_ledger_sig_msg", "hz::k_ledger_sig_verify"):
        assert name in rows, sorted(rows)
        assert rows[name]["scratch"] == 0, (name, rows[name])
    assert "lds" in rows["hz::k_ledger_l1"], rows["hz::k_ledger_l1"]
    assert rows["hz::k_ledger_l1"]["lds"] == 55808   # DESIGN 8f's layout, below the 65536 a workgroup may have


def test_new_symbols_are_declared_and_exported():
    from circuits_amd.capi import EXPORTS, LEDGER_MAX_L1, hz_l1tx, lib_path
    assert all(s in EXPORTS for s in NEW_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    assert all(s + "(" in header for s in NEW_SYMBOLS) and "#define HZ_LEDGER_MAX_L1 512" in header and "} hz_l1tx;" in header
    assert LEDGER_MAX_L1 == 512 and ctypes.sizeof(hz_l1tx) == 72
    assert "L1 transactions that create accounts or exit" in header
    if not os.path.exists(lib_path()):
        pytest.skip("the library was not built in this tree")
    c = ctypes.CDLL(lib_path())
    assert [s for s in NEW_SYMBOLS if not hasattr(c, s)] == []
