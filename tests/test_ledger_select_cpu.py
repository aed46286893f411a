"""A batch selected from a pool (hz_ledger_select_batch) without a device: the Python model of the procedure against the
retry loop over the existing refusal contract (ledger_create_common.model) -- the greedy walk IS what that contract defines --; the host
planner (hz_ledger_plan_select: local slots, the closure step, the argument errors, the caps) against the model; the HZ_HD routines of
csrc/ledger_select.h built for the host under the address and undefined-behaviour sanitizers; the build's resource remarks, the header's
paragraph and the exported symbols. What the device computes is guarded by tests/test_ledger_select.py."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import ledger_common as C
import ledger_l1_common as L1
import ledger_select_common as SC
from circuits_amd import HzError
from circuits_amd import builder as B
from circuits_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hz_ledger_select_batch", "hz_ledger_plan_select", "hz_ledger_select_ms"]


def _lib():
    from circuits_amd import lib
    if not os.path.exists(capi.lib_path()):
        pytest.skip("the library was not built in this tree")
    return lib()


def test_new_symbols_are_declared_and_exported():
    assert all(s in capi.EXPORTS for s in NEW_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    assert all(s + "(" in header for s in NEW_SYMBOLS) and "} hz_ledger_select_out;" in header
    for name, value in (("HZ_SELECT_MAX_POOL", capi.SELECT_MAX_POOL), ("HZ_SELECT_MAX_SLOTS", capi.SELECT_MAX_SLOTS), ("HZ_SELECT_PARTNER", capi.SELECT_PARTNER),
                        ("HZ_SELECT_FULL", capi.SELECT_FULL)):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == value, name
    assert (capi.SELECT_PARTNER, capi.SELECT_FULL) == (SC.PARTNER, SC.FULL) == (14, 15)
    assert ctypes.sizeof(capi.hz_ledger_select_out) == 6 * ctypes.sizeof(ctypes.c_void_p)
    if not os.path.exists(capi.lib_path()):
        pytest.skip("the library was not built in this tree")
    c = ctypes.CDLL(capi.lib_path())
    assert [s for s in NEW_SYMBOLS if not hasattr(c, s)] == []
    hz = _lib()
    assert hz.c.hz_ledger_select_ms.restype == ctypes.c_double and hz.c.hz_ledger_select_ms(None) == 0.0


def test_the_header_states_the_contract():
    header = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    at, scope = header.index(" * SELECT (DESIGN.md 8j)."), header.index(" * OUT OF SCOPE: L1 transactions that create accounts or exit through a call other than")
    assert header.index(" * ATOMIC (DESIGN.md 8i).") < at < scope
    para = header[at:scope]
    for word in NEW_SYMBOLS + ["rq_offset is ignored", "changes nothing resident", "beyond size", "does not touch the exit tree", "invalidates the *_dev",
                               "reasons 1 - 5, 7 - 9, 12, 13 or 16", "reason 6", "HZ_SELECT_PARTNER (14)", "HZ_SELECT_FULL (15)", "(linked transactions + 1)",
                               "one-directional"]:
        assert word in para, word


# ---- the model is the retry loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_the_model_is_the_retry_loop_over_the_refusal_contract(seed):
    """seeded pools without links on 16 accounts, two of them on another token and one about to overflow: the kept set and the reason of
    every drop equal what apply, drop the named row, repeat gives over ledger_create_common.model"""
    base = C.base_state(4)
    f0 = base.first_idx
    acc = SC.accounts(base, {3: {"tokenID": 2}, 9: {"tokenID": 2}, 5: {"balance": SC.LIMIT - 10}, 6: {"nonce": SC.NONCE_MAX}})
    l1_txs = [L1.own(acc, f0 + 1, 0, 0, 10 ** 6), L1.own(acc, f0 + 2, f0 + 4, 10 ** 40, 0)]   # a deposit; a transfer nullified by underflow
    pool = SC.spoilt_pool(acc, 24, seed, share=3)
    res = SC.model(acc, l1_txs, pool)
    kept, reasons, refusals = SC.retry_reference(SC.model_apply(acc), l1_txs, pool)
    assert res["kept"] == kept and res["verdict"] == reasons and res["rounds"] == 1
    assert refusals == len(pool) - len(kept) and (seed or 0 < refusals < len(pool))
    assert SC.retry_reference(SC.model_apply(acc), l1_txs, SC.compact(pool, res))[2] == 0   # what is kept applies as it stands


def test_the_model_names_every_dynamic_reason_and_the_cap():
    base = C.base_state(4)
    f0 = base.first_idx
    acc = SC.accounts(base, {5: {"balance": SC.LIMIT - 10}, 6: {"nonce": SC.NONCE_MAX}, 7: {"tokenID": 2}})
    big = B.float2fix(B.floor_fix2float(acc.state(f0)["balance"]))
    pool = [C.tx(f0, f0 + 5, 10, 0, nonce=0),            # 5: the receiver would reach 2^192
            C.tx(f0 + 6, f0 + 1, 1, 0, nonce=SC.NONCE_MAX),   # 12
            C.tx(f0, f0 + 7, 10, 0, nonce=0),            # 4
            C.tx(f0, f0 + 1, big, 0, nonce=0),           # kept: (nearly) everything f0 holds
            C.tx(f0, f0 + 2, 10 ** 3, 0, nonce=1),       # 3: only because the one before was kept
            C.tx(f0 + 1, f0 + 2, big, 0, nonce=0),       # kept: only because f0 + 1 was funded
            C.tx(f0 + 2, f0 + 3, 1, 0, nonce=0), C.tx(f0 + 3, f0 + 2, 1, 0, nonce=0)]
    assert SC.model(acc, [], pool)["verdict"] == [5, 12, 4, 0, 3, 0, 0, 0]
    res = SC.model(acc, [], pool, max_keep=3)
    assert res["verdict"] == [5, 12, 4, 0, 3, 0, 0, SC.FULL] and res["kept"] == [3, 5, 6]
    assert SC.model(acc, [L1.own(acc, f0 + 5, 0, 0, 10 ** 3)], pool) == ("refused", 0, 5)   # an L1 load past 2^192 refuses, as apply does


# ---- the planner -------------------------------------------------------------------------------------------------------------------------
def _slots_model(l1_txs, pool, aux=None):
    order, ss, sr = [], [], []

    def slot(a):
        if a not in order:
            order.append(a)
        return order.index(a)
    for i, t in enumerate(list(l1_txs) + list(pool)):
        if not t.get("fromIdx", 0):
            ss.append(-1)
            sr.append(-1)
            continue
        ss.append(slot(t["fromIdx"]))
        to = t.get("toIdx", 0) or (aux[i - len(l1_txs)] if aux and i >= len(l1_txs) else 0)
        sr.append(slot(to) if L1.has_amount(t) and to > 1 else -1)
    return {"slot_sender": ss, "slot_receiver": sr, "slot_account": order}


def test_the_planner_numbers_the_slots_by_first_appearance():
    hz = _lib()
    base = C.base_state(4)
    f0 = base.first_idx
    acc = SC.accounts(base)
    l1_txs = [L1.own(acc, f0 + 9, f0 + 2, 5, 7), L1.own(acc, f0 + 2, 1, 3, 0), L1.own(acc, f0 + 9, 0, 0, 1)]
    pool = SC.valid_pool(acc, 20, 3) + [{}, C.tx(f0 + 2, 1, 5, 0, nonce=0), dict(C.tx(f0 + 4, 0, 5, 0, nonce=0), toEthAddr=77), C.tx(f0 + 15, f0 + 15, 0, 0, nonce=0)]
    exp = _slots_model(l1_txs, pool)
    assert hz.ledger_plan_select(l1_txs, pool) == exp and exp["slot_receiver"][-2] == -1 and exp["slot_account"][:2] == [f0 + 9, f0 + 2]
    aux = [0] * len(pool)
    aux[-2] = f0 + 11
    exp = _slots_model(l1_txs, pool, aux)
    assert hz.ledger_plan_select(l1_txs, pool, aux_to_idx=aux) == exp and exp["slot_receiver"][-2] >= 0
    assert hz.ledger_plan_select([], []) == {"slot_sender": [], "slot_receiver": [], "slot_account": []}


def _closure(hz, pool, kept):
    got = hz.ledger_plan_select([], pool, kept=kept)
    exp = SC.closure([bool(t.get("fromIdx", 0)) for t in pool], SC.partners(pool), kept)
    assert (got["forced"], got["rq_offset"]) == exp
    return exp


def test_the_closure_step_over_all_distances():
    hz = _lib()
    base = C.base_state(4)
    acc = SC.accounts(base)
    for d in range(-6, 7):
        if d == 0:
            continue
        pool = SC.valid_pool(acc, 14, 1)
        i = 7
        SC.link(pool, i, i + d)
        forced, off = _closure(hz, pool, [1] * 14)
        assert forced[i] == int(not (1 <= d <= 3 or -4 <= d <= -1)) and off[i] == SC.offset_of(d) and sum(forced) == forced[i]
        # the distance counts kept transactions only: one dropped between the two brings the partner a row nearer
        between = [1] * 14
        between[i + (1 if d > 0 else -1) if abs(d) > 1 else 0] = 0
        forced, off = _closure(hz, pool, between)
        near = d - (1 if d > 1 else -1 if d < -1 else 0)
        assert off[i] == SC.offset_of(near) and forced[i] == int(off[i] == 0)
        gone = [1] * 14
        gone[i + d] = 0
        assert _closure(hz, pool, gone)[0][i] == 1   # the partner is not kept
        gone = [1] * 14
        gone[i] = 0
        assert _closure(hz, pool, gone) == ([0] * 14, [0] * 14)   # the reverse direction is unaffected
    pool = SC.valid_pool(acc, 6, 2)
    pool[2] = {}
    SC.link(pool, 0, 1)
    pool[3].update(partner=2)   # a NOP is never kept
    assert _closure(hz, pool, [1] * 6) == ([0, 0, 0, 1, 0, 0], [1, 0, 0, 0, 0, 0])


def test_chains_and_drops_that_move_a_partner_in_the_model_and_the_planner():
    hz = _lib()
    base = C.base_state(4)
    f0 = base.first_idx
    acc = SC.accounts(base)

    def transfers(n):
        return [C.tx(f0 + i, f0 + i + 1, 1 + i, 0, nonce=0) for i in range(n)]
    # a chain A -> B -> C whose last link is spoilt: one more walk per link
    pool = transfers(4)
    pool[3] = SC.spoil(acc, pool[3], "ahead")
    SC.link(pool, 2, 3)
    SC.link(pool, 1, 2)
    SC.link(pool, 0, 1)
    res = SC.model(acc, [], pool)
    assert res == {"verdict": [14, 14, 14, 2], "kept": [], "rq_offset": [0] * 4, "aux_to_idx": [0] * 4, "rounds": 4}
    assert _closure(hz, pool, [1, 1, 1, 0])[0] == [0, 0, 1, 0] and _closure(hz, pool, [1, 1, 0, 0])[0] == [0, 1, 0, 0]
    # a drop that brings a partner into reach: 0 requires 5, five rows away until 2 is dropped
    pool = transfers(6)
    SC.link(pool, 0, 5)
    assert SC.model(acc, [], pool)["verdict"] == [14, 0, 0, 0, 0, 0]
    pool[2] = SC.spoil(acc, pool[2], "overdraft")
    pool[1] = SC.spoil(acc, pool[1], "stale")
    res = SC.model(acc, [], pool)
    assert res["verdict"] == [0, 2, 3, 0, 0, 0] and res["rq_offset"][0] == 3 and res["rounds"] == 1
    # a drop that pulls one out of reach: 5 requires 1, four rows back -- until 0 is forced out, 5 needs nothing else; then forcing 4
    # out (its partner 0 is gone)... the forced set only grows, and the walk after it starts from the L1 run's balances again
    pool = transfers(6)
    SC.link(pool, 5, 1)
    SC.link(pool, 0, 4)
    res = SC.model(acc, [], pool)
    assert res["verdict"] == [14, 0, 0, 0, 0, 0] and res["rq_offset"][5] == 4 and res["rounds"] == 2
    pool = transfers(8)
    SC.link(pool, 7, 3)                            # four back: in reach
    pool.insert(5, C.tx(f0 + 12, f0 + 13, 1, 0, nonce=0))   # one more kept row between them
    pool[8]["partner"] = 3
    res = SC.model(acc, [], pool)
    assert res["verdict"][8] == 14 and res["rounds"] == 2
    # a forced-out pair frees room the next walk fills
    pool = transfers(5)
    SC.link(pool, 0, 4)
    res = SC.model(acc, [], pool, max_keep=3)
    assert res["verdict"] == [14, 0, 0, 0, SC.FULL] and res["kept"] == [1, 2, 3] and res["rounds"] == 2


def test_argument_errors_and_caps():
    hz = _lib()
    base = C.base_state(4)
    f0 = base.first_idx
    pool = [C.tx(f0 + i, f0 + i + 1, 1, 0, nonce=0) for i in range(4)]
    for bad, text in ((1, "tx 1: partner = 1 is the transaction itself"), (4, "tx 1: partner = 4 is outside the pool (-1 .. 3)"), (-2, "tx 1: partner = -2 is outside the pool")):
        with pytest.raises(HzError) as e:
            hz.ledger_plan_select([], pool, partner=[-1, bad, -1, -1])
        assert e.value.status == 1 and text in str(e.value), str(e.value)
    assert hz.ledger_plan_select([], pool[:1] + [{}] + pool[2:], partner=[-1, 1, -1, -1], kept=[1] * 4)["forced"] == [0] * 4   # a NOP's entry is not read
    with pytest.raises(HzError) as e:
        hz.ledger_plan_select([L1.l1(0, 0, 0, 5)], pool)
    assert e.value.status == 1 and "L1 tx 0: from_idx = 0" in str(e.value)
    with pytest.raises(HzError) as e:
        hz.ledger_plan_select([L1.l1(f0, 0, 0, 5)] * 513, pool)
    assert e.value.status == 1 and "at most 512" in str(e.value)
    with pytest.raises(HzError) as e:
        hz._check(hz.c.hz_ledger_plan_select(0, None, 3, None, None, None, None, None, None, None, None, None, None))
    assert e.value.status == 1 and "null argument" in str(e.value)
    with pytest.raises(SC.Refused):
        SC.model(SC.accounts(base), [], [dict(pool[0], partner=0)])
    with pytest.raises(SC.Refused):
        SC.model(SC.accounts(base), [], [dict(pool[0], partner=1)])
    # the pool cap at its edge: zero-amount transfers of one account, so that only the number of candidates counts
    P, S = capi.SELECT_MAX_POOL, capi.SELECT_MAX_SLOTS
    arr = capi.l2tx_array([C.tx(f0, f0, 0, 0, nonce=i) for i in range(P + 1)])
    head = (capi.hz_l2tx * P).from_buffer(arr)
    assert hz.ledger_plan_select([], head)["slot_account"] == [f0]
    with pytest.raises(HzError) as e:
        hz.ledger_plan_select([], arr)
    assert e.value.status == 1 and "tx %d does not fit" % P in str(e.value) and "HZ_SELECT_MAX_POOL" in str(e.value)
    # the slot cap at its edge: two L1 slots, then pool transaction i brings accounts 2 i + 2 and 2 i + 3
    l1_txs = [L1.l1(f0, f0 + 1, 5, 0)]
    many = [C.tx(f0 + 2 * i + 2, f0 + 2 * i + 3, 1, 0, nonce=0) for i in range(S // 2)]
    got = hz.ledger_plan_select(l1_txs, many[:S // 2 - 1])
    assert len(got["slot_account"]) == S and got["slot_receiver"][-1] == S - 1 and got["slot_account"] == list(range(f0, f0 + S))
    with pytest.raises(HzError) as e:
        hz.ledger_plan_select(l1_txs, many)
    assert e.value.status == 1 and "tx %d does not fit" % (S // 2 - 1) in str(e.value) and "HZ_SELECT_MAX_SLOTS" in str(e.value)
    one_more = many[:S // 2 - 1] + [C.tx(f0 + 5, f0 + S, 1, 0, nonce=1)]   # a receiver alone is the slot too many
    with pytest.raises(HzError) as e:
        hz.ledger_plan_select(l1_txs, one_more)
    assert "tx %d does not fit" % (S // 2 - 1) in str(e.value)
    one_more[-1] = C.tx(f0 + 5, f0 + S, 0, 0, nonce=1)   # without an amount it has no receiver
    assert len(hz.ledger_plan_select(l1_txs, one_more)["slot_account"]) == S


# ---- the routines on the host ------------------------------------------------------------------------------------------------------------
def test_host_build_of_the_select_routines_agrees_with_the_model(tmp_path):
    """csrc/ledger_select.h as a stand-alone host program under -fsanitize=address,undefined: select_step at debit == balance and +- 1,
    select_credit at a receiver balance of 2^192 - 1 +- 1, select_want at 0 / 65535 / 65536 and at nonce 2^40 - 1, select_offset and
    select_link over every distance, select_static's precedence"""
    text = SC.check_lines()
    n = len(text.splitlines())
    src = os.path.join(os.path.dirname(__file__), "native", "ledger_select_check.cpp")
    exe = str(tmp_path / "ledger_select_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and "cases=%d mismatches=0" % n in r.stdout, r.stdout + r.stderr
    lines = text.splitlines()   # the program does judge: one expectation changed is one mismatch
    at = next(i for i, ln in enumerate(lines) if ln.startswith("o 4 "))
    lines[at] = "o 4 4"
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 1 and "mismatches=1" in r.stdout, r.stdout + r.stderr


def test_the_select_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as RU
    path = os.path.join(RU.BUILD, "ledger.ru.txt")
    if not os.path.exists(path):
        pytest.skip("the library was not built in this tree (no build/ledger.ru.txt)")
    rows = {r["name"]: r for r in RU.table([path])}
    for name in ("hz::k_ledger_select", "hz::k_ledger_select_rq"):
        assert name in rows, sorted(rows)
        assert rows[name]["scratch"] == 0, (name, rows[name])
    assert 0 < rows["hz::k_ledger_select"]["lds"] <= 163840, rows["hz::k_ledger_select"]
