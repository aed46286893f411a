"""hz_ledger without a device: the host planner (hz_ledger_plan_l2) against a plain Python restatement, a Python model of the whole scheme
the kernels implement against BatchBuilder field by field, and the build's resource remarks of the ledger kernels."""
import os
import sys

import numpy as np
import pytest

import ledger_common as C
from circuits_amd import HzError, lib
from circuits_amd import builder as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 6


def _check_plan(txs, plan, idxs, k=K):
    got = lib().ledger_plan_l2(txs, plan, idxs, k)
    exp = C.plan_model(txs, plan, idxs)
    for name in ("ev_sender", "ev_receiver", "fee_slot", "last_event", "account", "prev_same"):
        assert got[name].tolist() == exp[name], name
    return got


@pytest.mark.parametrize("m", [1, 2, 65, 300])
def test_plan_matches_the_restatement_on_drawn_batches(m):
    base = C.base_state(K)
    txs = C.draw_batch(base, m, seed=7 + m, pool=24, n_tx=m + 3)
    got = _check_plan(txs, [1, 0, 0, 0], [base.first_idx + 5, 0, base.first_idx + 6, 0])
    assert got["account"].size == sum(1 + bool(t["amountF"] & ((1 << 35) - 1)) for t in txs if t) + 2


def test_plan_edge_batches():
    f0 = C.base_state(K).first_idx
    got = _check_plan([{}, {}, {}], [1], [0])
    assert got["account"].size == 0 and got["last_event"].tolist() == [-1, -1, -1]
    got = _check_plan([C.tx(f0 + 3, f0 + 3, 10)], [1], [f0 + 3])   # self-transfer, and the fee goes to the same account
    assert got["prev_same"].tolist() == [-1, 0, 1]
    got = _check_plan([C.tx(f0 + 3, f0 + 4, 0), C.tx(f0 + 4, f0 + 3, 7)], [1], [0])   # zero amount: no receiver event
    assert got["ev_receiver"].tolist() == [-1, 2]
    hot = [C.tx(f0 + 1 + i, f0, 5) for i in range(40)]
    got = _check_plan(hot, [1], [0])
    assert got["prev_same"][1::2].tolist() == [-1] + list(range(1, 78, 2))
    # plan tokens with zero padding: token 0 takes the first padding slot, as plan.index does; a token outside the plan takes none
    got = _check_plan([C.tx(f0, f0 + 1, 5, token=0), C.tx(f0, f0 + 1, 5, token=9), C.tx(f0, f0 + 1, 5, token=1)], [7, 1, 0, 0], [0, 0, 0, 0])
    assert got["fee_slot"].tolist() == [2, -1, 1]


def test_plan_argument_errors():
    f0 = 256
    for txs, plan, idxs, text in (([C.tx(f0, 0, 5)], [1], [0], "not supported yet"), ([C.tx(f0, 1, 5)], [1], [0], "not supported yet"),
                                   ([C.tx(f0 + 64, f0, 5)], [1], [0], "outside the state"), ([C.tx(f0, f0 + 64, 5)], [1], [0], "outside the state"),
                                   ([C.tx(f0, f0 + 1, 5)], [1], [f0 - 1], "outside the state"), ([C.tx(f0, f0 + 1, 5)], [1] * 65, [0] * 65, "fee slots")):
        with pytest.raises(HzError) as e:
            lib().ledger_plan_l2(txs, plan, idxs, K)
        assert e.value.status == 1 and text in str(e.value), str(e.value)


def _model_vs_builder(base, txs, plan, idxs):
    _, bb = C.builder_batch(base, txs, plan, idxs, 8)
    inp = bb.get_input()
    res = C.scheme_model(base.state, txs, plan, idxs)
    assert res[0] == "ok", res
    for name, vals in res[1].items():
        assert vals == inp[name], name
    assert res[2][:-1] == inp["imAccFeeOut"] and res[3] == inp["imFinalAccFee"]


def test_scheme_model_matches_the_builder_field_by_field():
    """pins the scheme the kernels implement: balances and nonces as prefix sums over each ACCOUNT's events, not transaction by transaction"""
    base = C.base_state(4)
    f0 = base.first_idx
    _model_vs_builder(base, C.draw_batch(base, 40, seed=11, pool=5, n_tx=44), [1, 0], [f0 + 2, 0])
    _model_vs_builder(base, C.draw_batch(base, 12, seed=12, pool=3), [0, 1, 1], [0, f0 + 1, f0 + 1])
    # a self-transfer; a transfer that empties the sender exactly, which then receives and spends again; the fee goes to the same account
    _model_vs_builder(base, [C.tx(f0 + 3, f0 + 3, 1000, 176, nonce=0), C.tx(f0 + 5, f0 + 4, base.state(f0 + 5)["balance"], 0, nonce=0),
                             C.tx(f0 + 4, f0 + 5, 500, 100, nonce=0), C.tx(f0 + 5, f0 + 4, 200, 192, nonce=1)], [1], [f0 + 5])


def test_scheme_model_lowest_failure_rule():
    base = C.base_state(4)
    f0 = base.first_idx
    big = B.float2fix(B.floor_fix2float(base.state(f0)["balance"] * 2))
    ok = C.tx(f0 + 1, f0 + 2, 10, nonce=0)
    cases = {1: C.tx(f0, f0 + 2, 10, token=2, nonce=5), 2: C.tx(f0, f0 + 2, big, nonce=1), 3: C.tx(f0, f0 + 2, big, nonce=0)}
    for reason, bad in cases.items():   # a transaction with several offences reports the lowest code; a later offence never wins
        assert C.scheme_model(base.state, [ok, bad, C.tx(f0 + 5, f0 + 2, 10, nonce=3)], [1], [0]) == ("refused", 1, reason)
    # the fee slot's token is reported after every transaction, with index m + j
    assert C.scheme_model(base.state, [ok], [1, 2], [0, f0 + 3]) == ("refused", 2, 6)
    # the builder raises for the reasons it checks
    for reason in (1, 3):
        with pytest.raises(ValueError):
            C.builder_batch(base, [ok, cases[reason]], [1], [0], 8)


def test_ledger_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as RU
    path = os.path.join(RU.BUILD, "ledger.ru.txt")
    if not os.path.exists(path):
        pytest.skip("the library was not built in this tree (no build/ledger.ru.txt)")
    rows = {r["name"]: r for r in RU.table([path])}
    names = [n for n in rows if n.startswith("hz::k_ledger_")]
    assert len(names) >= 7, sorted(rows)
    assert {n: rows[n]["scratch"] for n in names if rows[n]["scratch"]} == {}
