"""ComputeFee's bound of 128 bits without a device (tests/fee_bound_common.py): the plain-integer model against the oracle's ComputeFee
main on both boundary tables -- same accept / reject, same constraint, same feeOut --, the counts the tables promise, the ledger's
scheme models with refusal reason 16 against the retry loop, and the host build of ledger_fee_overflows over the whole float40 table."""
import os
import re
import subprocess

import pytest

import fee_bound_common as FB
import ledger_common as C
import ledger_l1_common as L1
import ledger_range_common as R
import ledger_select_common as SC
from circuits_amd import builder as B
from circuits_amd import capi
from oracle_binding import OracleCtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_tables_hold_what_they_promise():
    table = FB.float40_table()
    assert [s for s, _, _ in table] == list(range(256))
    reach = FB.reaching()
    assert [s for s, _, _ in reach] == list(range(FB.FIRST_REACHING, 256)) and len(reach) == 225
    for sel, below, above in reach:   # the builder's formula is the second opinion on the model's search
        lo, hi = B.compute_fee(B.float2fix(below), sel), B.compute_fee(B.float2fix(above), sel)
        assert lo.bit_length() == 128 and hi.bit_length() == 129, (sel, hex(below), hex(above))
        assert FB.verdict(B.float2fix(below), sel) == (FB.ACCEPTED, lo), (sel, hex(below))
        assert FB.verdict(B.float2fix(above), sel)[0] == (FB.OVF_SHIFTED if sel < 192 else FB.OVF_NOTSHIFTED), (sel, hex(above))
        assert B.float2fix(below) < B.float2fix(above)
        # nothing lies between the two: every exponent's neighbours of the pair are on the pair's sides
        for expo in range(32):
            m = FB._search(sel, expo)
            assert m == 0 or B.float2fix(FB.f40(m, expo)) <= B.float2fix(below)
            assert m == FB.MANT or B.float2fix(FB.f40(m + 1, expo)) >= B.float2fix(above)
    for sel, below, above in table[:FB.FIRST_REACHING]:
        assert above is None and below == FB.f40(FB.MANT, 31) and FB.verdict(B.float2fix(below), sel)[0] == FB.ACCEPTED
    exact = FB.exact_table()
    assert {s for s, _, _ in exact} == set(range(1, 256)) and len(exact) == 2 * 255 + 2 * len(FB.PAIR_253)
    assert (192, 1 << 128, FB.OVF_NOTSHIFTED) in exact and (192, (1 << 128) - 1, FB.ACCEPTED) in exact
    for sel, amount, name in exact:
        assert FB.verdict(amount, sel)[0] == name, (sel, amount)
        assert FB.verdict(amount, sel, 0) == (FB.ACCEPTED, 0)
    assert sum(name == FB.BITS for _, _, name in exact) == len(FB.PAIR_253) and any(FB.shifted(s) for s in FB.PAIR_253) and not all(FB.shifted(s) for s in FB.PAIR_253)


def test_the_launch_mixes_every_wavefront():
    cases = FB.compute_fee_cases()
    assert 1200 <= len(cases) <= 1600
    for w in range(0, len(cases), 64):
        wave = cases[w:w + 64]
        names = {v[0] for _, v in wave}
        assert FB.ACCEPTED in names and len(names) >= 3, w
        assert {FB.shifted(c["feeSel"]) for c, _ in wave} == {True, False}, w
    sels = {c["feeSel"] for c, v in cases if v[0] != FB.ACCEPTED}
    assert sels == set(range(1, 256))
    assert sum(c["applyFee"] == 0 for c, _ in cases) >= 225 and all(v == (FB.ACCEPTED, 0) for c, v in cases if c["applyFee"] == 0)


def test_the_model_against_the_oracle():
    cases = FB.compute_fee_cases()
    ids = FB.constraint_ids()
    o = OracleCtx("compute-fee", n_instances=len(cases))
    for k, (c, _) in enumerate(cases):
        o.set_inputs(c, instance=k)
    first = o.run()
    rejected = [k for k, (_, v) in enumerate(cases) if v[0] != FB.ACCEPTED]
    assert first is not None and first[0] == rejected[0]
    for k, (c, (name, fee)) in enumerate(cases):
        f = o.failure_of(k)
        if name == FB.ACCEPTED:
            assert f is None, (c, f)
            assert o.get("main.feeOut", instance=k) == fee, c
        else:
            assert f is not None and f[1] == ids[name], (c, name, f)


def test_all_selectors_is_narrowed_to_the_bound():
    rows = R.all_selectors_rows()
    assert [i for i, _, _ in rows] == list(range(256))
    moved = [(i, f, over) for i, f, over in rows if over is not None]
    assert len(moved) == 32
    fee = lambda f, i: B.compute_fee(B.float2fix(f), i)   # noqa: E731
    assert all(fee(f, i) < 1 << 128 for i, f, _ in rows)
    assert sorted({fee(over, i).bit_length() for i, _, over in moved})[0] == 129 and max(fee(over, i).bit_length() for i, _, over in moved) > 180
    for i, f, over in moved:
        assert f >> 35 == over >> 35 and (f & R.MANT) < (over & R.MANT)
        assert (f & R.MANT) == R.MANT or fee(f + 1, i) >> 128, i   # the largest mantissa of the exponent below the bound
    per_exponent = [sum((over or f) >> 35 == e for _, f, over in rows) for e in range(32)]
    assert [sum(f >> 35 == e for _, f, _ in rows) for e in range(32)] == per_exponent and min(per_exponent) >= 6 and per_exponent[31] == 8
    assert max(B.float2fix(f) for _, f, _ in rows) >> 128                                    # limb 4 of the amount
    assert sum(fee(f, i).bit_length() == 128 for i, f, _ in rows) >= 8                       # fees of 128 bits


def _over(st, sel, l1_rows=0):
    f0 = st.first_idx
    return R.txf(f0 + 1, f0 + 48, FB.float40_table()[sel][2], sel, nonce=0)


def test_the_scheme_models_refuse_with_reason_16():
    st = R.wide_state()
    f0 = st.first_idx
    plan, idxs = [1], [f0 + R.WIDE_FEE]
    ok = R.txf(f0 + 8, f0 + 9, R.f40(5, 0), 176, nonce=0)
    for sel, below, above in FB.reaching():
        under = R.txf(f0 + 1, f0 + 48, below, sel, nonce=0)
        assert C.scheme_model(st.state, [ok, under], plan, idxs)[0] == "ok", sel
        assert C.scheme_model(st.state, [ok, dict(under, amountF=above)], plan, idxs) == ("refused", 1, FB.REASON), sel
    over = _over(st, 200)
    poor = dict(over, fromIdx=f0 + 41)                                   # reason 3 at the same row is lower
    assert C.scheme_model(st.state, [ok, poor], plan, idxs) == ("refused", 1, 3)
    assert C.scheme_model(st.state, [over, dict(poor, toIdx=f0 + 49)], plan, idxs) == ("refused", 0, FB.REASON)
    assert C.scheme_model(st.state, [{}, dict(over, fromIdx=0)], plan, idxs)[0] == "ok"   # a NOP is not charged
    l1 = [dict(L1.own(st, f0 + 1, f0 + 47), amountF=over["amountF"], userFee=200)]   # nor is an L1 transfer
    assert L1.scheme_model(st.state, l1, [ok], plan, idxs)[0] == "ok"
    assert L1.scheme_model(st.state, l1, [ok, over], plan, idxs)[:3] == ("refused", 2, FB.REASON)
    import ledger_exit_common as X
    assert X.scheme_model(st.state, l1, [ok, dict(over, toIdx=1)], plan, idxs)[:3] == ("refused", 2, FB.REASON)   # an exit is charged


@pytest.mark.parametrize("seed", range(3))
def test_the_select_model_drops_what_the_retry_loop_drops(seed):
    """test_ledger_select_cpu's pools with overflowing fees put in: the kept set and every reason equal what apply, drop the named row,
    repeat gives over the scheme model that now knows reason 16"""
    base = C.base_state(4)
    f0 = base.first_idx
    acc = SC.accounts(base, {3: {"tokenID": 2}, 9: {"tokenID": 2}, 5: {"balance": SC.LIMIT - 10}, **{j: {"balance": 1 << 186} for j in (0, 1, 2, 4, 6, 7, 8, 10, 11, 12, 13, 14, 15)}})
    pool = SC.spoilt_pool(acc, 24, seed, share=3)
    table = FB.float40_table()
    for at, sel in ((0, 31), (5, 191), (11, 192), (17, 255), (23, 224)):
        pool[at] = dict(pool[at], amountF=table[sel][2], userFee=sel)
    pool[8] = dict(pool[8], amountF=table[100][1], userFee=100)   # just below: judged like any other row
    res = SC.model(acc, [], pool)
    kept, reasons, refusals = SC.retry_reference(SC.model_apply(acc), [], pool)
    assert res["kept"] == kept and res["verdict"] == reasons
    assert FB.REASON in reasons and not set(kept) & {0, 5, 11, 17, 23}
    assert all(reasons[i] and reasons[i] <= FB.REASON for i in (0, 5, 11, 17, 23))
    assert SC.retry_reference(SC.model_apply(acc), [], SC.compact(pool, res))[2] == 0


def test_the_header_names_the_reason():
    header = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    assert int(re.search(r"#define HZ_LEDGER_FEE_OVERFLOW (\d+)", header).group(1)) == capi.LEDGER_FEE_OVERFLOW == SC.FEE_OVERFLOW == FB.REASON == 16
    assert "amount x fee factor does not fit 128 bits (src/compute-fee.circom:89-91)" in header
    assert FB.REASON > capi.SELECT_FULL
    for name in ("DESIGN.md", "NOTES.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "reason 16" in text or "16 " in text, name
        assert "NOT fixed" not in text or "fee" not in text[text.index("NOT fixed") - 400:text.index("NOT fixed") + 400], name


def test_host_build_of_the_overflow_routine_over_the_float40_table(tmp_path):
    """tests/native/ledger_select_check.cpp takes ledger_fee and ledger_fee_overflows over every row of the float40 table (the u256 check
    does in tests/test_ledger_ranges_cpu.py); one flipped expectation is one mismatch"""
    text = SC.fee_lines()
    lines = text.splitlines()
    assert len(lines) == 256 + 225 and sum(ln.endswith(" 1") for ln in lines) == 225
    src = os.path.join(os.path.dirname(__file__), "native", "ledger_select_check.cpp")
    exe = str(tmp_path / "ledger_select_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and "cases=%d mismatches=0" % len(lines) in r.stdout, r.stdout + r.stderr[-2000:]
    at = next(i for i, ln in enumerate(lines) if ln.endswith(" 0") and int(ln.split()[2], 16) >= 31)
    lines[at] = lines[at][:-1] + "1"
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 1 and "mismatches=1" in r.stdout, r.stdout + r.stderr[-2000:]
