"""The ledger at the edges of its value ranges without a device (tests/ledger_range_common.py): the scheme models against BatchBuilder
field by field on every batch meant to be valid -- which proves the fixtures valid, no batch may be skipped or caught --, every expected
refusal by its lowest index and reason, the distribution the fixtures promise (all 32 exponents, fees up to the circuit's bound of 128 bits, both signs beside
a full nonce byte, all 64 slots), and the 256-bit routines of csrc/u256.h, ledger_fee.h and l1_float40 built for the host under the
address and undefined-behaviour sanitizers against Python integers."""
import os
import subprocess

import ledger_addr_common as A
import ledger_common as C
import ledger_l1_common as L1
import ledger_range_common as R
from circuits_amd import builder as B

N_LEVELS = 16


def _model_vs_builder(st, txs, plan, idxs, by_addr=False):
    """-> (the built BatchBuilder, the model's result), after the model has been compared with the builder field by field"""
    if by_addr:
        _, bb = A.builder_batch(st, txs, plan, idxs, N_LEVELS)
        res = A.scheme_model(st, txs, plan, idxs)
    else:
        _, bb = C.builder_batch(st, txs, plan, idxs, N_LEVELS)
        res = C.scheme_model(st.state, txs, plan, idxs)
    inp = bb.get_input()
    assert res[0] == "ok", res
    zero_rows = A.zero_amount_rows(txs) if by_addr else {}
    for name, vals in res[1].items():
        for i, (v, e) in enumerate(zip(vals, inp[name])):
            assert v == e or name in zero_rows.get(i, {}), (name, i)
    assert res[2][:-1] == inp["imAccFeeOut"] and res[3] == inp["imFinalAccFee"]
    return bb, res


def _refused(st, batch, index, reason):
    txs, plan, idxs = batch
    assert C.scheme_model(st.state, txs, plan, idxs) == ("refused", index, reason), (index, reason)


def test_wide_state_holds_what_it_promises():
    st = R.wide_state()
    f0, leaf = st.first_idx, st.state
    assert [leaf(f0 + j)["balance"] for j in (1, 2, 3, 4, 5)] == [1 << 191] * 4 + [(1 << 192) - 8]
    assert sorted(leaf(a)["nonce"] for a in st.role.values()) == [(1 << 32) - 2, (1 << 40) - 3, (1 << 40) - 1, (1 << 40) - 1]
    assert {leaf(a)["sign"] for a in st.role.values()} == {0, 1}
    assert {leaf(st.role[n])["sign"] for n in ("last0", "last1")} == {0, 1}
    assert [leaf(f0 + j)["tokenID"] for j in (31, 32, 33, 34)] == [R.TOK_MAX, R.TOK_MAX, R.TOK_B31, R.TOK_B31]
    for j in range(st.N):   # every leaf is a leaf, and the builder's leaf_fields round-trips the planes
        assert B.leaf_fields(leaf(f0 + j)) == [C.to_int(c[j]) for c in st.cols]


def test_all_selectors_against_the_builder():
    st = R.wide_state()
    txs, plan, idxs = R.all_selectors(st)
    assert [t["userFee"] for t in txs] == list(range(256))
    assert {t["amountF"] >> 35 for t in txs} == set(range(32))
    assert {t["amountF"] & R.MANT for t in txs} >= set(R.MANTISSAS)
    fees = [B.compute_fee(B.float2fix(t["amountF"]), t["userFee"]) for t in txs]
    # the circuit takes no fee of 2^128 or more and neither does the ledger (reason 16): the fixture goes up to the bound, in 16 rows or more
    assert max(fees).bit_length() == 128 and sum(f.bit_length() == 128 for f in fees) >= 16 and max(B.float2fix(t["amountF"]) for t in txs) >> 128
    bb, res = _model_vs_builder(st, txs, plan, idxs)
    assert res[3] == [sum(fees)] and sum(fees).bit_length() > 131   # the accumulated fee does carry into limb 4


def test_nonce_carry_and_the_brim_against_the_builder():
    st = R.wide_state()
    f0 = st.first_idx
    txs, plan, idxs = R.nonce_carry(st)
    assert len(txs) == 6
    bb, res = _model_vs_builder(st, txs, plan, idxs)
    db, _ = C.builder_batch(st, txs, plan, idxs, N_LEVELS)
    assert db.leaves[st.role["n40m3"]]["nonce"] == R.NONCE_MAX and db.leaves[st.role["n32"]]["nonce"] == (1 << 32) + 1
    inp = bb.get_input()
    assert inp["nonce1"][:5] == [(1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 40) - 3, (1 << 40) - 2] and inp["tokenID3"][:2] == [1, R.TOK_MAX]
    valid, refused = R.to_the_brim(st)
    bb, res = _model_vs_builder(st, *valid)
    inp = bb.get_input()
    assert inp["balance2"][0] == (1 << 192) - 8 and inp["balance1"][1] == R.EXACT and B.float2fix(R.EXACT_F) >> 128
    for batch, index, reason in refused:
        _refused(st, batch, index, reason)
    assert [r for _, _, r in refused] == [5, 3]
    db, _ = C.builder_batch(st, *valid, N_LEVELS)
    assert db.leaves[f0 + 5]["balance"] == (1 << 192) - 1 and db.leaves[f0 + 6]["balance"] == 0


def test_reason_12_in_the_model():
    """the sender's nonce is 2^40 - 1: refused, alone or beside a later offence; reason 2 beside it reports 2; a transaction nonce of
    2^40 or more is reason 2. BatchBuilder does not wrap either: it leaves e0 = 1 + 2^72, which is not a leaf"""
    st = R.wide_state()
    cases = R.nonce_refusals(st)
    assert [(i, r) for _, i, r in cases] == [(1, 12), (0, 12), (1, 2), (3, 12), (1, 2)]
    for batch, index, reason in cases:
        _refused(st, batch, index, reason)
    txs, plan, idxs = cases[0][0]
    db, _ = C.builder_batch(st, txs, plan, idxs, N_LEVELS)
    assert B.leaf_fields(db.leaves[st.role["last1"]])[0] == 1 + (1 << 72) + (1 << 72)   # sign 1, and the carry out of the nonce on top of it


def test_fee_slots_64_against_the_builder():
    st = R.slots_state()
    plan, idxs = R.slots_plan(st)
    assert len(plan) == 64 and len(set(plan)) == 64 and not set(plan) & set(R.ABSENT) and set(plan) | set(R.ABSENT) == set(R.TOKENS_66)
    assert 6 <= idxs.count(0) <= 8 and all(st.state(a)["tokenID"] == t for t, a in zip(plan, idxs) if a)
    assert any(t >> 31 for t in plan)
    for m in (63, 64, 65, 129):
        txs, plan, idxs = R.fee_slots_64(st, m)
        assert len(txs) == m and len({t["tokenID"] for t in txs}) == min(m, 66)
        senders = {t["fromIdx"] for t in txs}
        assert senders & set(idxs)   # some fee accounts also send
        bb, res = _model_vs_builder(st, txs, plan, idxs)
        if m == 129:
            paid = [j for j, v in enumerate(res[3]) if v]
            assert len(paid) == 64   # every slot collects (the two absent tokens pay into none)
            assert sum(1 for t in txs if t["tokenID"] in R.ABSENT) >= 3
    txs, plan, idxs = R.fee_slots_64(st, 129, share=3)
    assert sum(A.is_to_addr(t) for t in txs) == 43
    _model_vs_builder(st, txs, plan, idxs, by_addr=True)


def test_l1_high_limbs_against_the_builder():
    st = R.wide_state()
    (l1_txs, l2_txs, plan, idxs), refused = R.l1_high_limbs(st)
    db, bb = L1.builder_batch(st, l1_txs, l2_txs, plan, idxs, N_LEVELS)
    inp = bb.get_input()
    res = L1.scheme_model(st.state, l1_txs, l2_txs, plan, idxs)
    assert res[0] == "ok", res
    for name, vals in res[1].items():
        assert vals == inp[name], name
    assert res[2][:-1] == inp["imAccFeeOut"] and res[3] == inp["imFinalAccFee"]
    assert res[4] == L1.builder_flags(bb, len(l1_txs)) == [0, 2, 0, 0, 0]
    for a, leaf in res[5].items():
        assert leaf == db.leaves[a], a
    f0 = st.first_idx
    assert db.leaves[f0 + 45]["balance"] == (1 << 192) - 1 and db.leaves[f0 + 41]["balance"] == 5 + R.V
    low = (1 << 128) - 1   # the underflow is decided by limb 4 alone
    assert st.state(f0 + 43)["balance"] & low == R.V & low and st.state(f0 + 43)["balance"] < R.V
    for (a, b, plan, idxs), row, reason in refused:
        assert L1.scheme_model(st.state, a, b, plan, idxs)[:3] == ("refused", row, reason)
    assert [r for _, _, r in refused] == [3, 5]


def test_signed_extremes_against_the_builder():
    import ledger_sig_common as S
    st = R.signed_state()
    for by_addr in (False, True):
        txs, plan, idxs = R.signed_extremes(st, by_addr)
        assert all(t["nonce"] == (1 << 40) - 2 and t["tokenID"] == R.TOK_MAX and t["maxNumBatch"] == (1 << 32) - 1 for t in txs)
        assert txs[0]["userFee"] == 255 and txs[0]["amountF"] == 31 << 35 and txs[3]["toBjjSign"] == 1 and txs[3]["toEthAddr"] == A.ANY
        bb, res = _model_vs_builder(st, txs, plan, idxs, by_addr=by_addr)
        cols = st.leaf_fields()
        assert S.verdicts(txs, cols, st.first_idx, 1) == [0, 0, 0, 0]
        inp = bb.get_input()
        assert inp["txCompressedData"][:4] == [S.message(t)[0] for t in txs] and [m["sigL2Hash"] for m in bb.tx_meta[:4]] == [S.message(t)[2] for t in txs]
        if by_addr:
            assert res[4] == [0, 0, 0, st.any]


def test_host_build_of_the_256_bit_routines_agrees_with_python(tmp_path):
    text = R.check_lines()
    n = len(text.splitlines())
    assert sum(ln.startswith("f ") for ln in text.splitlines()) == 160 and sum(ln.startswith("g ") for ln in text.splitlines()) == 256 * 160
    assert sum(ln.startswith("v ") for ln in text.splitlines()) == 256 + 225 and sum(ln.startswith("v ") and ln.endswith(" 1") for ln in text.splitlines()) == 225
    src = os.path.join(os.path.dirname(__file__), "native", "u256_check.cpp")
    exe = str(tmp_path / "u256_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and "cases=%d mismatches=0" % n in r.stdout, r.stdout + r.stderr[-2000:]
    # the program does judge: one expectation changed per kind of record is one mismatch each
    lines = text.splitlines()
    kinds = "fgvansol"
    for kind in kinds:
        at = next(i for i, ln in enumerate(lines) if ln.startswith(kind + " "))
        last = lines[at].split()[-1]
        lines[at] = " ".join(lines[at].split()[:-1] + ["%x" % (int(last, 16) ^ 1)])
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 1 and "mismatches=%d" % len(kinds) in r.stdout, r.stdout + r.stderr[-2000:]
