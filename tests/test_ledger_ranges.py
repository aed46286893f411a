"""The device-resident ledger at the edges of its value ranges (tests/ledger_range_common.py) against the Python BatchBuilder over the
same state with host hashing: all 256 fee selectors on amounts of every exponent, nonces that carry into and fill the byte beside the
sign bit, balances up to 2^192 - 1, token ids with bit 31 set, 64 fee slots on either side of the scan's chunk, L1 amounts with bits in
limb 4, signed transfers whose fields are at their maxima, the refusal of a nonce that would leave its field (reason 12), of planes that
are not leaves, and the circuit itself, which takes no fee of 2^128 or more (neither does the ledger: reason 16). Every comparison is on bytes, bit-exact; tests/test_ledger_ranges_cpu.py proves the fixtures."""
import types

import numpy as np
import pytest

import device_state_common as D
import ledger_addr_common as A
import ledger_common as C
import ledger_l1_common as L1
import ledger_range_common as R
import ledger_sig_common as S
import test_ledger as TL
import test_ledger_addr as TA
from circuits_amd import HzError
from circuits_amd import builder as B
from circuits_amd.capi import LEDGER_SIG_ARRAYS

pytestmark = pytest.mark.gpu
N_LEVELS = 16
N_SIB = N_LEVELS + 1


def _l2_batch(name):
    if name.startswith("fee_slots_64"):
        st = R.slots_state()
        return (st,) + R.fee_slots_64(st, int(name.rsplit("_", 1)[1]))
    st = R.wide_state()
    return (st,) + {"all_selectors": R.all_selectors, "nonce_carry": R.nonce_carry, "to_the_brim": lambda s: R.to_the_brim(s)[0]}[name](st)


@pytest.mark.parametrize("name", ["all_selectors", "nonce_carry", "to_the_brim", "fee_slots_64_63", "fee_slots_64_64", "fee_slots_64_65", "fee_slots_64_129"])
def test_apply_l2_parity_with_the_builder(hz, name):
    st, txs, plan, idxs = _l2_batch(name)
    lg = st.to_ledger(hz)
    assert lg.root() == st.root
    db, bb, got = TL._check(lg, st, txs, plan, idxs)
    if name == "nonce_carry":   # the nonce's high byte beside the sign bit, as the ledger holds it afterwards
        e0 = D.to_int(lg.accounts([st.role["n40m3"]])[0][0])
        assert (e0 >> 32) & R.NONCE_MAX == R.NONCE_MAX and e0 >> 72 == st.state(st.role["n40m3"])["sign"] == 0
        assert D.to_int(got["nonce1"][2]) == 1 << 32
    if name == "to_the_brim":
        f0 = st.first_idx
        assert D.to_int(lg.accounts([f0 + 5])[0][1]) == (1 << 192) - 1 and D.to_int(lg.accounts([f0 + 6])[0][1]) == 0
    if name == "all_selectors":
        assert max(D.to_int(r) for r in got["final_acc_fee"]).bit_length() > 131   # single fees stop at 128 bits (reason 16), their sum does not
    TL._final_tree_matches(lg, st, db)
    lg.close()


def test_fee_slots_64_with_receivers_named_by_address(hz):
    st = R.slots_state()
    txs, plan, idxs = R.fee_slots_64(st, 129, share=3)
    assert sum(A.is_to_addr(t) for t in txs) == 43
    lg = st.to_ledger(hz)
    db, bb, got = TA._check(lg, st, txs, plan, idxs)
    assert got["acc_fee_after"].shape == (129, 64, 32) and sum(r.any() for r in got["final_acc_fee"]) == 64
    TA._final_tree_matches(lg, st, db)
    lg.close()


def test_l1_high_limbs_parity_with_the_builder(hz):
    st = R.wide_state()
    (l1_txs, l2_txs, plan, idxs), _ = R.l1_high_limbs(st)
    n_l1 = len(l1_txs)
    lg = st.to_ledger(hz)
    got = lg.apply_batch(l1_txs, l2_txs, plan, idxs, 1, 1, n_sib=N_SIB)
    db, bb = L1.builder_batch(st, l1_txs, l2_txs, plan, idxs, N_LEVELS)
    exp = L1.expected_arrays(bb, l2_txs, n_l1)
    assert len(exp) == 28
    C.assert_same(got, exp)
    res = L1.scheme_model(st.state, l1_txs, l2_txs, plan, idxs)
    assert got["l1_flags"].tolist() == res[4] == L1.builder_flags(bb, n_l1) == [0, 2, 0, 0, 0]
    assert lg.root() == bb.new_state_root
    acc = L1.touched(l1_txs, l2_txs, idxs)
    assert (lg.accounts(acc) == C.leaf_rows(db, acc)).all()
    assert D.to_int(lg.accounts([st.first_idx + 45])[0][1]) == (1 << 192) - 1
    TL._final_tree_matches(lg, st, db)
    lg.close()


def _unchanged(lg, root, fields, everyone):
    assert lg.root() == root and (lg.accounts(everyone) == fields).all()
    with pytest.raises(HzError):
        lg.outputs_dev()


def _refused(e, index, reason):
    assert e.value.status == 4, str(e.value)
    assert "index %d " % index in str(e.value) and "reason %d:" % reason in str(e.value), str(e.value)


def test_refusals_at_the_edges_change_nothing(hz):
    """2^192 reached by a transfer and by a load, a balance one unit short, an underflow that limb 4 alone decided, and the nonce that
    would leave its field (reason 12) through every call that runs the scan: the lowest index and reason are named, outputs pre-filled with
    0xA5 stay untouched, root and fields are unchanged, and a following valid call is as on a fresh ledger"""
    st = R.wide_state()
    f0 = st.first_idx
    lg = st.to_ledger(hz)
    root, everyone = lg.root(), np.arange(f0, f0 + st.N)
    fields = lg.accounts(everyone)
    cases = R.to_the_brim(st)[1] + R.nonce_refusals(st)
    assert [r for _, _, r in cases] == [5, 3, 12, 12, 2, 12, 2]
    for (txs, plan, idxs), index, reason in cases:
        assert C.scheme_model(st.state, txs, plan, idxs) == ("refused", index, reason)
        into = {name: np.full(shape, 0xA5, dtype=np.uint8) for name, shape in lg.shapes(len(txs), len(plan), N_SIB)}
        with pytest.raises(HzError) as e:
            lg.apply_l2(txs, plan, idxs, n_sib=N_SIB, into=into)
        _refused(e, index, reason)
        assert all((a == 0xA5).all() for a in into.values()), (index, reason)
        _unchanged(lg, root, fields, everyone)
    # reason 12 through the other calls that run the scan: by address, signed (valid signatures: 12 is the only offence), behind an L1 run
    (txs, plan, idxs), index, reason = R.nonce_refusals(st)[0]
    assert reason == 12
    with pytest.raises(HzError) as e:
        lg.apply_l2_addr(txs, plan, idxs, 1, 1, n_sib=N_SIB)
    _refused(e, index, 12)
    assert "the next nonce is not a leaf field" in str(e.value)
    signed = [S.sign(st, dict(t)) for t in txs]
    into = {name: np.full(shape, 0xA5, dtype=np.uint8) for name, shape in lg.shapes(len(txs), len(plan), N_SIB)}
    into.update({name: np.full((len(txs), 32), 0xA5, dtype=np.uint8) for name in LEDGER_SIG_ARRAYS})
    with pytest.raises(HzError) as e:
        lg.apply_l2_signed(signed, plan, idxs, S.CHAIN_ID, 1, n_sib=N_SIB, into=into)
    _refused(e, index, 12)
    assert all((a == 0xA5).all() for a in into.values())
    with pytest.raises(HzError) as e:
        lg.apply_l2_addr(signed, plan, idxs, S.CHAIN_ID, 1, n_sib=N_SIB, verify=True)
    _refused(e, index, 12)
    deposit = [R.top_l1(st, f0 + 41, 0, load=True)]
    with pytest.raises(HzError) as e:
        lg.apply_batch(deposit, txs, plan, idxs, 1, 1, n_sib=N_SIB)
    _refused(e, 1 + index, 12)
    _unchanged(lg, root, fields, everyone)
    # the L1 refusals
    for (l1_txs, l2_txs, plan, idxs), row, reason in R.l1_high_limbs(st)[1]:
        rows = len(l1_txs) + len(l2_txs)
        into = {name: np.full(shape, 0xA5, dtype=np.uint8) for name, shape in lg.shapes(rows, len(plan), N_SIB)}
        into.update(auxToIdx=np.full((rows, 32), 0xA5, dtype=np.uint8), l1_flags=np.full(len(l1_txs), 0xA5, dtype=np.uint8))
        with pytest.raises(HzError) as e:
            lg.apply_batch(l1_txs, l2_txs, plan, idxs, 1, 1, n_sib=N_SIB, into=into)
        _refused(e, row, reason)
        assert all((a == 0xA5).all() for a in into.values()), (row, reason)
        _unchanged(lg, root, fields, everyone)
    # a following valid call is as if the refused ones had not been made
    txs, plan, idxs = R.nonce_carry(st)
    got = lg.apply_l2(txs, plan, idxs, n_sib=N_SIB)
    fresh = st.to_ledger(hz)
    exp = fresh.apply_l2(txs, plan, idxs, n_sib=N_SIB)
    C.assert_same(got, exp)
    assert D.to_int(got["old_root"][0]) == root and lg.root() == fresh.root()
    # ... and the account that has just reached 2^40 - 1 cannot send again, on the resident nonce alone
    again = [R.txf(st.role["n40m3"], f0 + 9, R.f40(5, 0), 0, nonce=R.NONCE_MAX)]
    with pytest.raises(HzError) as e:
        lg.apply_l2(again, [1], [0], n_sib=N_SIB)
    _refused(e, 0, 12)
    assert lg.root() == fresh.root()
    lg.close()
    fresh.close()


def _sig_arrays(bb, m):
    inp = bb.get_input()
    return {"tx_compressed_data": C.to_bytes(inp["txCompressedData"][:m]), "tx_compressed_data_v2": C.to_bytes(inp["txCompressedDataV2"][:m]),
            "sig_l2_hash": C.to_bytes([meta["sigL2Hash"] for meta in bb.tx_meta[:m]])}


def test_signed_extremes(hz):
    """nonce 2^40 - 2, token 2^32 - 1, userFee 255, exponent 31 and maxNumBatch 2^32 - 1 together: the packed words and the message are the
    builder's, the signatures are accepted, all 27 arrays are the builder's; one flipped bit of the nonce's high byte, or a nonce of 2^40
    or more that the message's mask would fold onto the right one, is refused with reason 2"""
    st = R.signed_state()
    f0 = st.first_idx
    # hz_ledger_apply_l2_signed
    txs, plan, idxs = R.signed_extremes(st)
    lg = st.to_ledger(hz)
    root = lg.root()
    assert lg.verify_l2(txs, S.CHAIN_ID, 1).tolist() == [0, 0, 0, 0]
    for edit in (lambda t: dict(t, nonce=t["nonce"] ^ (1 << 39)), lambda t: dict(t, nonce=t["nonce"] ^ (1 << 32)), lambda t: dict(t, nonce=t["nonce"] + (1 << 40))):
        bad = [dict(t) for t in txs]
        bad[2] = S.sign(st, edit(bad[2]))
        with pytest.raises(HzError) as e:
            lg.apply_l2_signed(bad, plan, idxs, S.CHAIN_ID, 1, n_sib=N_SIB)
        _refused(e, 2, 2)
        assert lg.root() == root
    got = lg.apply_l2_signed(txs, plan, idxs, S.CHAIN_ID, 1, n_sib=N_SIB)
    db, bb = C.builder_batch(st, txs, plan, idxs, N_LEVELS)
    C.assert_same(got, C.expected_arrays(bb))
    C.assert_same(got, _sig_arrays(bb, 4))
    C.assert_same(got, S.expected_sig_arrays(txs))
    assert lg.root() == bb.new_state_root
    acc = C.touched(txs, idxs)
    assert (lg.accounts(acc) == C.leaf_rows(db, acc)).all()
    e0 = D.to_int(lg.accounts([f0 + 2])[0][0])
    assert (e0 >> 32) & R.NONCE_MAX == R.NONCE_MAX and e0 & 0xFFFFFFFF == R.TOK_MAX
    TL._final_tree_matches(lg, st, db)
    lg.close()
    # hz_ledger_apply_l2_addr with HZ_LEDGER_VERIFY_SIGS: the fourth is sent to the "any" address with a key of sign 1
    txs, plan, idxs = R.signed_extremes(st, by_addr=True)
    lg = st.to_ledger(hz)
    bad = [dict(t) for t in txs]
    bad[3] = S.sign(st, dict(bad[3], nonce=bad[3]["nonce"] ^ (1 << 36)))
    with pytest.raises(HzError) as e:
        lg.apply_l2_addr(bad, plan, idxs, S.CHAIN_ID, 1, n_sib=N_SIB, verify=True)
    _refused(e, 3, 2)
    got = lg.apply_l2_addr(txs, plan, idxs, S.CHAIN_ID, 1, n_sib=N_SIB, verify=True)
    db, bb = A.builder_batch(st, txs, plan, idxs, N_LEVELS)
    C.assert_same(got, A.expected_arrays(bb, txs))
    C.assert_same(got, _sig_arrays(bb, 4))
    assert D.to_int(got["auxToIdx"][3]) == st.any and int(got["sign2"][3][0]) == 1
    assert lg.root() == bb.new_state_root
    acc = A.touched(st, txs, idxs)
    assert (lg.accounts(acc) == C.leaf_rows(db, acc)).all()
    TA._final_tree_matches(lg, st, db)
    lg.close()


def test_load_refuses_planes_that_are_not_leaves(hz):
    """balance >= 2^192, e0 >= 2^73, ethAddr >= 2^160 (each below r): HZ_ERR_INPUT with the first offending account named, before the
    tree or the planes are touched; a valid load afterwards"""
    st = R.wide_state()
    f0 = st.first_idx
    lg = st.to_ledger(hz)
    root, everyone = lg.root(), np.arange(f0, f0 + st.N)
    fields = lg.accounts(everyone)
    for c, value, row, text in ((1, 1 << 192, 37, "balance >= 2^192"), (0, 1 << 73, 3, "e0 >= 2^73"), (0, (1 << 74) + 1, 0, "e0 >= 2^73"),
                                (3, 1 << 160, 63, "ethAddr >= 2^160"), (1, (1 << 253) + 5, 20, "balance >= 2^192")):
        assert value < B.P
        cols = [np.array(x) for x in st.leaf_fields()]
        cols[c][row] = D.to_bytes([value])[0]
        cols[3][63] = D.to_bytes([1 << 200])[0]   # a second, later offence: the first is named
        with pytest.raises(HzError) as e:
            lg.load(*cols)
        assert e.value.status == 4 and "account %d " % (f0 + row) in str(e.value) and text in str(e.value), str(e.value)
        assert lg.root() == root and (lg.accounts(everyone) == fields).all()
        fresh = hz.ledger(6, first_idx=f0)   # a ledger that holds nothing stays empty
        with pytest.raises(HzError) as e:
            fresh.load(*cols)
        assert e.value.status == 4
        with pytest.raises(HzError) as e:
            fresh.root()
        assert e.value.status == 1 and "hz_ledger_load" in str(e.value)
        fresh.close()
    # the largest leaves load: 2^192 - 1, e0 = 2^73 - 1, ethAddr = 2^160 - 1
    cols = [np.array(x) for x in st.leaf_fields()]
    cols[1][37], cols[0][3], cols[3][63] = D.to_bytes([(1 << 192) - 1])[0], D.to_bytes([(1 << 73) - 1])[0], D.to_bytes([(1 << 160) - 1])[0]
    lg.load(*cols)
    levels, _ = D.rebuild_levels(6, f0, cols)
    assert lg.root() == D.to_int(levels[0][0]) != root and (lg.accounts(everyone) == np.stack(cols, axis=1)).all()
    lg.close()


def test_the_circuit_accepts_the_edges(hz):
    """rollup-main at (8, 16, 2, 4) on nonce_carry plus two all_selectors rows of exponent 31 (fees of 128 bits, the largest the circuit
    takes: src/compute-fee.circom:89-91): l2_batch_inputs == BatchBuilder's dictionary key by key; the HIP context and the oracle accept
    it; hashGlobalInputs is the builder's.
    The two rows those replaced in the fixture (the same selectors and exponent, fees of 129 bits or more) make a batch the builder
    still builds inputs for: the oracle and the HIP context reject them at the first of the two rows with the overflow constraint, and
    the ledger refuses the same row with reason 16"""
    from oracle_binding import OracleCtx
    import fee_bound_common as FB
    shape = (8, 16, 2, 4)
    st = R.wide_state()
    carry, fee_tokens, fee_idxs = R.nonce_carry(st)
    rows, table = R.all_selectors(st)[0], R.all_selectors_rows()
    fee = lambda t: B.compute_fee(B.float2fix(t["amountF"]), t["userFee"])   # noqa: E731
    e31 = [t for t in rows if t["amountF"] >> 35 == 31]
    assert len(e31) == 8 and all(not fee(t) >> 128 for t in e31)
    two = sorted(e31, key=fee)[-2:]
    assert all(fee(t).bit_length() == 128 for t in two)
    above = [dict(t, amountF=table[t["userFee"]][2]) for t in two]
    assert all(t["amountF"] >> 35 == 31 and fee(t) >> 128 for t in above)

    def batch(two):
        out, seen = [dict(t) for t in carry], {}
        for t in two:
            out.append(dict(t, nonce=seen.get(t["fromIdx"], 0)))
            seen[t["fromIdx"]] = seen.get(t["fromIdx"], 0) + 1
        for t in out:
            t["signer"] = S.signer(st, t["fromIdx"])
        return out
    g = hz.ctx("rollup-main", nTx=shape[0], nLevels=shape[1], maxL1Tx=shape[2], maxFeeTx=shape[3])
    # above the bound: the builder's inputs, since the ledger makes none
    txs = batch(above)
    _, bb = C.builder_batch(st, txs, fee_tokens + [0] * 2, fee_idxs + [0] * 2, shape[1], max_l1=shape[2])
    o = OracleCtx("rollup-main", *shape)
    o.set_inputs(bb.get_input())
    ref = o.run()
    name = FB.OVF_SHIFTED if above[0]["userFee"] < 192 else FB.OVF_NOTSHIFTED
    assert ref is not None and ref[1] == len(carry) and ref[2] == FB.constraint_ids()[name], ref
    g.set_inputs(bb.get_input())
    with pytest.raises(HzError) as e:
        g.run()
    assert (e.value.unit, e.value.constraint_id, e.value.lhs, e.value.rhs) == (ref[1], ref[2], ref[4], ref[5]), str(e.value)
    over = st.to_ledger(hz)
    like = types.SimpleNamespace(last_idx=st.first_idx + st.N - 1, num_batch=0)
    with pytest.raises(HzError) as e:
        B.l2_batch_inputs(over, like, txs, *shape, fee_tokens, fee_idxs, 1)
    _refused(e, len(carry), 16)
    assert over.root() == st.root
    over.close()
    # below it
    txs = batch(two)
    assert len(txs) == shape[0]
    db, bb = C.builder_batch(st, txs, fee_tokens + [0] * 2, fee_idxs + [0] * 2, shape[1], max_l1=shape[2])
    exp = bb.get_input()
    lg = st.to_ledger(hz)
    like = types.SimpleNamespace(last_idx=st.first_idx + st.N - 1, num_batch=0)
    inp, _ = B.l2_batch_inputs(lg, like, txs, *shape, fee_tokens, fee_idxs, 1)
    assert set(inp) == set(exp), set(inp) ^ set(exp)
    for name in exp:
        assert inp[name] == exp[name], name
    assert inp["nonce1"][2] == 1 << 32 and inp["nonce1"][4] == (1 << 40) - 2 and inp["tokenID1"][5] == R.TOK_MAX
    g.set_inputs(inp)
    g.run()
    assert g.get("main.hashGlobalInputs") == bb.get_hash_inputs()
    o = OracleCtx("rollup-main", *shape)
    o.set_inputs(inp)
    assert o.run() is None
    assert g.read_raw_bytes() == o.read_raw_bytes()
    lg.close()
