"""The standalone-main fuzz without a GPU (tests/standalone_fuzz_common.py, the generators of tests/fuzz_common.py): for DecodeTx,
FeeTx, HashState, the eight gadget templates and AySign2Ax as `component main`

  * the generators make what they claim -- the named edges, whole wavefronts laid out by the selector ComputeFee sees, a share of
    cases that violate two or more constraints at once, inputs outside the ranges RollupTx feeds for the mains that cannot fail;
  * the oracle on four threads equals the oracle on one, and a rejected witness is complete;
  * the oracle rejects a case exactly when its witness violates a constraint of the reference's own text
    (tests/golden/declared_forms/, recorded complete for these twelve: Poseidon, the SMT templates and the curve arithmetic stated).

The GPU half (tests/test_standalone_fuzz.py) holds the HIP kernels to the same oracle on the same lists."""
import pytest

import fuzz_common as FZ
import standalone_fuzz_common as SF

P = FZ.P
_JUDGED = {}


def judged(key):
    """[(rejected by the oracle, constraints of the recorded system its witness violates)] of the first N_CPU[key] cases, once"""
    if key not in _JUDGED:
        cases, parts, failures = SF.full_list(key)
        judge = SF.Judge(key)
        out = []
        for o, lo, cnt in parts:
            for k in range(cnt):
                if lo + k < SF.N_CPU[key]:
                    out.append((lo + k in failures, judge(o, k)))
        _JUDGED[key] = out
    return _JUDGED[key]


def _values(cases, f, path=()):
    return {FZ._get(d, f, path) % P for d in cases}


# ---- the generators ----------------------------------------------------------------------------------------------------------------
def test_decode_float_edges():
    v = _values(SF.cases_of("decode-float"), "in")
    m35 = (1 << 35) - 1
    assert {0, m35, 31 << 35, (31 << 35) | m35, (1 << 40) - 1, 1 << 40, (1 << 40) + 1, P - 1} <= v


@pytest.mark.parametrize("key", ["compute-fee", "balance-updater"])
def test_fee_selector_edges_and_wavefront_placement(key):
    cases = SF.cases_of(key)
    sel = _values(cases, "feeSel" if key == "compute-fee" else "feeSelector")
    assert {0, 191, 192, 207, 208, 255, 256, P - 1} <= sel and any(256 < s < 512 for s in sel)
    amt = _values(cases, "amount")
    assert {0, (1 << 128) - 1, 1 << 128, (1 << 192) - 1, 1 << 192, P - 1} <= amt and len(amt) > 100
    for f in (("applyFee",) if key == "compute-fee" else ("onChain", "nop", "nullifyLoadAmount", "nullifyAmount")):
        v = _values(cases, f)
        assert {0, 1, 2, P - 1} <= v and len(v) > 6, f
    if key == "balance-updater":
        for f in ("oldStBalanceSender", "oldStBalanceReceiver", "loadAmount"):
            assert {0, (1 << 192) - 1, 1 << 192, P - 1} <= _values(cases, f), f
    # the wavefronts (aligned runs of 64 instances) by the selector ComputeFee sees
    waves = [[FZ.is_bit(FZ.apply_fee_of(key, d)) for d in cases[w:w + FZ.WAVE]] for w in range(0, len(cases) - FZ.WAVE + 1, FZ.WAVE)]
    all_bits = [w for w, b in enumerate(waves) if all(b)]
    assert all_bits
    for w in all_bits[:1]:   # the product-free path with selectors and amounts out of range
        run = cases[w * FZ.WAVE:(w + 1) * FZ.WAVE]
        assert sum(d["feeSel" if key == "compute-fee" else "feeSelector"] % P >= 256 for d in run) >= 8 and sum(d["amount"] % P >= (1 << 128) for d in run) >= 8
    lone = {b.index(False) for b in waves if b.count(False) == 1}
    assert {0, 17, 63} <= lone, lone
    assert any(not any(b) for b in waves)
    if key == "balance-updater":   # a bit made of two non-bits
        assert any(FZ.is_bit(FZ.apply_fee_of(key, d)) and not FZ.is_bit(d["onChain"]) for d in cases)


def test_fee_accumulator_edges():
    kw = SF.kw_of("fee-accumulator")
    F = kw["maxFeeTx"]
    cases = SF.cases_of("fee-accumulator")
    where = [[j for j in range(F) if d["feePlanTokenID"][j] % P == d["tokenID"] % P] for d in cases]
    assert [] in where and any(w and w[0] == 0 and len(w) == 1 for w in where) and [F - 1] in where and list(range(F)) in where
    assert any(not w and any((t - d["tokenID"]) % P == P - 1 for t in d["feePlanTokenID"]) for d, w in zip(cases, where))
    assert any(d["fee2Charge"] == P - 1 and w and d["accFeeIn"][w[0]] == P - 1 for d, w in zip(cases, where))


def test_rollup_tx_states_edges():
    cases = SF.cases_of("rollup-tx-states")
    for f in FZ.STATES_BITS:
        assert {2, P - 1} <= _values(cases, f) and len(_values(cases, f)) >= 5, f
    assert {0, 1, 2, 255, 256} <= _values(cases, "toIdx")
    assert {(1 << 160) - 2, (1 << 160) - 1, 1 << 160} <= _values(cases, "toEthAddr")
    combos = {(d["tokenID1"] == d["tokenID"], d["tokenID2"] == d["tokenID"], d["ethAddr1"] == d["fromEthAddr"]) for d in cases if d["onChain"] == 1}
    assert len(combos) == 8
    assert any(d["fromIdx"] == 0 and d["auxFromIdx"] == 0 for d in cases)
    assert any(d["onChain"] == 0 and d["loadAmount"] and d["newAccount"] for d in cases)


def test_rq_tx_verifier_edges():
    cases = SF.cases_of("rq-tx-verifier")
    off = _values(cases, "rqTxOffset")
    assert set(range(10)) | {P - 1} <= off and any(10 <= o < 16 for o in off)
    wrong = [sum(d["rq" + k] % P != FZ._rq_selected(d, k, d["rqTxOffset"] % P & 7) % P for k in FZ.RQ_KINDS) for d in cases]
    assert all(wrong.count(c) >= 8 for c in (0, 1, 2, 3))
    # the requested value sits in a slot that is not the selected one
    assert any(w and any(d["rq" + k] in d["future" + k] + d["past" + k] and d["rq" + k] != FZ._rq_selected(d, k, d["rqTxOffset"] % P & 7) for k in FZ.RQ_KINDS)
               for d, w in zip(cases, wrong))


def test_mux256_edges():
    cases = SF.cases_of("mux256")
    for pos in range(8):
        v = _values(cases, "s", (pos,))
        assert {0, 1, 2, P - 1} <= v and len(v) > 6, pos
    assert any(max(d["in"]) > (1 << 250) for d in cases)


def test_bits_compressed_edges():
    cases = SF.cases_of("bits-compressed-2-ay-sign")
    flat = [d["bjjCompressed"] for d in cases]
    assert any(all(b == 1 for b in bits[:254]) for bits in flat)   # ay = 2^254 - 1 >= P before the reduction
    assert {2, P - 1} <= {bits[255] for bits in flat} and any(bits[255] not in (0, 1, 2, P - 1) for bits in flat)
    assert any(bits[i] == 2 for bits in flat for i in (0, 253)) and any(bits[i] == P - 1 for bits in flat for i in range(254))


def test_ay_sign_2_ax_edges():
    from circuits_amd import builder as B
    cases = SF.cases_of("ay-sign-2-ax")
    by_ay = {}
    for d in cases:
        by_ay.setdefault(d["ay"] % P, set()).add(d["sign"] % P)
    named = [0, 1, P - 1, 2, P - 2, B.BASE8[1], FZ.bjj_order8_point()[1], 1 << 253, (1 << 253) - 1, (1 << 253) + 1]
    for y in named:
        assert {0, 1, 2, P - 1} <= by_ay[y], y
    full = [y for y, s in by_ay.items() if {0, 1, 2, P - 1} <= s]
    assert sum(FZ.bjj_x_of(y) is not None for y in full) >= 8 and sum(FZ.bjj_x_of(y) is None for y in full) >= 8
    assert FZ.bjj_x_of(1) == 0 and FZ.bjj_x_of(P - 1) == 0 and 1 in by_ay[1] and 1 in by_ay[P - 1]   # sign = 1 where x = 0


def test_hash_state_edges():
    cases = SF.cases_of("hash-state")
    for f, w in FZ.HASH_STATE_WIDTH.items():
        assert {0, 1, P - 1, (1 << w) - 1, (1 << w) % P, (1 << w) + 1} <= _values(cases, f), f
    assert any(not FZ.is_bit(d["sign"]) for d in cases) and any(d["nonce"] >= (1 << 40) for d in cases)


def test_decode_tx_edges():
    L = SF.kw_of("decode-tx")["nLevels"]
    cases = SF.cases_of("decode-tx")
    for f in FZ.DECODE_TX_BITS:
        assert {2, P - 1} <= _values(cases, f), f
    for f, w in FZ.DECODE_TX_WIDTH.items():
        assert any((1 << w) <= d[f] % P < (1 << (w + 1)) for d in cases), f
    assert {(1 << L) - 1, (1 << 48) - 1} <= _values(cases, "inIdx") and any(d["auxFromIdx"] >> 48 == 1 for d in cases)
    assert any(not FZ.is_bit(b) for d in cases for b in d["fromBjjCompressed"][:255]) and any(not FZ.is_bit(d["fromBjjCompressed"][255]) for d in cases)


def test_fee_tx_edges():
    L = SF.kw_of("fee-tx")["nLevels"]
    cases = SF.cases_of("fee-tx")
    idx = [d["feeIdx"] % P for d in cases]
    assert 0 in idx and any(v >= (1 << L) for v in idx) and any(v and idx.count(v) > 1 for v in idx)
    assert any(d["feeIdx"] and d["feePlanToken"] != d["tokenID"] for d in cases)
    for f in ("balance", "accFee"):
        assert {(1 << 192) - 1, P - 1} <= _values(cases, f), f
    assert any(d["siblings"] == [0] * (L + 1) and d["feeIdx"] for d in cases)


@pytest.mark.parametrize("key", SF.NEVER_FAIL)
def test_mains_that_cannot_fail_get_inputs_out_of_range(key):
    cases = SF.cases_of(key)
    assert 2 * sum(SF.out_of_range(key, d) for d in cases) >= len(cases)


# ---- the oracle on these lists -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SF.MAINS)
def test_oracle_threads_equal_serial_and_the_mix_holds(key):
    cases, _, _ = SF.full_list(key)
    n = len(cases)
    parts = FZ.run_oracle_threads(key, SF.shape_of(key), cases, n_threads=4)
    one = FZ.run_oracle_threads(key, SF.shape_of(key), cases, n_threads=1)
    failures = FZ.oracle_failures(parts)
    assert failures == FZ.oracle_failures(one) == SF.full_list(key)[2]
    SF.check_mix(key, n, failures)
    # the same list rotated (the second step of the GPU half) is the same multiset: the mix holds for it as it stands
    o1 = one[0][0]
    wl = o1.witness_len()
    for o, lo, cnt in parts:
        assert o.unwritten()[0] == 0   # a rejected witness is still complete
        for k in (0, cnt // 2, cnt - 1):
            assert o.read_bytes(0, wl, k) == o1.read_bytes(0, wl, lo + k)
    assert o1.unwritten()[0] == 0
    if key not in SF.NEVER_FAIL:   # one instance alone: there is a first rejected case and a first accepted one
        assert min(failures) < n and min(k for k in range(n) if k not in failures) < n


@pytest.mark.parametrize("key", SF.MAINS)
def test_oracle_rejects_exactly_what_violates_the_recorded_system(key):
    res = judged(key)
    assert len(res) == SF.N_CPU[key]
    for k, (rejected, bad) in enumerate(res):
        assert rejected == bool(bad), (key, k, rejected, bad[:3])
    if key in SF.NEVER_FAIL:
        assert not any(r for r, _ in res)
    else:
        assert any(r for r, _ in res) and not all(r for r, _ in res)


@pytest.mark.parametrize("key", list(SF.MIN_IDS))
def test_a_tenth_of_the_cases_violates_two_constraints_at_once(key):
    """the order of the reports matters only where more than one constraint fails: by the recorded system, over the cases solved above"""
    res = judged(key)
    double = sum(len(bad) >= 2 for _, bad in res)
    if key == "decode-float":   # ONE constraint of DecodeFloat can fail (Num2Bits(40)'s sum; the bits it writes are bits whatever comes in)
        assert double == 0 and SF.MIN_IDS[key] == 1
        return
    assert 10 * double >= len(res), (key, double, len(res))
