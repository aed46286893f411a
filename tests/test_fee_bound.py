"""ComputeFee's bound of 128 bits (src/compute-fee.circom:89-91) on everything on the device that computes a fee, against one
plain-integer model (tests/fee_bound_common.py, proven against the oracle in tests/test_fee_bound_cpu.py).
The witness kernels: the ComputeFee, BalanceUpdater, RollupTx and RollupMain mains on the amounts on either side of the bound -- the
whole buffer bit for bit and the first failure (instance, unit, constraint, operands) of every instance against the oracle, the verdict
against the model. The ledger: every selector's largest amount below the bound is applied and equals the builder field by field, the
smallest amount above it is refused with reason 16 through all seven apply calls, ranked as the contract says, dropped by
hz_ledger_select_batch, and the ledger accepts exactly the batches RollupMain accepts."""
import re
import types

import numpy as np
import pytest

import fee_bound_common as FB
import fuzz_common as FZ
import ledger_common as C
import ledger_l1_common as L1
import ledger_range_common as R
import ledger_select_common as SC
import ledger_sig_common as S
import test_ledger as TL
from circuits_amd import HzError
from circuits_amd import builder as B
from circuits_amd import capi
from circuits_amd.capi import ConstraintError
from oracle_binding import OracleCtx

pytestmark = pytest.mark.gpu
N_LEVELS = 16
N_SIB = N_LEVELS + 1
SHAPE = (8, N_LEVELS, 2, 4)
FLAG_LATENCY, FLAG_SOLO = 2, 4   # HZ_FLAG_LATENCY, HZ_FLAG_SOLO


def _run(g):
    try:
        g.run()
    except ConstraintError as e:
        return e
    return None


def _names(cases):
    return "feeSel %d amount %d applyFee %d" % (cases["feeSel"], cases["amount"], cases["applyFee"])


def _against_the_model(g, verdicts, label):
    """the first failure of every instance is the model's constraint; -> the accepted instances"""
    ids = FB.constraint_ids()
    got = {f[0]: f[2] for f in g.failures()}
    for k, (name, _) in enumerate(verdicts):
        if name == FB.ACCEPTED:
            assert k not in got, "%s: the model accepts, the kernel reports %s" % (label(k), FZ.constraint_name(got[k]))
        else:
            assert k in got, "%s: the model rejects (%s), the kernel accepts" % (label(k), name)
            assert got[k] == ids[name], "%s: the model names %s, the kernel %s" % (label(k), name, FZ.constraint_name(got[k]))
    return [k for k, (name, _) in enumerate(verdicts) if name == FB.ACCEPTED]


# ---- ComputeFee main ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fee_launch():
    cases = FB.compute_fee_cases()
    inputs = [c for c, _ in cases]
    return inputs, [v for _, v in cases], FZ.run_oracle_threads("compute-fee", (), inputs)


def test_compute_fee_main_over_both_tables(hz, fee_launch):
    """one launch of about 1 240 instances: every selector's pair of the float40 table and of the exact table, the pairs around a
    product of 2^253, the overflowing amounts with applyFee = 0; every wavefront mixes accepted and rejected lanes of both branches.
    A second launch with one lane per wavefront on a non-bit applyFee (the whole wavefront then takes the general path): the other
    lanes' buffers and verdicts are those of the first launch"""
    inputs, verdicts, parts = fee_launch
    n = len(inputs)
    assert {c["feeSel"] for c, v in zip(inputs, verdicts) if v[0] != FB.ACCEPTED} >= set(range(FB.FIRST_REACHING, 256))
    label = lambda k: _names(inputs[k])   # noqa: E731
    g = hz.ctx("compute-fee", n_instances=n)
    FZ.set_all_inputs(g, inputs)
    err = _run(g)
    accepted = _against_the_model(g, verdicts, label)   # first: its messages name the selector and the amount
    FZ.compare_instanced(g, parts, n)
    assert FZ.check_failures(g, parts, err) == sum(v[0] != FB.ACCEPTED for v in verdicts)
    wl, row = g.witness_len(), g.lookup("main.feeOut")
    first = np.frombuffer(g.read_raw_bytes(), dtype=np.uint8).reshape(wl, n, 32).copy()
    for k in accepted:
        assert int.from_bytes(first[row, k].tobytes(), "little") == verdicts[k][1], label(k)
    first_failures = {f[0]: f[1:3] + f[4:6] for f in g.failures()}
    # the general path: lane 5 of every wavefront carries applyFee = 2 (the mux's selectors are then no bits: the oracle is its judge)
    odd = list(range(5, n, 64))
    inputs2 = [dict(c, applyFee=2) if k in odd else c for k, c in enumerate(inputs)]
    parts2 = FZ.run_oracle_threads("compute-fee", (), [inputs2[k] for k in odd], n_threads=1)
    FZ.set_all_inputs(g, inputs2)
    err2 = _run(g)
    second = np.frombuffer(g.read_raw_bytes(), dtype=np.uint8).reshape(wl, n, 32)
    rest = np.setdiff1d(np.arange(n), odd)
    assert np.array_equal(second[:, rest], first[:, rest])
    ref = np.frombuffer(parts2[0][0].read_raw_bytes(), dtype=np.uint8).reshape(wl, len(odd), 32)
    assert np.array_equal(second[:, odd], ref)
    second_failures = {f[0]: f[1:3] + f[4:6] for f in g.failures()}
    assert {k: v for k, v in second_failures.items() if k not in odd} == {k: v for k, v in first_failures.items() if k not in odd}
    assert {odd.index(k): v for k, v in second_failures.items() if k in odd} == FZ.oracle_failures(parts2)
    assert (err2 is None) == (not second_failures) and (err2 is None or err2.instance == min(second_failures))


# ---- BalanceUpdater main ------------------------------------------------------------------------------------------------------------------
def test_balance_updater_main_over_the_float40_table(hz):
    """every selector's pair as an L2 row of a sender that can pay, and the overflowing amount on an onChain = 1 row and on a nop = 1 row,
    which the circuit does not charge (accepted)"""
    names = "oldStBalanceSender oldStBalanceReceiver amount loadAmount feeSelector onChain nop nullifyLoadAmount nullifyAmount".split()
    inputs, verdicts = [], []
    for sel, below, above in FB.float40_table():
        rows = [(below, 0, 0)] + ([(above, 0, 0), (above, 1, 0), (above, 0, 1)] if above is not None else [])
        for f, on_chain, nop in rows:
            amount = FB.amount_of(f)
            inputs.append(dict(zip(names, (R.RICH, 10 ** 20, amount, 0, sel, on_chain, nop, 0, 0))))
            verdicts.append(FB.verdict(amount, sel, int(not on_chain and not nop)))
    n = len(inputs)
    assert n == 256 + 3 * 225 and sum(v[0] != FB.ACCEPTED for v in verdicts) == 225
    label = lambda k: "feeSelector %d amount %d onChain %d nop %d" % tuple(inputs[k][f] for f in ("feeSelector", "amount", "onChain", "nop"))   # noqa: E731
    parts = FZ.run_oracle_threads("balance-updater", (), inputs)
    g = hz.ctx("balance-updater", n_instances=n)
    FZ.set_all_inputs(g, inputs)
    err = _run(g)
    accepted = _against_the_model(g, verdicts, label)
    FZ.compare_instanced(g, parts, n)
    assert FZ.check_failures(g, parts, err) == 225
    row = g.lookup("main.fee2Charge")
    fees = np.frombuffer(g.read_raw_bytes(row * n, n), dtype=np.uint8).reshape(n, 32)
    for k in accepted:
        assert int.from_bytes(fees[k].tobytes(), "little") == verdicts[k][1], label(k)


# ---- RollupTx and RollupMain --------------------------------------------------------------------------------------------------------------
def _rows(st, picks):
    """transfers of the rich accounts (offsets 1 .. 4, two rows each at most) to the receivers: picks = [(selector, float40)]"""
    f0, seen, out = st.first_idx, {}, []
    for i, (sel, f) in enumerate(picks):
        frm = f0 + 1 + i % 4
        out.append(dict(R.txf(frm, f0 + 48 + i, f, sel, nonce=seen.get(frm, 0)), signer=S.signer(st, frm)))
        seen[frm] = seen.get(frm, 0) + 1
    return out


def _batches(st):
    """[(label, txs, the row above the bound or None)]: the eight "below" rows together; then, per selector, the "above" row on one
    transaction among "below" rows of the other selectors"""
    pairs = FB.pairs()
    assert len(pairs) == 8 and {31, 191, 192, 255} <= {s for s, _, _ in pairs} and any(s < 192 for s, _, _ in pairs) and any(s >= 192 for s, _, _ in pairs)
    out = [("below: " + ", ".join("selector %d amount %d" % (s, FB.amount_of(lo)) for s, lo, _ in pairs), _rows(st, [(s, lo) for s, lo, _ in pairs]), None)]
    for at, (sel, _, hi) in enumerate(pairs):
        picks = [(s, lo) for s, lo, _ in pairs]
        picks[at] = (sel, hi)
        out.append(("selector %d amount %d at row %d" % (sel, FB.amount_of(hi), at), _rows(st, picks), at))
    return out


FEE_PLAN = ([1, 0, 0, 0], lambda st: [st.first_idx + R.WIDE_FEE, 0, 0, 0])


def _built(st, txs):
    return C.builder_batch(st, txs, FEE_PLAN[0], FEE_PLAN[1](st), N_LEVELS, max_l1=SHAPE[2])[1]


def test_rollup_tx_main_on_the_boundary_pairs(hz):
    """the standalone RollupTx inputs the builder makes of the eight pairs (it builds inputs for such a fee, as upstream does): one
    launch of 16 instances, "below" and "above" alternating"""
    st = R.wide_state()
    pairs = FB.pairs()
    picks = [(s, f) for s, lo, hi in pairs[:4] for f in (lo, hi)]
    picks2 = [(s, f) for s, lo, hi in pairs[4:] for f in (lo, hi)]
    inputs, verdicts, labels = [], [], []
    for half in (picks, picks2):
        bb = _built(st, _rows(st, half))
        for i, (sel, f) in enumerate(half):
            inputs.append(bb.get_single_tx_input(i)[0])
            verdicts.append(FB.verdict(FB.amount_of(f), sel))
            labels.append("selector %d amount %d" % (sel, FB.amount_of(f)))
    n = len(inputs)
    assert n == 16 and [v[0] == FB.ACCEPTED for v in verdicts] == [True, False] * 8
    parts = FZ.run_oracle_threads("rollup-tx", (0, N_LEVELS, 0, SHAPE[3]), inputs, n_threads=4)
    g = hz.ctx("rollup-tx", nLevels=N_LEVELS, maxFeeTx=SHAPE[3], n_instances=n)
    FZ.set_all_inputs(g, inputs)
    err = _run(g)
    _against_the_model(g, verdicts, lambda k: labels[k])
    FZ.compare_instanced(g, parts, n)
    assert FZ.check_failures(g, parts, err) == 8


@pytest.fixture(scope="module")
def main_batches():
    """the nine RollupMain batches with the builder's inputs and the oracle's answer, computed once"""
    st = R.wide_state()
    out = []
    for label, txs, above in _batches(st):
        bb = _built(st, txs)
        inp = bb.get_input()
        o = OracleCtx("rollup-main", *SHAPE)
        o.set_inputs(inp)
        out.append((label, txs, above, bb, inp, o, o.run()))
    return st, out


@pytest.mark.parametrize("flags", [0, FLAG_LATENCY, FLAG_LATENCY | FLAG_SOLO])
def test_rollup_main_on_the_boundary_pairs(hz, main_batches, flags):
    """RollupMain at (8, 16, 2, 4) on the wide state: the batch of eight "below" rows is accepted by the HIP context and the oracle with
    the builder's hashGlobalInputs; each batch with one "above" row is rejected with C_RTX_FEE_OVF_SHIFTED / _NOTSHIFTED at the oracle's
    unit, which is that row; the whole buffer is the oracle's either way. In the plain, the latency and the latency | solo schedule"""
    st, batches = main_batches
    ids = FB.constraint_ids()
    g = hz.ctx("rollup-main", nTx=SHAPE[0], nLevels=SHAPE[1], maxL1Tx=SHAPE[2], maxFeeTx=SHAPE[3], flags=flags)
    for label, txs, above, bb, inp, o, ref in batches:
        g.set_inputs(inp)
        err = _run(g)
        if above is None:
            assert ref is None and err is None, "%s: %s" % (label, err)
            assert g.get("main.hashGlobalInputs") == bb.get_hash_inputs(), label
        else:
            sel = txs[above]["userFee"]
            name = FB.verdict(FB.amount_of(txs[above]["amountF"]), sel)[0]
            assert name == (FB.OVF_SHIFTED if sel < 192 else FB.OVF_NOTSHIFTED)
            assert ref is not None and (ref[1], ref[2]) == (above, ids[name]), (label, ref)
            assert err is not None, "%s: the oracle rejects, the HIP context accepts" % label
            assert (err.instance, err.unit, err.constraint_id, err.lhs, err.rhs) == (ref[0], ref[1], ref[2], ref[4], ref[5]), (label, str(err), ref)
        assert g.read_raw_bytes() == o.read_raw_bytes(), label


def test_the_ledger_accepts_exactly_the_batches_rollup_main_accepts(hz, main_batches):
    """the same nine batches through hz_ledger_apply_l2: accepted where the oracle accepts (and every array is the builder's), refused
    with reason 16 at the row whose unit the circuit names where it does not"""
    st, batches = main_batches
    plan, idxs = FEE_PLAN[0], FEE_PLAN[1](st)
    lg = st.to_ledger(hz)
    root = lg.root()
    for label, txs, above, bb, inp, o, ref in batches:
        txs = [{k: v for k, v in t.items() if k != "signer"} for t in txs]
        if ref is None:
            fresh = st.to_ledger(hz)
            got = _applied(lambda: fresh.apply_l2(txs, plan, idxs, n_sib=N_SIB), txs)
            C.assert_same(got, C.expected_arrays(bb))
            assert fresh.root() == bb.new_state_root, label
            fresh.close()
        else:
            with pytest.raises(HzError) as e:
                lg.apply_l2(txs, plan, idxs, n_sib=N_SIB)
            _refused(e, ref[1], FB.REASON, label)
            assert lg.root() == root
    lg.close()


# ---- the ledger ---------------------------------------------------------------------------------------------------------------------------
def _applied(call, txs):
    """call(); a refusal is reported with the selector and the amount of the row it names"""
    try:
        return call()
    except HzError as e:
        at = re.search(r"refused at index (\d+) ", str(e))
        row = txs[int(at.group(1))] if at and int(at.group(1)) < len(txs) else {}
        pytest.fail("selector %s amount %s (amountF %#x): %s" % (row.get("userFee"), FB.amount_of(row.get("amountF", 0)), row.get("amountF", 0), e))


def _refused(e, index, reason, label=""):
    assert e.value.status == 4, (label, str(e.value))
    assert "index %d " % index in str(e.value) and "reason %d:" % reason in str(e.value), (label, str(e.value))
    if reason == FB.REASON:
        assert "amount x fee factor does not fit 128 bits (src/compute-fee.circom:89-91)" in str(e.value), str(e.value)


def _spread(st, rows):
    """[(selector, float40)] as transfers of the four rich accounts, nonces counted"""
    f0, seen, out = st.first_idx, {}, []
    for i, (sel, f) in enumerate(rows):
        frm = f0 + 1 + i % 4
        out.append(R.txf(frm, f0 + 48 + i % 16, f, sel, nonce=seen.get(frm, 0)))
        seen[frm] = seen.get(frm, 0) + 1
    return out


def test_every_selector_is_accepted_just_below_the_bound(hz):
    """the 225 "below" rows (fees of exactly 128 bits) in batches of 63, 64, 65 and 33 transactions: every array is the builder's"""
    st = R.wide_state()
    reach = FB.reaching()
    assert len(reach) == 225 and all(FB.fee_of(lo, s).bit_length() == 128 for s, lo, _ in reach)
    lg, db, at = st.to_ledger(hz), None, 0
    plan, idxs = [1], [st.first_idx + R.WIDE_FEE]
    done = set()
    for size in (63, 64, 65, 33):
        chunk = reach[at:at + size]
        at += size
        # explicit nonces: the senders go on from where the last batch left them
        txs = _spread(st, [(s, lo) for s, lo, _ in chunk])
        for t in txs:
            t["nonce"] += sum(1 for s in done if s[0] == t["fromIdx"])
        done |= {(t["fromIdx"], t["nonce"]) for t in txs}
        assert len(txs) == size
        db, bb, got = _applied(lambda: TL._check(lg, st, txs, plan, idxs, db=db), txs)
        assert max(C.to_int(r) for r in got["acc_fee_after"][-1]).bit_length() >= 128
    assert at == 225
    TL._final_tree_matches(lg, st, db)
    lg.close()


def _state_of(lg, st):
    everyone = np.arange(st.first_idx, st.first_idx + st.N)
    return lg.root(), lg.accounts(everyone).tobytes(), lg.exit_tree().root(), lg.exit_tree().size()


CALLS = ("apply_l2", "apply_l2_signed", "apply_l2_addr", "apply_batch", "apply_batch_exits", "apply_batch_creates", "apply_batch_atomic")


def _call(lg, st, name, l1_txs, txs, plan, idxs):
    if name == "apply_l2":
        return lg.apply_l2(txs, plan, idxs, n_sib=N_SIB)
    if name == "apply_l2_signed":   # (a row that is signed already is not signed again)
        return lg.apply_l2_signed([t if "s" in t else S.sign(st, dict(t)) for t in txs], plan, idxs, S.CHAIN_ID, 1, n_sib=N_SIB)
    if name == "apply_l2_addr":
        return lg.apply_l2_addr(txs, plan, idxs, S.CHAIN_ID, 1, n_sib=N_SIB)
    return getattr(lg, name)(l1_txs, txs, plan, idxs, S.CHAIN_ID, 1, n_sib=N_SIB)


@pytest.mark.parametrize("call", range(7))
def test_every_selector_is_refused_just_above_the_bound(hz, call):
    """the 225 "above" rows (fees of exactly 129 bits) and the 32 rows all_selectors used to hold (129 to 183 bits), dealt over the
    seven apply calls (every call gets 36 or more selectors of both branches): a batch of four valid transfers with the row at index 2,
    behind an L1 deposit where the call takes one, as an exit through the calls that take exits. Refused with reason 16 at the row's own
    index; root, planes and exit tree are unchanged"""
    st = R.wide_state()
    f0 = st.first_idx
    name = CALLS[call]
    rows = [(s, hi) for s, _, hi in FB.reaching()] + [(i, over) for i, _, over in R.all_selectors_rows() if over is not None]
    assert len(rows) == 225 + 32 and all(FB.fee_of(f, s) >> 128 for s, f in rows)
    mine = rows[call::7]
    assert len(mine) >= 36 and sum(s < 192 for s, _ in mine) >= 2 and sum(s >= 192 for s, _ in mine) >= 2
    plan, idxs = [1], [f0 + R.WIDE_FEE]
    l1_txs = [R.top_l1(st, f0 + 41, 0, load=True)] if name.startswith("apply_batch") else []
    exits = name in ("apply_batch_exits", "apply_batch_creates", "apply_batch_atomic")
    lg = st.to_ledger(hz)
    before = _state_of(lg, st)
    around = _spread(st, [(50, R.f40(5, 0)), (176, R.f40(7, 3)), (0, 0), (100, R.f40(9, 1))])
    if name == "apply_l2_signed":
        around = [S.sign(st, t) for t in around]
    for k, (sel, f) in enumerate(mine):
        txs = around[:2] + [dict(_spread(st, [(0, 0), (0, 0), (sel, f)])[2])] + around[3:]
        if exits and k % 2:
            txs[2]["toIdx"] = 1
        with pytest.raises(HzError) as e:
            _call(lg, st, name, l1_txs, txs, plan, idxs)
        _refused(e, len(l1_txs) + 2, FB.REASON, "%s: selector %d amount %d" % (name, sel, FB.amount_of(f)))
        assert name.replace("apply", "hz_ledger_apply") in str(e.value)
    assert _state_of(lg, st) == before
    with pytest.raises(HzError):
        lg.outputs_dev()
    # the batch without the row is applied as on a fresh ledger
    txs = _spread(st, [(50, R.f40(5, 0)), (176, R.f40(7, 3)), (100, R.f40(9, 1))])
    got, fresh = _call(lg, st, name, l1_txs, txs, plan, idxs), st.to_ledger(hz)
    exp = _call(fresh, st, name, l1_txs, txs, plan, idxs)
    assert set(got) == set(exp) and all(got[n].tobytes() == exp[n].tobytes() for n in got) and lg.root() == fresh.root() != before[0]
    lg.close()
    fresh.close()


def test_the_rank_of_the_reason(hz):
    """16 at row i beside 3 at row i reports 3; beside 3 at row i + 1 it reports 16 at i; beside 9 anywhere it reports 9; beside 2 at a
    lower row that row"""
    st = R.wide_state()
    f0 = st.first_idx
    plan, idxs = [1], [f0 + R.WIDE_FEE]
    over = FB.float40_table()[200][2]
    ok = R.txf(f0 + 8, f0 + 9, R.f40(5, 0), 176, nonce=0)
    rich = R.txf(f0 + 1, f0 + 48, over, 200, nonce=0)
    poor = R.txf(f0 + 41, f0 + 48, over, 200, nonce=0)            # holds 5: reason 3 beside 16
    short = R.txf(f0 + 41, f0 + 49, R.f40(6, 0), 0, nonce=0)      # reason 3 alone
    lg = st.to_ledger(hz)
    root = lg.root()
    for txs, index, reason in (([ok, poor], 1, 3), ([ok, rich, short], 1, FB.REASON), ([dict(ok, nonce=4), rich], 0, 2), ([rich, dict(ok, nonce=4)], 0, FB.REASON)):
        assert C.scheme_model(st.state, txs, plan, idxs) == ("refused", index, reason)
        with pytest.raises(HzError) as e:
            lg.apply_l2(txs, plan, idxs, n_sib=N_SIB)
        _refused(e, index, reason)
    nobody = dict(R.txf(f0 + 8, 0, R.f40(5, 0), 0, nonce=0), toEthAddr=0xDEAD << 100)   # reason 9, behind and before the row
    for txs, index in (([rich, ok, nobody], 2), ([nobody, rich], 0)):
        with pytest.raises(HzError) as e:
            lg.apply_l2_addr(txs, plan, idxs, S.CHAIN_ID, 1, n_sib=N_SIB)
        _refused(e, index, 9)
    assert lg.root() == root
    lg.close()


def test_rows_the_circuit_does_not_charge(hz):
    """a NOP that carries an overflowing amount_f and user_fee, and an L1 transfer of an overflowing amount: accepted, and every array
    is the builder's"""
    st = R.wide_state()
    f0 = st.first_idx
    plan, idxs = [1], [f0 + R.WIDE_FEE]
    over = FB.float40_table()[255][2]
    nop = dict(R.txf(0, 0, over, 255, nonce=0), tokenID=0)
    ok = R.txf(f0 + 8, f0 + 9, R.f40(5, 0), 176, nonce=0)
    lg = st.to_ledger(hz)
    got = _applied(lambda: lg.apply_l2([ok, nop], plan, idxs, n_sib=N_SIB), [ok, nop])
    db, bb = C.builder_batch(st, [ok, {}], plan, idxs, N_LEVELS)
    C.assert_same(got, C.expected_arrays(bb))
    assert lg.root() == bb.new_state_root
    lg.close()
    l1_txs = [dict(L1.own(st, f0 + 1, f0 + 47), amountF=FB.float40_table()[191][2], userFee=191)]
    assert B.float2fix(l1_txs[0]["amountF"]) * B.fee_table()[191] >> 188
    lg = st.to_ledger(hz)
    got = _applied(lambda: lg.apply_batch(l1_txs, [ok], plan, idxs, 1, 1, n_sib=N_SIB), l1_txs + [ok])
    db, bb = L1.builder_batch(st, l1_txs, [ok], plan, idxs, N_LEVELS)
    C.assert_same(got, L1.expected_arrays(bb, [ok], 1))
    assert got["l1_flags"].tolist() == [0] and lg.root() == bb.new_state_root
    lg.close()


# ---- select -------------------------------------------------------------------------------------------------------------------------------
def _pool(st, acc):
    """130 candidates, amounts only: overflowing rows at 0, 30, 63, 64 and 127 (both edges of the staging tile, the middle), each
    followed later by a row of the same sender and nonce that is kept only because it was dropped"""
    f0 = st.first_idx
    a, b = f0 + 1, f0 + 2
    t = FB.float40_table()
    v = SC.valid_pool(acc, 123, 21, senders=[8, 9] + list(range(48, 64)))   # a and b send nothing here
    over = lambda frm, sel: R.txf(frm, f0 + 48, t[sel][2], sel, nonce=0)   # noqa: E731
    pool = ([over(a, 31)] + v[:29] + [over(b, 192)] + v[29:61] + [over(a, 191), over(b, 255)] + v[61:] +
            [over(a, 224), R.txf(a, f0 + 48, t[100][1], 100, nonce=0), R.txf(b, f0 + 49, R.f40(5, 0), 0, nonce=0)])
    assert len(pool) == 130 and [i for i, x in enumerate(pool) if FB.fee_of(x["amountF"], x["userFee"]) >> 128] == [0, 30, 63, 64, 127]
    return pool


def test_select_drops_what_the_circuit_rejects(hz):
    """verdict bytes, kept set and rounds are the model's; the retry loop over hz_ledger_apply_batch_atomic keeps the same set for the
    same reasons; with the overflowing row at 127 as the partner of a linked transaction the requirer is forced out in a second walk"""
    st = R.wide_state()
    acc = SC.accounts(st)
    pool = _pool(st, acc)
    lg, other = st.to_ledger(hz), st.to_ledger(hz)
    root = lg.root()
    exp = SC.model(acc, [], pool)
    got = lg.select_batch([], pool, S.CHAIN_ID, 1, verify=False)
    assert got == exp, (got, exp)
    assert [got["verdict"][i] for i in (0, 30, 63, 64, 127, 128, 129)] == [FB.REASON] * 5 + [0, 0] and got["rounds"] == 1 and lg.root() == root

    def apply(l1, rows):
        try:
            other.apply_batch_atomic(l1, rows, [1], [0], S.CHAIN_ID, 1, n_sib=N_SIB, verify=False)
        except HzError as e:
            assert e.status == 4, str(e)
            at = re.search(r"refused at index (\d+) .*reason (\d+):", str(e))
            return int(at.group(1)) - len(l1), int(at.group(2))
        return None
    kept, reasons, refusals = SC.retry_reference(apply, [], pool)
    assert kept == got["kept"] and reasons == got["verdict"] and refusals == 130 - len(kept) >= 5
    lg.apply_batch_atomic([], capi.select_compact(pool, got), [1], [0], S.CHAIN_ID, 1, n_sib=N_SIB, verify=False)
    assert lg.root() == other.root()
    lg.close()
    other.close()
    linked = [dict(x) for x in pool]
    SC.link(linked, 129, 127)
    lg = st.to_ledger(hz)
    exp = SC.model(acc, [], linked)
    got = lg.select_batch([], linked, S.CHAIN_ID, 1, verify=False)
    assert got == exp, (got, exp)
    assert got["verdict"][129] == SC.PARTNER and got["verdict"][127] == FB.REASON and got["rounds"] == 2
    lg.close()


def test_the_circuit_accepts_the_batch_select_keeps(hz):
    """rollup-main at (8, 16, 2, 4): a pool of eight with two rows above the bound (one per branch) and the "below" rows of the same
    selectors; what select keeps applies, and the HIP context and the oracle accept the inputs made from it"""
    st = R.wide_state()
    f0 = st.first_idx
    acc = SC.accounts(st)
    t = FB.float40_table()
    picks = [(31, t[31][1]), (191, t[191][2]), (191, t[191][1]), (255, t[255][2]), (255, t[255][1]), (100, R.f40(7, 2)), (192, t[192][1]), (224, t[224][1])]
    pool, seen = [], {}
    for i, (sel, f) in enumerate(picks):
        frm = f0 + 1 + i % 4
        pool.append(S.sign(st, R.txf(frm, f0 + 48 + i, f, sel, nonce=seen.get(frm, 0))))
        if not FB.fee_of(f, sel) >> 128:
            seen[frm] = seen.get(frm, 0) + 1
    lg = st.to_ledger(hz)
    like = types.SimpleNamespace(last_idx=f0 + st.N - 1, num_batch=0)
    (inp, _, nullified, exit_root, new_last), sel = B.ledger_select_batch_inputs(lg, like, [], pool, *SHAPE, [1], [f0 + R.WIDE_FEE], S.CHAIN_ID, verify=True)
    assert sel == SC.model(acc, [], pool, verify=True, max_keep=8)
    assert sel["verdict"] == [0, FB.REASON, 0, FB.REASON, 0, 0, 0, 0]
    g = hz.ctx("rollup-main", nTx=SHAPE[0], nLevels=SHAPE[1], maxL1Tx=SHAPE[2], maxFeeTx=SHAPE[3])
    g.set_inputs(inp)
    g.run()
    assert g.get("main.hashGlobalInputs") == B.hash_global_inputs(inp, nullified, new_last, lg.root(), exit_root, *SHAPE)
    o = OracleCtx("rollup-main", *SHAPE)
    o.set_inputs(inp)
    assert o.run() is None
    assert g.read_raw_bytes() == o.read_raw_bytes()
    lg.close()
