"""Atomic transactions on the device-resident ledger (hz_ledger_apply_batch_atomic, hz_ledger_verify_l2_atomic): the link
check of src/rq-tx-verifier.circom and the message with its rq fields, on ledgers of 16 accounts. Parity with hz_ledger_apply_batch_creates
where nothing links; RollupMain itself (the HIP context and the oracle) on the ledger's inputs with the links of tests/scenarios.py's
atomic_pair; every offset, accepted and with each rq field off by one; the places whose link fields are zero; a link across a wavefront
edge; the signature's commitment to the link; precedence among the refusal reasons and atomicity; the mempool filter. The model is
ledger_atomic_common's, itself checked against the oracle on the CPU."""
import types

import numpy as np
import pytest

import device_state_common as D
import ledger_atomic_common as Q
import ledger_common as C
import ledger_create_common as K
import ledger_sig_common as S
from circuits_amd import HzError
from circuits_amd import builder as B
from circuits_amd import capi

pytestmark = pytest.mark.gpu
N_LEVELS = 16
N_SIB = N_LEVELS + 1
PLAN, IDXS = [1], [0]


@pytest.fixture(scope="module")
def base():
    return C.base_state(4)


def _dense(hz, base):
    return base.to_ledger(hz)


def _growing(hz, base, room=4):
    return K.Accounts.of(base).to_ledger(hz, base.N + room, n_sib_max=N_SIB)


def _apply(lg, l1_txs, l2_txs, verify=False, **kw):
    return lg.apply_batch_atomic(l1_txs, l2_txs, PLAN, IDXS, S.CHAIN_ID, 1, n_sib=N_SIB, verify=verify, **kw)


def _refused(call, row, reason):
    with pytest.raises(HzError) as e:
        call()
    assert e.value.status == 4 and "index %d " % row in str(e.value) and "reason %d:" % reason in str(e.value), str(e.value)


def _same_bytes(a, b):
    assert set(a) == set(b), set(a) ^ set(b)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name


def _linked(base, n_l1, m, offsets, nop=None, signed_dest=False):
    """m transfers behind n_l1 rows, linked at offsets {i: k} with the fields their targets have, signed over them"""
    txs = Q.transfers(base, m, offsets=offsets, signed_dest=signed_dest)
    if nop is not None:
        txs[nop] = {}
    return Q.sign_all(base, Q.derive(n_l1, txs))


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("verify", [False, True])
@pytest.mark.parametrize("kind", ["dense", "growing"])
def test_without_links_every_output_is_apply_batch_creates(hz, base, kind, verify):
    make = _dense if kind == "dense" else _growing
    l1_txs, l2_txs = Q.deposits(base, 2), Q.sign_all(base, Q.transfers(base, 5)) + [{}]
    ref = make(hz, base)
    exp = ref.apply_batch_creates(l1_txs, l2_txs, PLAN, IDXS, S.CHAIN_ID, 1, n_sib=N_SIB, verify=verify)
    assert ("sig_l2_hash" in exp) == verify
    zeros = (capi.hz_l2rq * len(l2_txs))()
    for rq in (False, None, zeros):   # rq == NULL (asked for, and because no dictionary holds a link), and m entries of zeros
        lg = make(hz, base)
        got = _apply(lg, l1_txs, l2_txs, verify=verify, rq=rq)
        _same_bytes(got, exp)
        assert lg.root() == ref.root() and (lg.rq_ms() > 0.0) == (rq is zeros)
        lg.close()
    ref.close()


def test_without_sigs_the_link_fields_are_v2_and_zeros(hz, base):
    """sigs == NULL where hz_ledger_apply_batch_creates takes it (nothing verified, no receiver by address): zero rq entries give that
    call's outputs byte for byte, a pair linked by V2 alone is accepted, and the same pair with one V2 off by one is refused"""
    l1_txs, plain = Q.deposits(base, 2), Q.transfers(base, 4)
    ref, lg = _dense(hz, base), _dense(hz, base)
    exp = ref.apply_batch_creates(l1_txs, plain, PLAN, IDXS, S.CHAIN_ID, 1, n_sib=N_SIB, sigs=False)
    root = lg.root()
    pair = Q.derive(2, Q.transfers(base, 4, offsets={1: 1, 2: 7}))
    assert pair[1][Q.RQ_FIELDS[0]] and not pair[1][Q.RQ_FIELDS[1]] and not pair[1][Q.RQ_FIELDS[2]]
    _refused(lambda: _apply(lg, l1_txs, pair[:2] + [Q.off_by_one(pair[2], Q.RQ_FIELDS[0])] + pair[3:], sigs=False), 2 + 2, Q.REASON)
    assert lg.root() == root
    _same_bytes(_apply(lg, l1_txs, plain, sigs=False, rq=(capi.hz_l2rq * 4)()), exp)
    assert lg.root() == ref.root() and lg.rq_ms() > 0.0
    lg2 = _dense(hz, base)
    _same_bytes(_apply(lg2, l1_txs, pair, sigs=False), exp)   # the links change no output
    for x in (ref, lg, lg2):
        x.close()


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------------
def test_the_circuit_accepts_the_ledgers_inputs(hz, base):
    """rollup-main at (8, 16, 4, 4): two L1 deposits, then atomic_pair's links -- 0 requires the next (1), 1 the previous (7) and carries
    maxNumBatch and a signed toEthAddr / toBjjAy / toBjjSign, 2 the transaction three ahead (3), 4 the one two back (6) -- signed and
    verified on the device. ledger_atomic_batch_inputs == BatchBuilder's dictionary signal for signal; sig_l2_hash is build_hash_sig; the
    HIP context and the oracle accept; once more with every state-dependent signal left on the device"""
    from oracle_binding import OracleCtx
    shape = (8, N_LEVELS, 4, 4)
    f0 = base.first_idx
    a, b = f0, f0 + 1
    l1_txs = Q.deposits(base, 2)
    l2_txs = [dict(C.tx(a, b, 10, 50, nonce=0), rqOffset=1),
              dict(C.tx(b, a, 20, 60, nonce=0), rqOffset=7, maxNumBatch=5, toEthAddr=0xABCDEF << 100, toBjjAy=Q.P - 2, toBjjSign=1),
              dict(C.tx(a, b, 1, 0, nonce=1), rqOffset=3), C.tx(a, b, 2, 0, nonce=2), dict(C.tx(b, a, 3, 0, nonce=1), rqOffset=6), C.tx(b, a, 4, 0, nonce=2)]
    l2_txs = [dict(t, signer=S.signer(base, t["fromIdx"])) for t in l2_txs]
    fee_tokens, fee_idxs = [1], [f0 + 2]
    txs = [dict(t) for t in l1_txs] + [dict(t) for t in l2_txs]
    _, bb = C.builder_batch(base, txs, fee_tokens + [0] * 3, fee_idxs + [0] * 3, shape[1], max_l1=shape[2])
    exp = bb.get_input()
    assert exp["rqOffset"] == [0, 0, 1, 7, 3, 0, 6, 0] and exp["rqToBjjAy"][2] == Q.P - 2 and exp["rqToEthAddr"][2] == 0xABCDEF << 100
    assert exp["rqTxCompressedDataV2"][3] == exp["txCompressedDataV2"][2] and exp["rqTxCompressedDataV2"][4] == exp["txCompressedDataV2"][7]
    lg = _dense(hz, base)
    like = types.SimpleNamespace(last_idx=f0 + base.N - 1, num_batch=0)
    inp, _, nullified, exit_root, new_last = B.ledger_atomic_batch_inputs(lg, like, l1_txs, l2_txs, *shape, fee_tokens, fee_idxs, S.CHAIN_ID, verify=True)
    assert set(inp) == set(exp), set(inp) ^ set(exp)
    for name in exp:
        assert inp[name] == exp[name], name
    assert lg.rq_ms() > 0.0 and lg.root() == bb.new_state_root and new_last == like.last_idx == f0 + base.N - 1
    sig = lg.sig_outputs_dev()   # of the call ledger_atomic_batch_inputs made
    import torch

    class _Dev:
        def __init__(self, ptr, n):
            self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    hashes = torch.as_tensor(_Dev(sig["sig_l2_hash"], 32 * 6), device="cuda:0").cpu().numpy().reshape(6, 32)
    signed = [dict(t, **{f: exp[f][2 + i] for f in Q.RQ_FIELDS}) for i, t in enumerate(l2_txs)]
    assert [D.to_int(r) for r in hashes] == [B.build_hash_sig(t, S.CHAIN_ID) for t in signed]
    assert hashes[0].tobytes() != C.to_bytes([B.build_hash_sig(l2_txs[0], S.CHAIN_ID)]).tobytes()   # not the message with three zeros
    assert B.hash_global_inputs(inp, nullified, new_last, lg.root(), exit_root, *shape) == bb.get_hash_inputs()
    g = hz.ctx("rollup-main", nTx=shape[0], nLevels=shape[1], maxL1Tx=shape[2], maxFeeTx=shape[3])
    g.set_inputs(inp)
    g.run()
    assert g.get("main.hashGlobalInputs") == bb.get_hash_inputs()
    witness = g.read_raw_bytes()
    o = OracleCtx("rollup-main", *shape)
    o.set_inputs(inp)
    assert o.run() is None
    lg2 = _dense(hz, base)
    like = types.SimpleNamespace(last_idx=f0 + base.N - 1, num_batch=0)
    inp2, dev, _, _, _ = B.ledger_atomic_batch_inputs(lg2, like, l1_txs, l2_txs, *shape, fee_tokens, fee_idxs, S.CHAIN_ID, host_outputs=False, verify=True)
    assert set(inp2) | set(dev) == set(exp) and not set(inp2) & set(dev) and {"balance1", "siblings2", "imStateRoot"} <= set(dev)
    assert all(inp2[f] == exp[f] for f in ("rqOffset",) + Q.RQ_FIELDS)
    g.clear_inputs()
    g.set_inputs(inp2)
    for name, (ptr, count) in dev.items():
        g.set_input_dev(name, ptr, count)
    g.run()
    assert g.read_raw_bytes() == witness
    lg.close()
    lg2.close()


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(1, 8))
def test_every_offset(hz, base, k):
    """transaction 4 of 9, behind 3 L1 rows, links at k: accepted with its target's link fields and refused with reason 13 at row 7 with
    each of the three off by one, alone (signed over what is submitted: the signature is not the cause). k = 2 and k = 6: the oracle
    rejects BatchBuilder's inputs for the broken batches and accepts the good one"""
    n_l1, m, i = 3, 9, 4
    l1_txs = Q.deposits(base, n_l1)
    good = _linked(base, n_l1, m, {i: k}, signed_dest=True)   # every row signs a destination of its own: all three link fields are nonzero
    row = Q.target_row(n_l1 + i, k, n_l1, n_l1 + m)
    assert row == n_l1 + i + (k if k <= 3 else k - 8) and good[i][Q.RQ_FIELDS[0]] == B.build_tx_compressed_data_v2(good[row - n_l1])
    assert (good[i][Q.RQ_FIELDS[1]], good[i][Q.RQ_FIELDS[2]]) == (good[row - n_l1]["toEthAddr"], good[row - n_l1]["toBjjAy"]) and good[i][Q.RQ_FIELDS[1]] > 1 << 150
    neighbours = []
    for j in (row - n_l1 - 1, row - n_l1 + 1):   # the fields of the target's neighbours are refused: a lane that read the wrong entry would show
        wrong = list(good)
        wrong[i] = S.sign(base, dict(good[i], **dict(zip(Q.RQ_FIELDS[1:], Q.link_fields(good[j])[1:]))))
        assert Q.first_refusal(n_l1, wrong) == (n_l1 + i, Q.REASON)
        neighbours.append(wrong)
    lg = _dense(hz, base)
    root = lg.root()
    shape = (12, N_LEVELS, 3, 2)
    for wrong in neighbours:
        _refused(lambda: _apply(lg, l1_txs, wrong, verify=True), n_l1 + i, Q.REASON)
    for f in Q.RQ_FIELDS:
        bad = list(good)
        bad[i] = S.sign(base, Q.off_by_one(good[i], f))
        assert Q.first_refusal(n_l1, bad) == (n_l1 + i, Q.REASON)
        _refused(lambda: _apply(lg, l1_txs, bad, verify=True), n_l1 + i, Q.REASON)
        _refused(lambda: _apply(lg, l1_txs, bad), n_l1 + i, Q.REASON)   # the same without the flag: the V2 rows of the packing alone
        assert lg.root() == root
        if k in (2, 6) and f == Q.RQ_FIELDS[0]:
            assert not Q.oracle_accepts(Q.builder_inputs(base, l1_txs, bad, shape), shape)
    assert Q.first_refusal(n_l1, good) is None
    got = _apply(lg, l1_txs, good, verify=True)
    assert D.to_int(got["sig_l2_hash"][i]) == B.build_hash_sig(good[i], S.CHAIN_ID) and lg.root() != root and lg.rq_ms() > 0.0
    if k in (2, 6):
        assert Q.oracle_accepts(Q.builder_inputs(base, l1_txs, good, shape), shape)
    lg.close()


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------------
ZERO_CASES = {   # name: (n_l1, transaction, its offset, a transaction made a NOP)
    "offset 0": (2, 1, 0, None), "before row 0": (0, 0, 7, None), "past the last row": (2, 3, 2, None), "an L1 row": (2, 0, 7, None), "an L2 NOP": (2, 1, 1, 2)}


@pytest.mark.parametrize("name", sorted(ZERO_CASES))
def test_a_link_at_nothing_holds_iff_the_rq_fields_are_zero(hz, base, name):
    n_l1, i, k, nop = ZERO_CASES[name]
    l1_txs = Q.deposits(base, n_l1)
    good = _linked(base, n_l1, 4, {i: k} if k else None, nop=nop)
    assert Q.link_target(n_l1, good, i) == -1 and good[i].get("rqOffset", 0) == k and not any(good[i].get(f, 0) for f in Q.RQ_FIELDS)
    lg = _dense(hz, base)
    root = lg.root()
    shape = (8, N_LEVELS, 2, 2)
    for f in Q.RQ_FIELDS:
        bad = list(good)
        bad[i] = S.sign(base, dict(good[i], **{f: 1}))
        _refused(lambda: _apply(lg, l1_txs, bad, verify=(f == Q.RQ_FIELDS[1])), n_l1 + i, Q.REASON)
        assert lg.root() == root
    assert not Q.oracle_accepts(Q.builder_inputs(base, l1_txs, bad, shape), shape)   # the last of them
    _apply(lg, l1_txs, good, verify=True)
    assert lg.root() != root
    assert Q.oracle_accepts(Q.builder_inputs(base, l1_txs, good, shape), shape)
    lg.close()


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------------
def test_a_link_across_the_wavefront_edge(hz, base):
    """n_l1 = 3, m = 70: transaction 63 links forward to 64, 64 back to 63 -- lanes of two wavefronts, and rows that are not the lanes'
    indices. With 64's amount changed after 63 committed to it, 63's link is broken at row 3 + 63; 64's own link still holds"""
    n_l1, m = 3, 70
    l1_txs = Q.deposits(base, n_l1)
    good = _linked(base, n_l1, m, {63: 1, 64: 7}, signed_dest=True)
    lg = _dense(hz, base)
    root = lg.root()
    bad = list(good)
    bad[64] = S.sign(base, dict(good[64], amountF=good[64]["amountF"] + 1))
    assert Q.verdicts(n_l1, bad) == [Q.REASON if j == 63 else 0 for j in range(m)]
    _refused(lambda: _apply(lg, l1_txs, bad, verify=True), n_l1 + 63, Q.REASON)
    _refused(lambda: _apply(lg, l1_txs, bad), n_l1 + 63, Q.REASON)
    for f, key in zip(Q.RQ_FIELDS[1:], ("toEthAddr", "toBjjAy")):   # 63 committed to 64's signed destination; 62's or 65's is not it
        for j in (62, 65):
            wrong = list(good)
            wrong[63] = S.sign(base, dict(good[63], **{f: good[j][key]}))
            _refused(lambda: _apply(lg, l1_txs, wrong, verify=True), n_l1 + 63, Q.REASON)
    assert lg.root() == root
    got = _apply(lg, l1_txs, good, verify=True)
    assert [D.to_int(got["sig_l2_hash"][j]) for j in (63, 64)] == [B.build_hash_sig(good[j], S.CHAIN_ID) for j in (63, 64)]
    assert D.to_int(got["tx_compressed_data_v2"][64]) == good[63][Q.RQ_FIELDS[0]] and lg.root() != root
    lg.close()


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------------
def test_the_signature_commits_to_the_link(hz, base):
    """signed over zero rq fields, submitted with the matching nonzero ones: the link holds, the signature does not"""
    n_l1 = 2
    l1_txs = Q.deposits(base, n_l1)
    good = _linked(base, n_l1, 4, {0: 1, 1: 7})
    unsigned_link = dict(good[0])
    unsigned_link.update(S.sign(base, {k: v for k, v in good[0].items() if k not in Q.RQ_FIELDS}))   # s, r8x, r8y over three zeros
    assert [unsigned_link[f] for f in S.SIG_FIELDS] != [good[0][f] for f in S.SIG_FIELDS] and all(unsigned_link[f] == good[0][f] for f in Q.RQ_FIELDS)
    txs = [unsigned_link] + good[1:]
    assert Q.first_refusal(n_l1, txs) is None
    lg = _dense(hz, base)
    root = lg.root()
    _refused(lambda: _apply(lg, l1_txs, txs, verify=True), n_l1, 7)
    assert lg.root() == root
    _apply(lg, l1_txs, txs)
    assert lg.root() != root
    lg.close()


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------------
def test_precedence_and_atomicity(hz, base):
    """on a growing ledger, in a batch with a create row and an exit: 2 and 13 on one row give 2; 13 on a lower row beats 3 on a higher
    one; 9 on a higher row still comes first. Nothing resident changes, and the valid batch then gives what a fresh ledger gives"""
    f0, n_l1 = base.first_idx, 2
    l1_txs = [K.create_for(K.account(0), load=10 ** 6), Q.deposits(base, 1)[0]]
    good = Q.derive(n_l1, Q.transfers(base, 5, offsets={1: 1, 2: 7}) + [C.tx(f0 + 9, K.EXIT, 2, 0, nonce=0)])
    broken = Q.off_by_one(good[1], Q.RQ_FIELDS[2])
    lg = _growing(hz, base)
    everyone = np.arange(f0, f0 + base.N)
    root, fields = lg.root(), lg.accounts(everyone)

    def unchanged():
        assert lg.root() == root and (lg.accounts(everyone) == fields).all() and lg.size() == base.N and lg.last_idx() == f0 + base.N - 1
        assert lg.exit_tree().size() == 0 and lg.exit_tree().root() == 0 and lg.state_smt().size() == base.N
        with pytest.raises(HzError):
            lg.outputs_dev()
    into = {name: np.full(shape, 0xA5, dtype=np.uint8) for name, shape in lg.shapes(n_l1 + len(good), 1, N_SIB)}
    _refused(lambda: _apply(lg, l1_txs, good[:1] + [dict(broken, nonce=broken["nonce"] + 3)] + good[2:], into=dict(into)), n_l1 + 1, 2)
    unchanged()
    assert all((a == 0xA5).all() for a in into.values())   # no output was written
    poor = dict(good[4], amountF=B.floor_fix2float(base.state(good[4]["fromIdx"])["balance"] * 4))
    _refused(lambda: _apply(lg, l1_txs, good[:1] + [broken] + good[2:4] + [poor] + good[5:]), n_l1 + 1, Q.REASON)
    unchanged()
    _refused(lambda: _apply(lg, l1_txs, good[:1] + [broken] + good[2:4] + [poor] + good[5:], verify=True), n_l1, 7)   # unsigned: row 2 first
    unchanged()
    nobody = dict(C.tx(f0 + 4, 0, 5, 0, nonce=0), toEthAddr=0x1234567)
    _refused(lambda: _apply(lg, l1_txs, good[:1] + [broken] + good[2:4] + [nobody] + good[5:]), n_l1 + 4, 9)
    unchanged()
    got = _apply(lg, l1_txs, good)
    fresh = _growing(hz, base)
    exp = fresh.apply_batch_creates(l1_txs, [{k: v for k, v in t.items() if k not in Q.RQ_FIELDS + ("rqOffset",)} for t in good], PLAN, IDXS, S.CHAIN_ID, 1, n_sib=N_SIB)
    _same_bytes(got, exp)
    assert lg.root() == fresh.root() != root and lg.size() == base.N + 1 and lg.exit_tree().root() == fresh.exit_tree().root() != 0
    lg.close()
    fresh.close()


# ---- 8 -----------------------------------------------------------------------------------------------------------------------------------
def test_verify_l2_atomic(hz, base):
    """one mixed list at current_num_batch = 5: a good pair, a broken link (13), a forged signature beside a broken link (7), an expired
    maxNumBatch beside one (8), a plain transfer; nothing resident changes. With zero rq fields the verdicts and arrays are verify_l2's"""
    current = 5
    txs = Q.derive(0, Q.transfers(base, 6, offsets={0: 1, 1: 7, 2: 1, 3: 7, 4: 3}))
    txs[2] = Q.off_by_one(txs[2], Q.RQ_FIELDS[0])
    txs[3] = Q.off_by_one(txs[3], Q.RQ_FIELDS[1])
    txs[4] = dict(txs[4], maxNumBatch=2, rqToBjjAy=77)   # row 7 does not exist: zeros are wanted
    txs = Q.sign_all(base, txs)
    txs[3] = S.forge(txs[3], "s")
    cols = base.leaf_fields()
    sig, link = S.verdicts(txs, cols, base.first_idx, current), Q.verdicts(0, txs)
    assert sig == [0, 0, 0, 7, 8, 0] and link == [0, 0, 13, 13, 13, 0]
    lg = _dense(hz, base)
    root = lg.root()
    got, arrays = lg.verify_l2_atomic(txs, S.CHAIN_ID, current, outputs=True)
    assert got.tolist() == [s or q for s, q in zip(sig, link)] == [0, 0, 13, 7, 8, 0] and lg.rq_ms() > 0.0 and lg.root() == root
    C.assert_same(arrays, S.expected_sig_arrays(txs))
    assert hz.ledger_plan_atomic(0, txs)["verdict"] == link   # the host's routines agree with the kernel's
    plain = Q.sign_all(base, Q.transfers(base, 6)) + [{}]
    plain[1] = S.forge(plain[1], "r8")
    exp, exp_arrays = lg.verify_l2(plain, S.CHAIN_ID, current, outputs=True)
    assert exp.tolist() == [0, 7, 0, 0, 0, 0, 0]
    for rq in (None, (capi.hz_l2rq * len(plain))()):
        got, arrays = lg.verify_l2_atomic(plain, S.CHAIN_ID, current, outputs=True, rq=rq)
        assert got.tobytes() == exp.tobytes()
        _same_bytes(arrays, exp_arrays)
    lg.close()


# ---- 9 -----------------------------------------------------------------------------------------------------------------------------------
def test_into_fills_the_callers_arrays_with_what_a_fresh_call_returns(hz, base):
    """a create, a deposit, a linked pair of transfers and an exit, verified, on a growing ledger of capacity 32 that holds 16 accounts, 7
    siblings: once into fresh arrays, then on the reloaded ledger into arrays of the caller's that hold 0xAA everywhere, one optional
    name missing among them -- the same arrays come back, the missing one beside them, every byte as in the fresh call"""
    acc = K.Accounts.of(base)
    lg = acc.to_ledger(hz, 32, n_sib_max=7)
    l1_txs = [K.create_for(K.account(0), load=50), Q.deposits(base, 1)[0]]
    txs = Q.transfers(base, 3, offsets={0: 1, 1: 7})
    txs[2]["toIdx"] = B.EXIT_IDX
    l2_txs = Q.sign_all(base, Q.derive(len(l1_txs), txs))

    def call(**kw):
        return lg.apply_batch_atomic(l1_txs, l2_txs, PLAN, IDXS, S.CHAIN_ID, 1, n_sib=7, verify=True, **kw)
    fresh = call()
    root = lg.root()
    every = [name for name, _, _ in capi.LEDGER_ARRAYS] + list(capi.LEDGER_SIG_ARRAYS) + ["auxToIdx", "l1_flags"] + list(capi.LEDGER_EXIT_ARRAYS + capi.LEDGER_CREATE_ARRAYS)
    assert list(fresh) == every and fresh["siblings1"].shape == (5, 7, 32)
    assert fresh["new_exit"][4].any() and fresh["aux_from_idx"][0].any() and fresh["sig_l2_hash"].any() and lg.rq_ms() > 0.0   # each kind of row did its work
    lg.load_accounts(*acc.cols())
    into = {name: np.full_like(a, 0xAA) for name, a in fresh.items() if name != "exit_root_after"}
    got = call(into=into)
    assert lg.root() == root and list(got) == every
    assert all(got[name] is into[name] for name in into) and got["exit_root_after"].shape == (5, 32)
    _same_bytes(got, fresh)
    lg.close()
