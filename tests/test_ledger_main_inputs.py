"""RollupMain's packed inputs of an applied batch, written on the device (hz_ledger_main_inputs), on ledgers of 16 accounts:
byte equality with capi.pack_inputs over the dictionary builder.ledger_*_batch_inputs(host_outputs=True) gives on a twin ledger, for every
kind of apply call that carries a chain id, verified and unverified; the field edges of the computed rows; rows across wavefront and block
edges; a signal without rows; the circuit itself on a staged buffer; two batches in two slots of one buffer; residency and the refusals.
Transactions are signed before they reach either route, so the unverified route sees the same s, r8x and r8y as the verified one.
hz_ledger_apply_l2_signed exists only verified (unverified it is hz_ledger_apply_l2, which has no chain id and is refused)."""
import types

import numpy as np
import pytest

import ledger_addr_common as A
import ledger_atomic_common as Q
import ledger_common as C
import ledger_create_common as K
import ledger_exit_common as X
import ledger_l1_common as L1
import ledger_main_inputs_common as M
import ledger_sig_common as S
from circuits_amd import HzError
from circuits_amd import builder as B
from circuits_amd import capi

pytestmark = pytest.mark.gpu
SHAPE = (8, 16, 4, 4)
N_SIB = SHAPE[1] + 1
P = B.P
EDGE_KEY = (P - 1) | 1 << 254 | 1 << 255   # bits 254 and 255 set over the ay bits of r - 1


@pytest.fixture(scope="module")
def base():
    return C.base_state(4)


@pytest.fixture(scope="module")
def ctx(hz):
    g = hz.ctx("rollup-main", nTx=SHAPE[0], nLevels=SHAPE[1], maxL1Tx=SHAPE[2], maxFeeTx=SHAPE[3])
    yield g
    g.close()


def _dense(hz, st):
    return st.to_ledger(hz)


def _growing(hz, st, room=4):
    return K.Accounts.of(st).to_ledger(hz, st.N + room, n_sib_max=N_SIB)


def _like(st):
    return types.SimpleNamespace(last_idx=st.first_idx + st.N - 1, num_batch=0)


def _signed(st, l2_txs, n_l1=0, chain_id=S.CHAIN_ID):
    """the rq fields of linked transactions derived, then every active transaction signed by its sender's key: explicit on both routes"""
    return [S.sign(st, t, chain_id) for t in Q.derive(n_l1, l2_txs)]


def _device_bytes(ptr, n):
    import torch

    class _Dev:
        def __init__(self, ptr, n):
            self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    return torch.as_tensor(_Dev(ptr, n), device="cuda:0").cpu().numpy().tobytes()


def _packed(lg, g, old_last):
    addr, nbytes, buf = lg.main_inputs(g, old_last)
    assert nbytes == g.packed_layout()[0] and buf.numel() == nbytes and lg.main_inputs_ms() > 0.0
    return buf.cpu().numpy().tobytes()


def _same(g, got, inp):
    lay = g.packed_layout()
    exp = capi.pack_inputs(lay, inp)
    assert M.first_difference(lay, got, exp) is None, M.first_difference(lay, got, exp)


# ---- the batches of test 1: name -> (the state, dense or growing, the builder's route, L1 rows, L2 rows) --------------------------------
def _atomic_rows(base):
    """tests/test_ledger_atomic.py::test_the_circuit_accepts_the_ledgers_inputs: two deposits, then atomic_pair's links"""
    a, b = base.first_idx, base.first_idx + 1
    l2 = [dict(C.tx(a, b, 10, 50, nonce=0), rqOffset=1),
          dict(C.tx(b, a, 20, 60, nonce=0), rqOffset=7, maxNumBatch=5, toEthAddr=0xABCDEF << 100, toBjjAy=Q.P - 2, toBjjSign=1),
          dict(C.tx(a, b, 1, 0, nonce=1), rqOffset=3), C.tx(a, b, 2, 0, nonce=2), dict(C.tx(b, a, 3, 0, nonce=1), rqOffset=6), C.tx(b, a, 4, 0, nonce=2)]
    return Q.deposits(base, 2), l2


def _case(name, base):
    f0 = base.first_idx
    if name == "apply_l2_signed":
        return base, "dense", "l2", [], Q.transfers(base, 3, signed_dest=True) + [{}] + Q.transfers(base, 3, start=5)
    if name == "apply_l2_addr":
        sp = A.special_state(4)
        txs = [C.tx(f0, f0 + 1, 9, 1, nonce=0), A.to_addr(C.tx(f0 + 1, 0, 5, 0, nonce=0), sp.state(f0 + 7)), A.to_addr(C.tx(f0 + 3, 0, 6, 0, nonce=0), sp.state(sp.any_a)),
               {}, C.tx(f0 + 4, f0 + 6, 0, 0, nonce=0)]
        return sp, "dense", "l2", [], txs
    if name == "apply_batch":
        l1 = Q.deposits(base, 2) + [L1.own(base, f0 + 3, f0 + 4, 5)]
        return base, "dense", "batch", l1, Q.transfers(base, 2, start=6, signed_dest=True) + [{}] + Q.transfers(base, 1, start=9)
    if name == "apply_batch_exits":
        l1 = [L1.own(base, f0 + 2, 0, 0, 11), X.fx(base, f0 + 5, 3)]
        return base, "dense", "exits", l1, [C.tx(f0, f0 + 1, 4, 1, nonce=0), X.x2(f0 + 1, 4, nonce=0), {}, X.x2(f0 + 5, 2, nonce=0)]
    if name == "apply_batch_creates":
        l1 = [K.create(EDGE_KEY, token=1, eth=0xC0FFEE << 96, load=10 ** 6), L1.own(base, f0 + 1, 0, 0, 7), K.create_for(K.account(3), load=5)]
        return base, "growing", "creates", l1, [C.tx(f0, f0 + base.N, 4, 1, nonce=0), {}, C.tx(f0 + 2, f0 + 3, 1, 0, nonce=0)]
    if name == "creates_call_without_a_create_row":   # from_bjj == NULL on the call that takes keys
        return base, "growing", "creates", Q.deposits(base, 2), Q.transfers(base, 3, start=4)
    assert name == "apply_batch_atomic"
    return (base, "growing", "atomic") + _atomic_rows(base)


ROUTES = {"l2": B.l2_batch_inputs, "batch": B.ledger_batch_inputs, "exits": B.ledger_exit_batch_inputs, "creates": B.ledger_create_batch_inputs,
          "atomic": B.ledger_atomic_batch_inputs}
CASES = ["apply_l2_signed", "apply_l2_addr", "apply_batch", "apply_batch_exits", "apply_batch_creates", "creates_call_without_a_create_row", "apply_batch_atomic"]


def _route(route, lg, like, l1, l2, shape, fee_tokens, fee_idxs, chain_id, host_outputs, verify):
    if route == "l2":
        return B.l2_batch_inputs(lg, like, l2, *shape, fee_tokens, fee_idxs, chain_id, host_outputs=host_outputs, verify=verify)
    return ROUTES[route](lg, like, l1, l2, *shape, fee_tokens, fee_idxs, chain_id, host_outputs=host_outputs, verify=verify)


def _both(hz, g, st, kind, route, l1, l2, shape, fee_tokens, fee_idxs, chain_id, verify):
    """ledger A through the builder and pack_inputs, ledger B through the same apply and main_inputs -> (the dictionary, B's bytes, B)"""
    make = _dense if kind == "dense" else _growing
    lg_a, lg_b = make(hz, st), make(hz, st)
    like_a, like_b = _like(st), _like(st)
    inp = _route(route, lg_a, like_a, l1, l2, shape, fee_tokens, fee_idxs, chain_id, True, verify)[0]
    _route(route, lg_b, like_b, l1, l2, shape, fee_tokens, fee_idxs, chain_id, False, verify)
    got = _packed(lg_b, g, _like(st).last_idx)
    assert lg_a.root() == lg_b.root() and like_a.last_idx == like_b.last_idx == lg_b.last_idx()
    lg_a.close()
    return inp, got, lg_b


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------------
# (apply_l2_signed unverified is hz_ledger_apply_l2: no chain id, refused -- test_refusals_leave_the_buffer_untouched)
@pytest.mark.parametrize("name,verify", [(n, v) for n in CASES for v in (False, True) if v or n != "apply_l2_signed"])
def test_byte_equality_for_every_kind_of_call(hz, ctx, base, name, verify):
    st, kind, route, l1, l2 = _case(name, base)
    inp, got, lg = _both(hz, ctx, st, kind, route, l1, _signed(st, l2, len(l1)), SHAPE, [1], [st.first_idx + 2], S.CHAIN_ID, verify)
    _same(ctx, got, inp)
    if name == "apply_batch_creates":
        assert inp["fromIdx"][0] == 0 and inp["newAccount"][:3] == [1, 0, 1] and inp["fromBjjCompressed"][0][254:] == [1, 1] and inp["auxFromIdx"][0] == st.first_idx + st.N
    if name == "apply_batch_atomic":
        assert inp["rqOffset"] == [0, 0, 1, 7, 3, 0, 6, 0]
    lg.close()


def test_byte_equality_without_sigs(hz, ctx, base):
    """sigs == NULL where hz_ledger_apply_batch takes it: the signed destination and the signature are zeros"""
    l1, l2 = Q.deposits(base, 2), Q.transfers(base, 4) + [{}, {}]
    plan, idxs = [1, 0, 0, 0], [base.first_idx + 2, 0, 0, 0]
    lg_a, lg_b = _dense(hz, base), _dense(hz, base)
    inp = B.ledger_batch_inputs(lg_a, _like(base), l1, l2, *SHAPE, [1], [base.first_idx + 2], S.CHAIN_ID)[0]
    lg_b.apply_batch(l1, l2, plan, idxs, S.CHAIN_ID, 1, n_sib=N_SIB, outputs=False, sigs=False)
    _same(ctx, _packed(lg_b, ctx, _like(base).last_idx), inp)
    assert inp["s"] == [0] * 8 and lg_a.root() == lg_b.root()
    lg_a.close()
    lg_b.close()


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------------
def test_field_edges_in_the_computed_rows(hz):
    """chain id 0xFFFF, a token id with bit 31, amountF and loadAmountF 2^40 - 1, maxNumBatch 2^32 - 1, toBjjSign 1, userFee 255 at a small
    amount, fromEthAddr and toEthAddr 2^160 - 1, an s with its top limb set; nonces 2^40 - 2 and account indices just below 2^48"""
    token, chain, top = 0x80000001, 0xFFFF, (1 << 40) - 1
    f0 = (1 << 48) - 64
    keys = [K.account(200 + j) for j in range(16)]
    leaves = [{"tokenID": token, "nonce": (1 << 40) - 2, "sign": a.sign, "balance": 10 ** 50, "ay": a.ay, "ethAddr": (1 << 160) - 1 if j == 1 else a.eth_addr}
              for j, a in enumerate(keys)]
    acc = K.Accounts(leaves, first_idx=f0)
    shape = (8, 16, 4, 4)
    l1 = [{"onChain": 1, "fromIdx": f0 + 1, "toIdx": f0 + 2, "amountF": top, "loadAmountF": top, "tokenID": token, "fromEthAddr": (1 << 160) - 1},
          K.create(EDGE_KEY, token=token, eth=(1 << 160) - 1, load=1)]
    edge = {"maxNumBatch": (1 << 32) - 1, "toBjjSign": 1, "toEthAddr": (1 << 160) - 1, "toBjjAy": P - 1, "s": P - 1, "r8x": P - 2, "r8y": (1 << 253) + 5}
    l2 = [dict(C.tx(f0 + 3, f0 + 15, 0, 0, token=token, nonce=(1 << 40) - 2), amountF=top, **edge),
          dict(C.tx(f0 + 4, f0 + 5, 3, 255, token=token, nonce=(1 << 40) - 2), **edge), {},
          dict(C.tx(f0 + 15, f0 + 3, 1, 1, token=token, nonce=(1 << 40) - 2), s=1 << 253, r8x=7, r8y=9)]
    g = hz.ctx("rollup-main", nTx=shape[0], nLevels=shape[1], maxL1Tx=shape[2], maxFeeTx=shape[3])
    lg_a, lg_b = acc.to_ledger(hz, 20, n_sib_max=N_SIB), acc.to_ledger(hz, 20, n_sib_max=N_SIB)
    like_a, like_b = types.SimpleNamespace(last_idx=f0 + 15, num_batch=(1 << 32) - 2), types.SimpleNamespace(last_idx=f0 + 15, num_batch=(1 << 32) - 2)
    inp = B.ledger_atomic_batch_inputs(lg_a, like_a, l1, l2, *shape, [token], [f0 + 7], chain)[0]
    B.ledger_atomic_batch_inputs(lg_b, like_b, l1, l2, *shape, [token], [f0 + 7], chain, host_outputs=False)
    got = _packed(lg_b, g, f0 + 15)
    _same(g, got, inp)
    assert inp["txCompressedData"][2] >> 216 == 0x100 and inp["txCompressedData"][3] >> 216 == 0x1FF and inp["globalChainID"] == chain
    assert inp["currentNumBatch"] == (1 << 32) - 1 and inp["amountF"][0] == inp["loadAmountF"][0] == inp["amountF"][2] == top and inp["fromIdx"][2] == f0 + 3
    assert lg_a.root() == lg_b.root() and lg_b.last_idx() == f0 + 16
    for x in (lg_a, lg_b, g):
        x.close()


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------------
def _wide_l2(base, m, nops):
    out = Q.transfers(base, m, amount=1)
    for i, t in enumerate(out):
        t.update(s=3 * i + 1, r8x=5 * i + 2, r8y=7 * i + 3, toBjjAy=P - 9 - i, toEthAddr=(0xBEEF << 120) + i, maxNumBatch=1000 + i, toBjjSign=i & 1)
    for i in nops:
        out[i] = {}
    nonce = {}
    for t in out:   # the nonces counted over what is left
        if t:
            t["nonce"] = nonce.get(t["fromIdx"], 0)
            nonce[t["fromIdx"]] = t["nonce"] + 1
    return out


@pytest.mark.parametrize("run", ["l1_66_l2_64", "no_l1", "every_l2_a_nop"])
def test_row_and_lane_edges(hz, base, run):
    """(130, 16, 66, 4), packed bytes only. 66 L1 rows -- creates at rows 0, 63, 64 and 65, so key bits and L1 packing cross lanes 63 / 64 /
    65 -- and 64 L2 rows, so the rows cross 127 / 128 / 129; the NOPs lie at rows 127, 128 and the last row (L2 rows 61 .. 63: a batch of 66
    L1 rows has no L2 row 64), and in the run without L1 rows at rows 63, 64 and the last row; once with every L2 row a NOP"""
    shape = (130, 16, 66, 4)
    f0 = base.first_idx
    creates = (0, 63, 64, 65)
    l1 = [K.create((P - 7 - r) | (r & 1) << 255 | 1 << 254, token=1, eth=(0xFACE << 100) + r, load=r + 1) if r in creates else
          L1.own(base, f0 + r % 16, f0 + (r + 5) % 16 if r % 3 == 0 else 0, r % 4 if r % 3 == 0 else 0, r) for r in range(66)]
    if run == "no_l1":
        l1, l2 = [], _wide_l2(base, 130, (63, 64, 129))
    elif run == "every_l2_a_nop":
        l2 = [{} for _ in range(64)]
    else:
        l2 = _wide_l2(base, 64, (61, 62, 63))
    g = hz.ctx("rollup-main", nTx=shape[0], nLevels=shape[1], maxL1Tx=shape[2], maxFeeTx=shape[3])
    lg_a, lg_b = _growing(hz, base, room=8), _growing(hz, base, room=8)
    inp = B.ledger_atomic_batch_inputs(lg_a, _like(base), l1, l2, *shape, [1], [f0 + 2], S.CHAIN_ID)[0]
    B.ledger_atomic_batch_inputs(lg_b, _like(base), l1, l2, *shape, [1], [f0 + 2], S.CHAIN_ID, host_outputs=False)
    _same(g, _packed(lg_b, g, _like(base).last_idx), inp)
    assert lg_a.root() == lg_b.root() and sum(inp["newAccount"]) == (4 if l1 else 0) and len(inp["fromIdx"]) == 130
    for x in (lg_a, lg_b, g):
        x.close()


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------------
def test_a_signal_without_rows(hz, base):
    """maxFeeTx = 1, shape (3, 16, 2, 1): imStateRootFee has no rows. Byte equality, and the context runs on the staged buffer"""
    shape = (3, 16, 2, 1)
    f0 = base.first_idx
    l1, l2 = Q.deposits(base, 1), _signed(base, [C.tx(f0 + 1, f0 + 2, 5, 1, nonce=0)], 1)
    g = hz.ctx("rollup-main", nTx=shape[0], nLevels=shape[1], maxL1Tx=shape[2], maxFeeTx=shape[3])
    assert dict(g.input_names())["imStateRootFee"] == 0
    lg_a, lg_b = _dense(hz, base), _dense(hz, base)
    inp, _, nullified, exit_root = B.ledger_exit_batch_inputs(lg_a, _like(base), l1, l2, *shape, [1], [f0 + 3], S.CHAIN_ID, verify=True)
    B.ledger_exit_batch_inputs(lg_b, _like(base), l1, l2, *shape, [1], [f0 + 3], S.CHAIN_ID, host_outputs=False, verify=True)
    addr, nbytes, buf = lg_b.main_inputs(g, _like(base).last_idx)
    _same(g, buf.cpu().numpy().tobytes(), inp)
    g.stage(0, addr, nbytes)
    g.run()
    assert g.get("main.hashGlobalInputs") == B.hash_global_inputs(inp, nullified, _like(base).last_idx, lg_b.root(), exit_root, *shape)
    for x in (lg_a, lg_b, g):
        x.close()


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------------
def test_the_circuit_accepts_the_packed_batch(hz, ctx, base):
    """case 1's atomic batch through builder.ledger_packed_batch: the staged context runs, hashGlobalInputs is BatchBuilder's, the witness
    is the one the same batch gives through set_inputs, and the oracle accepts the dictionary"""
    from oracle_binding import OracleCtx
    f0 = base.first_idx
    l1, l2 = _atomic_rows(base)
    l2 = [dict(t, signer=S.signer(base, t["fromIdx"])) for t in l2]
    fee_tokens, fee_idxs = [1], [f0 + 2]
    _, bb = C.builder_batch(base, [dict(t) for t in l1] + [dict(t) for t in l2], fee_tokens + [0] * 3, fee_idxs + [0] * 3, SHAPE[1], max_l1=SHAPE[2])
    lg_a = _growing(hz, base)
    inp = B.ledger_atomic_batch_inputs(lg_a, _like(base), l1, l2, *SHAPE, fee_tokens, fee_idxs, S.CHAIN_ID, verify=True)[0]
    ctx.clear_inputs()
    ctx.set_inputs(inp)
    ctx.run()
    assert ctx.get("main.hashGlobalInputs") == bb.get_hash_inputs()
    witness = ctx.read_raw_bytes()
    lg_b, like = _growing(hz, base), _like(base)
    ctx.clear_inputs()
    addr, nullified, exit_root, new_last = B.ledger_packed_batch(lg_b, ctx, like, l1, l2, fee_tokens, fee_idxs, S.CHAIN_ID, verify=True)
    ctx.run()
    assert ctx.get("main.hashGlobalInputs") == bb.get_hash_inputs() and ctx.read_raw_bytes() == witness
    assert (nullified, exit_root, new_last) == ([0] * 8, 0, f0 + base.N - 1) and like.num_batch == 1 and lg_b.root() == lg_a.root() == bb.new_state_root
    assert _device_bytes(addr, ctx.packed_layout()[0]) == capi.pack_inputs(ctx.packed_layout(), inp)
    o = OracleCtx("rollup-main", *SHAPE)
    o.set_inputs(inp)
    assert o.run() is None
    lg_a.close()
    lg_b.close()


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------------
def test_two_batches_in_two_slots(hz, base):
    """a context of two instances: batch 1 packed into slot 0 of one buffer, batch 2 -- applied on the state batch 1 left -- into slot 1, one
    stage_range, one run: both instances' hashGlobalInputs are the BatchBuilder chain's, and slot 0 is unchanged by the second apply"""
    import torch
    f0 = base.first_idx
    fee_tokens, fee_idxs = [1], [f0 + 2]
    plan, idxs = fee_tokens + [0] * 3, fee_idxs + [0] * 3
    l1_1, l2_1 = _atomic_rows(base)
    l1_2, l2_2 = [L1.own(base, f0 + 12, 0, 0, 9)], Q.transfers(base, 5, start=4)
    db, hashes = None, []
    for l1, l2 in ((l1_1, l2_1), (l1_2, l2_2)):
        rows = [dict(t) for t in l1] + [dict(t, signer=S.signer(base, t["fromIdx"])) for t in l2]
        db, bb = C.builder_batch(base, rows + [{} for _ in range(SHAPE[0] - len(rows))], plan, idxs, SHAPE[1], db=db, max_l1=SHAPE[2])
        hashes.append(bb.get_hash_inputs())
    g = hz.ctx("rollup-main", nTx=SHAPE[0], nLevels=SHAPE[1], maxL1Tx=SHAPE[2], maxFeeTx=SHAPE[3], n_instances=2)
    nbytes = g.packed_layout()[0]
    buf = torch.zeros(2 * nbytes, dtype=torch.uint8, device="cuda:0")
    lg, last = _dense(hz, base), f0 + base.N - 1
    slot0 = None
    for k, (l1, l2) in enumerate(((l1_1, l2_1), (l1_2, l2_2))):
        padded = _signed(base, l2, len(l1)) + [{} for _ in range(SHAPE[0] - len(l1) - len(l2))]
        lg.apply_resident(l1, padded, plan, idxs, S.CHAIN_ID, k + 1, n_sib=N_SIB, verify=True, atomic=True)
        lg.main_inputs(g, last, d_packed=buf.data_ptr() + k * nbytes)
        if k == 0:
            slot0 = buf[:nbytes].cpu().numpy().tobytes()
    assert buf[:nbytes].cpu().numpy().tobytes() == slot0 and buf[nbytes:].cpu().numpy().tobytes() != slot0
    g.stage_range(0, 2, buf.data_ptr(), nbytes)
    g.run()
    assert [g.get("main.hashGlobalInputs", instance=i) for i in range(2)] == hashes and hashes[0] != hashes[1]
    assert lg.root() == db.state.root
    lg.close()
    g.close()


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------------
def _apply_atomic(lg, base, verify=True, rows=None):
    l1, l2 = rows or _atomic_rows(base)
    padded = _signed(base, l2, len(l1)) + [{} for _ in range(SHAPE[0] - len(l1) - len(l2))]
    return lg.apply_resident(l1, padded, [1, 0, 0, 0], [base.first_idx + 2, 0, 0, 0], S.CHAIN_ID, 1, n_sib=N_SIB, verify=verify, atomic=True)


def test_nothing_resident_changes_and_no_output_is_invalidated(hz, ctx, base):
    lg = _growing(hz, base)
    _apply_atomic(lg, base)
    everyone = np.arange(base.first_idx, base.first_idx + base.N)
    R, F = SHAPE[0], SHAPE[3]

    def snapshot():
        out = {"root": lg.root(), "planes": lg.accounts(everyone).tobytes(), "size": lg.size()}
        return out

    def device_outputs():
        out = {}
        for (name, shape), ptr in zip(capi.Ledger.shapes(R, F, N_SIB), lg.outputs_dev().values()):
            out[name] = _device_bytes(ptr, int(np.prod(shape)))
        for getter in (lg.exit_outputs_dev, lg.create_outputs_dev):
            for name, ptr in getter().items():
                out[name] = _device_bytes(ptr, 32 if name.startswith("new_") and name != "new_exit" else R * 32)
        for name, ptr in lg.sig_outputs_dev().items():
            out[name] = _device_bytes(ptr, 6 * 32)   # the six L2 rows
        out["auxToIdx"] = _device_bytes(lg.aux_to_idx_dev(), R * 32)
        out["l1_flags"] = _device_bytes(lg.l1_flags_dev(), 2)
        return out
    before = device_outputs()
    first = _packed(lg, ctx, base.first_idx + base.N - 1)
    after = device_outputs()          # the getters still hand out, and what they hand out is unchanged
    assert after == before and len(before) == 27 + 6 + 6 + 3 + 2
    second = _packed(lg, ctx, base.first_idx + base.N - 1)   # again, into another buffer
    assert second == first and device_outputs() == before
    state = snapshot()                # (hz_ledger_accounts reuses the call's buffers: last)
    twin = _growing(hz, base)
    _apply_atomic(twin, base)
    assert state == {"root": twin.root(), "planes": twin.accounts(everyone).tobytes(), "size": twin.size()}
    lg.close()
    twin.close()


def _refused_untouched(hz, lg, g, old_last, word, nbytes=None):
    import torch
    nbytes = g.packed_layout()[0] if nbytes is None else nbytes
    buf = torch.full((g.packed_layout()[0] + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    st = hz.c.hz_ledger_main_inputs(lg.h, g.h, old_last, buf.data_ptr(), nbytes)
    msg = hz.c.hz_last_error().decode()
    assert st == 1 and word in msg, (st, msg)
    assert bool((buf == 0xA5).all())


def test_refusals_leave_the_buffer_untouched(hz, ctx, base):
    f0, last = base.first_idx, base.first_idx + base.N - 1
    none_yet = "no successful apply call with a chain id"
    lg = _dense(hz, base)
    _refused_untouched(hz, lg, ctx, last, none_yet)                                   # no apply yet
    plain = Q.transfers(base, 8)
    lg.apply_l2(plain, [1, 0, 0, 0], [f0 + 2, 0, 0, 0], n_sib=N_SIB, outputs=False)
    _refused_untouched(hz, lg, ctx, last, none_yet)                                   # hz_ledger_apply_l2: no chain id
    lg.close()
    # the calls that invalidate the *_dev outputs, each after a good apply
    signed = _signed(base, Q.transfers(base, 3, start=8))

    def fresh():
        lg = _dense(hz, base)
        _apply_atomic(lg, base)
        return lg
    lg = fresh()
    assert len(_packed(lg, ctx, last)) == ctx.packed_layout()[0]
    with pytest.raises(HzError) as e:                                                  # a refused apply: reason 2, a stale nonce
        _apply_atomic(lg, base)
    assert e.value.status == 4 and "reason 2:" in str(e.value)
    _refused_untouched(hz, lg, ctx, last, none_yet)
    lg.close()
    for invalidate in (lambda lg: lg.verify_l2(signed, S.CHAIN_ID, 1), lambda lg: lg.verify_l2_atomic(signed, S.CHAIN_ID, 1), lambda lg: lg.resolve_l2(signed),
                       lambda lg: lg.select_batch([], signed, S.CHAIN_ID, 2), lambda lg: (lg.exit_keep(1), lg.withdraw_rows([1], [f0], SHAPE[1]))):
        lg = fresh()
        invalidate(lg)
        _refused_untouched(hz, lg, ctx, last, none_yet)
        lg.close()
    # the shape check
    lg = fresh()
    for kw, word in (({"nTx": 9}, "does not fill"), ({"maxL1Tx": 1}, "does not fill"), ({"maxFeeTx": 3}, "does not fill"), ({"nLevels": 17}, "does not fill")):
        params = dict(nTx=SHAPE[0], nLevels=SHAPE[1], maxL1Tx=SHAPE[2], maxFeeTx=SHAPE[3])
        params.update(kw)
        other = hz.ctx("rollup-main", **params)
        _refused_untouched(hz, lg, other, last, word)
        other.close()
    other = hz.ctx("hash-state")
    st = hz.c.hz_ledger_main_inputs(lg.h, other.h, last, 32, 32)
    assert st == 1 and "not a rollup-main context" in hz.c.hz_last_error().decode()
    other.close()
    _refused_untouched(hz, lg, ctx, last, "bytes = ", nbytes=ctx.packed_layout()[0] - 32)
    for args in ((None, ctx.h, last, 32, 32), (lg.h, None, last, 32, 32), (lg.h, ctx.h, last, None, ctx.packed_layout()[0])):
        assert hz.c.hz_ledger_main_inputs(*args) == 1 and "null argument" in hz.c.hz_last_error().decode()
    assert len(_packed(lg, ctx, last + 5)) == ctx.packed_layout()[0]                  # a dense ledger takes the caller's old_last_idx
    lg.close()
    lg = _growing(hz, base)
    _apply_atomic(lg, base, rows=([K.create_for(K.account(1), load=3)], Q.transfers(base, 2)))
    assert lg.last_idx() == last + 1
    _refused_untouched(hz, lg, ctx, last + 1, "old_last_idx")                          # the last idx AFTER the batch is not it
    assert len(_packed(lg, ctx, last)) == ctx.packed_layout()[0]
    lg.close()


def test_the_checked_route_reports_an_element_that_is_no_field_element(hz, ctx, base):
    """r8x of an L2 row set to r in the device buffer: staged, and hz_witness_check answers HZ_ERR_INPUT"""
    import torch
    lg = _growing(hz, base)
    _apply_atomic(lg, base)
    addr, nbytes, buf = lg.main_inputs(ctx, base.first_idx + base.N - 1)
    off = {n: o for n, o, _, _ in ctx.packed_layout()[1]}["r8x"] + 3 * 32
    buf[off:off + 32] = torch.from_numpy(np.frombuffer(P.to_bytes(32, "little"), dtype=np.uint8).copy()).to(buf.device)
    ctx.clear_inputs()
    ctx.stage(0, addr, nbytes)
    with pytest.raises(HzError) as e:
        ctx.run()
    assert e.value.status == 4, str(e.value)
    ctx.clear_inputs()
    lg.close()
