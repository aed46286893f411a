"""hz_ledger_apply_l2_signed / hz_ledger_verify_l2 (csrc/ledger_sig.hip) on the device: parity with the unsigned path on a
twin ledger and with the builder's packed values, every signature edge against the Python model and the circuit (the oracle's
rollup-main), the refusal discipline across old and new reasons, the mempool filter, the argument errors, and the circuit itself on the
inputs builder.l2_batch_inputs(verify=True) makes. Every comparison is on bytes or integers, bit-exact."""
import types

import numpy as np
import pytest

import device_state_common as D
import fuzz_common as F
import ledger_common as C
import ledger_sig_common as S
from circuits_amd import HzError
from circuits_amd import builder as B
from circuits_amd.capi import LEDGER_SIG_ARRAYS

pytestmark = pytest.mark.gpu
K, N_SIB = 6, 7
P = B.P


def _ledger(hz, base, cols=None):
    if cols is None:
        return base.to_ledger(hz)
    lg = hz.ledger(K, first_idx=base.first_idx)
    lg.load(*cols)
    return lg


def _everyone(base):
    return np.arange(base.first_idx, base.first_idx + base.N)


@pytest.mark.parametrize("m", [1, 5, 65, 130])
def test_parity_with_the_unsigned_path_and_the_builder(hz, m):
    base = C.base_state(K)
    txs = S.signed_batch(base, m, seed=3000 + m, pool=24, n_tx=m + 3)
    plan, idxs = [1, 0, 0, 0], [base.first_idx + 3, 0, 0, 0]
    lg, twin = _ledger(hz, base), _ledger(hz, base)
    got = lg.apply_l2_signed(txs, plan, idxs, S.CHAIN_ID, 1, n_sib=N_SIB)
    assert lg.sig_ms() > 0 and set(lg.sig_outputs_dev()) == set(LEDGER_SIG_ARRAYS) and len(lg.outputs_dev()) == 27   # valid until the next call
    exp = twin.apply_l2(txs, plan, idxs, n_sib=N_SIB)
    assert len(exp) == 27
    C.assert_same(got, exp)
    assert lg.root() == twin.root() and (lg.accounts(_everyone(base)) == twin.accounts(_everyone(base))).all()
    _, bb = C.builder_batch(base, txs, plan, idxs, 16)
    inp = bb.get_input()
    builder = {"tx_compressed_data": C.to_bytes(inp["txCompressedData"]), "tx_compressed_data_v2": C.to_bytes(inp["txCompressedDataV2"]),
               "sig_l2_hash": C.to_bytes([meta["sigL2Hash"] for meta in bb.tx_meta])}
    C.assert_same(got, builder)
    C.assert_same(got, S.expected_sig_arrays(txs))
    lg.close()
    twin.close()


N_CHUNKS = 6


@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_signature_edges_against_the_model_and_the_circuit(hz, chunk):
    """every applicable case of fuzz_common.signature_edge_cases as transaction 1 of a batch of 3: the ledger's verdict is the model's,
    and the oracle's rollup-main accepts the batch's inputs iff the ledger accepted the batch"""
    from oracle_binding import OracleCtx
    base = S.edge_state()   # indices below 2^6: the shape below can hold them
    f0 = base.first_idx
    edges = S.edge_batches(base)
    labels = [lb for lb, _, _ in edges]
    # the cap: nothing is left out but sign1=2 and the fromIdx=0 / onChain=1 gates
    single = {"s": 1, "r8x": B.BASE8[0], "r8y": B.BASE8[1], "ay1": 1, "sign1": 0, "onChain": 0, "fromIdx": f0 + 2}
    every = [lb for lb, _ in F.signature_edge_cases(dict(single, s=edges[0][1][1]["s"])) if " & " not in lb]
    assert sorted(labels) == sorted(lb for lb in every if lb != "sign1=2") and len(labels) == len(every) - 1 >= 26
    shape = (4, K, 0, 2)
    ran = 0
    for label, txs, cols in edges[chunk::N_CHUNKS]:
        model = S.verdicts(txs, cols, f0)
        lg = _ledger(hz, base, cols)
        assert lg.verify_l2(txs, S.CHAIN_ID, 1).tolist() == model, label
        like = types.SimpleNamespace(last_idx=f0 + base.N - 1, num_batch=0)
        try:
            inp, _ = B.l2_batch_inputs(lg, like, txs, *shape, [1], [f0 + 40], S.CHAIN_ID, verify=True)
            accepted = True
        except HzError as e:
            assert e.status == 4 and "index 1 " in str(e) and "reason 7:" in str(e), (label, str(e))
            accepted = False
            twin = _ledger(hz, base, cols)
            like = types.SimpleNamespace(last_idx=f0 + base.N - 1, num_batch=0)
            inp, _ = B.l2_batch_inputs(twin, like, txs, *shape, [1], [f0 + 40], S.CHAIN_ID)
            twin.close()
        assert accepted == (model == [0, 0, 0]), (label, model)
        o = OracleCtx("rollup-main", *shape)
        o.set_inputs(inp)
        assert (o.run() is None) == accepted, label
        lg.close()
        ran += 1
    assert ran == len(edges[chunk::N_CHUNKS]) and sum(len(edges[c::N_CHUNKS]) for c in range(N_CHUNKS)) == len(edges)


def _refused(lg, txs, plan, idxs, current, index, reason, root, fields, everyone):
    into = {name: np.full(shape, 0xA5, dtype=np.uint8) for name, shape in lg.shapes(len(txs), len(plan), N_SIB)}
    into.update({name: np.full((len(txs), 32), 0xA5, dtype=np.uint8) for name in LEDGER_SIG_ARRAYS})
    with pytest.raises(HzError) as e:
        lg.apply_l2_signed(txs, plan, idxs, S.CHAIN_ID, current, n_sib=N_SIB, into=into)
    assert e.value.status == 4, str(e.value)
    assert "index %d " % index in str(e.value) and "reason %d:" % reason in str(e.value), str(e.value)
    assert len(into) == 30 and all((a == 0xA5).all() for a in into.values())
    for f in (lg.outputs_dev, lg.sig_outputs_dev):   # before any other call, which would withdraw them anyway
        with pytest.raises(HzError):
            f()
    assert lg.root() == root and (lg.accounts(everyone) == fields).all()


def test_refusals_across_old_and_new_reasons_change_nothing(hz):
    base = C.base_state(K)
    f0 = base.first_idx
    lg = _ledger(hz, base)
    root, everyone = lg.root(), _everyone(base)
    fields = lg.accounts(everyone)
    good = S.signed_batch(base, 130, seed=4242, pool=40)
    plan, idxs = [1], [f0 + 50]

    def batch(edits):
        out = [dict(t) for t in good]
        for i, f in edits.items():
            out[i] = f(out[i])
        return out
    wrong_nonce = lambda t: S.sign(base, dict(t, nonce=t["nonce"] + 7))   # noqa: E731  signed over the wrong nonce: reason 2 only
    too_much = lambda t: S.sign(base, dict(t, amountF=B.floor_fix2float(base.state(t["fromIdx"])["balance"] * 4)))   # noqa: E731
    forged = lambda t: S.forge(t, "s")   # noqa: E731
    late = lambda t: S.sign(base, dict(t, maxNumBatch=2))   # noqa: E731
    args = (root, fields, everyone)
    _refused(lg, batch({129: forged, 64: wrong_nonce}), plan, idxs, 1, 64, 2, *args)
    _refused(lg, batch({64: forged, 129: too_much}), plan, idxs, 1, 64, 7, *args)
    _refused(lg, batch({10: lambda t: S.forge(t, "r8"), 100: lambda t: S.forge(t, "malleable")}), plan, idxs, 1, 10, 7, *args)
    _refused(lg, batch({70: late}), plan, idxs, 5, 70, 8, *args)
    _refused(lg, batch({70: lambda t: forged(late(t))}), plan, idxs, 5, 70, 7, *args)
    _refused(lg, batch({3: lambda t: S.forge(t, "r8")}), plan, idxs, 1, 3, 7, *args)
    # a following valid call is as if the refused ones had not been made
    got = lg.apply_l2_signed(good, plan, idxs, S.CHAIN_ID, 1, n_sib=N_SIB)
    fresh = _ledger(hz, base)
    exp = fresh.apply_l2_signed(good, plan, idxs, S.CHAIN_ID, 1, n_sib=N_SIB)
    C.assert_same(got, exp)
    assert D.to_int(got["old_root"][0]) == root and lg.root() == fresh.root()
    lg.close()
    fresh.close()


def test_verify_l2_is_a_filter_that_changes_nothing(hz):
    base = C.base_state(K)
    lg = _ledger(hz, base)
    root, everyone = lg.root(), _everyone(base)
    fields = lg.accounts(everyone)
    txs = S.signed_batch(base, 68, seed=77, pool=30, n_tx=70)
    txs[0] = S.forge(txs[0], "malleable")
    txs[63] = S.sign(base, dict(txs[63], maxNumBatch=3))
    txs[64] = S.forge(txs[64], "stale")
    txs[67] = S.forge(txs[67], "r8")
    cur = 9
    model = S.verdicts(txs, base.leaf_fields(), base.first_idx, cur)
    assert model[0] == 7 and model[63] == 8 and model[64] == 7 and model[67] == 7 and model[68:] == [0, 0] and sum(v != 0 for v in model) >= 4
    got, arrays = lg.verify_l2(txs, S.CHAIN_ID, cur, outputs=True)
    assert got.tolist() == model
    C.assert_same(arrays, S.expected_sig_arrays(txs))
    assert set(lg.sig_outputs_dev()) == set(LEDGER_SIG_ARRAYS)
    with pytest.raises(HzError):
        lg.outputs_dev()
    assert lg.root() == root and (lg.accounts(everyone) == fields).all()
    lg.close()


def test_verify_l2_bad_entries_at_the_wavefront_edges(hz):
    """the issue's filter case: a batch of 70 with bad entries at 0, 63, 64 and 69, of mixed causes"""
    base = C.base_state(K)
    lg = _ledger(hz, base)
    root = lg.root()
    txs = S.signed_batch(base, 70, seed=78, pool=30)
    txs[0] = S.forge(txs[0], "s")
    txs[63] = S.forge(txs[63], "malleable")
    txs[64] = S.sign(base, dict(txs[64], maxNumBatch=1))
    txs[69] = S.forge(txs[69], "r8")
    model = S.verdicts(txs, base.leaf_fields(), base.first_idx, 2)
    assert [i for i, v in enumerate(model) if v] == [0, 63, 64, 69] and model[64] == 8
    assert lg.verify_l2(txs, S.CHAIN_ID, 2).tolist() == model
    assert lg.root() == root
    lg.close()


def test_argument_errors(hz):
    base = C.base_state(K)
    f0 = base.first_idx
    lg = _ledger(hz, base)
    root = lg.root()
    ok = S.sign(base, C.tx(f0, f0 + 1, 5, nonce=0))
    plan, idxs = [1], [0]
    for edit, chain, status, text in (({"s": P}, 1, 4, "s is not below"), ({"r8x": P + 1}, 1, 4, "r8x is not below"), ({"r8y": (1 << 256) - 1}, 1, 4, "r8y is not below"),
                                      ({"toBjjAy": P}, 1, 4, "to_bjj_ay is not below"), ({"toEthAddr": 1 << 160}, 1, 1, "160 bits"), ({}, 1 << 16, 1, "chain_id"),
                                      ({"toBjjSign": 2}, 1, 1, "to_bjj_sign"), ({"toIdx": 0}, 1, 1, "not supported yet"), ({"toIdx": 1}, 1, 1, "not supported yet"),
                                      ({"toIdx": f0 + 64}, 1, 1, "outside the state"), ({"fromIdx": f0 - 1}, 1, 1, "outside the state")):
        for call in (lambda t, c: lg.apply_l2_signed([t], plan, idxs, c, 1, n_sib=N_SIB), lambda t, c: lg.verify_l2([t], c, 1)):
            with pytest.raises(HzError) as e:
                call(dict(ok, **edit), chain)
            assert e.value.status == status and text in str(e.value), (edit, str(e.value))
    for n_sib, text in ((5, "n_sib"),):
        with pytest.raises(HzError) as e:
            lg.apply_l2_signed([ok], plan, idxs, 1, 1, n_sib=n_sib)
        assert e.value.status == 1 and text in str(e.value)
    import ctypes
    arr = (ctypes.c_uint8 * 64)()
    assert lg.L.c.hz_ledger_apply_l2_signed(lg.h, 1, ctypes.addressof(arr), None, 1, 1, 1, ctypes.addressof(arr), ctypes.addressof(arr), N_SIB, None, None) == 1
    assert lg.L.c.hz_ledger_verify_l2(lg.h, 1, ctypes.addressof(arr), None, 1, 1, ctypes.addressof(arr), None) == 1
    assert lg.root() == root
    empty = hz.ledger(K, first_idx=f0)
    with pytest.raises(HzError) as e:
        empty.verify_l2([ok], 1, 1)
    assert e.value.status == 1 and "hz_ledger_load" in str(e.value)
    empty.close()
    lg.close()


def test_the_circuit_accepts_the_verified_inputs(hz):
    """l2_batch_inputs(verify=True) == BatchBuilder's dictionary key by key; the HIP rollup-main context runs on it; once more with the
    state-dependent signals and the two packed transaction signals handed over on the device: identical witness bytes"""
    shape = (8, 16, 2, 4)
    base = C.base_state(K)
    keys = base.keys()
    txs = C.draw_batch(base, 6, seed=77, pool=6)
    for t in txs:
        t["signer"] = keys[int(base.key_idx[t["fromIdx"] - base.first_idx])]
    fee_tokens, fee_idxs = [1], [base.first_idx + 20]
    _, bb = C.builder_batch(base, txs + [{}, {}], fee_tokens + [0] * 3, fee_idxs + [0] * 3, shape[1], max_l1=shape[2])
    exp = bb.get_input()
    lg = base.to_ledger(hz)
    like = types.SimpleNamespace(last_idx=base.first_idx + base.N - 1, num_batch=0)
    inp, _ = B.l2_batch_inputs(lg, like, txs, *shape, fee_tokens, fee_idxs, 1, verify=True)
    assert set(inp) == set(exp), set(inp) ^ set(exp)
    for name in exp:
        assert inp[name] == exp[name], name
    g = hz.ctx("rollup-main", nTx=shape[0], nLevels=shape[1], maxL1Tx=shape[2], maxFeeTx=shape[3])
    g.set_inputs(inp)
    g.run()
    assert g.get("main.hashGlobalInputs") == bb.get_hash_inputs()
    witness = g.read_raw_bytes()
    lg2 = base.to_ledger(hz)
    like = types.SimpleNamespace(last_idx=base.first_idx + base.N - 1, num_batch=0)
    inp2, dev = B.l2_batch_inputs(lg2, like, txs, *shape, fee_tokens, fee_idxs, 1, host_outputs=False, verify=True)
    assert set(inp2) | set(dev) == set(exp) and not set(inp2) & set(dev) and {"txCompressedData", "txCompressedDataV2"} <= set(dev)
    g.clear_inputs()
    g.set_inputs(inp2)
    for name, (ptr, count) in dev.items():
        g.set_input_dev(name, ptr, count)
    g.run()
    assert g.read_raw_bytes() == witness
    lg.close()
    lg2.close()
