"""L2 transfers to an address or key on the device-resident ledger (hz_ledger_apply_l2_addr) against the Python BatchBuilder
over the same state with host hashing and auxToIdx given: every output array, auxToIdx, the root, the resident fields and the tree
afterwards; supplied receivers; refusals 9 - 11; the lookup alone against the model; argument errors; and the circuit itself (the HIP
rollup-main context and the oracle) on the inputs builder.l2_batch_inputs makes. Every comparison is on bytes, bit-exact."""
import types

import numpy as np
import pytest

import device_state_common as D
import ledger_addr_common as A
import ledger_common as C
import ledger_sig_common as S
from circuits_amd import HzError
from circuits_amd import builder as B

pytestmark = pytest.mark.gpu
N_LEVELS = 16


def _aux_array(aux, m):
    return None if aux is None else np.array([a or 0 for a in aux] + [0] * (m - len(aux)), dtype=np.uint64)


def _check(lg, st, txs, plan, idxs, db=None, aux=None, n_levels=N_LEVELS):
    got = lg.apply_l2_addr(txs, plan, idxs, 1, 1, n_sib=n_levels + 1, aux_to_idx=_aux_array(aux, len(txs)))
    db, bb = A.builder_batch(st, txs, plan, idxs, n_levels, db=db, aux=aux)
    C.assert_same(got, A.expected_arrays(bb, txs))
    assert lg.root() == bb.new_state_root
    acc = A.touched(st, txs, idxs, aux)
    assert (lg.accounts(acc) == C.leaf_rows(db, acc)).all()
    return db, bb, got


def _final_tree_matches(lg, st, db):
    cols = [np.array(c) for c in st.leaf_fields()]
    for i, leaf in db.leaves.items():
        for c, v in enumerate(B.leaf_fields(leaf)):
            cols[c][i - st.first_idx] = D.to_bytes([v])[0]
    levels, value = D.rebuild_levels(st.k, st.first_idx, cols)
    got_levels, got_value = lg.tree().download()
    for d, (g, e) in enumerate(zip(got_levels, levels)):
        assert (g == e).all(), "level %d differs" % d
    assert (got_value == value).all()
    assert (lg.accounts(np.arange(st.first_idx, st.first_idx + st.N)) == np.stack(cols, axis=1)).all()


def _fee_accounts(st):
    """the lowest account of token 1 and of token 2"""
    tok = [st.state(st.first_idx + j)["tokenID"] for j in range(st.N)]
    return [st.first_idx + tok.index(1), st.first_idx + tok.index(2), 0, 0]


# (k, m, seed): the seeds are chosen on the CPU so that the batch names receivers by address and by key and its table has a probe chain
@pytest.mark.parametrize("k,m,seed", [(4, 1, 24), (4, 5, 0), (9, 63, 0), (9, 64, 0), (9, 65, 0), (9, 130, 0)])
def test_parity_with_the_builder(hz, k, m, seed):
    st = A.mixed_state(k)
    txs = A.draw_batch(st, m, seed, n_tx=m + (m > 1))
    by_addr = [t for t in txs if A.is_to_addr(t)]
    assert len(by_addr) >= max(1, m // 5)
    found, table = A.resolve_model(st, txs, skip_zero=True)
    if m > 1:
        assert table.longest >= 2   # a query that does not sit at its hash: the kernel's probe has to walk
    if k == 9:   # the lowest holder and a higher one in different workgroups of k_ledger_resolve
        t = next(t for t in by_addr if t["toEthAddr"] != A.ANY)
        holders = [j for j in range(st.N) if A.matches(st.state(st.first_idx + j), t["tokenID"], t["toEthAddr"], 0, 0)]
        assert holders[0] // 256 != holders[-1] // 256
        assert any(t["toEthAddr"] == A.ANY for t in by_addr)
    lg = st.to_ledger(hz)
    assert lg.root() == st.root
    assert lg.resolve_l2(txs).tolist() == A.resolve_model(st, txs)[0]
    db, bb, got = _check(lg, st, txs, [1, 2, 0, 0], _fee_accounts(st))
    assert [D.to_int(r) for r in got["auxToIdx"]] == [f if A.is_to_addr(t) else 0 for f, t in zip(found, txs)]
    assert lg.resolve_ms() > 0.0
    _final_tree_matches(lg, st, db)
    lg.close()


def test_supplied_receivers(hz):
    """aux_to_idx equal to the resolved receivers gives identical bytes; a valid holder that is not the lowest is accepted and applied"""
    st = A.mixed_state(6)
    txs = A.draw_batch(st, 20, seed=3, pool=30)
    plan, idxs = [1, 2], _fee_accounts(st)[:2]
    found, _ = A.resolve_model(st, txs, skip_zero=True)
    assert sum(1 for f in found if f) >= 4
    a, b = st.to_ledger(hz), st.to_ledger(hz)
    got_a = a.apply_l2_addr(txs, plan, idxs, 1, 1, n_sib=7)
    got_b = b.apply_l2_addr(txs, plan, idxs, 1, 1, n_sib=7, aux_to_idx=np.array(found, dtype=np.uint64))
    C.assert_same(got_b, got_a)
    assert a.root() == b.root() and b.resolve_ms() == 0.0
    everyone = np.arange(st.first_idx, st.first_idx + st.N)
    assert (a.accounts(everyone) == b.accounts(everyone)).all()
    a.close()
    b.close()
    sp = A.special_state(6)
    f0, leaf = sp.first_idx, sp.state
    shared = [i for i in range(f0, f0 + sp.N) if leaf(i)["ethAddr"] == leaf(f0 + 2)["ethAddr"] and leaf(i)["tokenID"] == 1]
    assert len(shared) >= 3
    txs = [A.to_addr(C.tx(f0 + 1, 0, 700, 176, nonce=0), leaf(shared[0])), A.to_addr(C.tx(f0 + 1, 0, 5, 0, nonce=1), leaf(sp.any_a))]
    lg = sp.to_ledger(hz)
    db, _, got = _check(lg, sp, txs, [1], [f0 + 3], aux=[shared[-1], sp.any_c])
    assert [D.to_int(r) for r in got["auxToIdx"]] == [shared[-1], sp.any_c]
    _final_tree_matches(lg, sp, db)
    lg.close()


def _edge_batches(sp):
    f0, leaf = sp.first_idx, sp.state
    own7 = A.to_addr(C.tx(f0 + 7, 0, 900, 176, nonce=0), leaf(f0 + 7))
    low = A.brute_force(sp, A.to_addr(C.tx(f0 + 1, 0, 1), leaf(f0 + 2)))
    return {
        "receiver_sends_before_and_after": [C.tx(f0 + 7, f0 + 1, 50, 100, nonce=0), A.to_addr(C.tx(f0 + 1, 0, 70, 0, nonce=0), leaf(f0 + 7)),
                                            C.tx(f0 + 7, f0 + 1, 5, 192, nonce=1)],
        "own_address": [own7, C.tx(f0 + 7, f0 + 1, 5, 0, nonce=1), A.to_addr(C.tx(low, 0, 12, 1, nonce=0), leaf(low))],
        "two_addresses_one_account": [A.to_addr(C.tx(f0 + 1, 0, 33, 1, nonce=0), leaf(sp.any_a)), A.to_addr(C.tx(f0 + 1, 0, 34, 1, nonce=1), leaf(sp.any_c)),
                                      C.tx(f0 + 1, sp.any_a, 35, 1, nonce=2)],
        "one_address_two_tokens": [A.to_addr(C.tx(f0 + 1, 0, 33, 1, nonce=0), leaf(f0 + 2)), A.to_addr(C.tx(f0 + 9, 0, 33, 1, token=2, nonce=0), leaf(f0 + 9))],
        "zero_amounts": [A.to_addr(C.tx(f0 + 1, 0, 0, 200, nonce=0), leaf(f0 + 7)), dict(C.tx(f0 + 1, 0, 0, 0, nonce=1), toEthAddr=12345),
                         A.to_addr(C.tx(f0 + 1, 0, 0, 1, nonce=2), leaf(sp.any_b)), A.to_addr(C.tx(f0 + 1, 0, 3, 1, nonce=3), leaf(f0 + 7))],
    }


@pytest.mark.parametrize("name", ["receiver_sends_before_and_after", "own_address", "two_addresses_one_account", "one_address_two_tokens", "zero_amounts"])
def test_edge_orders(hz, name):
    sp = A.special_state(6)
    txs = _edge_batches(sp)[name]
    lg = sp.to_ledger(hz)
    db, _, got = _check(lg, sp, txs, [1, 2], [sp.first_idx + 40, 0])
    aux = [D.to_int(r) for r in got["auxToIdx"]]
    if name == "own_address":
        assert aux[0] == txs[0]["fromIdx"] and aux[2] == txs[2]["fromIdx"]
    if name == "two_addresses_one_account":
        assert aux == [sp.any_a, sp.any_a, 0]
    if name == "zero_amounts":
        assert aux == [0, 0, 0, sp.first_idx + 7]
        assert [D.to_int(r) for r in got["ethAddr2"][:3]] == [t["toEthAddr"] for t in txs[:3]] and not got["siblings2"][:3].any()
        assert D.to_int(got["ay2"][2]) == txs[2]["toBjjAy"] and D.to_int(got["sign2"][2]) == txs[2]["toBjjSign"] and not got["ay2"][:2].any()
        assert [int(r[0]) for r in got["tokenID2"][:3]] == [1, 1, 1] and not got["balance2"][:3].any() and not got["nonce2"][:3].any()
    _final_tree_matches(lg, sp, db)
    lg.close()


def test_refusals_name_the_offence_and_change_nothing(hz):
    sp = A.special_state(6)
    f0, leaf = sp.first_idx, sp.state
    lg = sp.to_ledger(hz)
    root = lg.root()
    everyone = np.arange(f0, f0 + sp.N)
    fields = lg.accounts(everyone)
    ok = C.tx(f0 + 3, f0 + 4, 10, 176, nonce=0)
    nobody = dict(C.tx(f0 + 1, 0, 5, nonce=0), toEthAddr=12345)
    to7 = A.to_addr(C.tx(f0 + 1, 0, 5, nonce=0), leaf(f0 + 7))
    to_a = A.to_addr(C.tx(f0 + 1, 0, 5, nonce=0), leaf(sp.any_a))
    poor = C.tx(f0 + 3, f0 + 4, B.float2fix(B.floor_fix2float(leaf(f0 + 3)["balance"] * 2)), nonce=0)
    signed = [S.sign(sp, dict(ok)), S.sign(sp, dict(to7))]
    forged = [signed[0], S.forge(signed[1], "s")]
    cases = [   # (txs, aux, verify, index, reason)
        ([ok, nobody], None, False, 1, 9),
        ([C.tx(f0 + 30 + i, f0 + 4, 10, nonce=7 if i == 3 else 0) for i in range(5)] + [nobody], None, False, 5, 9),   # 9 comes first, as specified: not the nonce at 3
        ([ok, to7], [0, f0 + 3], False, 1, 10),
        ([ok, to_a], [0, sp.any_b], False, 1, 11),
        ([ok, to7], [0, f0 + 9], False, 1, 4),        # 10 beside 4 at one index: the lowest reason
        ([poor, to7], [0, f0 + 9], False, 0, 3),      # a lower index wins over both
        (forged, None, True, 1, 7),
    ]
    for txs, aux, verify, index, reason in cases:
        assert A.scheme_model(sp, txs, [1], [f0 + 40], aux=aux)[:3] == ("refused", index, reason) or reason == 7
        into = {name: np.full(shape, 0xA5, dtype=np.uint8) for name, shape in lg.shapes(len(txs), 1, 7)}
        into.update({name: np.full((len(txs), 32), 0xA5, dtype=np.uint8) for name in ("auxToIdx", "tx_compressed_data", "tx_compressed_data_v2", "sig_l2_hash")})
        with pytest.raises(HzError) as e:
            lg.apply_l2_addr(txs, [1], [f0 + 40], 1, 1, n_sib=7, verify=verify, aux_to_idx=_aux_array(aux, len(txs)), into=into)
        assert e.value.status == 4, (reason, str(e.value))
        assert "index %d " % index in str(e.value) and "reason %d:" % reason in str(e.value), (reason, str(e.value))
        assert all((a == 0xA5).all() for a in into.values()), reason
        assert lg.root() == root and (lg.accounts(everyone) == fields).all(), reason
        for call in (lg.outputs_dev, lg.aux_to_idx_dev):
            with pytest.raises(HzError):
                call()
    # a good signature over toIdx = 0 passes, and the batch is then as on a fresh ledger
    got = lg.apply_l2_addr(signed, [1], [f0 + 40], 1, 1, n_sib=7, verify=True)
    fresh = sp.to_ledger(hz)
    exp = fresh.apply_l2_addr(signed, [1], [f0 + 40], 1, 1, n_sib=7)
    C.assert_same(got, exp)
    C.assert_same(got, S.expected_sig_arrays(signed))
    assert D.to_int(got["old_root"][0]) == root and lg.root() == fresh.root() and D.to_int(got["auxToIdx"][1]) == f0 + 7
    assert lg.aux_to_idx_dev()
    lg.close()
    fresh.close()


def test_resolve_alone(hz):
    sp = A.special_state(6)
    f0, leaf = sp.first_idx, sp.state
    lg = sp.to_ledger(hz)
    root = lg.root()
    fields = lg.accounts(np.arange(f0, f0 + sp.N))
    txs = [A.to_addr(C.tx(f0 + 1, 0, 5), leaf(f0 + 2)), A.to_addr(C.tx(f0 + 9, 0, 5, token=2), leaf(f0 + 9)), A.to_addr(C.tx(f0 + 1, 0, 5), leaf(sp.any_c)),
           A.to_addr(C.tx(f0 + 1, 0, 5), leaf(sp.any_b)), dict(C.tx(f0 + 1, 0, 5), toEthAddr=12345), dict(C.tx(f0 + 1, 0, 5, token=3), toEthAddr=leaf(f0 + 2)["ethAddr"]),
           dict(C.tx(f0 + 1, 0, 5), toEthAddr=A.ANY, toBjjAy=leaf(sp.any_a)["ay"], toBjjSign=1 - leaf(sp.any_a)["sign"]),
           A.to_addr(C.tx(f0 + 1, 0, 0), leaf(f0 + 7)), C.tx(f0 + 1, f0 + 3, 5), {}, dict(A.to_addr(C.tx(f0 + 1, 0, 5), leaf(f0 + 7)), fromIdx=0)]
    exp, _ = A.resolve_model(sp, txs)
    assert exp[2:4] == [sp.any_a, sp.any_b] and exp[4:7] == [0, 0, 0] and exp[7] == f0 + 7 and exp[8:] == [0, 0, 0]
    assert lg.resolve_l2(txs).tolist() == exp
    assert lg.resolve_l2([]).tolist() == [] and lg.resolve_l2([{}, C.tx(f0 + 1, f0 + 3, 5)]).tolist() == [0, 0]
    assert lg.root() == root and (lg.accounts(np.arange(f0, f0 + sp.N)) == fields).all()
    lg.close()


def test_argument_errors(hz):
    import ctypes
    from circuits_amd.capi import l2tx_array
    sp = A.special_state(6)
    f0, leaf = sp.first_idx, sp.state
    lg = sp.to_ledger(hz)
    root = lg.root()
    to7 = A.to_addr(C.tx(f0 + 1, 0, 5, nonce=0), leaf(f0 + 7))
    with pytest.raises(HzError) as e:
        lg.aux_to_idx_dev()
    assert e.value.status == 1 and "hz_ledger_apply_l2_addr" in str(e.value)
    arr = l2tx_array([to7])
    plan, idxs = np.array([1], dtype=np.uint32), np.array([0], dtype=np.uint64)
    sig_ptrs = (ctypes.c_void_p * 3)()
    c = hz.c
    assert c.hz_ledger_apply_l2_addr(lg.h, 1, ctypes.addressof(arr), None, 0, None, 1, 1, 1, plan.ctypes.data, idxs.ctypes.data, 7, None, None, None) == 1
    assert "null sigs" in hz.c.hz_last_error().decode()
    from circuits_amd.capi import l2sig_array
    sigs = l2sig_array([to7])
    assert c.hz_ledger_apply_l2_addr(lg.h, 1, ctypes.addressof(arr), ctypes.addressof(sigs), 0, None, 1, 1, 1, plan.ctypes.data, idxs.ctypes.data, 7, None,
                                     ctypes.addressof(sig_ptrs), None) == 1
    assert "sig_out without HZ_LEDGER_VERIFY_SIGS" in hz.c.hz_last_error().decode()
    for txs, aux, text in (([to7], [f0 + 64], "outside the state"), ([to7], [0], "outside the state"), ([C.tx(f0, 1, 5)], None, "not supported yet"),
                           ([dict(to7, toEthAddr=1 << 160)], None, "more than 160 bits"), ([C.tx(f0, f0 + 64, 5)], None, "outside the state")):
        with pytest.raises(HzError) as e:
            lg.apply_l2_addr(txs, [1], [0], 1, 1, n_sib=7, aux_to_idx=_aux_array(aux, 1))
        assert e.value.status == 1 and text in str(e.value), str(e.value)
    # the four earlier entry points keep their answer
    for call in (lambda: lg.apply_l2([to7], [1], [0], n_sib=7), lambda: lg.apply_l2_signed([to7], [1], [0], 1, 1, n_sib=7), lambda: lg.verify_l2([to7], 1, 1),
                 lambda: hz.ledger_plan_l2([to7], [1], [0], 6)):
        with pytest.raises(HzError) as e:
            call()
        assert e.value.status == 1 and "a transfer to an address) is not supported yet" in str(e.value), str(e.value)
    assert lg.root() == root
    lg.close()


def test_the_circuit_accepts_the_ledgers_inputs(hz):
    """a transfer, a transferToEthAddr, a transferToBjj, a zero-amount transfer to an address and NOPs, all signed and verified on the
    device: l2_batch_inputs == BatchBuilder's dictionary key by key except the leaf-2 rows of the zero-amount transaction, where the
    oracle is the judge; the HIP rollup-main context and the oracle accept; once more with every state-dependent signal and auxToIdx
    left on the device"""
    from oracle_binding import OracleCtx
    shape = (8, 16, 2, 4)
    sp = A.special_state(6)
    f0, leaf = sp.first_idx, sp.state
    txs = [C.tx(f0 + 1, f0 + 2, 1000, 176, nonce=0), A.to_addr(C.tx(f0 + 1, 0, 2000, 100, nonce=1), leaf(f0 + 7)),
           A.to_addr(C.tx(f0 + 3, 0, 3000, 192, nonce=0), leaf(sp.any_b)), A.to_addr(C.tx(f0 + 3, 0, 0, 1, nonce=1), leaf(f0 + 2)),
           A.to_addr(C.tx(f0 + 7, 0, 40, 0, nonce=0), leaf(sp.any_c))]
    for t in txs:
        t["signer"] = S.signer(sp, t["fromIdx"])
    zero = A.zero_amount_rows(txs)
    assert list(zero) == [3]
    fee_tokens, fee_idxs = [1], [f0 + 20]
    db, bb = A.builder_batch(sp, txs + [{}, {}, {}], fee_tokens + [0] * 3, fee_idxs + [0] * 3, shape[1], max_l1=shape[2])
    exp = bb.get_input()
    assert exp["auxToIdx"][:5] == [0, f0 + 7, sp.any_b, 0, sp.any_a]
    lg = sp.to_ledger(hz)
    like = types.SimpleNamespace(last_idx=f0 + sp.N - 1, num_batch=0)
    inp, _ = B.l2_batch_inputs(lg, like, txs, *shape, fee_tokens, fee_idxs, 1, verify=True)
    assert set(inp) == set(exp), set(inp) ^ set(exp)
    for name in exp:
        if name in zero[3]:
            assert inp[name][:3] + inp[name][4:] == exp[name][:3] + exp[name][4:] and inp[name][3] == zero[3][name] != exp[name][3], name
        else:
            assert inp[name] == exp[name], name
    g = hz.ctx("rollup-main", nTx=shape[0], nLevels=shape[1], maxL1Tx=shape[2], maxFeeTx=shape[3])
    g.set_inputs(inp)
    g.run()
    assert g.get("main.hashGlobalInputs") == bb.get_hash_inputs()
    witness = g.read_raw_bytes()
    o = OracleCtx("rollup-main", *shape)
    o.set_inputs(inp)
    assert o.run() is None
    lg2 = sp.to_ledger(hz)
    like = types.SimpleNamespace(last_idx=f0 + sp.N - 1, num_batch=0)
    inp2, dev = B.l2_batch_inputs(lg2, like, txs, *shape, fee_tokens, fee_idxs, 1, host_outputs=False, verify=True)
    assert set(inp2) | set(dev) == set(exp) and not set(inp2) & set(dev) and "auxToIdx" in dev
    g.clear_inputs()
    g.set_inputs(inp2)
    for name, (ptr, count) in dev.items():
        g.set_input_dev(name, ptr, count)
    g.run()
    assert g.read_raw_bytes() == witness
    lg.close()
    lg2.close()
