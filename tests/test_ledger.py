"""The device-resident ledger (hz_ledger, csrc/ledger.hip) against the Python BatchBuilder over the same DenseState with host hashing:
every output array, the root, the resident fields and the tree afterwards; refusals; and the circuit itself (the HIP rollup-main context
and the oracle) on the inputs builder.l2_batch_inputs makes of the ledger's outputs. Every comparison is on bytes, bit-exact."""
import types

import numpy as np
import pytest

import device_state_common as D
import ledger_common as C
from circuits_amd import HzError
from circuits_amd import builder as B

pytestmark = pytest.mark.gpu
N_LEVELS = 16


def _check(lg, base, txs, plan, idxs, db=None, n_levels=N_LEVELS):
    got = lg.apply_l2(txs, plan, idxs, n_sib=n_levels + 1)
    db, bb = C.builder_batch(base, txs, plan, idxs, n_levels, db=db)
    C.assert_same(got, C.expected_arrays(bb))
    assert lg.root() == bb.new_state_root
    acc = C.touched(txs, idxs)
    if acc:
        assert (lg.accounts(acc) == C.leaf_rows(db, acc)).all()
    return db, bb, got


def _final_tree_matches(lg, base, db):
    cols = [np.array(c) for c in base.leaf_fields()]
    for i, leaf in db.leaves.items():
        for c, v in enumerate(B.leaf_fields(leaf)):
            cols[c][i - base.first_idx] = D.to_bytes([v])[0]
    levels, value = D.rebuild_levels(base.k, base.first_idx, cols)
    got_levels, got_value = lg.tree().download()
    for d, (g, e) in enumerate(zip(got_levels, levels)):
        assert (g == e).all(), "level %d differs" % d
    assert (got_value == value).all()
    assert (lg.accounts(np.arange(base.first_idx, base.first_idx + base.N)) == np.stack(cols, axis=1)).all()


@pytest.mark.parametrize("k,m,n_tx,pool", [(4, 1, 1, None), (6, 5, 8, 12), (6, 65, 65, 24), (13, 512, 512, None)])
def test_parity_with_the_builder(hz, k, m, n_tx, pool):
    base = C.base_state(k)
    lg = base.to_ledger(hz)
    assert lg.root() == base.root
    txs = C.draw_batch(base, m, seed=1000 + m, pool=pool, n_tx=n_tx)
    plan, idxs = [1, 0, 0, 0], [base.first_idx + 3, 0, 0, 0]
    db, _, _ = _check(lg, base, txs, plan, idxs)
    _final_tree_matches(lg, base, db)
    lg.close()


def _edge_batches(base):
    f0, bal = base.first_idx, lambda i: base.state(i)["balance"]   # noqa: E731
    one = ([1], [f0 + 40])
    out = {
        "hot_receiver_300": ([C.tx(f0 + 1 + i % 60, f0, 1000 + i, 176, nonce=i // 60) for i in range(300)],) + one,
        "one_sender_70": ([C.tx(f0 + 2, f0 + 3 + i % 5, 10 ** 6 + i, SEL, nonce=i) for i, SEL in zip(range(70), C.SELECTORS * 10)],) + one,
        "ping_pong": ([C.tx(f0 + 4 + i % 2, f0 + 5 - i % 2, 12345 + i, 100, nonce=i // 2) for i in range(9)],) + one,
        "self_transfer": ([C.tx(f0 + 6, f0 + 6, 777, 176, nonce=0), C.tx(f0 + 6, f0 + 7, 5, 0, nonce=1)],) + one,
        "zero_amount": ([C.tx(f0 + 8, f0 + 9, 0, 200, nonce=0), C.tx(f0 + 9, f0 + 8, 0, 0, nonce=0), C.tx(f0 + 8, f0 + 9, 3, 1, nonce=1)],) + one,
        "empty_exactly_then_refill": ([C.tx(f0 + 10, f0 + 11, bal(f0 + 10), 0, nonce=0), C.tx(f0 + 11, f0 + 10, 5000, 176, nonce=0),
                                       C.tx(f0 + 10, f0 + 11, 200, 192, nonce=1)],) + one,
        "fee_receiver_sends_and_receives": ([C.tx(f0 + 40, f0 + 12, 999, 176, nonce=0), C.tx(f0 + 12, f0 + 40, 555, 191, nonce=0)],) + one,
        "two_slots_one_account": ([C.tx(f0 + 13, f0 + 14, 10 ** 9, 176, nonce=0)], [1, 1, 0], [f0 + 15, f0 + 15, 0]),
        "selector_255": ([C.tx(f0 + 16, f0 + 17, 3, 255, nonce=0)],) + one,
    }
    return out


@pytest.mark.parametrize("name", ["hot_receiver_300", "one_sender_70", "ping_pong", "self_transfer", "zero_amount", "empty_exactly_then_refill",
                                  "fee_receiver_sends_and_receives", "two_slots_one_account", "selector_255"])
def test_edge_orders(hz, name):
    base = C.base_state(6)
    lg = base.to_ledger(hz)
    txs, plan, idxs = _edge_batches(base)[name]
    db, _, got = _check(lg, base, txs, plan, idxs)
    if name == "zero_amount":
        assert not got["siblings2"][0].any() and got["tokenID2"][0][0] == 1 and not got["balance2"][0].any()
    _final_tree_matches(lg, base, db)
    lg.close()


def test_token_zero_against_a_zero_padded_plan(hz):
    """accounts of token 0: their fee goes to the FIRST zero of the plan, padding included, as plan.index does"""
    base = C.base_state(6)
    cols = [np.array(c) for c in base.leaf_fields()]
    cols[0][:, 0] = 0   # tokenID 0 everywhere (e0's low 32 bits)
    cols[0][:, 1:4] = 0
    lg = hz.ledger(6, first_idx=base.first_idx)
    lg.load(*cols)
    f0 = base.first_idx
    txs = [C.tx(f0 + 1, f0 + 2, 10 ** 7, 176, token=0, nonce=0), C.tx(f0 + 2, f0 + 1, 10 ** 6, 100, token=0, nonce=0)]
    got = lg.apply_l2(txs, [5, 0, 0], [0, f0 + 3, 0], n_sib=7)
    fees = [B.compute_fee(10 ** 7, 176), B.compute_fee(10 ** 6, 100)]
    assert [D.to_int(r) for r in got["final_acc_fee"]] == [0, sum(fees), 0]
    assert [D.to_int(r) for r in got["acc_fee_after"][0]] == [0, fees[0], 0]
    before = D.to_int(cols[1][3])
    assert D.to_int(got["balance3"][1]) == before and D.to_int(lg.accounts([f0 + 3])[0][1]) == before + sum(fees)
    levels, _ = D.rebuild_levels(6, f0, [lg.accounts(np.arange(f0, f0 + 64))[:, c] for c in range(4)])
    assert D.to_int(levels[0][0]) == lg.root() == D.to_int(got["new_root"][0])
    lg.close()


def test_two_calls_equal_two_builder_batches(hz):
    base = C.base_state(6)
    lg = base.to_ledger(hz)
    plan, idxs = [1, 0], [base.first_idx + 9, 0]
    first = C.draw_batch(base, 20, seed=5, pool=10)
    db, _, _ = _check(lg, base, first, plan, idxs)
    nonce = {}
    for t in first:
        nonce[t["fromIdx"]] = nonce.get(t["fromIdx"], 0) + 1
    second = [C.tx(t["fromIdx"], t["toIdx"], 1000 + i, 100, nonce=nonce.get(t["fromIdx"], 0)) for i, t in enumerate(first[:1])]
    second += [C.tx(base.first_idx + 50 + i, first[0]["fromIdx"], 77, 176, nonce=0) for i in range(5)]
    _check(lg, base, second, plan, idxs, db=db)
    _final_tree_matches(lg, base, db)
    lg.close()


def _refusals(base):
    f0 = base.first_idx
    big = B.float2fix(B.floor_fix2float(base.state(f0)["balance"] * 2))
    ok = C.tx(f0 + 1, f0 + 2, 10, 176, nonce=0)
    one = ([1, 2], [f0 + 40, 0])
    return {   # reason -> (txs, plan, idxs, index named); each batch holds a second, later offence of another kind
        1: ([ok, C.tx(f0, f0 + 2, 10, token=2, nonce=0), C.tx(f0 + 5, f0 + 2, 10, nonce=3)],) + one + (1,),
        2: ([ok, C.tx(f0, f0 + 2, big, nonce=1), C.tx(f0 + 5, f0 + 2, 10, token=2, nonce=0)],) + one + (1,),
        3: ([C.tx(f0, f0 + 2, big, nonce=0), C.tx(f0 + 5, f0 + 2, 10, nonce=3)],) + one + (0,),
        4: ([ok, C.tx(f0 + 3, f0 + 2, 10, token=2, nonce=0), C.tx(f0, f0 + 2, big, nonce=0)],) + one + (1,),
        5: ([ok, C.tx(f0 + 3, f0 + 4, 10, 176, nonce=0)], [1, 1], [f0 + 40, f0 + 41], 0),   # made overflow below by a rich receiver
        6: ([ok, C.tx(f0 + 3, f0 + 4, 10, nonce=0)], [1, 2], [f0 + 40, f0 + 41], 3),
    }


def test_refusals_name_the_lowest_offence_and_change_nothing(hz):
    base = C.base_state(6)
    f0 = base.first_idx
    cols = [np.array(c) for c in base.leaf_fields()]
    tok2 = f0 + 3   # one account of token 2 (for a sender of the right token whose RECEIVER is wrong), one balance just below 2^192
    cols[0][tok2 - f0, 0] = 2
    cols[1][f0 + 4 - f0] = D.to_bytes([(1 << 192) - 5])[0]
    lg = hz.ledger(6, first_idx=f0)
    lg.load(*cols)
    root = lg.root()
    everyone = np.arange(f0, f0 + 64)
    fields = lg.accounts(everyone)
    cases = _refusals(base)
    cases[4] = ([cases[4][0][0], C.tx(f0 + 6, tok2, 10, token=1, nonce=0), cases[4][0][2]],) + cases[4][1:]
    cases[5] = ([cases[5][0][0], C.tx(f0 + 6, f0 + 4, 10, 176, nonce=0), C.tx(f0, f0 + 2, 10, nonce=9)],) + cases[5][1:3] + (1,)
    cases[6] = ([cases[6][0][0], C.tx(f0 + 6, f0 + 7, 10, nonce=0)], [1, 1], [f0 + 40, tok2], 3)
    for reason, (txs, plan, idxs, index) in sorted(cases.items()):
        into = {name: np.full(shape, 0xA5, dtype=np.uint8) for name, shape in lg.shapes(len(txs), len(plan), 7)}
        with pytest.raises(HzError) as e:
            lg.apply_l2(txs, plan, idxs, n_sib=7, into=into)
        assert e.value.status == 4, (reason, str(e.value))
        assert "index %d " % index in str(e.value) and "reason %d:" % reason in str(e.value), (reason, str(e.value))
        assert all((a == 0xA5).all() for a in into.values()), reason
        assert lg.root() == root and (lg.accounts(everyone) == fields).all(), reason
        with pytest.raises(HzError):
            lg.outputs_dev()
    # a following valid call is as if the refused ones had not been made
    ok = [C.tx(f0 + 1, f0 + 2, 10, 176, nonce=0)]
    got = lg.apply_l2(ok, [1], [f0 + 40], n_sib=7)
    fresh = hz.ledger(6, first_idx=f0)
    fresh.load(*cols)
    exp = fresh.apply_l2(ok, [1], [f0 + 40], n_sib=7)
    C.assert_same(got, exp)
    assert D.to_int(got["old_root"][0]) == root and lg.root() == fresh.root()
    lg.close()
    fresh.close()


def test_argument_errors(hz):
    base = C.base_state(6)
    f0 = base.first_idx
    empty = hz.ledger(6, first_idx=f0)
    with pytest.raises(HzError) as e:
        empty.apply_l2([C.tx(f0, f0 + 1, 5)], [1], [0], n_sib=7)
    assert e.value.status == 1 and "hz_ledger_load" in str(e.value)
    empty.close()
    lg = base.to_ledger(hz)
    root = lg.root()
    many = [C.tx(f0 + i % 64, f0 + (i + 1) % 64, 1) for i in range(32769)]
    for txs, plan, idxs, n_sib, text in (([C.tx(f0, 0, 5)], [1], [0], 7, "not supported yet"), ([C.tx(f0, 1, 5)], [1], [0], 7, "not supported yet"),
                                          ([C.tx(f0, f0 + 64, 5)], [1], [0], 7, "outside the state"), ([C.tx(f0 - 1, f0, 5)], [1], [0], 7, "outside the state"),
                                          ([C.tx(f0, f0 + 1, 5)], [1], [f0 + 64], 7, "outside the state"), (many, [1], [0], 7, "updates in one call"),
                                          ([C.tx(f0, f0 + 1, 5)], [1], [0], 5, "n_sib"), ([C.tx(f0, f0 + 1, 5)], [1] * 65, [0] * 65, 7, "fee slots")):
        with pytest.raises(HzError) as e:
            lg.apply_l2(txs, plan, idxs, n_sib=n_sib)
        assert e.value.status == 1 and text in str(e.value), str(e.value)
    assert lg.root() == root
    lg.close()


def test_the_circuit_accepts_the_ledgers_inputs(hz):
    """l2_batch_inputs == BatchBuilder's dictionary key by key; the HIP rollup-main context and the oracle accept it; once more with the
    state-dependent signals handed over on the device"""
    from oracle_binding import OracleCtx
    shape = (8, 16, 2, 4)
    base = C.base_state(6)
    keys = base.keys()
    txs = C.draw_batch(base, 6, seed=77, pool=6)
    for t in txs:
        t["signer"] = keys[int(base.key_idx[t["fromIdx"] - base.first_idx])]
    fee_tokens, fee_idxs = [1], [base.first_idx + 20]
    db, bb = C.builder_batch(base, txs + [{}, {}], fee_tokens + [0] * 3, fee_idxs + [0] * 3, shape[1], max_l1=shape[2])
    exp = bb.get_input()
    lg = base.to_ledger(hz)
    like = types.SimpleNamespace(last_idx=base.first_idx + base.N - 1, num_batch=0)
    inp, _ = B.l2_batch_inputs(lg, like, txs, *shape, fee_tokens, fee_idxs, 1)
    assert set(inp) == set(exp), set(inp) ^ set(exp)
    for name in exp:
        assert inp[name] == exp[name], name
    g = hz.ctx("rollup-main", nTx=shape[0], nLevels=shape[1], maxL1Tx=shape[2], maxFeeTx=shape[3])
    g.set_inputs(inp)
    g.run()
    assert g.get("main.hashGlobalInputs") == bb.get_hash_inputs()
    witness = g.read_raw_bytes()
    o = OracleCtx("rollup-main", *shape)
    o.set_inputs(inp)
    assert o.run() is None
    # the same batch on a fresh ledger, the state-dependent signals never crossing the host
    lg2 = base.to_ledger(hz)
    like = types.SimpleNamespace(last_idx=base.first_idx + base.N - 1, num_batch=0)
    inp2, dev = B.l2_batch_inputs(lg2, like, txs, *shape, fee_tokens, fee_idxs, 1, host_outputs=False)
    assert set(inp2) | set(dev) == set(exp) and not set(inp2) & set(dev)
    g.clear_inputs()
    g.set_inputs(inp2)
    for name, (ptr, count) in dev.items():
        g.set_input_dev(name, ptr, count)
    g.run()
    assert g.read_raw_bytes() == witness
    lg.close()
    lg2.close()


def test_one_handle_regrows_its_call_buffers(hz):
    """3, 120 and 3 transfers with F = 2 on one ledger of k = 6, with n_sib = k, k + 3, k: the per-call buffers (the ledger's and its tree's)
    are grown by the second call and reused by the third; every output of every call, the zero padding beyond depth k included, the
    resident fields and the final tree are the builder's"""
    k = 6
    base = C.base_state(k)
    lg = base.to_ledger(hz)
    plan, idxs = [1, 0], [base.first_idx + 9, 0]
    rng, nonce, db = np.random.default_rng(77), {}, None
    for m, n_sib in [(3, k), (120, k + 3), (3, k)]:
        txs = []
        for i in range(m):
            f, t = (base.first_idx + int(x) for x in rng.integers(0, base.N, size=2))
            txs.append(C.tx(f, t, 1000 + i, C.SELECTORS[i % len(C.SELECTORS)], nonce=nonce.get(f, 0)))
            nonce[f] = nonce.get(f, 0) + 1
        db, _, got = _check(lg, base, txs, plan, idxs, db=db, n_levels=n_sib - 1)
        assert got["siblings1"].shape == (m, n_sib, 32) and got["siblings3"].shape == (2, n_sib, 32)
    _final_tree_matches(lg, base, db)
    lg.close()
