"""L1 deposits and forced transfers on the device-resident ledger (hz_ledger_apply_batch) against the Python BatchBuilder
over the same state with host hashing: every output array, the flag bytes, the root and the resident fields afterwards, on seeded batches
that hold every nullifier cause and on the named edges; refusals; the call without an L1 run against hz_ledger_apply_l2_addr byte for
byte; argument errors; 512 L1 transactions at once against the model; and the circuit itself (the HIP rollup-main context and the
oracle) on the inputs builder.ledger_batch_inputs makes. Every comparison is on bytes, bit-exact."""
import types

import numpy as np
import pytest

import device_state_common as D
import ledger_addr_common as A
import ledger_common as C
import ledger_l1_common as L1
import ledger_sig_common as S
from circuits_amd import HzError
from circuits_amd import builder as B

pytestmark = pytest.mark.gpu
N_LEVELS = 16
EDGES = ("underflow_chain", "deposit_transfer_spends_its_load", "load_nullified_then_underflow", "self_transfer", "from_eth_addr_mismatch",
         "receiver_token_mismatch", "zero_amount_deposit", "one_account_pair", "l2_funded_by_l1_deposit")


class _DevArr:
    """a device array of the library as torch sees it (CUDA array interface)"""
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _d2h(ptr, n, typestr="|u1"):
    import torch
    return torch.as_tensor(_DevArr(ptr, n, typestr), device="cuda:0").cpu().numpy()


def _check(lg, st, l1_txs, l2_txs, plan, idxs, n_tx=None):
    """one batch on the ledger and through the builder: all 27 arrays, auxToIdx, the flags, the root, the touched accounts"""
    n_l1 = len(l1_txs)
    l2 = list(l2_txs) + [{} for _ in range((n_tx or 0) - n_l1 - len(l2_txs))]
    got = lg.apply_batch(l1_txs, l2, plan, idxs, 1, 1, n_sib=N_LEVELS + 1)
    assert lg.l1_ms() > 0.0   # the device pointers are valid until the ledger's next call: read them now
    assert _d2h(lg.l1_flags_dev(), n_l1).tobytes() == got["l1_flags"].tobytes()
    assert _d2h(lg.outputs_dev()["balance1"], 32 * (n_l1 + len(l2))).tobytes() == got["balance1"].tobytes()
    db, bb = L1.builder_batch(st, l1_txs, l2, plan, idxs, N_LEVELS)
    exp = L1.expected_arrays(bb, l2, n_l1)
    assert len(exp) == 28 and set(exp) <= set(got)
    C.assert_same(got, exp)
    assert got["l1_flags"].tolist() == L1.builder_flags(bb, n_l1)
    assert lg.root() == bb.new_state_root
    acc = L1.touched(l1_txs, l2, idxs)
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


@pytest.mark.parametrize("n", range(len(L1.SEEDS)))
def test_parity_with_the_builder(hz, n):
    k, st, l1_txs, l2_txs = L1.seeded_batches()[n]
    lg = st.to_ledger(hz)
    db, bb, got = _check(lg, st, l1_txs, l2_txs, [1, 2, 0, 0], L1.fee_accounts(st), n_tx=len(l1_txs) + len(l2_txs) + 1)
    res = L1.scheme_model(st.state, l1_txs, l2_txs, [1, 2, 0, 0], L1.fee_accounts(st))
    assert got["l1_flags"].tolist() == res[4]
    _final_tree_matches(lg, st, db)
    lg.close()


@pytest.mark.parametrize("name", EDGES)
def test_named_edges(hz, name):
    sp = A.special_state(6)
    f0 = sp.first_idx
    l1_txs, l2_txs = L1.edge_batches(sp)[name]
    lg = sp.to_ledger(hz)
    db, bb, got = _check(lg, sp, l1_txs, l2_txs, [1, 2], [f0 + 40, 0])
    nullified = [(f >> 1) & 1 for f in got["l1_flags"].tolist()]
    if name == "underflow_chain":
        assert nullified == [1, 1, 0]
    if name == "receiver_token_mismatch":   # the receiver row is present, and keeps its balance
        assert nullified == [1] and got["siblings2"][0].any() and int(got["tokenID2"][0][0]) == 2
        assert D.to_int(got["balance2"][0]) == sp.state(f0 + 9)["balance"] == D.to_int(lg.accounts([f0 + 9])[0][1])
    if name == "zero_amount_deposit":       # processor 2 is a NOP: all six leaf-2 rows are zero, tokenID2 too
        assert not any(got[f + "2"][:2].any() for f in C.LEAF) and not got["siblings2"][:2].any()
    if name == "l2_funded_by_l1_deposit":
        assert nullified == [0] and D.to_int(got["balance1"][1]) == sp.state(f0 + 1)["balance"] + L1.load_of(l1_txs[0])
    _final_tree_matches(lg, sp, db)
    lg.close()


def test_l2_refused_after_a_nullified_l1_transfer(hz):
    """the L2 transfer that counted on a nullified L1 transfer is refused with reason 3 at its own row; nothing is written"""
    sp = A.special_state(6)
    f0 = sp.first_idx
    l1_txs, l2_txs = L1.refused_after_nullified(sp)
    assert L1.scheme_model(sp.state, l1_txs, l2_txs, [1], [f0 + 40])[:3] == ("refused", 2, 3)
    lg = sp.to_ledger(hz)
    root = lg.root()
    everyone = np.arange(f0, f0 + sp.N)
    fields = lg.accounts(everyone)
    into = {name: np.full(shape, 0xA5, dtype=np.uint8) for name, shape in lg.shapes(3, 1, 7)}
    into.update(auxToIdx=np.full((3, 32), 0xA5, dtype=np.uint8), l1_flags=np.full(1, 0xA5, dtype=np.uint8))
    with pytest.raises(HzError) as e:
        lg.apply_batch(l1_txs, l2_txs, [1], [f0 + 40], 1, 1, n_sib=7, into=into)
    assert e.value.status == 4 and "index 2 " in str(e.value) and "reason 3:" in str(e.value), str(e.value)
    assert all((a == 0xA5).all() for a in into.values())
    assert lg.root() == root and (lg.accounts(everyone) == fields).all()
    for call in (lg.outputs_dev, lg.aux_to_idx_dev, lg.l1_flags_dev):
        with pytest.raises(HzError):
            call()
    # without that transfer the batch goes through, on the ledger that refused
    db, bb, got = _check(lg, sp, l1_txs, l2_txs[:1], [1], [f0 + 40])
    assert got["l1_flags"].tolist() == [2]
    lg.close()


def test_without_an_l1_run_it_is_apply_l2_addr(hz):
    st = A.mixed_state(6)
    txs = A.draw_batch(st, 20, seed=3, pool=30)
    assert sum(A.is_to_addr(t) for t in txs) >= 4
    plan, idxs = [1, 2], L1.fee_accounts(st)[:2]
    a, b = st.to_ledger(hz), st.to_ledger(hz)
    got_a = a.apply_l2_addr(txs, plan, idxs, 1, 1, n_sib=7)
    got_b = b.apply_batch([], txs, plan, idxs, 1, 1, n_sib=7)
    assert set(got_b) == set(got_a) | {"l1_flags"} and got_b["l1_flags"].size == 0
    for name in got_a:
        assert got_a[name].tobytes() == got_b[name].tobytes(), name
    everyone = np.arange(st.first_idx, st.first_idx + st.N)
    assert a.root() == b.root() and (a.accounts(everyone) == b.accounts(everyone)).all() and b.l1_ms() == 0.0
    # verified signatures too; and no hz_l2sig array at all where no destination is signed
    base = C.base_state(6)
    signed = S.signed_batch(base, 12, seed=5)
    c, d = base.to_ledger(hz), base.to_ledger(hz)
    got_c = c.apply_l2_addr(signed, [1], [0], 1, 1, n_sib=7, verify=True)
    got_d = d.apply_batch([], signed, [1], [0], 1, 1, n_sib=7, verify=True)
    for name in got_c:
        assert got_c[name].tobytes() == got_d[name].tobytes(), name
    plain = C.draw_batch(base, 12, seed=6)
    e, f = base.to_ledger(hz), base.to_ledger(hz)
    got_e = e.apply_l2_addr(plain, [1], [0], 1, 1, n_sib=7)
    got_f = f.apply_batch([], plain, [1], [0], 1, 1, n_sib=7, sigs=False)
    for name in got_e:
        assert got_e[name].tobytes() == got_f[name].tobytes(), name
    assert c.root() == d.root() and e.root() == f.root()
    for lg in (a, b, c, d, e, f):
        lg.close()


def test_argument_errors_and_reason_5(hz):
    rs = L1.rich_state(6)
    f0, leaf = rs.first_idx, rs.state
    lg = rs.to_ledger(hz)
    root = lg.root()
    ok = L1.own(rs, f0 + 3, f0 + 4, 10)
    to7 = A.to_addr(C.tx(f0 + 3, 0, 5, nonce=0), leaf(f0 + 7))
    for l1_txs, l2_txs, text in (([dict(ok, fromIdx=0)], [], "creates an account"), ([dict(ok, toIdx=1)], [], "an exit"),
                                 ([dict(ok, fromIdx=f0 + 64)], [], "outside the state"), ([dict(ok, toIdx=f0 + 64)], [], "outside the state"),
                                 ([dict(ok, toIdx=5)], [], "outside the state"), ([dict(ok, amountF=1 << 40)], [], "amount_f has more than 40 bits"),
                                 ([dict(ok, loadAmountF=1 << 40)], [], "load_amount_f has more than 40 bits"),
                                 ([dict(ok, fromEthAddr=1 << 160)], [], "more than 160 bits"), ([ok] * 513, [], "at most 512"),
                                 ([dict(ok, toIdx=0)], [], "no receiver"), ([ok], [C.tx(f0 + 3, 1, 5)], "not supported yet"),
                                 ([ok], [C.tx(f0 + 3, f0 + 64, 5)], "outside the state")):
        with pytest.raises(HzError) as e:
            lg.apply_batch(l1_txs, l2_txs, [1], [0], 1, 1, n_sib=7)
        assert e.value.status == 1 and text in str(e.value), str(e.value)
    with pytest.raises(HzError) as e:   # too many updates: the L1 events count
        lg.apply_batch([ok], [C.tx(f0 + 3, f0 + 4, 5)] * 32767 + [C.tx(f0 + 3, f0 + 4, 0)], [1], [0], 1, 1, n_sib=7, outputs=False)
    assert e.value.status == 1 and "updates in one call" in str(e.value), str(e.value)
    with pytest.raises(HzError) as e:
        lg.apply_batch([ok], [to7], [1], [0], 1, 1, n_sib=7, sigs=False)
    assert e.value.status == 1 and "null sigs" in str(e.value), str(e.value)
    with pytest.raises(HzError) as e:
        lg.l1_flags_dev()
    assert e.value.status == 1 and "hz_ledger_apply_batch" in str(e.value)
    # reason 9 keeps its precedence: it is reported whatever else is wrong, at the L2 transaction's row
    nobody = dict(C.tx(f0 + 3, 0, 5, nonce=0), toEthAddr=12345)
    with pytest.raises(HzError) as e:
        lg.apply_batch([ok, L1.own(rs, f0 + 1, 0, 0, load=5000)], [C.tx(f0 + 4, f0 + 3, 1, nonce=9), nobody], [1], [0], 1, 1, n_sib=7)
    assert e.value.status == 4 and "index 3 " in str(e.value) and "reason 9:" in str(e.value), str(e.value)
    # reason 5 through loadAmount: account f0 + 1 holds 2^192 - 1000
    l1_txs = [ok, L1.own(rs, f0 + 1, 0, 0, load=5000)]
    assert L1.scheme_model(rs.state, l1_txs, [], [1], [0])[:3] == ("refused", 1, 5)
    with pytest.raises(HzError) as e:
        lg.apply_batch(l1_txs, [], [1], [0], 1, 1, n_sib=7)
    assert e.value.status == 4 and "index 1 " in str(e.value) and "reason 5:" in str(e.value), str(e.value)
    assert lg.root() == root
    # a load the same transaction passes on leaves the balance below 2^192: accepted
    got = lg.apply_batch([L1.own(rs, f0 + 1, f0 + 3, 5000, load=5000)], [], [1], [0], 1, 1, n_sib=7)
    assert got["l1_flags"].tolist() == [0] and lg.l1_ms() > 0.0
    assert D.to_int(lg.accounts([f0 + 1])[0][1]) == (1 << 192) - 1000 and lg.l1_ms() == 0.0   # the ledger has been used otherwise since
    lg.apply_batch([ok], [], [1], [0], 1, 1, n_sib=7)
    assert lg.l1_ms() > 0.0
    with pytest.raises(HzError):   # l1_ms is the last call's: not the time of the batch before a refused one
        lg.apply_batch([ok, L1.own(rs, f0 + 1, 0, 0, load=5000)], [], [1], [0], 1, 1, n_sib=7)
    assert lg.l1_ms() == 0.0
    lg.apply_batch([ok], [], [1], [0], 1, 1, n_sib=7)
    with pytest.raises(HzError):
        lg.apply_batch([dict(ok, toIdx=1)], [], [1], [0], 1, 1, n_sib=7)
    assert lg.l1_ms() == 0.0
    lg.close()


def _model_fields(st, after):
    cols = [np.array(c) for c in st.leaf_fields()]
    for a, leaf in after.items():
        for c, v in enumerate(B.leaf_fields(leaf)):
            cols[c][a - st.first_idx] = D.to_bytes([v])[0]
    return cols


def test_capacity_512_l1_transactions(hz):
    """HZ_LEDGER_MAX_L1 transactions, each with an amount, a sender and a receiver of its own: 1024 distinct accounts, every local slot of
    the kernel's LDS in use; then 512 on one pair of accounts (the longest chain): fields and flags against the model, the root against
    a second ledger loaded with the model's fields. No Python hashing"""
    k = 11
    st = C.base_state(k)
    f0 = st.first_idx
    rng = np.random.default_rng(11)
    accounts = f0 + rng.permutation(st.N)[:1024]
    l1_txs = []
    for i in range(512):
        frm, to = int(accounts[2 * i]), int(accounts[2 * i + 1])
        bal, kind = st.state(frm)["balance"], i % 8
        amount = L1.float_floor(2 * bal + 10) if kind == 2 else L1.float_floor(bal // 3)   # never zero: every receiver takes a slot
        l1_txs.append(L1.own(st, frm, to, amount, load=L1.float_floor(bal // 7) if kind in (1, 3, 6) else 0, token=2 if kind == 3 else None,
                             eth=5 if kind == 4 else None))
    assert all(L1.has_amount(t) for t in l1_txs)
    plan = hz.ledger_plan_batch(l1_txs, [], [1], [0], k, first_idx=f0)
    assert plan["slot_account"].size == 1024 and int(plan["l1_slot_receiver"].max()) == 1023 and len(set(plan["slot_account"].tolist())) == 1024
    res = L1.scheme_model(st.state, l1_txs, [], [1], [0])
    assert res[0] == "ok" and len(res[5]) == 1024 and {0, 2, 3} == set(res[4])   # (a nullified load alone needs a zero amount: a named edge)
    lg = st.to_ledger(hz)
    got = lg.apply_batch(l1_txs, [], [1], [0], 1, 1, n_sib=k)
    assert got["l1_flags"].tolist() == res[4]
    everyone = np.arange(f0, f0 + st.N)
    cols = _model_fields(st, res[5])
    assert (lg.accounts(everyone) == np.stack(cols, axis=1)).all()
    for name in ("balance1", "balance2", "tokenID1", "tokenID2"):
        assert [D.to_int(r) for r in got[name]] == res[1][name], name
    other = hz.ledger(k, first_idx=f0)
    other.load(*cols)
    assert lg.root() == other.root() == D.to_int(got["new_root"][0])
    # one pair, 512 times: every step reads what the step before it wrote
    a, b = int(accounts[0]), int(accounts[1])
    leaf_of = lambda i: dict(st.state(i), **{f: v for f, v in res[5].get(i, {}).items()})   # noqa: E731
    pair = []
    for i in range(512):
        frm, to = (a, b) if i % 2 == 0 else (b, a)
        pair.append(L1.own(st, frm, to, L1.float_floor(st.state(a)["balance"] // (2 + i % 5)) if i % 7 else L1.float_floor(3 * (st.state(a)["balance"] + st.state(b)["balance"]))))
    res2 = L1.scheme_model(leaf_of, pair, [], [1], [0])
    assert res2[0] == "ok" and 74 <= sum(f >> 1 for f in res2[4]) < 512
    got = lg.apply_batch(pair, [], [1], [0], 1, 1, n_sib=k)
    assert got["l1_flags"].tolist() == res2[4]
    assert [D.to_int(r) for r in got["balance1"]] == res2[1]["balance1"] and [D.to_int(r) for r in got["balance2"]] == res2[1]["balance2"]
    cols = _model_fields(st, {**res[5], **res2[5]})
    assert (lg.accounts(everyone) == np.stack(cols, axis=1)).all()
    other.load(*cols)
    assert lg.root() == other.root()
    lg.close()
    other.close()


def test_the_circuit_accepts_the_ledgers_inputs(hz):
    """rollup-main at (8, 16, 4, 4): a deposit, a forceTransfer nullified by underflow and a depositTransfer, then three signed L2
    transfers (one to an address) and NOPs. ledger_batch_inputs == BatchBuilder's dictionary signal for signal; the HIP context and the
    oracle accept; hashGlobalInputs is the builder's; once more with every state-dependent signal left on the device"""
    from oracle_binding import OracleCtx
    shape = (8, 16, 4, 4)
    sp = A.special_state(6)
    f0, leaf = sp.first_idx, sp.state
    a, b, c = f0 + 1, f0 + 3, f0 + 4
    l1_txs = [L1.own(sp, a, 0, 0, load=70000), L1.own(sp, b, c, L1.float_floor(2 * leaf(b)["balance"] + 10)),
              L1.own(sp, c, a, L1.float_floor(leaf(c)["balance"] // 4), load=900)]
    l2_txs = [C.tx(a, b, 1000, 176, nonce=0), A.to_addr(C.tx(a, 0, 2000, 100, nonce=1), leaf(f0 + 7)), C.tx(c, a, 30, 0, nonce=0)]
    for t in l2_txs:
        t["signer"] = S.signer(sp, t["fromIdx"])
    fee_tokens, fee_idxs = [1], [f0 + 20]
    db, bb = L1.builder_batch(sp, l1_txs, l2_txs, fee_tokens + [0] * 3, fee_idxs + [0] * 3, shape[1], n_tx=shape[0], max_l1=shape[2])
    exp = bb.get_input()
    assert [m["isAmountNullified"] for m in bb.tx_meta] == [0, 1, 0, 0, 0, 0, 0, 0] and exp["onChain"] == [1, 1, 1, 0, 0, 0, 0, 0]
    lg = sp.to_ledger(hz)
    like = types.SimpleNamespace(last_idx=f0 + sp.N - 1, num_batch=0)
    inp, _, nullified = B.ledger_batch_inputs(lg, like, l1_txs, l2_txs, *shape, fee_tokens, fee_idxs, 1, verify=True)
    assert set(inp) == set(exp), set(inp) ^ set(exp)
    for name in exp:
        assert inp[name] == exp[name], name
    assert nullified == [m["isAmountNullified"] for m in bb.tx_meta]
    assert B.hash_global_inputs(inp, nullified, like.last_idx, lg.root(), 0, *shape) == bb.get_hash_inputs()
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
    inp2, dev, _ = B.ledger_batch_inputs(lg2, like, l1_txs, l2_txs, *shape, fee_tokens, fee_idxs, 1, host_outputs=False, verify=True)
    assert set(inp2) | set(dev) == set(exp) and not set(inp2) & set(dev) and "auxToIdx" in dev and "balance2" in dev
    g.clear_inputs()
    g.set_inputs(inp2)
    for name, (ptr, count) in dev.items():
        g.set_input_dev(name, ptr, count)
    g.run()
    assert g.read_raw_bytes() == witness
    lg.close()
    lg2.close()
