"""L2 exits and L1 forceExits on the device-resident ledger (hz_ledger_apply_batch_exits) against the Python BatchBuilder over
the same state with host hashing: all 27 arrays, the six exit arrays, auxToIdx, the L1 flags, the state root and the exit root, the touched
accounts, the exit leaves, and the device pointers against the host copies, on seeded batches that mix every row kind and on the named
edges; refusals; a batch without exits against hz_ledger_apply_batch byte for byte; the existing calls; argument errors; 512 forceExits at
once against the model; the circuit itself (the HIP rollup-main context and the oracle) on the inputs builder.ledger_exit_batch_inputs
makes; and Withdraw over the ledger's exit tree. Every comparison is on bytes, bit-exact.

Reason 5 on an exit leaf. The case the feature was specified with -- an account of balance 2^192 - 1 exits all of it, is refilled and
exits again -- cannot be built: an amount is a float40, below 2^138, so no row moves 2^192 - 1, and an exit leaf starts every batch at 0
and takes at most 65536 amounts, so it stays below 2^154 (tests/test_ledger_exit_cpu.py asserts the arithmetic). The scan keeps the
check; it is exercised at the boundary by the model and by tests/native/ledger_exit_check.cpp on values passed in, not here."""
import types

import numpy as np
import pytest

import device_state_common as D
import ledger_addr_common as A
import ledger_common as C
import ledger_exit_common as X
import ledger_l1_common as L1
import ledger_sig_common as S
from circuits_amd import HzError
from circuits_amd import builder as B

pytestmark = pytest.mark.gpu
N_LEVELS = 16


class _DevArr:
    """a device array of the library as torch sees it (CUDA array interface)"""
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _d2h(ptr, n, typestr="|u1"):
    import torch
    return torch.as_tensor(_DevArr(ptr, n, typestr), device="cuda:0").cpu().numpy()


def _check(lg, st, l1_txs, l2_txs, plan, idxs, n_tx=None):
    """one batch on the ledger and through the builder: the 27 arrays, the six exit arrays, auxToIdx, the flags, both roots, the touched
    accounts, the exit leaves; the device pointers against the host copies"""
    n_l1 = len(l1_txs)
    l2 = list(l2_txs) + [{} for _ in range((n_tx or 0) - n_l1 - len(l2_txs))]
    R = n_l1 + len(l2)
    got = lg.apply_batch_exits(l1_txs, l2, plan, idxs, 1, 1, n_sib=N_LEVELS + 1)
    exit_ms = lg.exit_ms()
    xdev = lg.exit_outputs_dev()   # the device pointers are valid until the ledger's next call: read them now
    for name in X.EXIT_ARRAYS:
        assert _d2h(xdev[name], 32 * (1 if name == "new_exit_root" else R)).tobytes() == got[name].tobytes(), name
    dev = lg.outputs_dev()
    for name in ("balance2", "tokenID2", "ethAddr2"):
        assert _d2h(dev[name], 32 * R).tobytes() == got[name].tobytes(), name
    assert _d2h(dev["siblings2"], 32 * R * (N_LEVELS + 1)).tobytes() == got["siblings2"].tobytes()
    if n_l1:
        assert _d2h(lg.l1_flags_dev(), n_l1).tobytes() == got["l1_flags"].tobytes()
    db, bb = X.builder_batch(st, l1_txs, l2, plan, idxs, N_LEVELS)
    exp = X.expected_arrays(bb, l2, n_l1)
    assert len(exp) == 34 and set(exp) <= set(got)
    C.assert_same(got, exp)
    assert got["l1_flags"].tolist() == L1.builder_flags(bb, n_l1)
    assert lg.root() == bb.new_state_root
    tree = lg.exit_tree()
    assert tree.root() == bb.new_exit_root == D.to_int(got["new_exit_root"][0]) and tree.size() == len(bb.exit_leaves)
    acc = X.touched(st, l1_txs, l2, idxs)
    assert (lg.accounts(acc) == C.leaf_rows(db, acc)).all()
    keys = sorted(bb.exit_leaves)
    if keys:
        assert (lg.exit_accounts(keys) == X.exit_leaf_rows(bb, keys)).all()
    assert (exit_ms > 0.0) == bool(keys)
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


@pytest.mark.parametrize("n", range(len(X.SEEDS)))
def test_parity_with_the_builder(hz, n):
    k, st, l1_txs, l2_txs = X.seeded_batches()[n]
    lg = st.to_ledger(hz)
    db, bb, got = _check(lg, st, l1_txs, l2_txs, [1, 2, 0, 0], L1.fee_accounts(st), n_tx=len(l1_txs) + len(l2_txs) + 1)
    assert X.kinds_of(bb, l1_txs, l2_txs) & {"force_exit", "l2_exit"}
    _final_tree_matches(lg, st, db)
    lg.close()


@pytest.mark.parametrize("name", X.EDGES)
def test_named_edges(hz, name):
    sp = X.exit_state(6)
    f0 = sp.first_idx
    a = f0 + 1
    l1_txs, l2_txs = X.edge_batches(sp)[name]
    lg = sp.to_ledger(hz)
    db, bb, got = _check(lg, sp, l1_txs, l2_txs, [1, 2], [f0 + 40, 0])
    ints = lambda arr: [D.to_int(r) for r in got[arr]]   # noqa: E731
    if name == "first_exit_into_empty_tree":
        assert ints("new_exit") == [1] and ints("is_old0_2") == [1] and ints("old_key2") == [0] and ints("exit_root_after")[0] != 0
    if name in ("second_key_meets_a_leaf", "keys_sharing_low_bits"):
        assert ints("is_old0_2") == [1, 0] and ints("old_key2") == [0, a] and ints("old_value2")[1] == B.hash_state(bb.exit_leaves[a])
    if name == "same_account_twice":
        assert ints("new_exit") == [1, 0, 0] and ints("balance2")[2] == L1.amount_of(l2_txs[0]) and got["siblings2"][1].any()   # (row 1 is a transfer)
        assert ints("exit_root_after")[0] == ints("exit_root_after")[1] != ints("exit_root_after")[2]
    if name == "zero_amount_exit":
        assert ints("tokenID2") == [0, 1] and not got["siblings2"].any() and ints("exit_root_after") == [0, 0] and lg.exit_tree().size() == 0
    if name == "exit_whole_balance_with_fee":
        assert D.to_int(lg.accounts([f0 + 6])[0][1]) == 0 and D.to_int(lg.exit_accounts([f0 + 6])[0][1]) == X.WHOLE
    if name.startswith("force_exit_nullified"):   # an insert with balance 0 and flag bit 1
        assert got["l1_flags"].tolist() == [2] and ints("new_exit") == [1] and D.to_int(lg.exit_accounts([a])[0][1]) == 0
    if name == "force_exit_then_l2_exit_same_idx":
        assert ints("new_exit") == [1, 0] and ints("balance2")[1] == L1.amount_of(l1_txs[0])
    if name == "nullified_force_exit_then_l2_exit":   # an update from 0
        assert ints("new_exit") == [1, 0] and ints("balance2")[1] == 0 and ints("tokenID2")[1] == 1
    _final_tree_matches(lg, sp, db)
    lg.close()


def test_a_refused_batch_writes_nothing_and_leaves_the_exit_tree_empty(hz):
    """an L2 exit above the sender's balance is reason 3 at its row: the root, the fields of all 64 accounts and the output buffers
    pre-filled with 0xA5 are unchanged, and the exit tree -- which held the batch before -- is empty afterwards"""
    sp = X.exit_state(6)
    f0 = sp.first_idx
    lg = sp.to_ledger(hz)
    db, bb, _ = _check(lg, sp, [], [X.x2(f0 + 3, 500, nonce=0)], [1], [f0 + 40])
    assert lg.exit_tree().size() == 1
    root = lg.root()
    everyone = np.arange(f0, f0 + sp.N)
    fields = lg.accounts(everyone)
    leaf = lambda i: db.leaves[i] if i in db.leaves else sp.state(i)   # noqa: E731
    l1_txs = [X.fx(sp, f0 + 4, 1000)]
    over = [C.tx(f0 + 8, f0 + 4, 5, nonce=0), X.x2(f0 + 1, L1.float_floor(2 * leaf(f0 + 1)["balance"]), nonce=0), X.x2(f0 + 3, 5, nonce=1)]
    assert X.scheme_model(leaf, l1_txs, over, [1], [f0 + 40])[:3] == ("refused", 2, 3)
    into = {name: np.full(shape, 0xA5, dtype=np.uint8) for name, shape in lg.shapes(4, 1, 7)}
    into.update(auxToIdx=np.full((4, 32), 0xA5, dtype=np.uint8), l1_flags=np.full(1, 0xA5, dtype=np.uint8))
    into.update({name: np.full((1 if name == "new_exit_root" else 4, 32), 0xA5, dtype=np.uint8) for name in X.EXIT_ARRAYS})
    with pytest.raises(HzError) as e:
        lg.apply_batch_exits(l1_txs, over, [1], [f0 + 40], 1, 1, n_sib=7, into=into)
    assert e.value.status == 4 and "index 2 " in str(e.value) and "reason 3:" in str(e.value), str(e.value)
    assert len(into) == 35 and all((arr == 0xA5).all() for arr in into.values())
    assert lg.root() == root and (lg.accounts(everyone) == fields).all()
    tree = lg.exit_tree()
    assert tree.size() == 0 and tree.root() == 0 and lg.exit_ms() == 0.0
    for call in (lg.outputs_dev, lg.exit_outputs_dev, lg.aux_to_idx_dev, lg.l1_flags_dev, lambda: lg.exit_accounts([f0 + 3])):
        with pytest.raises(HzError):
            call()
    # without that exit the batch goes through, on the ledger that refused, from the empty exit tree
    got = lg.apply_batch_exits(l1_txs, [over[0], over[2]], [1], [f0 + 40], 1, 1, n_sib=7)
    assert [D.to_int(r) for r in got["new_exit"]] == [1, 0, 1] and lg.exit_tree().size() == 2
    lg.close()


def test_a_batch_without_exits_is_apply_batch(hz):
    k, st, l1_txs, l2_txs = L1.seeded_batches()[0]
    plan, idxs = [1, 2, 0, 0], L1.fee_accounts(st)
    a, b = st.to_ledger(hz), st.to_ledger(hz)
    got_a = a.apply_batch(l1_txs, l2_txs, plan, idxs, 1, 1, n_sib=k + 1)
    got_b = b.apply_batch_exits(l1_txs, l2_txs, plan, idxs, 1, 1, n_sib=k + 1)
    assert set(got_b) == set(got_a) | set(X.EXIT_ARRAYS)
    for name in got_a:
        assert got_a[name].tobytes() == got_b[name].tobytes(), name
    assert not any(got_b[name].any() for name in X.EXIT_ARRAYS)
    xdev = b.exit_outputs_dev()
    assert not _d2h(xdev["exit_root_after"], 32 * (len(l1_txs) + len(l2_txs))).any() and not _d2h(xdev["new_exit_root"], 32).any()
    everyone = np.arange(st.first_idx, st.first_idx + st.N)
    assert a.root() == b.root() and (a.accounts(everyone) == b.accounts(everyone)).all()
    assert b.exit_tree().size() == 0 and b.exit_tree().root() == 0 and b.exit_ms() == 0.0
    # signatures verified, and a batch of L2 transfers alone
    base = C.base_state(6)
    signed = S.signed_batch(base, 12, seed=5)
    c, d = base.to_ledger(hz), base.to_ledger(hz)
    got_c = c.apply_batch([], signed, [1], [0], 1, 1, n_sib=7, verify=True)
    got_d = d.apply_batch_exits([], signed, [1], [0], 1, 1, n_sib=7, verify=True)
    for name in got_c:
        assert got_c[name].tobytes() == got_d[name].tobytes(), name
    assert c.root() == d.root()
    for lg in (a, b, c, d):
        lg.close()


def test_the_existing_calls_keep_refusing_an_exit(hz):
    sp = X.exit_state(6)
    f0 = sp.first_idx
    lg = sp.to_ledger(hz)
    root = lg.root()
    ex = S.sign(sp, X.x2(f0 + 3, 5, nonce=0))
    ok = L1.own(sp, f0 + 3, f0 + 4, 10)
    for call in (lambda: lg.apply_l2([ex], [1], [0], n_sib=7), lambda: lg.apply_l2_signed([ex], [1], [0], 1, 1, n_sib=7),
                 lambda: lg.apply_l2_addr([ex], [1], [0], 1, 1, n_sib=7), lambda: lg.apply_batch([ok], [ex], [1], [0], 1, 1, n_sib=7),
                 lambda: lg.apply_batch([X.fx(sp, f0 + 3, 10)], [], [1], [0], 1, 1, n_sib=7), lambda: lg.verify_l2([ex], 1, 1)):
        with pytest.raises(HzError) as e:
            call()
        assert e.value.status == 1 and "an exit" in str(e.value) and "not supported yet" in str(e.value), str(e.value)
    assert lg.resolve_l2([ex]).tolist() == [0]   # the lookup refuses nothing and never looks at an exit
    assert lg.root() == root
    # the new call takes the same signed exit, verified on the device: the signed message carries to_idx = 1
    got = lg.apply_batch_exits([], [ex], [1], [0], 1, 1, n_sib=7, verify=True)
    assert D.to_int(got["tx_compressed_data"][0]) == B.build_tx_compressed_data(ex, 1) and D.to_int(got["sig_l2_hash"][0]) == B.build_hash_sig(ex, 1)
    with pytest.raises(HzError) as e:
        lg.apply_batch_exits([], [dict(ex, nonce=1, s=ex["s"] ^ 1)], [1], [0], 1, 1, n_sib=7, verify=True)
    assert e.value.status == 4 and "reason 7:" in str(e.value), str(e.value)
    # and an apply of the other five empties the exit tree: it is the last batch's
    lg.apply_batch_exits([], [dict(X.x2(f0 + 3, 5), nonce=1)], [1], [0], 1, 1, n_sib=7)
    assert lg.exit_tree().size() == 1
    lg.apply_l2([C.tx(f0 + 3, f0 + 4, 5, nonce=2)], [1], [0], n_sib=7)
    assert lg.exit_tree().size() == 0
    with pytest.raises(HzError):
        lg.exit_accounts([f0 + 3])
    lg.close()


def test_argument_errors(hz):
    sp = X.exit_state(6)
    f0 = sp.first_idx
    lg = sp.to_ledger(hz)
    root = lg.root()
    with pytest.raises(HzError) as e:
        lg.exit_outputs_dev()
    assert e.value.status == 1 and "hz_ledger_apply_batch_exits" in str(e.value)
    ok, ex = X.fx(sp, f0 + 3, 10), X.x2(f0 + 3, 5, nonce=0)
    for l1_txs, l2_txs, text in (([dict(ok, fromIdx=0)], [], "creates an account"), ([dict(ok, fromIdx=f0 + 64)], [], "outside the state"),
                                 ([dict(ok, amountF=1 << 40)], [], "amount_f has more than 40 bits"), ([dict(ok, fromEthAddr=1 << 160)], [], "more than 160 bits"),
                                 ([ok] * 513, [], "at most 512"), ([], [dict(ex, fromIdx=f0 + 64)], "outside the state"),
                                 ([], [dict(ex, amountF=1 << 40)], "amount_f has more than 40 bits"), ([], [C.tx(f0 + 3, 5, 5)], "outside the state")):
        with pytest.raises(HzError) as e:
            lg.apply_batch_exits(l1_txs, l2_txs, [1], [0], 1, 1, n_sib=7)
        assert e.value.status == 1 and text in str(e.value), str(e.value)
    with pytest.raises(HzError) as e:   # too many updates: an exit operation counts as the receiver's update would
        lg.apply_batch_exits([ok], [ex] * 32767 + [dict(ex, amountF=0)], [1], [0], 1, 1, n_sib=7, outputs=False)
    assert e.value.status == 1 and "updates in one call" in str(e.value), str(e.value)
    # the leaf pair of f0 + 1 and f0 + 33 hangs at depth 6: an argument error from the planner, before anything is launched
    pair = [X.x2(f0 + 1, 5, nonce=0), X.x2(f0 + 33, 5, nonce=0)]
    with pytest.raises(HzError) as e:
        lg.apply_batch_exits([], pair, [1], [0], 1, 1, n_sib=6)
    assert e.value.status == 1 and "depth >= n_sib = 6" in str(e.value), str(e.value)
    assert lg.root() == root and lg.exit_tree().size() == 0
    got = lg.apply_batch_exits([], pair, [1], [0], 1, 1, n_sib=7)
    assert [D.to_int(r) for r in got["old_key2"]] == [0, f0 + 1] and lg.exit_tree().size() == 2
    with pytest.raises(HzError) as e:
        lg.exit_accounts([f0 + 1, f0 + 2])
    assert e.value.status == 1 and "key[1]" in str(e.value) and "not in the exit tree" in str(e.value), str(e.value)
    assert lg.exit_accounts([]).shape == (0, 4, 32)
    lg.close()


def test_capacity_512_force_exits_on_32_senders(hz):
    """HZ_LEDGER_MAX_L1 forceExits, sixteen on each of 32 senders -- valid, nullified by token, by address and by underflow, of zero amount --:
    flags, the leaf rows, newExit, the accounts and the exit leaves against the scheme model. No Python hashing: the exit root is
    checked against a sparse tree that is given the model's leaves"""
    sp = X.exit_state(6)
    f0 = sp.first_idx
    senders = [f0 + 10 + i for i in range(32)]
    l1_txs = []
    for r in range(16):
        for i, s in enumerate(senders):
            bal, kind = sp.state(s)["balance"], (r + i) % 8
            amount = L1.float_floor(3 * bal) if kind == 2 else 0 if kind == 5 else L1.float_floor(bal // 40)
            l1_txs.append(X.fx(sp, s, amount, load=L1.float_floor(bal // 50) if kind in (1, 3) else 0, token=7 if kind == 3 else None,
                               eth=5 if kind == 4 else None))
    assert len(l1_txs) == 512
    res = X.scheme_model(sp.state, l1_txs, [], [1], [0])
    assert res[0] == "ok" and len(res[7]) == 32 and {0, 1, 2, 3} >= set(res[4]) >= {0, 2, 3} and sum(res[6]) == 32
    lg = sp.to_ledger(hz)
    got = lg.apply_batch_exits(l1_txs, [], [1], [0], 1, 1, n_sib=N_LEVELS + 1)
    assert got["l1_flags"].tolist() == res[4] and [D.to_int(r) for r in got["new_exit"]] == res[6]
    for name in ("balance1", "balance2", "tokenID2", "sign2", "ay2", "ethAddr2", "nonce2"):
        assert [D.to_int(r) for r in got[name]] == res[1][name], name
    roots = [D.to_int(r) for r in got["exit_root_after"]]
    assert roots[-1] == D.to_int(got["new_exit_root"][0]) == lg.exit_tree().root() and lg.exit_tree().size() == 32
    assert all(roots[i] == roots[i - 1] for i in range(1, 512) if not L1.has_amount(l1_txs[i]))
    keys = sorted(res[7])
    model_rows = np.stack([C.to_bytes(B.leaf_fields(res[7][key])) for key in keys])
    assert (lg.exit_accounts(keys) == model_rows).all()
    assert (lg.accounts(senders) == np.stack([C.to_bytes(B.leaf_fields(res[5][s])) for s in senders])).all()
    other = hz.smt(N_LEVELS + 1)
    other.apply(keys, model_rows)
    assert other.root() == roots[-1]
    other.close()
    lg.close()


def _circuit_batch(sp):
    f0, leaf = sp.first_idx, sp.state
    a, b, c = f0 + 1, f0 + 3, f0 + 4
    l1_txs = [L1.own(sp, a, 0, 0, load=70000), X.fx(sp, b, L1.float_floor(leaf(b)["balance"] // 4), load=900),
              X.fx(sp, c, L1.float_floor(2 * leaf(c)["balance"] + 10))]
    l2_txs = [C.tx(a, b, 1000, 176, nonce=0), X.x2(a, 3000, 100, nonce=1), X.x2(b, 2000, 176, nonce=0), A.to_addr(C.tx(a, 0, 2000, 100, nonce=2), leaf(f0 + 7)),
              X.x2(c, 0, 1, nonce=0)]
    for t in l2_txs:
        t["signer"] = S.signer(sp, t["fromIdx"])
    return l1_txs, l2_txs


def test_the_circuit_accepts_the_ledgers_inputs(hz):
    """rollup-main at (8, 16, 4, 4): a deposit, a forceExit with a load and a forceExit nullified by underflow, then signed L2 rows -- a
    transfer, an exit that inserts, an exit that updates the forceExit's leaf, a transfer to an address, an exit of zero amount.
    ledger_exit_batch_inputs == BatchBuilder's dictionary signal for signal; hashGlobalInputs is computed with the ledger's exit root; the
    HIP context and the oracle accept; once more with every state-dependent signal left on the device"""
    from oracle_binding import OracleCtx
    shape = (8, 16, 4, 4)
    sp = X.exit_state(6)
    f0 = sp.first_idx
    l1_txs, l2_txs = _circuit_batch(sp)
    fee_tokens, fee_idxs = [1], [f0 + 20]
    db, bb = X.builder_batch(sp, l1_txs, l2_txs, fee_tokens + [0] * 3, fee_idxs + [0] * 3, shape[1], n_tx=shape[0], max_l1=shape[2])
    exp = bb.get_input()
    assert [m["isAmountNullified"] for m in bb.tx_meta] == [0, 0, 1, 0, 0, 0, 0, 0] and exp["newExit"] == [0, 1, 1, 0, 1, 0, 0, 0]
    lg = sp.to_ledger(hz)
    like = types.SimpleNamespace(last_idx=f0 + sp.N - 1, num_batch=0)
    inp, _, nullified, exit_root = B.ledger_exit_batch_inputs(lg, like, l1_txs, l2_txs, *shape, fee_tokens, fee_idxs, 1, verify=True)
    assert set(inp) == set(exp), set(inp) ^ set(exp)
    for name in exp:
        assert inp[name] == exp[name], name
    assert nullified == [m["isAmountNullified"] for m in bb.tx_meta] and exit_root == bb.new_exit_root != 0
    assert B.hash_global_inputs(inp, nullified, like.last_idx, lg.root(), exit_root, *shape) == bb.get_hash_inputs()
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
    inp2, dev, _, exit_root2 = B.ledger_exit_batch_inputs(lg2, like, l1_txs, l2_txs, *shape, fee_tokens, fee_idxs, 1, host_outputs=False, verify=True)
    assert set(inp2) | set(dev) == set(exp) and not set(inp2) & set(dev) and {"newExit", "oldValue2", "imExitRoot", "balance2"} <= set(dev)
    assert exit_root2 == exit_root
    g.clear_inputs()
    g.set_inputs(inp2)
    for name, (ptr, count) in dev.items():
        g.set_input_dev(name, ptr, count)
    g.run()
    assert g.read_raw_bytes() == witness
    lg.close()
    lg2.close()


def test_withdraw_over_the_ledgers_exit_tree(hz):
    """withdraw_input reads the exit tree and the exit leaves of a ledger batch through builder.LedgerExits as it reads a built batch's: the
    same inputs as from the builder, accepted by the oracle's Withdraw and by the HIP Withdraw, for an inserted and for an updated leaf"""
    from oracle_binding import OracleCtx
    sp = X.exit_state(6)
    f0 = sp.first_idx
    l1_txs, l2_txs = _circuit_batch(sp)
    db, bb = X.builder_batch(sp, l1_txs, l2_txs, [1], [f0 + 20], N_LEVELS)
    lg = sp.to_ledger(hz)
    lg.apply_batch_exits(l1_txs, l2_txs, [1], [f0 + 20], 1, 1, n_sib=N_LEVELS + 1, outputs=False)
    view = B.LedgerExits(lg)
    inserted, updated = f0 + 1, f0 + 3
    assert bb.exit_leaves[updated]["balance"] == L1.amount_of(l1_txs[1]) + 2000 and set(bb.exit_leaves) == {f0 + 1, f0 + 3, f0 + 4}
    g = hz.ctx("withdraw", nLevels=N_LEVELS)
    for idx in (inserted, updated, f0 + 4):
        w_in, w_hash = B.withdraw_input(view, idx, N_LEVELS)
        assert (w_in, w_hash) == B.withdraw_input(bb, idx, N_LEVELS)
        o = OracleCtx("withdraw", nLevels=N_LEVELS)
        o.set_inputs(w_in)
        assert o.run() is None
        g.set_inputs(w_in)
        g.run()
        assert g.read_raw_bytes() == o.read_raw_bytes()
    with pytest.raises(HzError):
        view.exit_leaves[f0 + 2]
    lg.close()
