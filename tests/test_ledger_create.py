"""L1 rows that create accounts on the growing ledger (hz_ledger_create_growing, hz_ledger_apply_batch_creates) against the
Python BatchBuilder over the same accounts with host hashing, at nLevels = 16: the 27 arrays, the six exit arrays, the six create arrays,
auxToIdx and the L1 flags, the roots, size and last_idx, the touched and created accounts, proofs on the state tree for an old and a new
account, the device pointers against the host copies. From genesis, on 5 and on 64 loaded accounts, over three consecutive batches, with
receivers named by address; the load alone; a growing ledger without create rows against a dense one byte for byte; refusals; argument
errors; 512 creates at once; the circuit itself (the HIP rollup-main context and the oracle). Every comparison is on bytes, bit-exact."""
import ctypes
import types

import numpy as np
import pytest

import device_state_common as D
import ledger_common as C
import ledger_create_common as K
import ledger_exit_common as X
import ledger_l1_common as L1
from circuits_amd import HzError
from circuits_amd import builder as B
from circuits_amd import capi

pytestmark = pytest.mark.gpu
N_LEVELS = 16


class _DevArr:
    """a device array of the library as torch sees it (CUDA array interface)"""
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _d2h(ptr, n, typestr="|u1"):
    import torch
    return torch.as_tensor(_DevArr(ptr, n, typestr), device="cuda:0").cpu().numpy()


def _proofs_match(lg, db, keys):
    """hz_smt_proofs on the ledger's state tree against the builder's tree: found, the value and the zero-padded siblings"""
    got = lg.state_smt().proofs(keys, n_sib=N_LEVELS + 1)
    for i, key in enumerate(keys):
        f = db.state.find(key)
        assert f["found"] and got["found"][i] == 1, key
        assert D.to_int(got["value"][i]) == f["foundValue"] == B.hash_state(db.leaves[key]), key
        sib = list(f["siblings"]) + [0] * (N_LEVELS + 1 - len(f["siblings"]))
        assert [D.to_int(r) for r in got["siblings"][i]] == sib, key


def _check(lg, acc, db, l1_txs, l2_txs, plan, idxs, verify=False):
    """one batch on the ledger and through the builder on db -> (the model's dictionary, the built batch, the ledger's arrays)"""
    n_l1, R = len(l1_txs), len(l1_txs) + len(l2_txs)
    m = K.model(acc, l1_txs, l2_txs, plan, idxs)
    assert isinstance(m, dict), m
    got = lg.apply_batch_creates(l1_txs, K.sign_all(l2_txs) if verify else l2_txs, plan, idxs, 1, db.num_batch + 1, n_sib=N_LEVELS + 1, verify=verify)
    create_ms = lg.create_ms()
    cdev = lg.create_outputs_dev()   # the device pointers are valid until the ledger's next call: read them now
    for name in K.CREATE_ARRAYS:
        assert _d2h(cdev[name], 32 * (1 if name == "new_last_idx" else R)).tobytes() == got[name].tobytes(), name
    xdev, dev = lg.exit_outputs_dev(), lg.outputs_dev()
    assert _d2h(xdev["exit_root_after"], 32 * R).tobytes() == got["exit_root_after"].tobytes()
    for name in ("balance1", "ay1", "state_root_after"):
        assert _d2h(dev[name], 32 * R).tobytes() == got[name].tobytes(), name
    assert _d2h(dev["siblings1"], 32 * R * (N_LEVELS + 1)).tobytes() == got["siblings1"].tobytes()
    assert _d2h(lg.l1_flags_dev(), n_l1).tobytes() == got["l1_flags"].tobytes()
    old_accounts = [a for a in K.touched(m, l2_txs, idxs) if a not in m["slots"]]
    db, bb = K.builder_batch(db, l1_txs, l2_txs, plan, idxs, N_LEVELS, aux_to=m["aux_to_idx"])
    exp = K.expected_arrays(bb, l2_txs, n_l1)
    assert len(exp) == 40 and set(exp) <= set(got)
    C.assert_same(got, exp)
    assert got["l1_flags"].tolist() == L1.builder_flags(bb, n_l1)
    assert lg.root() == bb.new_state_root == lg.state_smt().root()
    assert lg.last_idx() == bb.new_last_idx == D.to_int(got["new_last_idx"][0]) and lg.size() == bb.new_last_idx - acc.first_idx + 1 == lg.state_smt().size()
    tree = lg.exit_tree()
    assert tree.root() == bb.new_exit_root and tree.size() == len(bb.exit_leaves)
    everyone = K.touched(m, l2_txs, idxs)
    assert (lg.accounts(everyone) == C.leaf_rows(db, everyone)).all()
    _proofs_match(lg, db, old_accounts[:1] + ([max(m["slots"])] if m["slots"] else []))   # one old and one new account
    assert create_ms > 0.0
    return m, bb, got


def _after(acc, db):
    """the accounts as the builder's database holds them now"""
    return K.Accounts([db.leaves[i] for i in range(acc.first_idx, db.last_idx + 1)], acc.first_idx)


def test_genesis(hz):
    """from the empty tree: the first row is the only one whose insert finds nothing (isOld0_1 = 1); a create that transfers to 256, one to
    itself, one nullified by underflow, one by the receiver's token, a key whose low bits are not below r with bits 254 and 255 set; then a
    deposit into a created account, a signed L2 transfer from one (verified on the device), an L2 exit from one, a fee slot on one"""
    acc = K.Accounts([])
    lg = acc.to_ledger(hz, 64)
    assert lg.root() == 0 and lg.size() == 0 and lg.last_idx() == 255
    l1_txs, l2_txs, plan, idxs = K.kinds_batch(acc)
    m, bb, got = _check(lg, acc, acc.db(), l1_txs, l2_txs, plan, idxs, verify=True)
    ints = lambda arr: [D.to_int(r) for r in got[arr]]   # noqa: E731
    assert ints("aux_from_idx")[:7] == list(range(256, 263)) and ints("is_old0_1") == [1] + [0] * 11 and ints("old_key1")[:2] == [0, 256]
    assert ints("old_value1")[0] == 0 and ints("old_value1")[1] != 0 and ints("out_idx_after") == list(range(256, 263)) + [262] * 5
    assert got["l1_flags"].tolist()[:7] == [0, 0, 0, 2, 2, 0, 0] and ints("balance1")[:7] == [0] * 7
    assert (ints("ay1")[5], ints("sign1")[5]) == K.decode_key(K.KEY_ABOVE_R) and ints("new_exit")[10] == 1
    assert D.to_int(got["sig_l2_hash"][0]) == B.build_hash_sig(K.sign_all(l2_txs)[0], 1)
    lg.close()


@pytest.mark.parametrize("name", ["dense64", "five"])
def test_the_same_kinds_on_a_loaded_state(hz, name):
    """on 2^6 accounts new key K meets K - 64 at depth 6 and both move to depth 7; on 5 accounts the tree is as ragged as it gets"""
    acc = K.Accounts.of(C.base_state(6)) if name == "dense64" else K.few_accounts(5)
    lg = acc.to_ledger(hz, acc.n + 16)
    db = acc.db()
    assert lg.root() == db.state.root and lg.size() == acc.n
    l1_txs, l2_txs, plan, idxs = K.kinds_batch(acc)
    m, bb, got = _check(lg, acc, db, l1_txs, l2_txs, plan, idxs, verify=True)
    new = acc.first_idx + acc.n
    ints = lambda arr: [D.to_int(r) for r in got[arr]]   # noqa: E731
    assert not any(ints("is_old0_1")) and all(ints("old_value1")[:7])
    if name == "dense64":
        assert ints("old_key1")[:7] == [new + j - 64 for j in range(7)]
    assert ints("balance2")[1] == acc.state(acc.first_idx)["balance"]   # the older account the second create pays
    lg.close()


def test_three_consecutive_batches_on_one_ledger(hz):
    acc = K.few_accounts(5)
    lg = acc.to_ledger(hz, 64)
    db = acc.db()
    for n, seed in enumerate((21, 22, 23)):
        l1_txs, l2_txs = K.draw_batch(acc, seed, n_create=4 + n, n0=10 * n)
        _, bb, _ = _check(lg, acc, db, l1_txs, l2_txs, [1, 2], [acc.first_idx, 0])
        assert lg.root() == bb.new_state_root == db.state.root
        acc = _after(acc, db)
    assert lg.size() == 5 + 4 + 5 + 6
    lg.close()


def test_a_transfer_by_address(hz):
    """the only holder of the address is created in the batch; then an older holder of the same address and token, which wins"""
    acc = K.few_accounts(5)
    f0 = acc.first_idx
    for older in (False, True):
        lg = acc.to_ledger(hz, 16)
        k = K.account(100) if older else K.account(0)   # account(100) is the key and address of account f0
        l1_txs = [K.create_for(k, load=10 ** 9)]
        l2_txs = [dict(C.tx(f0 + 1, 0, 10 ** 9, 100, nonce=0), toEthAddr=k.eth_addr)]
        m, bb, got = _check(lg, acc, acc.db(), l1_txs, l2_txs, [1], [0])
        assert D.to_int(got["auxToIdx"][1]) == (f0 if older else f0 + 5) == m["aux_to_idx"][1]
        assert D.to_int(lg.accounts([f0 + 5])[0][1]) == (10 ** 9 if older else 2 * 10 ** 9)
        lg.close()


def test_load_roots(hz):
    for k in (4, 6):
        st = C.base_state(k)
        lg = K.Accounts.of(st).to_ledger(hz, (1 << k) + 3)
        dense = st.to_ledger(hz)
        assert lg.root() == st.root == dense.root() and lg.size() == 1 << k and lg.last_idx() == st.first_idx + st.N - 1 and lg.state_smt().size() == 1 << k
        everyone = np.arange(st.first_idx, st.first_idx + st.N)
        assert (lg.accounts(everyone) == dense.accounts(everyone)).all()
        dense.close()
        # a reload resets the tree first
        five = K.few_accounts(5)
        lg.load_accounts(*five.cols())
        assert lg.root() == five.db().state.root and lg.size() == 5
        lg.load_accounts(*K.Accounts([]).cols())
        assert lg.root() == 0 and lg.size() == 0 and lg.last_idx() == st.first_idx - 1
        lg.close()
    # a refused load names the first offender and touches nothing
    five = K.few_accounts(5)
    lg = five.to_ledger(hz, 8)
    root = lg.root()
    cols = [np.array(c) for c in five.cols()]
    cols[1][3][24] = 1
    with pytest.raises(HzError) as e:
        lg.load_accounts(*cols)
    assert e.value.status == 4 and "account 259 (row 3)" in str(e.value) and "balance >= 2^192" in str(e.value), str(e.value)
    assert lg.root() == root and lg.size() == 5
    with pytest.raises(HzError) as e:
        lg.load_accounts(*K.few_accounts(9).cols())
    assert e.value.status == 1 and "capacity" in str(e.value)
    assert hz.c.hz_ledger_tree(lg.h) is None   # no dense tree to borrow
    lg.close()


def test_parity_with_the_dense_ledger(hz):
    """a growing ledger loaded with the same 2^k accounts, without create rows: every output of hz_ledger_apply_batch_exits equal byte for
    byte, and hz_ledger_apply_batch_creates adds the no-create values of its six arrays"""
    k, st, l1_txs, l2_txs = X.seeded_batches()[0]
    plan, idxs = [1, 2, 0, 0], L1.fee_accounts(st)
    dense, a, b = st.to_ledger(hz), K.Accounts.of(st).to_ledger(hz, st.N + 8), K.Accounts.of(st).to_ledger(hz, st.N)
    got_d = dense.apply_batch_exits(l1_txs, l2_txs, plan, idxs, 1, 1, n_sib=N_LEVELS + 1)
    got_a = a.apply_batch_exits(l1_txs, l2_txs, plan, idxs, 1, 1, n_sib=N_LEVELS + 1)
    got_b = b.apply_batch_creates(l1_txs, l2_txs, plan, idxs, 1, 1, n_sib=N_LEVELS + 1)
    assert set(got_a) == set(got_d) and set(got_b) == set(got_d) | set(K.CREATE_ARRAYS)
    for name in got_d:
        assert got_d[name].tobytes() == got_a[name].tobytes() == got_b[name].tobytes(), name
    R, last = len(l1_txs) + len(l2_txs), st.first_idx + st.N - 1
    for name in ("aux_from_idx", "is_old0_1", "old_key1", "old_value1"):
        assert not got_b[name].any(), name
    assert [D.to_int(r) for r in got_b["out_idx_after"]] == [last] * R and D.to_int(got_b["new_last_idx"][0]) == last
    everyone = np.arange(st.first_idx, st.first_idx + st.N)
    assert dense.root() == a.root() == b.root() and (dense.accounts(everyone) == a.accounts(everyone)).all() and (a.accounts(everyone) == b.accounts(everyone)).all()
    assert dense.exit_tree().root() == a.exit_tree().root() == b.exit_tree().root()
    # the dense ledger takes the new call too when no row creates
    got_e = st.to_ledger(hz).apply_batch_creates(l1_txs, l2_txs, plan, idxs, 1, 1, n_sib=N_LEVELS + 1)
    for name in got_b:
        assert got_e[name].tobytes() == got_b[name].tobytes(), name
    for lg in (dense, a, b):
        lg.close()


def test_a_refused_batch_that_contains_creates(hz):
    """reason 3 on an L2 row: root, size, last_idx and the accounts are unchanged, the would-be index does not exist, and the next accepted
    call hands out the same indices"""
    acc = K.few_accounts(5)
    f0 = acc.first_idx
    lg = acc.to_ledger(hz, 16)
    root, everyone = lg.root(), np.arange(f0, f0 + 5)
    fields = lg.accounts(everyone)
    k = [K.account(j) for j in range(2)]
    l1_txs = [K.create_for(k[0], load=10 ** 9), K.create_for(k[1], load=10 ** 9, amount=10 ** 8, to=f0)]
    over = [C.tx(f0 + 5, f0, 2 * 10 ** 9, 0, nonce=0)]
    assert K.model(acc, l1_txs, over, [1], [0]) == ("refused", 2, 3)
    with pytest.raises(HzError) as e:
        lg.apply_batch_creates(l1_txs, over, [1], [0], 1, 1, n_sib=N_LEVELS + 1)
    assert e.value.status == 4 and "index 2 " in str(e.value) and "reason 3:" in str(e.value), str(e.value)
    assert lg.root() == root and lg.size() == 5 and lg.last_idx() == f0 + 4 and (lg.accounts(everyone) == fields).all() and lg.state_smt().size() == 5
    with pytest.raises(HzError) as e:
        lg.accounts([f0 + 5])
    assert e.value.status == 1
    with pytest.raises(HzError):
        lg.create_outputs_dev()
    m, bb, got = _check(lg, acc, acc.db(), l1_txs, [C.tx(f0 + 5, f0, 10 ** 8, 0, nonce=0)], [1], [0])
    assert [D.to_int(r) for r in got["aux_from_idx"]] == [f0 + 5, f0 + 6, 0]
    lg.close()


def test_argument_errors(hz):
    acc = K.few_accounts(5)
    f0 = acc.first_idx
    lg = acc.to_ledger(hz, 8)
    root = lg.root()
    for l1_txs, l2_txs, text in K.arg_cases(acc):
        with pytest.raises(HzError) as e:
            lg.apply_batch_creates(l1_txs, l2_txs, [1], [0], 1, 1, n_sib=N_LEVELS + 1)
        assert e.value.status == 1 and text in str(e.value), str(e.value)
    ok = K.create_for(K.account(0), load=10)
    with pytest.raises(HzError) as e:   # size + creates > capacity
        lg.apply_batch_creates([ok] * 4, [], [1], [0], 1, 1, n_sib=N_LEVELS + 1)
    assert e.value.status == 1 and "the ledger is full" in str(e.value) and "L1 tx 3" in str(e.value), str(e.value)
    l1, arr, sigs = capi.l1tx_array([ok]), capi.l2tx_array([]), capi.l2sig_array([])   # from_bjj == NULL with a create row: the C call itself
    plan, idxs = np.array([1], dtype=np.uint32), np.array([0], dtype=np.uint64)
    with pytest.raises(HzError) as e:
        hz._check(hz.c.hz_ledger_apply_batch_creates(lg.h, 1, ctypes.addressof(l1), None, 0, ctypes.addressof(arr), ctypes.addressof(sigs), 0, None, 1, 1, 1,
                                                     plan.ctypes.data, idxs.ctypes.data, N_LEVELS + 1, None, None, None, None, None, None))
    assert e.value.status == 1 and "from_bjj == NULL" in str(e.value), str(e.value)
    for n_sib in (0, N_LEVELS + 2):
        with pytest.raises(HzError) as e:
            lg.apply_batch_creates([ok], [], [1], [0], 1, 1, n_sib=n_sib)
        assert e.value.status == 1 and "n_sib" in str(e.value)
    # the older calls that take L1 rows keep refusing a create, on a growing ledger as on a dense one; the other four take no L1 row
    dense = C.base_state(4).to_ledger(hz)
    for call in (lambda: lg.apply_batch([ok], [], [1], [0], 1, 1), lambda: lg.apply_batch_exits([ok], [], [1], [0], 1, 1),
                 lambda: dense.apply_batch([ok], [], [1], [0], 1, 1, n_sib=5), lambda: dense.apply_batch_exits([ok], [], [1], [0], 1, 1, n_sib=5)):
        with pytest.raises(HzError) as e:
            call()
        assert e.value.status == 1 and "creates an account" in str(e.value) and "not supported yet" in str(e.value), str(e.value)
    with pytest.raises(HzError) as e:   # a dense ledger given a create row
        dense.apply_batch_creates([ok], [], [1], [0], 1, 1, n_sib=5)
    assert e.value.status == 1 and "creates an account" in str(e.value) and "cannot grow" in str(e.value), str(e.value)
    dense.close()
    assert lg.root() == root and lg.size() == 5
    # the existing calls work on the live accounts of a growing ledger
    assert lg.apply_l2([C.tx(f0, f0 + 1, 5, nonce=0)], [1], [0])["balance1"].shape == (1, 32)
    assert lg.resolve_l2([dict(C.tx(f0, 0, 5, nonce=1), toEthAddr=acc.state(f0 + 1)["ethAddr"])]).tolist() == [f0 + 1]
    lg.close()
    # a depth refusal: on 64 accounts the new key 320 meets 256 at depth 6 and both would lie at depth 7
    st = K.Accounts.of(C.base_state(6))
    lg = st.to_ledger(hz, 80)
    root = lg.root()
    with pytest.raises(HzError) as e:
        lg.apply_batch_creates([ok], [], [1], [0], 1, 1, n_sib=7)
    assert e.value.status == 1 and "depth >= n_sib = 7" in str(e.value), str(e.value)
    assert lg.root() == root and lg.size() == 64
    got = lg.apply_batch_creates([ok], [], [1], [0], 1, 1, n_sib=8)
    assert D.to_int(got["old_key1"][0]) == 256 and lg.size() == 65
    lg.close()


def test_capacity_512_creates_in_one_call_from_genesis(hz):
    acc = K.Accounts([])
    lg = acc.to_ledger(hz, 512)
    keys = [K.account(j) for j in range(8)]
    l1_txs = []
    for j in range(K.MAX_L1):
        kind = j % 4
        to = 0 if kind == 0 or j == 0 else 256 + (j * 7919) % (j + 1)
        l1_txs.append(K.create_for(keys[j % 8], token=2 if kind == 3 else 1, load=(j + 1) * 10 ** 6, amount=(j + 1) * 10 ** 5 * (30 if kind == 2 else 1) if to else 0, to=to))
    m, bb, got = _check(lg, acc, acc.db(), l1_txs, [], [1], [0])
    assert lg.size() == 512 and set(got["l1_flags"].tolist()) == {0, 2}
    with pytest.raises(HzError) as e:
        lg.apply_batch_creates([l1_txs[0]], [], [1], [0], 1, 1, n_sib=N_LEVELS + 1)
    assert e.value.status == 1 and "the ledger is full" in str(e.value)
    lg.close()


def test_the_circuit_accepts_the_ledgers_inputs(hz):
    """rollup-main at (8, 16, 4, 4) from genesis: three creates (a deposit, a transfer to 256, one nullified by underflow) and a deposit into
    a created account, then signed L2 rows from created accounts -- a transfer, an exit, a transfer to an address created in the batch.
    ledger_create_batch_inputs == BatchBuilder's dictionary signal for signal; hashGlobalInputs is the builder's; the HIP context and the
    oracle accept; once more with every state-dependent signal left on the device"""
    from oracle_binding import OracleCtx
    shape = (8, 16, 4, 4)
    acc = K.Accounts([])
    k = [K.account(j) for j in range(3)]
    l1_txs = [K.create_for(k[0], load=10 ** 12), K.create_for(k[1], load=5 * 10 ** 11, amount=10 ** 11, to=256),
              K.create_for(k[2], load=10 ** 9, amount=3 * 10 ** 9, to=257), L1.l1(258, 0, 0, 10 ** 10, 1, k[2].eth_addr)]
    l2_txs = [dict(C.tx(256, 257, 10 ** 10, 100, nonce=0), signer=k[0]), dict(C.tx(257, K.EXIT, 10 ** 10, 176, nonce=0), signer=k[1]),
              dict(C.tx(256, 0, 10 ** 9, 1, nonce=1), signer=k[0], toEthAddr=k[2].eth_addr)]
    fee_tokens, fee_idxs = [1], [258]
    m = K.model(acc, l1_txs, l2_txs, fee_tokens, fee_idxs)
    db, bb = K.builder_batch(acc.db(), l1_txs, l2_txs, fee_tokens + [0] * 3, fee_idxs + [0] * 3, shape[1], aux_to=m["aux_to_idx"], n_tx=shape[0], max_l1=shape[2])
    exp = bb.get_input()
    assert exp["newAccount"] == [1, 1, 1, 0, 0, 0, 0, 0] and exp["auxFromIdx"][:3] == [256, 257, 258] and exp["imOutIdx"] == [256, 257] + [258] * 5
    assert [t["isAmountNullified"] for t in bb.tx_meta][:3] == [0, 0, 1] and exp["auxToIdx"][6] == 258
    lg = acc.to_ledger(hz, 16)
    like = types.SimpleNamespace(last_idx=255, num_batch=0)
    inp, _, nullified, exit_root, new_last = B.ledger_create_batch_inputs(lg, like, l1_txs, l2_txs, *shape, fee_tokens, fee_idxs, 1, verify=True)
    assert set(inp) == set(exp), set(inp) ^ set(exp)
    for name in exp:
        assert inp[name] == exp[name], name
    assert nullified == [t["isAmountNullified"] for t in bb.tx_meta] and exit_root == bb.new_exit_root != 0 and new_last == bb.new_last_idx == 258 == like.last_idx
    assert B.hash_global_inputs(inp, nullified, new_last, lg.root(), exit_root, *shape) == bb.get_hash_inputs()
    g = hz.ctx("rollup-main", nTx=shape[0], nLevels=shape[1], maxL1Tx=shape[2], maxFeeTx=shape[3])
    g.set_inputs(inp)
    g.run()
    assert g.get("main.hashGlobalInputs") == bb.get_hash_inputs()
    witness = g.read_raw_bytes()
    o = OracleCtx("rollup-main", *shape)
    o.set_inputs(inp)
    assert o.run() is None
    lg2 = acc.to_ledger(hz, 16)
    like = types.SimpleNamespace(last_idx=255, num_batch=0)
    inp2, dev, _, exit_root2, new_last2 = B.ledger_create_batch_inputs(lg2, like, l1_txs, l2_txs, *shape, fee_tokens, fee_idxs, 1, host_outputs=False, verify=True)
    assert set(inp2) | set(dev) == set(exp) and not set(inp2) & set(dev) and {"auxFromIdx", "oldValue1", "imOutIdx", "isOld0_1", "balance1"} <= set(dev)
    assert (exit_root2, new_last2) == (exit_root, new_last)
    g.clear_inputs()
    g.set_inputs(inp2)
    for name, (ptr, count) in dev.items():
        g.set_input_dev(name, ptr, count)
    g.run()
    assert g.read_raw_bytes() == witness
    lg.close()
    lg2.close()
