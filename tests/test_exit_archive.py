"""Exit trees of earlier batches kept on the ledger and Withdraw's inputs in bulk (hz_ledger_exit_keep, hz_ledger_withdraw_rows, DESIGN.md
8k) against the Python BatchBuilder at nLevels = 16: every row of every kept leaf against builder.withdraw_input over a sequence of batches
on one ledger and over the named edges, the statuses, the circuit itself (the HIP Withdraw fed from the device pointers, and the oracle),
the existing path (hz_smt_proofs + hz_ledger_exit_accounts on the live tree) across workgroup boundaries, forget / stats / argument errors,
slabs that roll over, and a growing ledger. Every comparison is on bytes, bit-exact.
The expected side of the sequence is ONE builder database carried across the batches (RollupDB, host hashing)."""
import functools

import numpy as np
import pytest

import device_state_common as D
import exit_archive_common as E
import ledger_common as C
import ledger_create_common as K
import ledger_exit_common as X
import ledger_l1_common as L1
from circuits_amd import HzError
from circuits_amd import builder as B
from circuits_amd.capi import WITHDRAW_ARRAYS, WITHDRAW_SIGNALS

pytestmark = pytest.mark.gpu
N_LEVELS = 16
PLAN = [1, 2]


def _idxs(sp):
    return [sp.first_idx + 40, 0]


# ---- the sequence: batch 1 with exits, a refused batch, batch 2 without exits, batch 3 with exits (one account exits again) ----------------
@functools.lru_cache(maxsize=None)
def _sequence():
    """-> (state, [(batch_num, l1_txs, l2_txs, built BatchBuilder or None for the refused one)]) on one builder database"""
    sp = X.exit_state(6)
    f0, leaf = sp.first_idx, sp.state
    a, b, c, far, w = f0 + 1, f0 + 3, f0 + 4, f0 + 33, f0 + 6
    part = lambda x, d=3: L1.float_floor(leaf(x)["balance"] // d)   # noqa: E731
    one = ([X.fx(sp, b, part(b, 4), load=900)], [X.x2(a, part(a), 100, nonce=0), C.tx(c, b, 1000, 176, nonce=0), X.x2(far, part(far), nonce=0), X.x2(b, 2000, 176, nonce=0)])
    refused = ([], [X.x2(w, L1.float_floor(3 * leaf(w)["balance"]), nonce=0)])
    two = ([L1.own(sp, c, 0, 0, load=70000)], [C.tx(c, a, 500, 100, nonce=1)])
    three = ([X.fx(sp, c, 4000)], [X.x2(a, 3000, 100, nonce=1), X.x2(w, X.WHOLE // 4, 1, nonce=0), X.x2(f0 + 9, 0, token=2, nonce=0), X.x2(f0 + 17, 7000, nonce=0)])
    db, out = None, []
    for num, (l1_txs, l2_txs) in ((1, one), (None, refused), (2, two), (3, three)):
        if num is None:
            out.append((None, l1_txs, l2_txs, None))
            continue
        db, bb = X.builder_batch(sp, l1_txs, l2_txs, PLAN, _idxs(sp), N_LEVELS, db=db)
        out.append((num, l1_txs, l2_txs, bb))
    assert set(out[0][3].exit_leaves) == {a, b, far} and out[2][3].exit_leaves == {} and set(out[3][3].exit_leaves) == {a, c, w, f0 + 17}
    assert out[2][3].new_exit_root == 0 and out[0][3].exit_leaves[a]["balance"] != out[3][3].exit_leaves[a]["balance"]
    return sp, out


def _run_sequence(hz):
    """the sequence on a fresh ledger, every successful batch kept under its number -> (ledger, state, {batch_num: BatchBuilder})"""
    sp, seq = _sequence()
    lg = sp.to_ledger(hz)
    bbs = {}
    for num, l1_txs, l2_txs, bb in seq:
        if num is None:
            with pytest.raises(HzError) as e:
                lg.apply_batch_exits(l1_txs, l2_txs, PLAN, _idxs(sp), 1, 1, n_sib=N_LEVELS + 1, outputs=False)
            assert e.value.status == 4 and "reason 3:" in str(e.value), str(e.value)
            continue
        if bb.exit_leaves:
            lg.apply_batch_exits(l1_txs, l2_txs, PLAN, _idxs(sp), 1, 1, n_sib=N_LEVELS + 1, outputs=False)
        else:   # another apply call: the tree it leaves is the empty one
            lg.apply_batch(l1_txs, l2_txs, PLAN, _idxs(sp), 1, 1, n_sib=N_LEVELS + 1, outputs=False)
        assert lg.root() == bb.new_state_root and lg.exit_tree().root() == bb.new_exit_root
        lg.exit_keep(num)
        bbs[num] = bb
    return lg, sp, bbs


def _found_pairs(bbs):
    return [(num, idx) for num, bb in sorted(bbs.items()) for idx in sorted(bb.exit_leaves)]


def _absent_queries(sp, bbs):
    """[(batch_num, idx, status)]: an unknown batch, an idx that meets another leaf, one that meets an empty slot, idx = 2^48, the empty tree"""
    f0 = sp.first_idx
    sh = E.Shape(sorted(bbs[3].exit_leaves))
    at_leaf, at_empty = E.absent_keys(sh, f0, f0 + 64)
    assert at_leaf is not None and at_empty is not None
    a = f0 + 1
    return [(99, a, E.NOT_KEPT), (0, a, E.NOT_KEPT), (3, at_leaf, E.ABSENT), (3, at_empty, E.ABSENT), (3, 1 << 48, E.ABSENT), (1, (1 << 48) | a, E.ABSENT),
            (3, (1 << 64) - 1, E.ABSENT), (2, a, E.ABSENT), (2, f0 + 33, E.ABSENT), (2, 0, E.ABSENT)]


def _guarded(n, n_levels):
    """the nine output arrays pre-filled with 0xA5, each with one more row than the call may write -> (whole arrays, the views to pass)"""
    whole = {name: np.full((n + 1, 32), 0xA5, dtype=np.uint8) for name in E.ROWS}
    whole["siblings_state"] = np.full((n + 1, n_levels + 1, 32), 0xA5, dtype=np.uint8)
    whole["status"] = np.full(n + 1, 0xA5, dtype=np.uint8)
    return whole, {name: arr[:n] for name, arr in whole.items()}


def _check_rows(got, queries, bbs, n_levels=N_LEVELS):
    """queries: [(batch_num, idx, expected status)]: a found row is builder.withdraw_input's, any other is zero"""
    assert got["status"].tolist() == [q[2] for q in queries]
    for i, (num, idx, status) in enumerate(queries):
        if status == E.FOUND:
            exp = E.expected_rows(bbs[num], idx, n_levels)
            assert D.to_int(exp["root_exit"]) == bbs[num].new_exit_root
            E.assert_row(got, i, exp, (num, idx))
        else:
            E.assert_zero_row(got, i, (num, idx))


def test_a_sequence_of_batches_on_one_ledger(hz):
    lg, sp, bbs = _run_sequence(hz)
    assert lg.exit_kept() == [1, 2, 3] and lg.exit_archive_stats()["snapshots"] == 3
    assert [lg.exit_root_of(k) for k in (1, 2, 3)] == [bbs[k].new_exit_root for k in (1, 2, 3)] and lg.exit_root_of(2) == 0
    everyone = np.arange(sp.first_idx, sp.first_idx + sp.N)
    live = (lg.root(), lg.exit_tree().root(), lg.exit_tree().size(), lg.accounts(everyone).tobytes(), lg.exit_accounts(sorted(bbs[3].exit_leaves)).tobytes())
    queries = [(num, idx, E.FOUND) for num, idx in _found_pairs(bbs)] + _absent_queries(sp, bbs)
    order = np.random.default_rng(3).permutation(len(queries))
    queries = [queries[i] for i in order]
    whole, into = _guarded(len(queries), N_LEVELS)
    got = lg.withdraw_rows([q[0] for q in queries], [q[1] for q in queries], N_LEVELS, into=into)
    assert all((arr[-1] == 0xA5).all() for arr in whole.values())   # nothing behind the n rows is written
    assert sum(1 for q in queries if q[2] == E.FOUND) == 7 and lg.withdraw_ms() > 0.0
    _check_rows(got, queries, bbs)
    # the device pointers hold the same bytes
    dev = lg.withdraw_rows_dev()
    for name in WITHDRAW_ARRAYS:
        assert _d2h(dev[name], got[name].size).tobytes() == got[name].tobytes(), name
    # the live side is what it was: keep and rows change nothing resident
    assert live == (lg.root(), lg.exit_tree().root(), lg.exit_tree().size(), lg.accounts(everyone).tobytes(), lg.exit_accounts(sorted(bbs[3].exit_leaves)).tobytes())
    # builder.ArchivedExits serves withdraw_input unchanged, as LedgerExits does for the live tree
    for num, idx in _found_pairs(bbs):
        assert B.withdraw_input(B.ArchivedExits(lg, num), idx, N_LEVELS) == B.withdraw_input(bbs[num], idx, N_LEVELS)
    assert B.withdraw_input(B.LedgerExits(lg), sp.first_idx + 1, N_LEVELS) == B.withdraw_input(bbs[3], sp.first_idx + 1, N_LEVELS)
    with pytest.raises(KeyError):
        B.ArchivedExits(lg, 2).exit_leaves[sp.first_idx + 1]
    with pytest.raises(KeyError):
        B.ArchivedExits(lg, 7)
    lg.close()


class _DevArr:
    """a device array of the library as torch sees it (CUDA array interface)"""
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _d2h(ptr, n, typestr="|u1"):
    import torch
    return torch.as_tensor(_DevArr(ptr, n, typestr), device="cuda:0").cpu().numpy()


def test_a_keep_leaves_the_device_outputs_of_the_apply_call_valid(hz):
    sp, seq = _sequence()
    _, l1_txs, l2_txs, bb = seq[0]
    lg = sp.to_ledger(hz)
    got = lg.apply_batch_exits(l1_txs, l2_txs, PLAN, _idxs(sp), 1, 1, n_sib=N_LEVELS + 1)
    lg.exit_keep(1)
    xdev, dev = lg.exit_outputs_dev(), lg.outputs_dev()
    R = len(l1_txs) + len(l2_txs)
    assert _d2h(xdev["exit_root_after"], 32 * R).tobytes() == got["exit_root_after"].tobytes()
    assert _d2h(dev["siblings2"], 32 * R * (N_LEVELS + 1)).tobytes() == got["siblings2"].tobytes()
    assert lg.exit_keep_ms() > 0.0
    lg.withdraw_rows([1], [sp.first_idx + 1], N_LEVELS)   # like verify_l2, this call does invalidate them
    with pytest.raises(HzError):
        lg.exit_outputs_dev()
    lg.close()


@pytest.mark.parametrize("name", X.EDGES)
def test_named_edges(hz, name):
    sp = X.exit_state(6)
    f0 = sp.first_idx
    l1_txs, l2_txs = X.edge_batches(sp)[name]
    db, bb = X.builder_batch(sp, l1_txs, l2_txs, PLAN, _idxs(sp), N_LEVELS)
    lg = sp.to_ledger(hz)
    lg.apply_batch_exits(l1_txs, l2_txs, PLAN, _idxs(sp), 1, 1, n_sib=N_LEVELS + 1, outputs=False)
    lg.exit_keep(5)
    lg.apply_l2([{}], PLAN, _idxs(sp), n_sib=N_LEVELS + 1, outputs=False)   # the live tree is gone
    assert lg.exit_tree().size() == 0 and lg.exit_root_of(5) == bb.new_exit_root
    keys = sorted(bb.exit_leaves)
    queries = [(5, k, E.FOUND) for k in keys] + [(5, f0 + 2, E.ABSENT)]
    got = lg.withdraw_rows([q[0] for q in queries], [q[1] for q in queries], N_LEVELS)
    _check_rows(got, queries, {5: bb})
    a = f0 + 1
    if name in ("first_exit_into_empty_tree", "exit_whole_balance_with_fee"):   # the root is the single leaf: no sibling
        assert len(keys) == 1 and not got["siblings_state"][0].any() and got["root_exit"][0].any()
    if name == "keys_sharing_low_bits":   # five zero siblings in a chain of one-child nodes, then the other leaf
        assert keys == [a, f0 + 33] and not got["siblings_state"][:2, :5].any() and got["siblings_state"][:2, 5].any(axis=1).all() and not got["siblings_state"][:2, 6:].any()
    if name == "same_account_twice":   # the accumulated balance
        assert D.to_int(got["balance"][0]) == L1.amount_of(l2_txs[0]) + L1.amount_of(l2_txs[2])
    if name == "force_exit_then_l2_exit_same_idx":
        assert D.to_int(got["balance"][0]) == L1.amount_of(l1_txs[0]) + L1.amount_of(l2_txs[0])
    if name.startswith("force_exit_nullified"):
        assert keys == [a] and D.to_int(got["balance"][0]) == 0 and got["status"][0] == 0 and got["ay"][0].any()
    if name == "zero_amount_exit":   # an empty tree is a legitimate entry
        assert keys == [] and lg.exit_root_of(5) == 0 and got["status"].tolist() == [E.ABSENT]
    lg.close()


def test_statuses(hz):
    lg, sp, bbs = _run_sequence(hz)
    f0 = sp.first_idx
    a, far = f0 + 1, f0 + 33
    # batch 1 holds the keys_sharing_low_bits pair: a and far hang below six siblings. Withdraw(5) takes six: one too few
    assert a in bbs[1].exit_leaves and far in bbs[1].exit_leaves and len(bbs[1].exit_tree.find(a)["siblings"]) == 6
    queries = [(1, a, E.DEEP), (3, f0 + 17, None), (1, far, E.DEEP), (1, f0 + 3, None)] + _absent_queries(sp, bbs)
    depth = {(num, idx): len(bbs[num].exit_tree.find(idx)["siblings"]) for num, idx, s in queries if s is None}
    queries = [(num, idx, (E.DEEP if depth[(num, idx)] >= 6 else E.FOUND) if s is None else s) for num, idx, s in queries]
    assert [q[2] for q in queries[:4]].count(E.FOUND) >= 1
    whole, into = _guarded(len(queries), 5)
    got = lg.withdraw_rows([q[0] for q in queries], [q[1] for q in queries], 5, into=into)
    assert all((arr[-1] == 0xA5).all() for arr in whole.values())
    _check_rows(got, queries, bbs, n_levels=5)
    # the same queries at N_LEVELS: found
    at16 = [(num, idx, E.FOUND if s == E.DEEP else s) for num, idx, s in queries]
    _check_rows(lg.withdraw_rows([q[0] for q in at16], [q[1] for q in at16], N_LEVELS), at16, bbs)
    # a null array is not written and the others are; no output at all leaves the device arrays
    some = {"status": np.full(len(at16), 0xA5, dtype=np.uint8), "balance": np.full((len(at16), 32), 0xA5, dtype=np.uint8)}
    part = lg.withdraw_rows([q[0] for q in at16], [q[1] for q in at16], N_LEVELS, into=some)
    assert set(part) == {"status", "balance"} and part["status"].tolist() == [q[2] for q in at16]
    assert lg.withdraw_rows([q[0] for q in at16], [q[1] for q in at16], N_LEVELS, outputs=False) == {}
    assert _d2h(lg.withdraw_rows_dev()["status"], len(at16)).tolist() == [q[2] for q in at16]
    # n_levels + 1 = 64 siblings and n_levels = 0 (one sibling: only a root leaf fits)
    _check_rows(lg.withdraw_rows([1, 3], [a, f0 + 17], 63), [(1, a, E.FOUND), (3, f0 + 17, E.FOUND)], bbs, n_levels=63)
    assert lg.withdraw_rows([1, 3, 2], [a, f0 + 17, a], 0)["status"].tolist() == [E.DEEP, E.DEEP, E.ABSENT]
    assert lg.withdraw_rows([], [], N_LEVELS)["status"].shape == (0,)
    lg.close()


def test_the_circuit_takes_the_rows_from_the_device(hz):
    """a withdraw context of as many instances as there are kept leaves, its eight inputs set from hz_ledger_withdraw_rows_dev with
    instance -1: the whole buffer equals the oracle's Withdraw on builder.withdraw_input's dictionaries, hashGlobalInputs the Python SHA-256"""
    from oracle_binding import OracleCtx
    lg, sp, bbs = _run_sequence(hz)
    pairs = _found_pairs(bbs)
    order = np.random.default_rng(5).permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    n = len(pairs)
    lg.withdraw_rows([p[0] for p in pairs], [p[1] for p in pairs], N_LEVELS, outputs=False)
    dev = lg.withdraw_rows_dev()
    g = hz.ctx("withdraw", nLevels=N_LEVELS, n_instances=n)
    for name, signal in WITHDRAW_SIGNALS.items():
        g.set_input_dev(signal, dev[name], n * (N_LEVELS + 1 if name == "siblings_state" else 1), instance=-1)
    g.run()
    o = OracleCtx("withdraw", nLevels=N_LEVELS, n_instances=n)
    for i, (num, idx) in enumerate(pairs):
        w_in, w_hash = B.withdraw_input(bbs[num], idx, N_LEVELS)
        o.set_inputs(w_in, instance=i)
        assert g.get("main.hashGlobalInputs", instance=i) == w_hash
    assert o.run() is None
    assert g.read_raw_bytes() == o.read_raw_bytes()
    lg.close()


# ---- against the existing path, across workgroup boundaries ----------------------------------------------------------------------------------
def test_512_exits_against_the_live_trees_proofs(hz):
    """one batch of 512 L2 exits of distinct senders on 2^10 accounts. hz_smt_proofs on the live tree and hz_ledger_exit_accounts give the
    expectation for the 512 keys and the 512 absent ones; after the keep and a batch that empties the live tree, n = 1, 63, 64, 65 and 1024
    queries with repeated leaves"""
    base = C.base_state(10)
    f0 = base.first_idx
    rng = np.random.default_rng(17)
    senders = sorted(f0 + int(x) for x in rng.choice(base.N, size=512, replace=False))
    l2_txs = [X.x2(s, L1.float_floor(base.state(s)["balance"] // 8), nonce=0) for s in senders]
    lg = base.to_ledger(hz)
    lg.apply_batch_exits([], l2_txs, [1], [0], 1, 1, n_sib=N_LEVELS + 1, outputs=False)
    everyone = np.arange(f0, f0 + base.N, dtype=np.uint64)
    tree = lg.exit_tree()
    assert tree.size() == 512
    root = tree.root()
    proofs = tree.proofs(everyone, n_sib=N_LEVELS + 1)
    assert int(proofs["found"].sum()) == 512
    fields = np.zeros((base.N, 4, 32), dtype=np.uint8)
    fields[np.array(senders) - f0] = lg.exit_accounts(senders)
    lg.exit_keep(8)
    lg.apply_l2([C.tx(senders[0], senders[1], 5, nonce=1)], [1], [0], n_sib=N_LEVELS + 1, outputs=False)
    assert lg.exit_tree().size() == 0
    for n in (1, 63, 64, 65, 1024):
        at = rng.integers(0, base.N, size=n)
        if n == 1:
            at[0] = senders[7] - f0
        got = lg.withdraw_rows([8] * n, everyone[at], N_LEVELS)
        found = proofs["found"][at].astype(bool)
        assert (got["status"] == np.where(found, E.FOUND, E.ABSENT)).all() and (n < 63 or (found.any() and not found.all()))
        e0 = fields[at, 0]
        exp = {"siblings_state": proofs["siblings"][at], "eth_addr": fields[at, 3], "balance": fields[at, 1], "ay": fields[at, 2],
               "root_exit": np.repeat(D.to_bytes([root]), n, axis=0), "idx": D.to_bytes([int(k) for k in everyone[at]]),
               "token_id": D.to_bytes([D.to_int(r) & 0xFFFFFFFF for r in e0]), "sign": D.to_bytes([(D.to_int(r) >> 72) & 1 for r in e0])}
        for name, arr in exp.items():
            arr = np.array(arr)
            arr[~found] = 0
            assert got[name].tobytes() == arr.tobytes(), (n, name)
    lg.close()


def test_slabs_roll_over_and_are_freed(hz):
    """twelve batches of 512 forceExits, each kept: a snapshot lies inside one slab, a new slab comes only when the current one is full,
    and a slab goes when every snapshot in it is forgotten; every kept batch still answers, from whichever slab"""
    base = C.base_state(10)
    f0 = base.first_idx
    senders = [f0 + 2 * i + (i % 3 == 0) for i in range(512)]
    lg = base.to_ledger(hz)
    roots, used = {}, []
    for k in range(1, 13):
        l1_txs = [X.fx(base, s, 1000 + k) for s in senders[k:] + senders[:k]]
        lg.apply_batch_exits(l1_txs, [], [1], [0], 1, 1, n_sib=N_LEVELS + 1, outputs=False)
        roots[k] = lg.exit_tree().root()
        lg.exit_keep(k)
        st = lg.exit_archive_stats()
        used.append(st["bytes_used"])
        assert st["snapshots"] == k and st["bytes_used"] <= st["bytes_reserved"]
    per = used[0]
    assert used == [per * k for k in range(1, 13)] and 512 * (32 + 128 + 12) < per < 2 * 512 * (32 + 128 + 12 + 40)
    st = lg.exit_archive_stats()
    per_slab = (1 << 20) // per
    assert st["slabs"] == -(-12 // per_slab) == 2 and st["bytes_reserved"] >= 2 << 20
    got = lg.withdraw_rows(list(range(1, 13)), [senders[5]] * 12, N_LEVELS)
    assert not got["status"].any() and [D.to_int(r) for r in got["root_exit"]] == [roots[k] for k in range(1, 13)]
    assert [D.to_int(r) for r in got["balance"]] == [1000 + k for k in range(1, 13)]
    lg.exit_forget(per_slab)            # one snapshot of the first slab is left: the slab stays
    assert lg.exit_archive_stats()["slabs"] == 2 and lg.exit_kept() == list(range(per_slab, 13))
    lg.exit_forget(per_slab + 1)        # none is left: the slab is freed
    st = lg.exit_archive_stats()
    assert st["slabs"] == 1 and st["snapshots"] == 12 - per_slab and st["bytes_used"] == per * (12 - per_slab) and lg.exit_kept() == list(range(per_slab + 1, 13))
    got = lg.withdraw_rows([per_slab, per_slab + 1, 12], [senders[5]] * 3, N_LEVELS)
    assert got["status"].tolist() == [E.NOT_KEPT, 0, 0] and [D.to_int(r) for r in got["root_exit"][1:]] == [roots[per_slab + 1], roots[12]]
    lg.exit_forget(100)
    assert lg.exit_archive_stats()["slabs"] == 0 and lg.exit_archive_stats()["bytes_used"] == 0 and lg.exit_kept() == []
    lg.close()


# ---- forget, stats, argument errors ------------------------------------------------------------------------------------------------------------
def test_forget_and_argument_errors(hz):
    lg, sp, bbs = _run_sequence(hz)
    f0 = sp.first_idx
    queries = [(num, idx, E.FOUND) for num, idx in _found_pairs(bbs)] + [(2, f0 + 1, E.ABSENT)]
    ask = lambda: lg.withdraw_rows([q[0] for q in queries], [q[1] for q in queries], N_LEVELS)   # noqa: E731
    before = ask()
    lg.exit_forget(2)
    assert lg.exit_kept() == [2, 3]
    after = ask()
    assert after["status"].tolist() == [E.NOT_KEPT if q[0] == 1 else q[2] for q in queries]
    for i, q in enumerate(queries):
        for name in E.ROWS + ("siblings_state",):
            assert after[name][i].tobytes() == (bytes(before[name][i].size) if q[0] == 1 else before[name][i].tobytes()), (q, name)
    with pytest.raises(HzError) as e:
        lg.exit_root_of(1)
    assert e.value.status == 1 and "not kept" in str(e.value)
    lg.exit_forget(0)
    lg.exit_forget(2)   # nothing below: nothing happens
    assert lg.exit_kept() == [2, 3]
    # argument errors, and the archive answers as before after each
    for call, text in ((lambda: lg.exit_keep(3), "not above the last kept batch"), (lambda: lg.exit_keep(2), "not above the last kept batch"),
                       (lambda: lg.exit_keep(0), "not above the last kept batch"), (lambda: lg.withdraw_rows([3], [f0 + 1], -1), "n_levels + 1 = 0"),
                       (lambda: lg.withdraw_rows([3], [f0 + 1], 64), "n_levels + 1 = 65"),
                       (lambda: lg.L._check(lg.L.c.hz_ledger_withdraw_rows(lg.h, 1, None, None, N_LEVELS, None)), "null argument"),
                       (lambda: lg.L._check(lg.L.c.hz_ledger_withdraw_rows(lg.h, (1 << 20) + 1, 8, 8, N_LEVELS, None)), "at most 2^20"),
                       (lambda: lg.L._check(lg.L.c.hz_ledger_exit_root_of(lg.h, 3, None)), "null argument"),
                       (lambda: lg.L._check(lg.L.c.hz_ledger_exit_kept(lg.h, None, 4, None)), "null argument"),
                       (lambda: lg.L._check(lg.L.c.hz_ledger_withdraw_rows_dev(lg.h, None)), "null argument")):
        with pytest.raises(HzError) as e:
            call()
        assert e.value.status == 1 and text in str(e.value), str(e.value)
        again = ask()
        assert all(again[name].tobytes() == after[name].tobytes() for name in WITHDRAW_ARRAYS) and lg.exit_kept() == [2, 3]
    # keep / forget cycles of batches of one size: the archive does not grow
    stats = []
    for k in range(4, 10):
        lg.apply_batch_exits([X.fx(sp, f0 + 3, 100 + k), X.fx(sp, f0 + 4, 100 + k)], [], PLAN, _idxs(sp), 1, 1, n_sib=N_LEVELS + 1, outputs=False)
        lg.exit_keep(k)
        lg.exit_forget(k)
        stats.append(lg.exit_archive_stats())
        assert lg.exit_kept() == [k] and D.to_int(lg.withdraw_rows([k], [f0 + 3], N_LEVELS)["balance"][0]) == 100 + k
    assert all(s == stats[0] for s in stats) and stats[0]["snapshots"] == 1 and stats[0]["slabs"] == 1
    # a reload starts a new history
    lg.load(*sp.leaf_fields())
    assert lg.exit_kept() == [] and lg.exit_archive_stats()["slabs"] == 0 and lg.withdraw_rows([9], [f0 + 3], N_LEVELS)["status"].tolist() == [E.NOT_KEPT]
    lg.exit_keep(0)   # batch number 0 of the new history (hz_ledger_load leaves the live exit tree as it is)
    assert lg.exit_kept() == [0] and lg.exit_root_of(0) == lg.exit_tree().root() != 0 and lg.exit_archive_stats()["slabs"] == 1
    lg.close()


# ---- a growing ledger ------------------------------------------------------------------------------------------------------------------------------
def test_a_growing_ledger_keeps_the_exit_of_a_created_account(hz):
    acc = K.Accounts([])
    lg = acc.to_ledger(hz, 64)
    l1_txs, l2_txs, plan, idxs = K.kinds_batch(acc)
    m = K.model(acc, l1_txs, l2_txs, plan, idxs)
    assert isinstance(m, dict), m
    db, bb = K.builder_batch(acc.db(), l1_txs, l2_txs, plan, idxs, N_LEVELS, aux_to=m["aux_to_idx"])
    created = set(m["slots"])
    assert bb.exit_leaves and set(bb.exit_leaves) & created
    lg.apply_batch_creates(l1_txs, l2_txs, plan, idxs, 1, 1, n_sib=N_LEVELS + 1, outputs=False)
    assert lg.root() == bb.new_state_root and lg.exit_tree().root() == bb.new_exit_root
    lg.exit_keep(1)
    lg.apply_batch_creates([], [{}], plan, idxs, 1, 2, n_sib=N_LEVELS + 1, outputs=False)
    assert lg.exit_tree().size() == 0
    queries = [(1, k, E.FOUND) for k in sorted(bb.exit_leaves)] + [(1, acc.first_idx + 63, E.ABSENT)]
    _check_rows(lg.withdraw_rows([q[0] for q in queries], [q[1] for q in queries], N_LEVELS), queries, {1: bb})
    assert lg.exit_root_of(1) == bb.new_exit_root
    lg.close()
