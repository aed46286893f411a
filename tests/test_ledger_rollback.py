"""hz_ledger's undo journal and rollback (hz_ledger_journal / _applied / _rollback). The oracle is a TWIN ledger: X loads a
state S, applies A (...), rolls back and applies B; Y loads S and applies B. Every output array of B, the root, hz_ledger_accounts of every
account and -- on a dense ledger hz_state_download, on a growing one the proofs of every account out of the resident pools -- must be
byte-equal between X and Y, and B touches accounts that A touched. States of 16 accounts unless a case says otherwise.
On a growing ledger the proofs (of every account and of four absent keys), the root and the size are the only read path there is: pool
entries no proof reaches and the shape's host vectors are judged by tests/native/ledger_journal_check.cpp, field by field, not here."""
import types

import numpy as np
import pytest

import ledger_addr_common as A
import ledger_atomic_common as Q
import ledger_common as C
import ledger_create_common as K
import ledger_exit_common as X
import ledger_l1_common as L1
import ledger_sig_common as S
from circuits_amd import HzError
from circuits_amd import builder as B

pytestmark = pytest.mark.gpu
SHAPE = (8, 16, 4, 4)
N_SIB = SHAPE[1] + 1
P = B.P
CHAIN = S.CHAIN_ID
EDGE_KEY = (P - 1) | 1 << 254 | 1 << 255


@pytest.fixture(scope="module")
def base():
    return C.base_state(4)


def _dense(hz, st, depth=4):
    lg = st.to_ledger(hz)
    lg.journal(depth)
    return lg


def _growing(hz, st, room=8, depth=4):
    lg = K.Accounts.of(st).to_ledger(hz, st.N + room, n_sib_max=N_SIB)
    lg.journal(depth)
    return lg


def _signed(st, l2_txs, n_l1=0):
    return [S.sign(st, t, CHAIN) for t in Q.derive(n_l1, l2_txs)]


def _snapshot(lg):
    """everything resident the caller can read: last, because hz_ledger_accounts reuses the call's buffers"""
    n = lg.size()
    everyone = np.arange(lg.first_idx, lg.first_idx + n)
    out = {"root": lg.root(), "size": n, "last_idx": lg.last_idx()}
    if hasattr(lg, "n_sib_max"):   # growing: shape and pools, through the proofs of every account and of a few absent keys
        keys = np.concatenate([everyone, everyone[-1:] + 1 + np.arange(4)]).astype(np.uint64)
        out.update({"proof_" + k: np.asarray(v).tobytes() for k, v in lg.state_smt().proofs(keys, n_sib=N_SIB).items()})
        out["smt_size"] = lg.state_smt().size()
    else:
        levels, value = lg.tree().download()
        out["levels"] = b"".join(a.tobytes() for a in levels)
        out["value"] = value.tobytes()
    out["planes"] = lg.accounts(everyone).tobytes() if n else b""
    return out


def _same_outputs(got, exp):
    assert set(got) == set(exp) and len(exp) >= 27, sorted(set(got) ^ set(exp))
    for name in exp:
        assert got[name].tobytes() == exp[name].tobytes(), name


# ---- the seven forms as A; B is a batch with exits (and creates on a growing ledger) over accounts A touched ---------------------------------
def _atomic_rows(base):
    a, b = base.first_idx, base.first_idx + 1
    l2 = [dict(C.tx(a, b, 10, 50, nonce=0), rqOffset=1),
          dict(C.tx(b, a, 20, 60, nonce=0), rqOffset=7, maxNumBatch=5, toEthAddr=0xABCDEF << 100, toBjjAy=P - 2, toBjjSign=1),
          dict(C.tx(a, b, 1, 0, nonce=1), rqOffset=3), C.tx(a, b, 2, 0, nonce=2), dict(C.tx(b, a, 3, 0, nonce=1), rqOffset=6), C.tx(b, a, 4, 0, nonce=2)]
    return Q.deposits(base, 2), l2


def _form_a(name, base):
    """-> (dense or growing, lambda ledger: the outputs of A)"""
    f0 = base.first_idx
    plan, idxs = [1], [f0 + 2]
    if name == "apply_l2":
        txs = Q.transfers(base, 6)
        return "dense", lambda lg: lg.apply_l2(txs, plan, idxs, n_sib=N_SIB)
    if name == "apply_l2_signed":
        txs = _signed(base, Q.transfers(base, 3, signed_dest=True) + [{}] + Q.transfers(base, 3, start=5))
        return "dense", lambda lg: lg.apply_l2_signed(txs, plan, idxs, CHAIN, 1, n_sib=N_SIB)
    if name == "apply_l2_addr":
        txs = _signed(base, [C.tx(f0, f0 + 1, 9, 1, nonce=0), A.to_addr(C.tx(f0 + 1, 0, 5, 0, nonce=0), base.state(f0 + 7)), {}, C.tx(f0 + 4, f0 + 5, 0, 0, nonce=0)])
        return "dense", lambda lg: lg.apply_l2_addr(txs, plan, idxs, CHAIN, 1, n_sib=N_SIB, verify=True)
    if name == "apply_batch":
        l1 = Q.deposits(base, 2) + [L1.own(base, f0 + 3, f0 + 4, 5)]
        txs = _signed(base, Q.transfers(base, 2, start=0, signed_dest=True) + [{}] + Q.transfers(base, 1, start=5), len(l1))
        return "dense", lambda lg: lg.apply_batch(l1, txs, plan, idxs, CHAIN, 1, n_sib=N_SIB, verify=True)
    if name == "apply_batch_exits":
        l1 = [L1.own(base, f0 + 2, 0, 0, 11), X.fx(base, f0 + 5, 3)]
        txs = _signed(base, [C.tx(f0, f0 + 1, 4, 1, nonce=0), X.x2(f0 + 1, 4, nonce=0), {}, X.x2(f0 + 5, 2, nonce=0)], len(l1))
        return "dense", lambda lg: lg.apply_batch_exits(l1, txs, plan, idxs, CHAIN, 1, n_sib=N_SIB, verify=True)
    if name == "apply_batch_creates":
        l1 = [K.create(P - 77, token=1, eth=0xBEEF << 90, load=10 ** 5), L1.own(base, f0 + 1, 0, 0, 7), K.create(P - 78 | 1 << 255, token=1, eth=5, load=9)]
        txs = _signed(base, [C.tx(f0, f0 + base.N + 1, 4, 1, nonce=0), X.x2(f0 + 5, 2, nonce=0), C.tx(f0 + 2, f0 + 3, 1, 0, nonce=0)], len(l1))
        return "growing", lambda lg: lg.apply_batch_creates(l1, txs, plan, idxs, CHAIN, 1, n_sib=N_SIB, verify=True)
    assert name == "apply_batch_atomic"
    l1, l2 = _atomic_rows(base)
    txs = _signed(base, l2, len(l1))
    return "growing", lambda lg: lg.apply_batch_atomic(l1, txs, plan, idxs, CHAIN, 1, n_sib=N_SIB, verify=True)


def _batch_b(kind, base):
    f0 = base.first_idx
    plan, idxs = [1], [f0 + 2]
    if kind == "dense":
        l1 = [L1.own(base, f0 + 1, 0, 0, 9), X.fx(base, f0 + 5, 3)]
        txs = _signed(base, [C.tx(f0, f0 + 1, 6, 1, nonce=0), X.x2(f0 + 1, 3, nonce=0), C.tx(f0 + 3, f0, 2, 0, nonce=0), {}, C.tx(f0 + 4, f0 + 6, 1, 100, nonce=0)], len(l1))
        return lambda lg: lg.apply_batch_exits(l1, txs, plan, idxs, CHAIN, 1, n_sib=N_SIB, verify=True)
    l1 = [K.create(EDGE_KEY, token=1, eth=0xC0FFEE << 96, load=10 ** 6), L1.own(base, f0 + 1, 0, 0, 7), K.create(P - 99, token=1, eth=77, load=5)]
    txs = _signed(base, [C.tx(f0, f0 + base.N, 4, 1, nonce=0), X.x2(f0 + 1, 3, nonce=0), C.tx(f0 + 2, f0 + 3, 1, 0, nonce=0), C.tx(f0 + 5, f0 + base.N + 1, 1, 0, nonce=0)], len(l1))
    return lambda lg: lg.apply_batch_creates(l1, txs, plan, idxs, CHAIN, 1, n_sib=N_SIB, verify=True)


FORMS = ["apply_l2", "apply_l2_signed", "apply_l2_addr", "apply_batch", "apply_batch_exits", "apply_batch_creates", "apply_batch_atomic"]


@pytest.mark.parametrize("name", FORMS)
def test_every_form_is_undone_and_applies_again(hz, base, name):
    """X: A, back to mark 0, B -- against Y: B. Then X back to 0 again and A a second time: A's first outputs byte for byte"""
    kind, apply_a = _form_a(name, base)
    apply_b = _batch_b(kind, base)
    make = _dense if kind == "dense" else _growing
    x, y = make(hz, base), make(hz, base, depth=0)
    assert x.applied() == 0
    s0 = _snapshot(x)
    first = apply_a(x)
    assert x.applied() == 1 and x.journal_stats()["records"] == 1 and x.journal_ms() > 0.0
    assert _snapshot(x) != s0
    x.rollback(0)
    assert x.applied() == 0 and x.journal_stats()["records"] == 0 and x.rollback_ms() > 0.0
    assert _snapshot(x) == s0
    got, exp = apply_b(x), apply_b(y)
    _same_outputs(got, exp)
    assert x.exit_tree().root() == y.exit_tree().root()
    assert _snapshot(x) == _snapshot(y)
    x.rollback(0)
    assert _snapshot(x) == s0
    again = apply_a(x)
    _same_outputs(again, first)
    x.close()
    y.close()


def test_two_batches_on_overlapping_accounts_at_once_and_one_by_one(hz, base):
    """A1 and A2 both touch accounts 0 .. 3 and the fee account: undone in one call the oldest saved value must win; one at a time every
    step is the twin's state. Rolling back to the current mark changes nothing and the *_dev getters still answer"""
    f0 = base.first_idx
    plan, idxs = [1], [f0 + 2]
    a1 = Q.transfers(base, 6)
    a2 = [C.tx(f0, f0 + 3, 5, 1, nonce=1), C.tx(f0 + 1, f0, 2, 100, nonce=1), C.tx(f0 + 3, f0 + 2, 1, 0, nonce=1), C.tx(f0 + 9, f0 + 1, 7, 0, nonce=0)]
    x, y1 = _dense(hz, base), _dense(hz, base, depth=0)
    s0 = _snapshot(x)
    x.apply_l2(a1, plan, idxs, n_sib=N_SIB)
    y1.apply_l2(a1, plan, idxs, n_sib=N_SIB)
    s1 = _snapshot(y1)
    x.apply_l2(a2, plan, idxs, n_sib=N_SIB)
    assert x.applied() == 2 and x.journal_stats()["records"] == 2 and x.journal_stats()["oldest_mark"] == 0
    # the current mark: a no-op that invalidates nothing
    dev = x.outputs_dev()
    x.rollback(2)
    assert x.outputs_dev() == dev and x.applied() == 2 and x.journal_stats()["records"] == 2
    s2 = _snapshot(x)
    x.rollback(0)
    assert _snapshot(x) == s0 and x.applied() == 0
    x.apply_l2(a1, plan, idxs, n_sib=N_SIB)
    x.apply_l2(a2, plan, idxs, n_sib=N_SIB)
    assert _snapshot(x) == s2
    x.rollback(1)
    assert _snapshot(x) == s1 and x.applied() == 1 and x.journal_stats()["records"] == 1
    x.rollback(0)
    assert _snapshot(x) == s0
    x.close()
    y1.close()


# ---- a growing ledger ----------------------------------------------------------------------------------------------------------------------
def test_creates_whose_inserts_move_existing_leaves(hz, base):
    """16 accounts from 256: key 272 meets leaf 256 at depth 4 and moves it one deeper, 273 moves 257, and so on. After the rollback the size,
    the root and the indices the next creates receive are the twin's"""
    f0 = base.first_idx
    plan, idxs = [1], [f0 + 2]
    a_l1 = [K.create(P - 300 - j, token=1, eth=900 + j, load=50 + j) for j in range(4)]
    a_l2 = [C.tx(f0, f0 + 17, 3, 0, nonce=0), C.tx(f0 + 1, f0, 1, 0, nonce=0)]
    b_l1 = [K.create(P - 500 - j | (j & 1) << 255, token=1, eth=1900 + j, load=70 + j) for j in range(3)]
    b_l2 = [C.tx(f0, f0 + 16, 2, 0, nonce=0), C.tx(f0 + 1, f0 + 18, 1, 1, nonce=0)]
    x, y = _growing(hz, base), _growing(hz, base, depth=0)
    size0 = x.state_smt().size()
    x.apply_batch_creates(a_l1, a_l2, plan, idxs, CHAIN, 1, n_sib=N_SIB, sigs=False)
    assert x.size() == 20 and x.last_idx() == f0 + 19 and x.state_smt().size() == size0 + 4
    x.rollback(0)
    assert x.size() == 16 and x.last_idx() == f0 + 15 and x.state_smt().size() == size0
    got = x.apply_batch_creates(b_l1, b_l2, plan, idxs, CHAIN, 1, n_sib=N_SIB, sigs=False)
    exp = y.apply_batch_creates(b_l1, b_l2, plan, idxs, CHAIN, 1, n_sib=N_SIB, sigs=False)
    _same_outputs(got, exp)
    assert C.to_int(got["aux_from_idx"][0]) == f0 + 16 and C.to_int(got["new_last_idx"][0]) == f0 + 18 and not got["is_old0_1"][0].any()   # 272 met a leaf
    assert _snapshot(x) == _snapshot(y)
    x.close()
    y.close()


def test_a_pool_reallocated_between_a_record_and_its_rollback(hz):
    """4090 loaded accounts: the leaf and value pools hold 4096 entries. A creates 2 (4092 leaves), B creates 16 (4108): B's prepare moves
    the pools to larger buffers while A's record is held. Back to mark 0 in one call: the records name entries, not addresses"""
    n, f0 = 4090, 256
    leaves = [{"tokenID": 1, "nonce": 0, "sign": j & 1, "balance": 10 ** 12 + j, "ay": 7000 + j, "ethAddr": 90000 + j} for j in range(n)]
    acc = K.Accounts(leaves, first_idx=f0)
    plan, idxs = [1], [f0 + 2]

    def creates(count, tag):
        return [K.create(P - tag - j, token=1, eth=tag + j, load=5 + j) for j in range(count)]
    a = (creates(2, 1000), [C.tx(f0, f0 + n, 3, 0, nonce=0), C.tx(f0 + 4089, f0 + 1, 2, 1, nonce=0)])
    b = (creates(16, 2000), [C.tx(f0, f0 + n + 5, 3, 0, nonce=1), C.tx(f0 + 1, f0 + 4089, 2, 1, nonce=0)])
    c = (creates(3, 3000), [C.tx(f0, f0 + n + 2, 4, 1, nonce=0), C.tx(f0 + 4089, f0, 2, 0, nonce=0)])
    x, y = acc.to_ledger(hz, n + 40, n_sib_max=N_SIB), acc.to_ledger(hz, n + 40, n_sib_max=N_SIB)
    x.journal(2)
    probe = np.concatenate([np.arange(f0, f0 + 40), np.arange(f0 + n - 40, f0 + n + 20)]).astype(np.uint64)

    def view(lg):
        out = {"root": lg.root(), "size": lg.size(), "smt_size": lg.state_smt().size()}
        out.update({k: np.asarray(v).tobytes() for k, v in lg.state_smt().proofs(probe, n_sib=N_SIB).items()})
        out["planes"] = lg.accounts(np.arange(f0, f0 + lg.size())).tobytes()
        return out
    s0 = view(x)
    for l1, l2 in (a, b):
        x.apply_batch_creates(l1, l2, plan, idxs, CHAIN, 1, n_sib=N_SIB, sigs=False)
    assert x.size() == n + 18 and x.state_smt().size() == n + 18 and x.applied() == 2
    x.rollback(0)
    assert view(x) == s0 == view(y)
    got = x.apply_batch_creates(*c, plan, idxs, CHAIN, 1, n_sib=N_SIB, sigs=False)
    exp = y.apply_batch_creates(*c, plan, idxs, CHAIN, 1, n_sib=N_SIB, sigs=False)
    _same_outputs(got, exp)
    assert C.to_int(got["new_last_idx"][0]) == f0 + n + 2 and view(x) == view(y)
    x.close()
    y.close()


# ---- exits and the archive -----------------------------------------------------------------------------------------------------------------
def test_kept_exit_trees_across_a_rollback(hz):
    """keep(1), apply, keep(2), back to before batch 2: batch 1 stays and answers as before, batch 2 is gone and can be kept again; the live
    exit tree is empty and its device outputs are refused"""
    sp = X.exit_state(6)
    f0, leaf = sp.first_idx, sp.state
    a, b, c, far, w = f0 + 1, f0 + 3, f0 + 4, f0 + 33, f0 + 6
    part = lambda v, d=3: L1.float_floor(leaf(v)["balance"] // d)   # noqa: E731
    plan, idxs = [1, 2], [f0 + 40, 0]
    one = ([X.fx(sp, b, part(b, 4), load=900)], [X.x2(a, part(a), 100, nonce=0), C.tx(c, b, 1000, 176, nonce=0), X.x2(far, part(far), nonce=0), X.x2(b, 2000, 176, nonce=0)])
    two = ([X.fx(sp, c, 4000)], [X.x2(a, 3000, 100, nonce=1), X.x2(w, X.WHOLE // 4, 1, nonce=0), X.x2(f0 + 17, 7000, nonce=0)])
    lg = sp.to_ledger(hz)
    lg.journal(4)
    lg.apply_batch_exits(*one, plan, idxs, 1, 1, n_sib=17, outputs=False)
    lg.exit_keep(1)
    queries = ([1, 1, 1, 2, 2], [a, b, far, a, w])
    rows1 = lg.withdraw_rows(*queries, 16)
    assert rows1["status"].tolist() == [0, 0, 0, 1, 1]
    stats1, mark = lg.exit_archive_stats(), lg.applied()
    lg.apply_batch_exits(*two, plan, idxs, 1, 2, n_sib=17, outputs=False)
    root2 = lg.exit_tree().root()
    lg.exit_outputs_dev()   # (answers: the apply was the ledger's last call)
    lg.exit_keep(2)
    rows2 = lg.withdraw_rows(*queries, 16)
    assert rows2["status"].tolist() == [0] * 5 and lg.exit_kept() == [1, 2] and lg.exit_archive_stats()["bytes_used"] > stats1["bytes_used"]
    lg.rollback(mark)
    assert lg.exit_kept() == [1] and lg.exit_archive_stats() == stats1
    assert lg.exit_tree().root() == 0 and lg.exit_tree().size() == 0
    with pytest.raises(HzError) as e:
        lg.exit_outputs_dev()
    assert e.value.status == 1
    with pytest.raises(HzError):
        lg.exit_accounts([a])
    back = lg.withdraw_rows(*queries, 16)
    for name in rows1:
        assert back[name].tobytes() == rows1[name].tobytes(), name
    with pytest.raises(HzError) as e:
        lg.exit_root_of(2)
    assert "batch 2 is not kept" in str(e.value)
    lg.apply_batch_exits(*two, plan, idxs, 1, 2, n_sib=17, outputs=False)
    assert lg.exit_tree().root() == root2
    lg.exit_keep(2)
    again = lg.withdraw_rows(*queries, 16)
    for name in rows2:
        assert again[name].tobytes() == rows2[name].tobytes(), name
    # nothing was kept when the first apply began: back to mark 0 drops every snapshot
    lg.rollback(0)
    assert lg.exit_kept() == [] and lg.exit_archive_stats()["bytes_used"] == 0
    lg.close()


# ---- lane and block edges ------------------------------------------------------------------------------------------------------------------
def _record_bytes(tree_entries, groups):
    """csrc/ledger_journal.h's journal_layout: elements, then uint32 entries rounded up to 32 bytes, for the tree part and the plane part"""
    r32 = lambda v: (v + 31) // 32 * 32   # noqa: E731
    return tree_entries * 32 + r32(tree_entries * 4) + 4 * groups * 32 + r32(groups * 4)


def _dense_entries(accounts, k):
    """what k_state_writeback replaces for a set of account offsets: the distinct nodes per depth 0 .. k, and one state hash per account"""
    return sum(len({j & ((1 << d) - 1) for j in accounts}) for d in range(k + 1)) + len(accounts)


@pytest.mark.parametrize("accounts,entries", [(list(range(63)), 252), (list(range(64)), 255), (list(range(63)) + [64, 65], 256), (list(range(65)), 257)])
def test_lane_and_block_edges_on_128_accounts(hz, accounts, entries):
    """2^7 accounts. The batch is a chain of transfers through the chosen accounts, the fee account among them, so exactly these are
    touched: 63 / 64 / 65 of them put the plane kernels' 4 G lanes at 252 / 256 / 260 -- across the 256-lane block -- and G across the
    64-lane wavefront. The tree's write-back list is the distinct nodes per depth plus a state hash per account: accounts 0 .. n - 1 give
    min(n, 2^d) nodes at depth d, so 64 accounts are 255 entries and 65 are 257; 65 accounts with only 63 residues modulo 64 (0 .. 62, 64,
    65: 64 and 65 share the depth-6 nodes of 0 and 1) are 256. The record's size says the lists were hit"""
    base = C.base_state(7)
    f0 = base.first_idx
    assert _dense_entries(accounts, 7) == entries
    txs = [C.tx(f0 + s, f0 + r, 1 + i % 3, 0, nonce=0) for i, (s, r) in enumerate(zip(accounts, accounts[1:]))]
    other = [C.tx(f0 + accounts[5], f0 + 100, 2, 1, nonce=0), C.tx(f0 + accounts[-1], f0 + accounts[0], 1, 0, nonce=0), C.tx(f0 + 70, f0 + 63, 1, 0, nonce=0)]
    plan, idxs = [1], [f0 + accounts[3]]
    x, y = _dense(hz, base), _dense(hz, base, depth=0)
    s0 = _snapshot(x)
    x.apply_l2(txs, plan, idxs, n_sib=8)
    st = x.journal_stats()
    assert st["records"] == 1 and st["bytes_used"] == _record_bytes(entries, len(accounts)) and st["bytes_reserved"] >= 4 * st["bytes_used"]
    x.rollback(0)
    assert _snapshot(x) == s0
    _same_outputs(x.apply_l2(other, plan, idxs, n_sib=8), y.apply_l2(other, plan, idxs, n_sib=8))
    assert _snapshot(x) == _snapshot(y)
    x.close()
    y.close()


def test_block_edge_of_the_pool_entries_on_a_growing_ledger(hz):
    """the same chain through 100 of 128 accounts on a growing ledger. The keys 256 .. 383 make the perfect tree of depth 7, and accounts
    0 .. 99 cover every residue modulo 64: all 127 nodes are touched, and a leaf hash and a value per account -- 327 pool entries in one
    record, so the pool kernels cross their block edge"""
    base = C.base_state(7)
    f0 = base.first_idx
    txs = [C.tx(f0 + j, f0 + j + 1, 1 + j % 3, 0, nonce=0) for j in range(99)]
    other = [C.tx(f0 + 5, f0 + 100, 2, 1, nonce=0), C.tx(f0 + 99, f0, 1, 0, nonce=0)]
    plan, idxs = [1], [f0 + 3]
    x, y = K.Accounts.of(base).to_ledger(hz, 130, n_sib_max=N_SIB), K.Accounts.of(base).to_ledger(hz, 130, n_sib_max=N_SIB)
    x.journal(1)
    s0 = _snapshot(x)
    x.apply_l2(txs, plan, idxs, n_sib=N_SIB)
    assert x.journal_stats()["bytes_used"] == _record_bytes(127 + 200, 100)
    x.rollback(0)
    assert _snapshot(x) == s0
    _same_outputs(x.apply_l2(other, plan, idxs, n_sib=N_SIB), y.apply_l2(other, plan, idxs, n_sib=N_SIB))
    assert _snapshot(x) == _snapshot(y)
    x.close()
    y.close()


# ---- refusals, marks, windows --------------------------------------------------------------------------------------------------------------
def _refused(lg, mark, *words):
    with pytest.raises(HzError) as e:
        lg.rollback(mark)
    assert e.value.status == 1 and all(w in str(e.value) for w in words), str(e.value)


def test_refusals_change_nothing(hz, base):
    f0 = base.first_idx
    plan, idxs = [1], [f0 + 2]
    lg = hz.ledger(4, first_idx=f0)
    _refused(lg, 0, "hz_ledger_rollback", "no accounts yet")   # before load
    lg.load(*base.leaf_fields())
    assert lg.journal_stats() == {"depth": 0, "records": 0, "oldest_mark": 0, "bytes_used": 0, "bytes_reserved": 0}
    lg.rollback(0)   # the current mark, journal or not
    batches = [[C.tx(f0 + j, f0 + j + 1, 2, 0, nonce=r) for j in range(4)] for r in range(3)]
    lg.apply_l2(batches[0], plan, idxs, n_sib=N_SIB)
    state = _snapshot(lg)
    _refused(lg, 0, "mark = 0", "applied = 1", "journal is off")   # the default
    _refused(lg, 2, "mark = 2", "applied = 1", "ahead")
    assert _snapshot(lg) == state and lg.applied() == 1
    with pytest.raises(HzError) as e:
        lg.journal(65)
    assert e.value.status == 1 and "depth = 65" in str(e.value)
    lg.journal(2)
    _refused(lg, 0, "mark = 0", "applied = 1", "0 records")   # applied before the journal was on
    lg.load(*base.leaf_fields())
    for txs in batches:
        lg.apply_l2(txs, plan, idxs, n_sib=N_SIB)
    state = _snapshot(lg)
    assert lg.journal_stats()["records"] == 2 and lg.journal_stats()["oldest_mark"] == 1 and lg.applied() == 3
    _refused(lg, 0, "mark = 0", "applied = 3", "2 records of depth 2")   # the ring has moved on
    _refused(lg, 4, "mark = 4", "applied = 3")
    assert _snapshot(lg) == state and lg.applied() == 3 and lg.journal_stats()["records"] == 2
    lg.rollback(1)   # the ring's far edge
    twin = base.to_ledger(hz)
    twin.apply_l2(batches[0], plan, idxs, n_sib=N_SIB)
    assert _snapshot(lg) == _snapshot(twin) and lg.applied() == 1 and lg.journal_stats()["records"] == 0
    lg.journal(0)
    assert lg.journal_stats()["depth"] == 0 and lg.journal_stats()["bytes_reserved"] == 0
    lg.close()
    twin.close()


def test_a_refused_apply_counts_nothing_and_a_load_resets(hz, base):
    f0 = base.first_idx
    plan, idxs = [1], [f0 + 2]
    lg = _dense(hz, base, depth=3)
    lg.apply_l2(Q.transfers(base, 4), plan, idxs, n_sib=N_SIB)
    before = (lg.applied(), lg.journal_stats(), lg.root())
    with pytest.raises(HzError) as e:
        lg.apply_l2([C.tx(f0, f0 + 1, 1, 0, nonce=5)], plan, idxs, n_sib=N_SIB)   # a stale nonce
    assert e.value.status == 4 and "reason 2:" in str(e.value)
    with pytest.raises(HzError):
        lg.apply_l2([C.tx(f0 + 99, f0 + 1, 1, 0, nonce=0)], plan, idxs, n_sib=N_SIB)   # an argument error
    # the calls that apply nothing do not count either
    signed = _signed(base, [C.tx(f0 + 4, f0 + 5, 1, 0, nonce=1)])
    lg.verify_l2(signed, CHAIN, 1)
    lg.resolve_l2(signed)
    lg.select_batch([], signed, CHAIN, 1)
    lg.withdraw_rows([1], [f0], 16)
    assert (lg.applied(), lg.journal_stats(), lg.root()) == before and before[0] == 1 and before[1]["records"] == 1
    lg.load(*base.leaf_fields())
    st = lg.journal_stats()
    assert lg.applied() == 0 and st["records"] == 0 and st["depth"] == 3 and st["oldest_mark"] == 0 and st["bytes_used"] == 0
    _refused(lg, 1, "mark = 1", "applied = 0")
    lg.close()


def test_main_inputs_and_selection_after_a_rollback(hz, base):
    """the main_inputs window closes with the rollback, and select_batch gives the verdicts it gave before A"""
    g = hz.ctx("rollup-main", nTx=SHAPE[0], nLevels=SHAPE[1], maxL1Tx=SHAPE[2], maxFeeTx=SHAPE[3])
    f0 = base.first_idx
    l1, l2 = _atomic_rows(base)
    padded = _signed(base, l2, len(l1)) + [{} for _ in range(SHAPE[0] - len(l1) - len(l2))]
    pool = _signed(base, Q.transfers(base, 6) + [C.tx(f0, f0 + 1, 1, 0, nonce=7), C.tx(f0 + 1, f0, 10 ** 30, 0, nonce=1)])
    lg = _dense(hz, base)
    sel0 = lg.select_batch([], pool, CHAIN, 1, verify=True)
    lg.apply_resident(l1, padded, [1, 0, 0, 0], [f0 + 2, 0, 0, 0], CHAIN, 1, n_sib=N_SIB, verify=True, atomic=True)
    lg.main_inputs(g, f0 + base.N - 1)
    sel1 = lg.select_batch([], pool, CHAIN, 1, verify=True)
    assert list(sel1["verdict"]) != list(sel0["verdict"])   # A moved the nonces of accounts 0 and 1
    lg.rollback(0)
    st = hz.c.hz_ledger_main_inputs(lg.h, g.h, f0 + base.N - 1, 32, g.packed_layout()[0])
    assert st == 1 and "no successful apply call" in hz.c.hz_last_error().decode()
    sel2 = lg.select_batch([], pool, CHAIN, 1, verify=True)
    assert set(sel2) == set(sel0)
    for k in sel0:
        assert np.array_equal(np.asarray(sel2[k]), np.asarray(sel0[k])), k
    lg.close()
    g.close()


def test_rollup_main_accepts_the_batch_applied_after_a_rollback(hz, base):
    """RollupMain(8, 16, 4, 4): A, back, then B through apply_resident + main_inputs + stage (builder.ledger_packed_batch). hz_witness_check
    passes and the witness is the oracle's for B on S"""
    from oracle_binding import OracleCtx
    f0 = base.first_idx
    fee_tokens, fee_idxs = [1], [f0 + 2]
    a_l1, a_l2 = _atomic_rows(base)
    a_rows = _signed(base, a_l2, len(a_l1)) + [{} for _ in range(SHAPE[0] - len(a_l1) - len(a_l2))]
    b_l1 = [L1.own(base, f0 + 1, 0, 0, 9), X.fx(base, f0 + 5, 3)]
    b_l2 = [dict(t, signer=S.signer(base, t["fromIdx"])) for t in [C.tx(f0, f0 + 1, 6, 1, nonce=0), X.x2(f0 + 1, 3, nonce=0), C.tx(f0 + 3, f0, 2, 0, nonce=0)]]
    g = hz.ctx("rollup-main", nTx=SHAPE[0], nLevels=SHAPE[1], maxL1Tx=SHAPE[2], maxFeeTx=SHAPE[3])
    lg = _dense(hz, base)
    lg.apply_resident(a_l1, a_rows, [1, 0, 0, 0], [f0 + 2, 0, 0, 0], CHAIN, 1, n_sib=N_SIB, verify=True, atomic=True)
    lg.rollback(0)
    like = types.SimpleNamespace(last_idx=f0 + base.N - 1, num_batch=0)
    B.ledger_packed_batch(lg, g, like, b_l1, b_l2, fee_tokens, fee_idxs, CHAIN, verify=True)
    g.enqueue()
    g.check()   # hz_witness_check: waits for the step and judges every range and constraint flag
    twin = base.to_ledger(hz)
    inp = B.ledger_exit_batch_inputs(twin, types.SimpleNamespace(last_idx=f0 + base.N - 1, num_batch=0), b_l1, b_l2, *SHAPE, fee_tokens, fee_idxs, CHAIN, verify=True)[0]
    o = OracleCtx("rollup-main", *SHAPE)
    o.set_inputs(inp)
    assert o.run() is None
    assert g.read_raw_bytes() == o.read_raw_bytes() and lg.root() == twin.root()
    for v in (lg, twin, g):
        v.close()


def test_capture_changes_no_result(hz, base):
    """depth 0 against depth 4: the outputs of the same apply are byte-equal, on a dense and on a growing ledger"""
    for kind in ("dense", "growing"):
        make = _dense if kind == "dense" else _growing
        apply_b = _batch_b(kind, base)
        off, on = make(hz, base, depth=0), make(hz, base, depth=4)
        _same_outputs(apply_b(on), apply_b(off))
        assert off.journal_ms() == 0.0 and on.journal_ms() > 0.0 and off.journal_stats()["bytes_reserved"] == 0
        assert _snapshot(on) == _snapshot(off)
        off.close()
        on.close()
