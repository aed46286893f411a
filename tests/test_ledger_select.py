"""A batch selected from a pool on the device-resident ledger (hz_ledger_select_batch), on ledgers of 16 accounts and pools of
at most 24 unless said otherwise. The verdicts, the kept list, the offsets and the number of walks against ledger_select_common's model
(itself checked against the refusal contract on the CPU); the retry loop over the real hz_ledger_apply_batch_atomic; what is kept applied
as it stands; RollupMain itself (the HIP context and the oracle) on the selected batch; residency; the staging tile's edges; the slot
capacity, which is the first launch with the kernel's whole LDS."""
import re
import types

import pytest

import ledger_atomic_common as Q
import ledger_common as C
import ledger_create_common as CR
import ledger_exit_common as X
import ledger_l1_common as L1
import ledger_select_common as SC
import ledger_sig_common as S
from circuits_amd import HzError
from circuits_amd import builder as B
from circuits_amd import capi

pytestmark = pytest.mark.gpu
N_LEVELS = 16
N_SIB = N_LEVELS + 1
PLAN, IDXS = [1], [0]
EDIT = {4: {"balance": 100}, 5: {"balance": SC.LIMIT - 10}, 6: {"nonce": SC.NONCE_MAX}, 7: {"tokenID": 2, "balance": 100}, 8: {"tokenID": 2}}


@pytest.fixture(scope="module")
def base():
    return C.base_state(4)


@pytest.fixture(scope="module")
def acc(base):
    """the base with a poor account (4), one about to overflow (5), one whose nonce is 2^40 - 1 (6), two on another token (7 poor, 8)"""
    return SC.accounts(base, EDIT)


def _ledger(hz, acc, room=4):
    return acc.to_ledger(hz, acc.n + room, n_sib_max=N_SIB)


def _sign(base, pool):
    return [S.sign(base, dict(t)) for t in pool]


def _apply(lg, l1_txs, rows, verify=True, cur=1):
    return lg.apply_batch_atomic(l1_txs, rows, PLAN, IDXS, S.CHAIN_ID, cur, n_sib=N_SIB, verify=verify)


def _check(lg, acc, l1_txs, pool, verify=True, cur=1, max_keep=None):
    """select_batch equals the model; nothing resident moved; -> the selection"""
    root = lg.root()
    exp = SC.model(acc, l1_txs, pool, current_num_batch=cur, max_keep=max_keep, verify=verify, capacity=acc.n + 4)
    got = lg.select_batch(l1_txs, pool, S.CHAIN_ID, cur, max_keep=max_keep, verify=verify)
    assert got == exp, (got, exp)
    assert lg.root() == root and lg.size() == acc.n and lg.select_ms() > 0.0
    return got


def _state(lg, acc):
    return lg.root(), lg.size(), lg.accounts(list(range(acc.first_idx, acc.first_idx + acc.n))).tobytes()


# ---- a pool in which nothing is spoilt ---------------------------------------------------------------------------------------------------
def test_a_valid_pool_is_kept_whole_and_applies_as_the_uncompacted_list(hz, base):
    acc = SC.accounts(base)
    l1_txs = Q.deposits(base, 2)
    pool = _sign(base, SC.valid_pool(acc, 24, 11))
    lg, ref = base.to_ledger(hz), base.to_ledger(hz)
    got = _check(lg, acc, l1_txs, pool)
    assert got["verdict"] == [0] * 24 and got["kept"] == list(range(24)) and got["rounds"] == 1 and got["rq_offset"] == [0] * 24
    a, b = _apply(lg, l1_txs, capi.select_compact(pool, got)), _apply(ref, l1_txs, pool)
    assert set(a) == set(b) and all(a[name].tobytes() == b[name].tobytes() for name in a)
    assert lg.root() == ref.root()
    lg.close()
    ref.close()


# ---- one spoilt transaction per reason ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reason", [1, 2, 3, 4, 5, 7, 8, 9, 12, 13])
def test_one_spoilt_transaction_per_reason(hz, base, acc, reason):
    """transaction 0 is rejected for `reason`; 1 has the nonce that follows the last KEPT transaction of its sender, so it is kept only
    because 0 was dropped; 2 spends what 0 would have brought its poor receiver, so it is dropped (3) only because of it"""
    f0 = base.first_idx
    x, y, z = f0, f0 + 4, f0 + 1
    if reason == 4:
        y, z = f0 + 7, f0 + 8            # on token 2
    if reason == 5:
        y = f0 + 5
    if reason == 12:
        x = f0 + 6
    n0 = acc.state(x)["nonce"]
    t0 = C.tx(x, y, 10 ** 6, 0, nonce=n0)
    t0.update({1: {"tokenID": 2}, 2: {"nonce": n0 + 5}, 3: {"amountF": B.fix2float(((1 << 35) - 1) * 10 ** 25)}, 8: {"maxNumBatch": 3},
               9: {"toIdx": 0, "toEthAddr": 0xDEAD << 100}, 13: {"rqToEthAddr": 5}}.get(reason, {}))
    t1 = C.tx(x, z if reason != 4 else f0 + 1, 10, 0, nonce=n0)
    t2 = C.tx(y, z, 5 * 10 ** 5, 0, token=acc.state(y)["tokenID"], nonce=acc.state(y)["nonce"])
    pool = _sign(base, [t0, t1, t2, C.tx(f0 + 2, f0 + 3, 7, 1, nonce=0)])
    if reason == 7:
        pool[0] = S.forge(pool[0], "s")
    lg = _ledger(hz, acc)
    got = _check(lg, acc, [], pool, cur=5)
    assert got["verdict"][0] == reason and got["verdict"][3] == 0
    if reason != 12:   # (nothing of a sender whose nonce is 2^40 - 1 is ever kept)
        assert got["verdict"][1] == 0
    if reason != 5:    # (the account about to overflow is not poor)
        assert got["verdict"][2] == 3
    _apply(lg, [], capi.select_compact(pool, got), cur=5)   # what is kept applies as it stands, signatures verified
    lg.close()


# ---- the retry loop over the real apply --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [7, 9])
def test_the_retry_loop_over_apply_batch_atomic_gives_the_same(hz, base, acc, seed):
    l1_txs = [L1.own(acc, base.first_idx + 1, 0, 0, 10 ** 6)]
    pool = _sign(base, SC.spoilt_pool(acc, 24, seed, share=6, senders=[0, 1, 2, 3, 9, 10, 11, 12, 13, 14, 15]))   # (the edited accounts only receive)
    pool[3] = S.forge(pool[3], "s")
    lg, other = _ledger(hz, acc), _ledger(hz, acc)
    got = _check(lg, acc, l1_txs, pool)
    assert 0 < 24 - len(got["kept"]) <= 10 and 7 in got["verdict"]

    def apply(l1, rows):
        try:
            _apply(other, l1, rows)
        except HzError as e:
            assert e.status == 4, str(e)
            at = re.search(r"refused at index (\d+) .*reason (\d+):", str(e))
            return int(at.group(1)) - len(l1), int(at.group(2))
        return None
    kept, reasons, refusals = SC.retry_reference(apply, l1_txs, pool)
    assert kept == got["kept"] and reasons == got["verdict"] and refusals == 24 - len(kept)
    _apply(lg, l1_txs, capi.select_compact(pool, got))
    assert lg.root() == other.root()   # the loop's last call applied the same rows
    lg.close()
    other.close()


# ---- L1 rows -----------------------------------------------------------------------------------------------------------------------------
def test_l1_rows_run_first_and_are_nullified_not_dropped(hz, base, acc):
    f0 = base.first_idx
    new = f0 + acc.n
    key = CR.account(40)
    l1_txs = [L1.own(acc, f0 + 4, 0, 0, 10 ** 6),                        # a deposit that funds pool transaction 0
              L1.own(acc, f0 + 7, f0 + 8, 10 ** 6, 0),                   # a transfer nullified by underflow: 8 gets nothing, 7 keeps its 100
              CR.create_for(key, load=10 ** 9),                          # account `new`
              X.fx(acc, f0 + 2, 1000)]                                   # a forceExit
    pool = _sign(base, [C.tx(f0 + 4, f0 + 1, 10 ** 5, 0, nonce=0),                                         # kept: funded by the deposit
                        C.tx(f0 + 7, f0 + 8, 500, 0, token=2, nonce=0),                                    # 3: the 10^6 never left 7... it holds 100
                        C.tx(f0 + 1, new, 77, 0, nonce=0),                                                 # the new account receives by index
                        dict(C.tx(f0 + 3, 0, 55, 0, nonce=0), toEthAddr=key.eth_addr),                     # and by address
                        X.x2(f0 + 9, 1234, 1, nonce=0)])                                                   # an L2 exit
    sent = dict(C.tx(new, f0 + 1, 10 ** 8, 100, nonce=0), signer=key)                                      # the new account sends, signed by its key
    pool.append(CR.sign_all([sent])[0])
    pool.append(_sign(base, [dict(C.tx(f0 + 10, 0, 9, 0, nonce=0), toEthAddr=CR.account(41).eth_addr)])[0])   # nobody holds it: 9
    lg = _ledger(hz, acc)
    got = _check(lg, acc, l1_txs, pool)
    assert got["verdict"] == [0, 3, 0, 0, 0, 0, 9] and got["aux_to_idx"] == [0, 0, 0, new, 0, 0, 0]
    out = _apply(lg, l1_txs, capi.select_compact(pool, got))
    assert lg.size() == acc.n + 1 and out["l1_flags"].tolist() == [0, 2, 0, 0]
    lg.close()


# ---- links -------------------------------------------------------------------------------------------------------------------------------
def _transfers(base, n):
    f0 = base.first_idx
    return [C.tx(f0 + i, f0 + i + 1 if i != 3 else f0 + 9, 1 + i, 0, nonce=0) for i in range(n)]   # (account 4 is poor: nobody needs it)


def test_links(hz, base, acc):
    lg = _ledger(hz, acc)
    # a pair is kept, each half naming the other
    pool = _transfers(base, 4)
    SC.link(pool, 1, 2)
    SC.link(pool, 2, 1)
    got = _check(lg, acc, [], _sign(base, pool))
    assert got["verdict"] == [0] * 4 and got["rq_offset"] == [0, 1, 7, 0] and got["rounds"] == 1
    # the required half spoilt: 14 for the requirer; the reverse direction is unaffected
    pool = _transfers(base, 4)
    pool[2] = SC.spoil(acc, pool[2], "ahead")
    SC.link(pool, 1, 2)
    got = _check(lg, acc, [], _sign(base, pool))
    assert got["verdict"] == [0, SC.PARTNER, 2, 0] and got["rounds"] == 2
    pool = _transfers(base, 4)
    SC.link(pool, 1, 2)
    pool[1] = SC.spoil(acc, pool[1], "ahead")
    got = _check(lg, acc, [], _sign(base, pool))
    assert got["verdict"] == [0, 2, 0, 0] and got["rounds"] == 1
    # pushed out of reach by the kept rows between the halves; brought into reach by a drop
    pool = _transfers(base, 3) + [C.tx(base.first_idx + 10 + i, base.first_idx + 11 + i, 1, 0, nonce=0) for i in range(4)]
    SC.link(pool, 0, 4)
    got = _check(lg, acc, [], _sign(base, pool))
    assert got["verdict"] == [SC.PARTNER] + [0] * 6 and got["rounds"] == 2
    pool[2] = SC.spoil(acc, pool[2], "overdraft")
    got = _check(lg, acc, [], _sign(base, pool))
    assert got["verdict"] == [0, 0, 3, 0, 0, 0, 0] and got["rq_offset"][0] == 3 and got["rounds"] == 1
    _apply(lg, [], capi.select_compact(_sign(base, pool), got))   # the offsets of the compacted batch are the circuit's
    lg.close()
    # a chain needs two extra walks
    lg = _ledger(hz, acc)
    pool = _transfers(base, 4)
    pool[2] = SC.spoil(acc, pool[2], "stale")
    SC.link(pool, 0, 1)
    SC.link(pool, 1, 2)
    got = _check(lg, acc, [], _sign(base, pool))
    assert got["verdict"] == [SC.PARTNER, SC.PARTNER, 2, 0] and got["rounds"] == 3
    # a link field off by one is 13, and the signature over other rq fields than the submitted ones 7
    pool = _transfers(base, 4)
    SC.link(pool, 0, 1)
    pool = _sign(base, pool)
    assert _check(lg, acc, [], pool[:1] + [S.sign(base, dict(pool[1], amountF=pool[1]["amountF"] + 1))] + pool[2:])["verdict"] == [13, 0, 0, 0]
    assert _check(lg, acc, [], [Q.off_by_one(pool[0], Q.RQ_FIELDS[0])] + pool[1:])["verdict"] == [7, 0, 0, 0]
    assert _check(lg, acc, [], [Q.off_by_one(pool[0], Q.RQ_FIELDS[0])] + pool[1:], verify=False)["verdict"] == [13, 0, 0, 0]
    lg.close()


def test_max_keep(hz, base, acc):
    lg = _ledger(hz, acc)
    pool = _sign(base, _transfers(base, 4) + [{}] + [C.tx(base.first_idx + 10, base.first_idx + 11, 1, 0, nonce=0)])
    got = _check(lg, acc, [], pool, max_keep=3)
    assert got["verdict"] == [0, 0, 0, SC.FULL, 0, SC.FULL] and got["kept"] == [0, 1, 2]
    assert _check(lg, acc, [], pool, max_keep=0)["kept"] == []
    # a forced-out pair frees room the next walk fills
    pool = _transfers(base, 5)
    pool[4] = C.tx(base.first_idx + 10, base.first_idx + 11, 1, 0, nonce=0)
    pool[1] = SC.spoil(acc, pool[1], "ahead")
    SC.link(pool, 0, 1)
    got = _check(lg, acc, [], _sign(base, pool), max_keep=2)
    assert got["verdict"] == [SC.PARTNER, 2, 0, 0, SC.FULL] and got["kept"] == [2, 3] and got["rounds"] == 2
    lg.close()


# ---- the circuit -------------------------------------------------------------------------------------------------------------------------
def test_the_circuit_accepts_the_selected_batch(hz, base):
    """rollup-main at (8, 16, 4, 4): two L1 deposits and a pool of nine -- a stale nonce, an overdraft, a linked pair that the drops bring
    two rows apart, one more than the batch has room for -- through ledger_select_batch_inputs: the HIP context and the oracle accept what the ledger hands them"""
    from oracle_binding import OracleCtx
    shape = (8, N_LEVELS, 4, 4)
    f0 = base.first_idx
    acc = SC.accounts(base)
    l1_txs = Q.deposits(base, 2)
    pool = [C.tx(f0 + i, f0 + i + 1, 10 + i, 50, nonce=0) for i in range(9)]
    pool[1] = SC.spoil(acc, pool[1], "stale")
    pool[2] = SC.spoil(acc, pool[2], "overdraft")
    SC.link(pool, 0, 4)
    SC.link(pool, 4, 0)
    pool[5].update(toEthAddr=0xABCDEF << 100, toBjjAy=Q.P - 2, toBjjSign=1, maxNumBatch=9)
    pool = _sign(base, pool)
    lg = base.to_ledger(hz)
    like = types.SimpleNamespace(last_idx=f0 + base.N - 1, num_batch=0)
    (inp, _, nullified, exit_root, new_last), sel = B.ledger_select_batch_inputs(lg, like, l1_txs, pool, *shape, [1], [f0 + 12], S.CHAIN_ID, verify=True)
    assert sel == SC.model(acc, l1_txs, pool, verify=True, max_keep=6)
    assert sel["verdict"] == [0, 2, 3, 0, 0, 0, 0, 0, SC.FULL] and sel["rq_offset"][0] == 2 and sel["rq_offset"][4] == 6
    assert inp["rqOffset"] == [0, 0, 2, 0, 6, 0, 0, 0]
    g = hz.ctx("rollup-main", nTx=shape[0], nLevels=shape[1], maxL1Tx=shape[2], maxFeeTx=shape[3])
    g.set_inputs(inp)
    g.run()
    assert g.get("main.hashGlobalInputs") == B.hash_global_inputs(inp, nullified, new_last, lg.root(), exit_root, *shape)
    o = OracleCtx("rollup-main", *shape)
    o.set_inputs(inp)
    assert o.run() is None
    assert g.read_raw_bytes() == o.read_raw_bytes()
    lg.close()


# ---- residency ---------------------------------------------------------------------------------------------------------------------------
def test_select_changes_nothing_resident(hz, base, acc):
    f0 = base.first_idx
    lg = _ledger(hz, acc)
    _apply(lg, [], _sign(base, [X.x2(f0 + 9, 1234, 1, nonce=0)]))   # the exit tree of the last batch holds a leaf
    now = SC.accounts(base, {**EDIT, 9: {"nonce": 1, "balance": acc.state(f0 + 9)["balance"] - 1234 - B.compute_fee(1234, 1)}})
    before, exit_root, exit_leaf = _state(lg, acc), lg.exit_tree().root(), lg.exit_accounts([f0 + 9]).tobytes()
    pool = _sign(base, SC.spoilt_pool(now, 20, 5) + [X.x2(f0 + 9, 99, 0, nonce=1)])
    l1_txs = [CR.create_for(CR.account(50), load=10 ** 9), X.fx(acc, f0 + 2, 1000)]
    got = _check(lg, now, l1_txs, pool)
    assert got["verdict"][-1] == 0 and 0 < len(got["kept"]) < 21
    assert _state(lg, acc) == before and lg.exit_tree().root() == exit_root and lg.exit_accounts([f0 + 9]).tobytes() == exit_leaf
    with pytest.raises(HzError) as e:   # an L1 load that takes a balance past 2^192 refuses the call, as apply does
        lg.select_batch([L1.own(now, f0 + 1, 0, 0, 5), L1.own(now, f0 + 5, 0, 0, 1000)], pool, S.CHAIN_ID, 1, verify=True)
    assert e.value.status == 4 and "refused at index 1 (L1 transaction 1), reason 5:" in str(e.value), str(e.value)
    assert _state(lg, acc) == before and lg.exit_tree().root() == exit_root and lg.exit_accounts([f0 + 9]).tobytes() == exit_leaf
    with pytest.raises(HzError) as e:   # the *_dev outputs of earlier calls are no longer handed out
        lg.outputs_dev()
    assert e.value.status == 1
    lg.close()


# ---- the staging tile's edges ------------------------------------------------------------------------------------------------------------
def test_drops_at_the_edges_of_the_staging_tile(hz, base):
    """a pool of 130, amounts only: drops at 63, 64 and 127, and a dependent pair across 63 | 64 -- 64 has the nonce that follows 63's, so
    it is dropped (2) only because 63 was (3); 65 repeats 63's nonce and is kept only because of it"""
    f0 = base.first_idx
    acc = SC.accounts(base)
    a, b = f0 + 14, f0 + 15
    v = SC.valid_pool(acc, 125, 21, senders=list(range(14)))   # a and b send nothing here
    pool = (v[:63] + [SC.spoil(acc, C.tx(a, f0 + 1, 5, 0, nonce=0), "overdraft"), C.tx(a, f0 + 1, 5, 0, nonce=1), C.tx(a, f0 + 1, 5, 0, nonce=0)] + v[63:124] +
            [C.tx(b, f0 + 2, 5, 0, nonce=1), C.tx(b, f0 + 2, 5, 0, nonce=0)] + v[124:])
    assert len(pool) == 130 and pool[64]["nonce"] == 1 and pool[127]["fromIdx"] == b
    lg = base.to_ledger(hz)
    got = _check(lg, acc, [], pool, verify=False)
    assert [got["verdict"][i] for i in (63, 64, 65, 127, 128)] == [3, 2, 0, 2, 0] and len(got["kept"]) == 127
    _apply(lg, [], capi.select_compact(pool, got), verify=False)
    lg.close()


# ---- the slot capacity -------------------------------------------------------------------------------------------------------------------
def test_a_pool_that_fills_every_slot(hz):
    """HZ_SELECT_MAX_SLOTS distinct accounts exactly, on a dense ledger of 2^12: transfers 2 i -> 2 i + 1, amounts only, no signatures,
    kept whole. The first launch with the kernel's whole LDS: the runtime accepts it"""
    S_ = capi.SELECT_MAX_SLOTS
    big = C.base_state(12)
    assert big.N == S_
    f0 = big.first_idx
    pool = [C.tx(f0 + 2 * i, f0 + 2 * i + 1, 3 + i % 7, 0, nonce=0) for i in range(S_ // 2)]
    assert len(hz.ledger_plan_select([], pool)["slot_account"]) == S_
    lg = big.to_ledger(hz)
    root = lg.root()
    got = lg.select_batch([], pool, S.CHAIN_ID, 1, sigs=False)
    assert got["verdict"] == [0] * (S_ // 2) and got["kept"] == list(range(S_ // 2)) and got["rounds"] == 1 and lg.root() == root
    lg.close()
