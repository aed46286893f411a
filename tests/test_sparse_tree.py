"""The sparse device-resident Merkle tree (hz_smt, csrc/smt_tree.hip) against an independent checker: the Python builder.SMT (no base, host
hashing) one op at a time; circomlib's SMTProcessor / SMTVerifier and the Withdraw main (the HIP contexts) accept what the device
returns. Every comparison is on bytes, bit-exact."""
import numpy as np
import pytest

import sparse_tree_common as C
from circuits_amd import HzError
from circuits_amd import builder as B

pytestmark = pytest.mark.gpu
N_SIB = C.N_SIB
NAMES = ("siblings", "old_key", "old_value", "is_old0", "fnc", "old_root", "new_root")


def _same(got, exp, m):
    for name in NAMES:
        assert got[name].shape == exp[name].shape, name
        bad = np.flatnonzero((got[name] != exp[name]).reshape(m, -1).any(axis=1))
        assert bad.size == 0, "%s differs at ops %s" % (name, bad[:8].tolist())


def _apply_and_check(tree, keys, fields, res, n_sib=N_SIB):
    got = tree.apply(keys, C.fields_array(fields), n_sib=n_sib)
    _same(got, C.expect_arrays(res, n_sib), len(keys))
    return got


@pytest.mark.parametrize("name", sorted(C.small_cases()))
def test_smallest_shapes(hz, name):
    keys, fields, t, res = C.replay_case(name)
    tree = hz.smt(N_SIB)
    assert tree.root() == 0 and tree.size() == 0
    got = _apply_and_check(tree, keys, fields, res)
    assert tree.root() == t.root and tree.size() == len(set(keys))
    if name == "one_insert":   # root = leaf hash, no sibling, isOld0 = 1
        assert C.to_int(got["new_root"][0]) == B.host().poseidon([keys[0], res[0]["value"], 1])
        assert not got["siblings"].any() and got["is_old0"][0] == 1 and got["fnc"][0] == 1 and not got["old_root"].any()
    if name == "share_10_bits":   # ten zero siblings; oldKey / oldValue of the met leaf
        assert not got["siblings"][1].any() and got["old_key"][1] == keys[0] and C.to_int(got["old_value"][1]) == res[0]["value"]
        assert got["is_old0"][1] == 0
    if name == "push_down_then_update_old":
        assert got["fnc"].tolist() == [1, 1, 0] and C.to_int(got["old_value"][2]) == res[0]["value"]
        assert C.to_int(got["siblings"][2][12]) == B.host().poseidon([keys[1], res[1]["value"], 1])
    tree.close()


def test_three_keys_in_both_orders_make_one_tree(hz):
    _, _, fwd, _ = C.replay_case("three_share_5_bits_fwd")
    keys, fields, _, _ = C.replay_case("three_share_5_bits_rev")
    tree = hz.smt(N_SIB)
    fkeys, ffields, _, _ = C.replay_case("three_share_5_bits_fwd")
    tree.apply(keys, C.fields_array([ffields[fkeys.index(k)] for k in keys]), n_sib=N_SIB)   # the forward case's values, reversed order
    assert tree.root() == fwd.root
    tree.close()


@pytest.mark.parametrize("m", [64, 4096])
def test_random_mix_matches_the_smt(hz, m):
    keys, fields, t, res = C.replay_mix(m, 100 + m)
    assert {r["fnc"] for r in res} == {0, 1}
    assert any(r["fnc"] == 1 and not r["isOld0"] and r["depth"] - r["find_depth"] >= 2 for r in res)   # a push-down of depth >= 2
    tree = hz.smt(N_SIB)
    _apply_and_check(tree, keys, fields, res)
    assert tree.root() == t.root and tree.size() == len(set(keys))
    tree.close()


def test_two_calls_equal_one_and_reset_empties(hz):
    keys, fields, t, res = C.replay_mix(600, 21)
    exp = C.expect_arrays(res, N_SIB)
    one, two = hz.smt(N_SIB), hz.smt(N_SIB)
    whole = one.apply(keys, C.fields_array(fields), n_sib=N_SIB)
    a = two.apply(keys[:250], C.fields_array(fields[:250]), n_sib=N_SIB)
    b = two.apply(keys[250:], C.fields_array(fields[250:]), n_sib=N_SIB)   # the second call sees the first one's tree
    _same(whole, exp, 600)
    _same({n: np.concatenate([a[n], b[n]]) for n in NAMES}, exp, 600)
    assert one.root() == two.root() == t.root and one.size() == two.size() == len(set(keys))
    two.reset()
    assert two.root() == 0 and two.size() == 0
    k2, f2, t2, r2 = C.replay_case("consecutive_64_from_256")   # reusable: the exit tree of the next batch
    _apply_and_check(two, k2, f2, r2)
    assert two.root() == t2.root and two.size() == 64
    one.close()
    two.close()


def test_outputs_are_smt_processor_witnesses(hz):
    """64 mixed ops as 64 instances of the smt-processor main (nLevels = 17): no failure, main.newRoot = new_root[j] for every one"""
    keys, fields, t, res = C.replay_mix(64, 164)
    assert {r["fnc"] for r in res} == {0, 1}
    tree = hz.smt(N_SIB)
    got = tree.apply(keys, C.fields_array(fields), n_sib=N_SIB)
    g = hz.ctx("smt-processor", nLevels=N_SIB, n_instances=64)
    for j in range(64):
        g.set_inputs(C.processor_inputs(keys, got, j, [r["value"] for r in res]), instance=j)
    g.run()
    assert g.failures() == []
    for j in range(64):
        assert g.get("main.newRoot", j) == C.to_int(got["new_root"][j]), "instance %d" % j
    assert C.to_int(got["new_root"][63]) == tree.root() == t.root
    tree.close()


def test_proofs_after_apply(hz):
    keys, fields, t, res = C.replay_mix(512, 7)
    tree = hz.smt(N_SIB)
    _apply_and_check(tree, keys, fields, res)
    held = sorted(set(keys))
    rng = np.random.default_rng(11)
    absent = [int(k) for k in rng.integers(0, 1 << 48, size=160) if int(k) not in set(held)]
    ask = held[:96] + absent
    finds = [t.find(k) for k in ask]
    assert sum(1 for f in finds if not f["found"] and f["isOld0"]) >= 8      # absent, the walk ends at an empty slot
    assert sum(1 for f in finds if not f["found"] and not f["isOld0"]) >= 8  # absent, the walk ends at another leaf
    p = tree.proofs(ask, n_sib=N_SIB)
    root = tree.root()
    assert root == t.root
    g = hz.ctx("smt-verifier", nLevels=N_SIB, n_instances=len(ask))
    for j, (key, f) in enumerate(zip(ask, finds)):
        sib = [C.to_int(s) for s in p["siblings"][j]]
        assert sib == list(f["siblings"]) + [0] * (N_SIB - len(f["siblings"])), "key %d" % key
        assert bool(p["found"][j]) == f["found"]
        if f["found"]:
            assert C.to_int(p["value"][j]) == f["foundValue"] and not p["not_found_value"][j].any()
            inp = {"oldKey": 0, "oldValue": 0, "isOld0": 0, "value": f["foundValue"], "fnc": 0}
        else:
            assert int(p["not_found_key"][j]) == f["notFoundKey"] and C.to_int(p["not_found_value"][j]) == f["notFoundValue"]
            assert bool(p["is_old0"][j]) == f["isOld0"] and not p["value"][j].any()
            inp = {"oldKey": int(p["not_found_key"][j]), "oldValue": C.to_int(p["not_found_value"][j]), "isOld0": int(p["is_old0"][j]), "value": 0, "fnc": 1}
        inp.update({"enabled": 1, "root": root, "siblings": sib, "key": key})
        g.set_inputs(inp, instance=j)
    g.run()
    assert g.failures() == []
    tree.close()


def test_exit_tree_end_to_end(hz):
    """the exits of a synthetic batch replayed through the device tree: every intermediate exit root and the batch's new_exit_root; the
    withdraw main accepts inputs built from the device's proofs"""
    bb = B.synthetic_batch(8, 16, 3, 4, n_accounts=6, exits=2)
    assert bb.exit_leaves
    ops, after, running = [], [], {}
    for i, tx in enumerate(bb.txs):   # an L2 exit moves `amount` into the sender's exit leaf: an insert the first time, an update after
        if tx.get("toIdx") == B.EXIT_IDX and tx.get("amount"):
            k = tx["fromIdx"]
            st = dict(bb.exit_leaves[k])
            st["balance"] = running.get(k, 0) + tx["amount"]
            running[k] = st["balance"]
            ops.append((k, st))
            after.append(bb.tx_meta[i]["exitRoot"])
    assert len(ops) == 2 and all(running[k] == bb.exit_leaves[k]["balance"] for k in running) and set(running) == set(bb.exit_leaves)
    tree = hz.smt(N_SIB)
    got = tree.apply([k for k, _ in ops], C.fields_array([B.leaf_fields(st) for _, st in ops]), n_sib=N_SIB)
    assert [C.to_int(r) for r in got["new_root"]] == after
    assert tree.root() == bb.new_exit_root

    class DeviceBatch:
        exit_tree, exit_leaves = B.DeviceSMT(tree), bb.exit_leaves
    idxs = list(bb.exit_leaves)
    g = hz.ctx("withdraw", nLevels=16, n_instances=len(idxs))
    for j, idx in enumerate(idxs):
        w = B.withdraw_input(DeviceBatch, idx, 16)
        assert w == B.withdraw_input(bb, idx, 16)
        g.set_inputs(w[0], instance=j)
    g.run()
    assert g.failures() == []
    tree.close()


def test_exit_tree_fixture_on_the_device(hz):
    tree = hz.smt(N_SIB)
    host_fx = B.ExitTreeFixture(40, seed=5)
    dev_fx = B.ExitTreeFixture(40, seed=5, sparse_tree=tree)
    assert dev_fx.exit_leaves == host_fx.exit_leaves and dev_fx.exit_tree.root == host_fx.exit_tree.root and tree.size() == 40
    for idx in (256, 270, 295):
        assert B.withdraw_input(dev_fx, idx, 16) == B.withdraw_input(host_fx, idx, 16)
    assert dev_fx.exit_tree.find(999)["found"] is False
    with pytest.raises(ValueError):
        B.ExitTreeFixture(4, sparse_tree=tree, device=0)
    tree.close()


def test_refused_calls_leave_the_tree_untouched(hz):
    keys, fields, t, res = C.replay_case("consecutive_64_from_256")
    tree = hz.smt(N_SIB)
    _apply_and_check(tree, keys, fields, res)
    root, size = tree.root(), tree.size()
    ok = C.fields_array(fields[:3])

    def refused(status, text, *a, **kw):
        with pytest.raises(HzError) as e:
            tree.apply(*a, **kw)
        assert e.value.status == status and text in str(e.value), str(e.value)
        assert tree.root() == root and tree.size() == size

    refused(4, "key[1]", [1000, 1 << 48, 1001], ok, n_sib=N_SIB)
    big = C.fields_array(fields[:3])
    big[2, 1] = C.to_bytes([C.P])[0]
    refused(4, "op 2", [1000, 1001, 1002], big, n_sib=N_SIB)
    # two keys equal in their low 17 bits: op 1 of the call is what SMTProcessor(17) cannot express (HZ_ERR_INPUT, which the header
    # numbers 4); op 0 is rolled back
    a = 0x1ABCD
    refused(4, "op 1", [a, a | 1 << 17, 1003], ok, n_sib=N_SIB)
    for n_sib in (0, 65, N_SIB + 1):
        refused(1, "n_sib", [1000, 1001, 1002], ok, n_sib=n_sib)
        with pytest.raises(HzError) as e:
            tree.proofs([256], n_sib=n_sib)
        assert e.value.status == 1
    with pytest.raises(HzError) as e:
        tree.proofs([1 << 48], n_sib=N_SIB)
    assert e.value.status == 4
    # a refused proofs call writes to none of its outputs, also not for the keys in front of the refused one
    mark = [np.full(3, 7, dtype=np.uint8), np.full(3, 7, dtype=np.uint64), np.full(3, 7, dtype=np.uint8)]
    ask = np.array([256, 1000, 1 << 48], dtype=np.uint64)
    st = hz.c.hz_smt_proofs(tree.h, 3, ask.ctypes.data, N_SIB, None, mark[0].ctypes.data, None, mark[1].ctypes.data, None, mark[2].ctypes.data)
    assert st == 4 and all((a == 7).all() for a in mark)
    out = tree.apply([], C.fields_array([]), n_sib=N_SIB)   # no op: fine, and nothing changes
    assert out["new_root"].shape == (0, 32) and tree.root() == root and tree.size() == size
    # later results are as if the refused calls had not been made
    k2 = [a, 1003, a]
    f2 = C.make_fields(k2, seed=3)
    t2, r2 = C.smt_replay(keys + k2, fields + f2)   # (a replay of its own: the shared one stays as it is)
    _apply_and_check(tree, k2, f2, r2[len(keys):])
    assert tree.root() == t2.root and tree.size() == size + 2
    for bad in (0, 65):
        with pytest.raises(HzError) as e:
            hz.smt(bad)
        assert e.value.status == 1
    tree.close()


def test_one_handle_regrows_its_call_buffers(hz):
    """3, 200 and 3 ops on one tree of n_sib_max = 10, with n_sib = 7, 10, 7: the per-call buffers are grown by the second call and reused
    by the third; every output of every call, the zero padding included, and the final root are the checker's"""
    calls = C.regrow_calls()
    assert [len(keys) for keys, _ in calls] == [3, 200, 3] and [n_sib for _, n_sib in calls] == [7, 10, 7]
    tree = hz.smt(10)
    t, n = None, 0
    for keys, n_sib in calls:
        fields = C.make_fields(keys, seed=50 + n)
        t, res = C.smt_replay(keys, fields, smt=t)
        assert all(r["depth"] < n_sib for r in res) and {r["fnc"] for r in res} == {0, 1}
        got = _apply_and_check(tree, keys, fields, res, n_sib=n_sib)
        assert got["siblings"].shape == (len(keys), n_sib, 32)
        n += len(keys)
    assert tree.root() == t.root and tree.size() == len({k for keys, _ in calls for k in keys})
    tree.close()
