"""The device-resident account tree (hz_state, csrc/state.hip) against an independent checker: the Python builder.SMT over a DenseState,
one update at a time with host hashing; circomlib's SMTProcessor / SMTVerifier as mains (the HIP contexts, and the oracle for the
processor) accept what the device returns. Every comparison is on bytes, bit-exact."""
import numpy as np
import pytest

import device_state_common as C
from circuits_amd import HzError
from circuits_amd import builder as B

pytestmark = pytest.mark.gpu
K = 13
N_LEVELS = 16   # the circuits' nLevels: SMTProcessor / SMTVerifier (nLevels + 1) take 17 siblings


def _device_state(hz, base):
    return base.to_device(hz)


def _same_arrays(state, levels, value):
    got_levels, got_value = state.download()
    assert len(got_levels) == len(levels)
    for d, (g, e) in enumerate(zip(got_levels, levels)):
        assert g.shape == e.shape and (g == e).all(), "level %d differs" % d
    assert (got_value == value).all()


def _check_apply(state, base, idx, fields, n_sib=N_LEVELS + 1, smt=None):
    got = state.apply(idx, C.fields_array(fields), n_sib=n_sib)
    t, res, vals = C.smt_apply(base, idx, fields, smt)
    exp = C.expect_arrays(res, n_sib)
    for name in ("old_value", "old_root", "new_root", "siblings"):
        bad = np.flatnonzero((got[name] != exp[name]).reshape(len(idx), -1).any(axis=1))
        assert bad.size == 0, "%s differs at updates %s" % (name, bad[:8].tolist())
    assert state.root() == t.root
    return t, res, vals, got


@pytest.mark.parametrize("k", [8, 13])
def test_load_builds_the_dense_state(hz, k):
    base = C.base_state(k)
    st = _device_state(hz, base)
    _same_arrays(st, base.levels, base.value)
    assert st.root() == base.root
    st.close()


@pytest.mark.parametrize("m", [1, 2, 64, 4096])
def test_apply_matches_the_smt(hz, m):
    base = C.base_state(K)
    st = _device_state(hz, base)
    idx, fields = C.draw_updates(base, m, seed=100 + m, pool=None if m > 64 else 24)
    assert m < 64 or len(set(idx)) < m   # the draw repeats accounts
    _check_apply(st, base, idx, fields)
    # the arrays hold the consolidated tree, and nothing outside the touched paths moved
    levels, value = C.rebuild_levels(K, base.first_idx, C.final_cols(base, idx, fields))
    _same_arrays(st, levels, value)
    st.close()


@pytest.mark.parametrize("name", ["same_account_5", "deepest_siblings_alternating", "bit0_pair", "restore_original"])
def test_apply_edge_orders(hz, name):
    base = C.base_state(K)
    st = _device_state(hz, base)
    idx, fields = C.edge_cases(base)[name]
    _, _, _, got = _check_apply(st, base, idx, fields, n_sib=K)
    if name == "restore_original":
        assert st.root() == base.root and C.to_int(got["new_root"][0]) != base.root
        _same_arrays(st, base.levels, base.value)
    st.close()


def test_apply_outputs_are_smt_processor_witnesses(hz):
    """the 64 updates as 64 instances of SMTProcessor(nLevels + 1) on the device: no failure, main.newRoot = new_root[j] for every one"""
    base = C.base_state(K)
    st = _device_state(hz, base)
    idx, fields = C.draw_updates(base, 64, seed=164, pool=24)
    got = st.apply(idx, C.fields_array(fields), n_sib=N_LEVELS + 1)
    vals = [B.host().poseidon(f) for f in fields]
    g = hz.ctx("smt-processor", nLevels=N_LEVELS + 1, n_instances=64)
    for j in range(64):
        g.set_inputs({"oldRoot": C.to_int(got["old_root"][j]), "siblings": [C.to_int(s) for s in got["siblings"][j]], "oldKey": idx[j],
                      "oldValue": C.to_int(got["old_value"][j]), "isOld0": 0, "newKey": idx[j], "newValue": vals[j], "fnc": [0, 1]}, instance=j)
    g.run()
    assert g.failures() == []
    for j in range(64):
        assert g.get("main.newRoot", j) == C.to_int(got["new_root"][j]), "instance %d" % j
    assert C.to_int(got["new_root"][63]) == st.root()
    st.close()


def test_proofs_after_apply(hz):
    base = C.base_state(K)
    st = _device_state(hz, base)
    idx, fields = C.draw_updates(base, 512, seed=7)
    t, _, _, _ = _check_apply(st, base, idx, fields)
    rng = np.random.default_rng(11)
    ask = [base.first_idx + int(x) for x in rng.integers(0, base.N, size=256)] + [base.first_idx, base.first_idx + base.N - 1] + idx[:8]
    sib, val = st.proofs(ask, n_sib=N_LEVELS + 1)
    root = st.root()
    g = hz.ctx("smt-verifier", nLevels=N_LEVELS + 1, n_instances=len(ask))
    for j, key in enumerate(ask):
        f = t.find(key)
        assert f["found"] and f["foundValue"] == C.to_int(val[j])
        assert [C.to_int(s) for s in sib[j]] == list(f["siblings"]) + [0] * (N_LEVELS + 1 - len(f["siblings"]))
        g.set_inputs({"enabled": 1, "root": root, "siblings": [C.to_int(s) for s in sib[j]], "oldKey": 0, "oldValue": 0, "isOld0": 0, "key": key,
                      "value": C.to_int(val[j]), "fnc": 0}, instance=j)
    g.run()
    assert g.failures() == []
    st.close()


def test_two_calls_consolidate_like_one(hz):
    base = C.base_state(K)
    idx, fields = C.draw_updates(base, 600, seed=21, pool=200)
    two, one = _device_state(hz, base), _device_state(hz, base)
    t, _, _, _ = _check_apply(two, base, idx[:300], fields[:300])
    _check_apply(two, base, idx[300:], fields[300:], smt=t)   # the second call sees the first one's tree
    one.apply(idx, C.fields_array(fields))
    assert one.root() == two.root() == t.root
    levels, value = C.rebuild_levels(K, base.first_idx, C.final_cols(base, idx, fields))
    _same_arrays(one, levels, value)
    _same_arrays(two, levels, value)
    one.close()
    two.close()


def test_errors_leave_the_tree_untouched(hz):
    base = C.base_state(8)
    st = _device_state(hz, base)
    root = st.root()
    ok_idx, ok_fields = C.draw_updates(base, 3, seed=5)
    for bad in (base.first_idx - 1, base.first_idx + base.N, base.first_idx + base.N + 12345):
        with pytest.raises(HzError) as e:
            st.apply([ok_idx[0], bad, ok_idx[2]], C.fields_array(ok_fields))
        assert e.value.status == 1 and str(bad) in str(e.value)
        assert st.root() == root
        with pytest.raises(HzError) as e:
            st.proofs([bad])
        assert e.value.status == 1
    out = st.apply([], C.fields_array([]))   # no update: fine, and nothing changes
    assert out["new_root"].shape == (0, 32) and st.root() == root
    with pytest.raises(HzError) as e:
        st.apply(ok_idx, C.fields_array(ok_fields), n_sib=7)
    assert e.value.status == 1 and "n_sib" in str(e.value)
    with pytest.raises(HzError) as e:
        st.proofs(ok_idx, n_sib=7)
    assert e.value.status == 1
    assert st.root() == root
    _same_arrays(st, base.levels, base.value)
    for k in (3, 25, -1):
        with pytest.raises(HzError) as e:
            hz.state(k)
        assert e.value.status == 1 and "k =" in str(e.value)
    fresh = hz.state(8)
    with pytest.raises(HzError) as e:   # nothing loaded yet
        fresh.root()
    assert e.value.status == 1
    fresh.close()
    st.close()


def test_download_feeds_the_native_builder(hz):
    from circuits_amd.native_builder import NativeRollupDB
    base = C.base_state(K)
    st = _device_state(hz, base)
    idx, fields = C.draw_updates(base, 256, seed=33)
    st.apply(idx, C.fields_array(fields))
    assert st.root() != base.root
    db = NativeRollupDB(base=B.DenseState.from_device(st, like=base))
    assert db.state_root == st.root()
    db.close()
    st.close()


def test_one_handle_regrows_its_call_buffers(hz):
    """3, 200 and 3 updates on one state of k = 6, with n_sib = k, k + 3, k: the per-call buffers are grown by the second call and reused
    by the third; every output of every call, the zero padding beyond depth k included, and the final tree are the checker's"""
    k = 6
    base = C.base_state(k)
    st = _device_state(hz, base)
    t, all_idx, all_fields = None, [], []
    for call, (m, n_sib) in enumerate([(3, k), (200, k + 3), (3, k)]):
        idx, fields = C.draw_updates(base, m, seed=300 + call)
        t, _, _, got = _check_apply(st, base, idx, fields, n_sib=n_sib, smt=t)
        assert got["siblings"].shape == (m, n_sib, 32)
        all_idx += idx
        all_fields += fields
    assert st.root() == t.root
    levels, value = C.rebuild_levels(k, base.first_idx, C.final_cols(base, all_idx, all_fields))
    _same_arrays(st, levels, value)
    st.close()
