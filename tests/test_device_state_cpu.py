"""The device-resident account tree (hz_state), the part that needs no GPU: the library refuses to run without a device, and a plain
model of the NODE-VERSION scheme of csrc/state.hip -- the sibling-version index, the hash order, the write-back -- agrees with the
Python SMT applying the same updates one at a time. The model pins the algorithm independently of any kernel."""
import pytest

import device_state_common as C
from circuits_amd import builder as B
from oracle_binding import OracleCtx

K = 6


def model_apply(levels, value, k, first_idx, idx, fields, H):
    """hz_state_apply's scheme on lists of ints: update j makes version j of the nodes on its path; a level reads its own child's version
    j and the other child's latest version below j (else the resident array). Returns the outputs; levels / value are updated in place."""
    m, N = len(idx), 1 << k
    res = [i & (N - 1) for i in idx]
    # the integer index: which earlier update made the version a thread reads; which version of a node is the last
    src = [[-1] * m for _ in range(k)]
    last = [[False] * m for _ in range(k + 1)]
    prev_same = [-1] * m
    for dd in range(k + 1):
        latest = {}
        for j in range(m):
            node = res[j] & ((1 << dd) - 1)
            if dd:
                src[dd - 1][j] = latest.get(node ^ (1 << (dd - 1)), -1)
            before = latest.get(node, -1)
            if dd == k:
                prev_same[j] = before
            if before >= 0:
                last[dd][before] = False
            last[dd][j] = True
            latest[node] = j
    uval = [H(f) for f in fields]
    old_value = [uval[prev_same[j]] if prev_same[j] >= 0 else value[idx[j] - first_idx] for j in range(m)]
    ver = [None] * (k + 1)
    ver[k] = [H([idx[j], uval[j], 1]) for j in range(m)]
    sib = [[0] * k for _ in range(m)]
    for d in range(k - 1, -1, -1):
        ver[d] = [0] * m
        for j in range(m):
            q = (res[j] & ((2 << d) - 1)) ^ (1 << d)
            s = ver[d + 1][src[d][j]] if src[d][j] >= 0 else levels[d + 1][q]
            sib[j][d] = s
            own = ver[d + 1][j]
            ver[d][j] = H([s, own]) if (res[j] >> d) & 1 else H([own, s])
    old_root = [levels[0][0]] + ver[0][:-1]
    new_root = list(ver[0])
    for d in range(k + 1):
        for j in range(m):
            if last[d][j]:
                levels[d][res[j] & ((1 << d) - 1)] = ver[d][j]
                if d == k:
                    value[idx[j] - first_idx] = uval[j]
    return {"siblings": sib, "old_value": old_value, "old_root": old_root, "new_root": new_root}


def _lists(base):
    return [[C.to_int(r) for r in lv] for lv in base.levels], [C.to_int(r) for r in base.value]


def _check_against_smt(base, idx, fields):
    H = B.host().poseidon
    levels, value = _lists(base)
    got = model_apply(levels, value, base.k, base.first_idx, idx, fields, H)
    t, res, vals = C.smt_apply(base, idx, fields)
    assert got["siblings"] == [r["siblings"] for r in res]
    assert got["old_value"] == [r["oldValue"] for r in res]
    assert got["old_root"] == [r["oldRoot"] for r in res]
    assert got["new_root"] == [r["newRoot"] for r in res]
    assert levels[0][0] == t.root
    # the write-back: the arrays equal a tree rebuilt from the final leaf fields, and nothing else
    exp_levels, exp_value = C.rebuild_levels(base.k, base.first_idx, C.final_cols(base, idx, fields))
    assert value == [C.to_int(r) for r in exp_value]
    for d in range(base.k + 1):
        assert levels[d] == [C.to_int(r) for r in exp_levels[d]], "level %d" % d
    return t, res, vals


@pytest.mark.parametrize("m", [1, 2, 64, 4096])
def test_version_model_matches_smt_random(m):
    base = C.base_state(K)
    idx, fields = C.draw_updates(base, m, seed=100 + m)
    assert m < 64 or len(set(idx)) < m   # the draw repeats accounts
    _check_against_smt(base, idx, fields)


@pytest.mark.parametrize("name", ["same_account_5", "deepest_siblings_alternating", "bit0_pair", "restore_original"])
def test_version_model_matches_smt_edge_orders(name):
    base = C.base_state(K)
    idx, fields = C.edge_cases(base)[name]
    t, res, _ = _check_against_smt(base, idx, fields)
    if name == "restore_original":
        assert t.root == base.root and res[0]["newRoot"] != base.root


def test_chosen_inputs_are_accepted_by_the_smt_processor():
    """the 64 updates, as the checker states them, are 64 valid instances of circomlib's SMTProcessor (oracle): every instance runs"""
    base = C.base_state(K)
    idx, fields = C.draw_updates(base, 64, seed=164)
    _, res, vals = C.smt_apply(base, idx, fields)
    cases = C.processor_inputs(idx, vals, res, K + 4)
    o = OracleCtx("smt-processor", nLevels=K + 4, n_instances=len(cases))
    for i, inp in enumerate(cases):
        o.set_inputs(inp, instance=i)
    assert o.run() is None
    for i, r in enumerate(res):
        assert o.get("main.newRoot", i) == r["newRoot"], "instance %d" % i


def test_state_needs_a_device():
    from circuits_amd import HzError, lib
    L = lib()
    if L.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(HzError) as e:
        L.state(8)
    assert e.value.status == 5
    with pytest.raises(HzError) as e:
        L.state(3)   # arguments are checked before the device is looked for
    assert e.value.status == 1


def test_dense_state_leaf_fields_are_what_build_hashed():
    """DenseState.leaf_fields (what to_device uploads) reproduces the arrays DenseState.build made"""
    base = C.base_state(K)
    levels, value = C.rebuild_levels(base.k, base.first_idx, base.leaf_fields())
    assert (value == base.value).all()
    for d in range(base.k + 1):
        assert (levels[d] == base.levels[d]).all()


def test_state_kernels_use_no_scratch():
    """the compiler's resource remarks of csrc/state.hip (build/state.ru.txt): the level kernels -- the dependent chain of a call -- and
    every other k_state_* kernel keep their state in registers"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import resource_usage as RU
    path = os.path.join(RU.BUILD, "state.ru.txt")
    if not os.path.exists(path):
        pytest.skip("the library was not built in this tree (no build/state.ru.txt)")
    rows = {r["name"]: r for r in RU.table([path])}
    for name in ("hz::k_state_level_apply", "hz::k_state_level_load", "hz::k_state_value", "hz::k_state_leaf_apply", "hz::k_state_leaf_load",
                 "hz::k_state_writeback", "hz::k_state_proofs"):
        assert name in rows, sorted(rows)
        assert rows[name]["scratch"] == 0, "%s uses %d bytes of scratch per lane" % (name, rows[name]["scratch"])


def test_growing_buffers_stay_empty_after_a_failed_allocation(tmp_path):
    """csrc/hostutil.h as a stand-alone host program (tests/native/devbuf_check.cpp): after a grow that fails, DevBuf and PinnedBuf hold
    p == nullptr and bytes == 0, a second grow of the same size fails again, grow(0) on an empty buffer succeeds. No device is needed:
    2^60 bytes are refused with a plain error return everywhere."""
    import os
    import subprocess
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "devbuf_check.cpp")
    exe = str(tmp_path / "devbuf_check")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O1", "-std=c++17", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "failures=0" in r.stdout, r.stdout + r.stderr
