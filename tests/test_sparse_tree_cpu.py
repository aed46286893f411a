"""The sparse device-resident Merkle tree (hz_smt), the part that needs no GPU: the host planner alone (hz_smt_plan: integers only) agrees
with a plain-Python restatement of the count rule, that restatement agrees with builder.SMT hashing on the host, and the library refuses
to make a tree without a device."""
import numpy as np
import pytest

import sparse_tree_common as C
from circuits_amd import HzError, lib


def _plan_matches_rule(keys, n_sib=C.N_SIB):
    got = lib().smt_plan(keys, n_sib)
    exp = C.count_rule(keys)
    assert got["depth"].tolist() == [e[0] for e in exp]
    assert got["fnc"].tolist() == [e[1] for e in exp]
    assert got["old_key"].tolist() == [e[2] for e in exp]
    assert got["is_old0"].tolist() == [e[3] for e in exp]
    return exp


def _rule_matches_smt(keys, res):
    exp = C.count_rule(keys)
    for j, (e, r) in enumerate(zip(exp, res)):
        assert e == (r["depth"], r["fnc"], r["oldKey"], 1 if r["isOld0"] else 0, r["find_depth"]), "op %d" % j


@pytest.mark.parametrize("name", sorted(C.small_cases()))
def test_plan_small_shapes(name):
    keys, _, _, res = C.replay_case(name)
    _plan_matches_rule(keys)
    _rule_matches_smt(keys, res)


def test_plan_small_shape_facts():
    """the smallest shapes, their facts stated outright"""
    L = lib()
    one = L.smt_plan([300], C.N_SIB)
    assert (one["depth"][0], one["fnc"][0], one["old_key"][0], one["is_old0"][0]) == (0, 1, 300, 1)
    a, b = C.small_cases()["share_10_bits"]
    two = L.smt_plan([a, b], C.N_SIB)
    assert two["depth"].tolist() == [0, 11] and two["old_key"].tolist() == [a, a] and two["is_old0"].tolist() == [1, 0]
    upd = L.smt_plan(C.small_cases()["push_down_then_update_old"], C.N_SIB)
    assert upd["depth"].tolist() == [0, 13, 13] and upd["fnc"].tolist() == [1, 1, 0]
    row = L.smt_plan(list(range(256, 320)), C.N_SIB)
    assert row["fnc"].all() and row["depth"].max() == 6


def test_plan_random_mix_4096():
    keys, _, _, res = C.replay_mix(4096, 4196)
    exp = _plan_matches_rule(keys)
    _rule_matches_smt(keys, res)
    assert {e[1] for e in exp} == {0, 1}
    assert any(e[1] == 1 and e[3] == 0 and e[0] - e[4] >= 2 for e in exp)   # a push-down of depth >= 2


def test_plan_refuses_what_the_processor_cannot_express():
    L = lib()
    a = 0x1ABCD
    with pytest.raises(HzError) as e:
        L.smt_plan([4, a, a | 1 << 17], 17)   # equal in their low 17 bits
    assert e.value.status == 4 and "op 2" in str(e.value)
    assert L.smt_plan([4, a, a | 1 << 17], 19)["depth"].tolist() == [0, 1, 18]
    with pytest.raises(HzError) as e:
        L.smt_plan([4, a, a ^ 1 << 16], 17)   # the leaf would sit at depth 17
    assert e.value.status == 4
    with pytest.raises(HzError) as e:
        L.smt_plan([1, 1 << 48], 17)
    assert e.value.status == 4 and "key[1]" in str(e.value)
    for n_sib in (0, 65):
        with pytest.raises(HzError) as e:
            L.smt_plan([1], n_sib)
        assert e.value.status == 1
    assert L.smt_plan([], 17)["depth"].size == 0


def test_sparse_tree_needs_a_device():
    L = lib()
    if L.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(HzError) as e:
        L.smt(17)
    assert e.value.status == 5
    for bad in (0, 65):
        with pytest.raises(HzError) as e:
            L.smt(bad)   # arguments are checked before the device is looked for
        assert e.value.status == 1


def test_sparse_tree_kernels_use_no_scratch():
    """the compiler's resource remarks of csrc/smt_tree.hip (build/smt_tree.ru.txt): every k_smt_* kernel keeps its state in registers"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import resource_usage as RU
    path = os.path.join(RU.BUILD, "smt_tree.ru.txt")
    assert os.path.exists(path), "no %s: the build leaves the compiler's resource remarks there; build the library in this tree" % path
    rows = {r["name"]: r for r in RU.table([path])}
    for name in ("hz::k_smt_leaf", "hz::k_smt_level", "hz::k_smt_gather", "hz::k_smt_writeback"):
        assert name in rows, sorted(rows)
        assert rows[name]["scratch"] == 0, "%s uses %d bytes of scratch per lane" % (name, rows[name]["scratch"])
