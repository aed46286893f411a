"""Exit trees of earlier batches kept on the ledger (hz_ledger_exit_keep, hz_ledger_withdraw_rows) without a device: the walk
over a frozen tree's integers (root, child, leaf_key) restated in plain Python against builder.SMT.find -- present keys, absent keys that
meet a leaf, absent keys that meet an empty slot --; the HZ_HD walk and row unpacking of csrc/ledger_archive.h built for the host under the
address and undefined-behaviour sanitizers against that model; the new symbols, the header's phrases, the build's resource remarks and
the argument errors that need no device.
The model tests hold the model against the existing builder: they validate what the host program is compared with. What the device
computes is guarded by tests/test_exit_archive.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import exit_archive_common as E
import ledger_exit_common as X
from circuits_amd import builder as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hz_ledger_exit_keep", "hz_ledger_exit_forget", "hz_ledger_exit_kept", "hz_ledger_exit_archive_stats", "hz_ledger_exit_root_of",
               "hz_ledger_withdraw_rows", "hz_ledger_withdraw_rows_dev", "hz_ledger_withdraw_ms", "hz_ledger_exit_keep_ms"]


def _key_lists():
    """[(name, keys in insertion order)]: the exit keys of the named edges and of the seeded batches, and drawn sets of 1 to 200 keys --
    small ranges (deep trees, shared low bits), 48-bit keys, consecutive keys"""
    out = [(name, keys) for name, keys in E.edge_key_lists().items()]
    out += [("seed %d" % n, X.plan_model(a, b, [1], [0])["exit_key"]) for n, (_, _, a, b) in enumerate(X.seeded_batches())]
    rng = np.random.default_rng(8)
    for n in (1, 2, 3, 7, 64, 200):
        out.append(("dense %d" % n, [256 + int(x) for x in rng.choice(4 * n, size=n, replace=False)]))
        out.append(("wide %d" % n, [int(x) for x in rng.integers(2, 1 << 48, size=n)]))
    out.append(("consecutive", list(range(256, 256 + 130))))
    out.append(("same residue", [256 + (i << 9) for i in range(12)]))   # every pair shares nine low bits: chains of one-child nodes
    return out


def _queries(sh, keys):
    """present keys, and absent ones of both kinds where the tree has them"""
    held = sorted(set(keys))
    lo = min(held) if held else 256
    at_leaf, at_empty = E.absent_keys(sh, max(lo - 70, 0), lo + 600)
    absent = [k for k in (at_leaf, at_empty) if k is not None]
    return held, absent, at_leaf, at_empty


def test_walk_model_is_the_builders_find():
    kinds = set()
    for name, keys in _key_lists():
        sh = E.Shape(keys)
        tree = B.SMT()
        value_of = lambda k: (k * 7919 + 13) % B.P   # noqa: E731
        for k in dict.fromkeys(keys):
            tree.insert(k, value_of(k))
        node, leaf, root = E.digests(sh, value_of)
        assert root == tree.root, name
        assert sorted(sh.leaf_key) == sorted(set(keys)) and len(sh.leaf_key) == len(set(keys))
        # the depth of every new leaf is what the key set says (ledger_exit_common.tree_plan_model)
        order = list(dict.fromkeys(keys))
        partial = E.Shape()
        for key, plan in zip(order, [p for p in X.tree_plan_model(order)]):
            partial.insert(key)
            assert E.walk_model(partial, key, 64)[1] == plan[3], (name, key)
        held, absent, at_leaf, at_empty = _queries(sh, keys)
        for key in held + absent:
            f = tree.find(key)
            status, depth, l, srcs = E.walk_model(sh, key, 64)
            assert (status == E.FOUND) == f["found"], (name, key)
            assert [E.digest_of(s, node, leaf) for s in srcs] == list(f["siblings"]) and depth == len(f["siblings"]), (name, key)
            if f["found"]:
                assert sh.leaf_key[l] == key and leaf[l] == tree._hash1(key, f["foundValue"])
                kinds.add("present")
            else:
                met = E.met_of(sh, key)
                assert (met is None) == f["isOld0"] and (met is None or met == f["notFoundKey"]), (name, key)
                kinds.add("empty" if met is None else "leaf")
            # a proof of fewer siblings: the same sources up to n_sib, DEEP exactly where hz_smt_proofs refuses (depth >= n_sib)
            for n_sib in {1, max(depth, 1), depth + 1}:
                s2, d2, l2, srcs2 = E.walk_model(sh, key, n_sib)
                assert d2 == depth and srcs2 == srcs[:n_sib]
                assert s2 == (E.ABSENT if status == E.ABSENT else E.DEEP if depth >= n_sib else E.FOUND)
        assert E.walk_model(sh, 1 << 48, 64) == (E.ABSENT, 0, 0, []) and E.walk_model(sh, (1 << 48) | (held[0] if held else 0), 64)[0] == E.ABSENT
    assert kinds == {"present", "empty", "leaf"}
    # the shapes the GPU tests name: a root that is the single leaf, the pair below a chain of one-child nodes, the empty tree
    lists = E.edge_key_lists()
    one = E.Shape(lists["first_exit_into_empty_tree"])
    assert one.root == -1 and one.nodes == 0 and E.walk_model(one, one.leaf_key[0], 17) == (E.FOUND, 0, 0, [])
    pair = E.Shape(lists["keys_sharing_low_bits"])
    a, far = lists["keys_sharing_low_bits"]
    assert a ^ far == 1 << 5 and pair.nodes == 6
    assert E.walk_model(pair, a, 7) == (E.FOUND, 6, 0, [0] * 5 + [E.LEAF << 30 | 1]) and E.walk_model(pair, far, 6)[0] == E.DEEP
    assert lists["zero_amount_exit"] == [] and E.walk_model(E.Shape(), a, 17) == (E.ABSENT, 0, 0, [])
    assert len(set(lists["same_account_twice"])) == 1 and len(lists["same_account_twice"]) == 2


def test_host_build_of_the_walk_agrees_with_the_model(tmp_path):
    """csrc/ledger_archive.h (archive_walk, the unpacking of tokenID and sign from e0) as a stand-alone host program under
    -fsanitize=address,undefined: every key list above with present and absent keys at n_sib = 1, the walk's own depth, one more and 64,
    keys of 2^48 and more, the empty tree; arrays of exactly the shape's size, so a read past an end is an error"""
    cases = []
    for name, keys in _key_lists():
        sh = E.Shape(keys)
        held, absent, _, _ = _queries(sh, keys)
        queries = []
        for key in held[:40] + absent + [1 << 48, (1 << 63) | 5]:
            depth = E.walk_model(sh, key, 64)[1]
            queries += [(key, n_sib) for n_sib in sorted({1, max(depth, 1), min(depth + 1, 64), 64})]
        cases.append((sh, queries))
    cases.append((E.Shape(), [(300, 1), (300, 17), (0, 64)]))
    e0s = [0, 1, 0xFFFFFFFF, 1 << 72, 0xFFFFFFFF | 1 << 72, 7 | ((1 << 40) - 1) << 32, 5 | ((1 << 40) - 1) << 32 | 1 << 72, 1 << 73 | 9]
    text, expect = E.check_lines(cases, e0s)
    assert sum(1 for ln in expect if ln.startswith("q 0 ")) > 100 and any(ln.startswith("q 2 ") for ln in expect) and any(ln.startswith("q 3 ") for ln in expect)
    src = os.path.join(os.path.dirname(__file__), "native", "exit_archive_check.cpp")
    exe = str(tmp_path / "exit_archive_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(expect)
    for n, (g, e) in enumerate(zip(got, expect)):
        assert g == e, (n, g, e)


def test_new_symbols_are_declared_and_exported():
    from circuits_amd.capi import EXPORTS, WITHDRAW_ARRAYS, lib_path
    assert all(s in EXPORTS for s in NEW_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    assert all(s + "(" in header for s in NEW_SYMBOLS) and "#define HZ_WITHDRAW_ARRAYS 9" in header and "} hz_withdraw_rows_out;" in header
    assert len(WITHDRAW_ARRAYS) == 9 and WITHDRAW_ARRAYS[:7] == E.ROWS
    members = header.split("#define HZ_WITHDRAW_ARRAYS 9")[1].split("} hz_withdraw_rows_out;")[0]
    assert [members.index(name) for name in WITHDRAW_ARRAYS] == sorted(members.index(name) for name in WITHDRAW_ARRAYS)
    if not os.path.exists(lib_path()):
        pytest.skip("the library was not built in this tree")
    c = ctypes.CDLL(lib_path())
    assert [s for s in NEW_SYMBOLS if not hasattr(c, s)] == []


def test_the_headers_out_of_scope_line_keeps_its_phrases():
    header = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    for phrase in ("exit trees of earlier batches kept resident, a resident address index", "L1 transactions that create accounts or exit",
                   "OUT OF SCOPE: L1 transactions"):
        assert phrase in header, phrase
    scope = header.split("OUT OF SCOPE: L1 transactions")[1].split("*/")[0]
    assert "persisting, or carrying across a reload, the exit trees" in scope and "hz_ledger_load / hz_ledger_load_accounts empty it" in header


def test_archive_kernels_use_no_scratch_and_no_lds():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as RU
    path = os.path.join(RU.BUILD, "ledger.ru.txt")
    if not os.path.exists(path):
        pytest.skip("the library was not built in this tree (no build/ledger.ru.txt)")
    rows = {r["name"]: r for r in RU.table([path])}
    for name in ("hz::k_withdraw_walk", "hz::k_withdraw_fill"):
        assert name in rows, sorted(rows)
        assert rows[name]["scratch"] == 0 and rows[name]["lds"] == 0, (name, rows[name])


def test_argument_errors_come_before_any_device_call():
    """without a ledger nothing can reach the device: the null ledger and, before it is even looked at, the count and the sibling number"""
    from circuits_amd import lib
    from circuits_amd.capi import lib_path
    if not os.path.exists(lib_path()):
        pytest.skip("the library was not built in this tree")
    hz = lib()
    c = hz.c
    b, k = np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint64)
    assert c.hz_ledger_exit_keep(None, 1) == 1 and "null ledger" in c.hz_last_error().decode()
    assert c.hz_ledger_exit_forget(None, 1) == 1
    assert c.hz_ledger_withdraw_rows(None, 4, b.ctypes.data, k.ctypes.data, 16, None) == 1 and "null ledger" in c.hz_last_error().decode()
    for args, text in (((4, b.ctypes.data, k.ctypes.data, 64, None), "n_levels + 1 = 65"), ((4, b.ctypes.data, k.ctypes.data, -1, None), "n_levels + 1 = 0"),
                       (((1 << 20) + 1, b.ctypes.data, k.ctypes.data, 16, None), "at most 2^20"), ((4, None, k.ctypes.data, 16, None), "null argument"),
                       ((4, b.ctypes.data, None, 16, None), "null argument")):
        assert c.hz_ledger_withdraw_rows(None, *args) == 1 and text in c.hz_last_error().decode(), (text, c.hz_last_error().decode())
    assert c.hz_ledger_withdraw_rows_dev(None, None) == 1 and c.hz_ledger_exit_root_of(None, 1, None) == 1
    n = ctypes.c_size_t(7)
    assert c.hz_ledger_exit_kept(None, None, 0, ctypes.byref(n)) == 1 and c.hz_ledger_exit_archive_stats(None, None, None, None, None) == 1
    assert c.hz_ledger_withdraw_ms(None) == 0.0 and c.hz_ledger_exit_keep_ms(None) == 0.0
