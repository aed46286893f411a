"""Shared by tests/test_exit_archive.py (GPU) and tests/test_exit_archive_cpu.py: exit trees of earlier batches kept on the ledger
(hz_ledger_exit_keep, hz_ledger_withdraw_rows). The tree's shape (root, child, leaf_key: smt_plan.h's integers) grown by
ordered inserts in plain Python, the walk over it restated, its digests computed with the builder's hasher, the input of
tests/native/exit_archive_check.cpp, and the expected rows of a query from builder.withdraw_input."""
import numpy as np

import ledger_common as C
import ledger_exit_common as X
from circuits_amd import builder as B

FOUND, NOT_KEPT, ABSENT, DEEP = 0, 1, 2, 3
ZERO, NODE, LEAF = 0, 1, 2
ROWS = ("root_exit", "eth_addr", "token_id", "balance", "idx", "sign", "ay")   # the seven single rows of hz_withdraw_rows_out, in its order
SIGNAL = {"root_exit": "rootExit", "eth_addr": "ethAddr", "token_id": "tokenID", "balance": "balance", "idx": "idx", "sign": "sign", "ay": "ay"}


class Shape:
    """a sparse tree's shape as the device's planner keeps it: a reference is 0 (empty), n + 1 (node n) or -(l + 1) (leaf l)"""

    def __init__(self, keys=()):
        self.root, self.child, self.leaf_key = 0, [], []
        for key in keys:
            self.insert(key)

    def _set(self, at, ref):
        if at is None:
            self.root = ref
        else:
            self.child[at] = ref

    def insert(self, key):
        """the key's leaf, made at the shallowest depth where the key is alone (a key that is there already: its leaf)"""
        ref, at, f = self.root, None, 0
        while ref > 0:
            at = (ref - 1) * 2 + ((key >> f) & 1)
            ref = self.child[at]
            f += 1
        if ref < 0 and self.leaf_key[-ref - 1] == key:
            return -ref - 1
        leaf = len(self.leaf_key)
        self.leaf_key.append(key)
        if ref == 0:
            self._set(at, -leaf - 1)
            return leaf
        e = f   # the key met another key's leaf: both move below the first depth at or past f where they differ
        while not ((key ^ self.leaf_key[-ref - 1]) >> e) & 1:
            e += 1
        for d in range(f, e + 1):
            n = len(self.child) // 2
            self.child += [0, 0]
            self._set(at, n + 1)
            at = n * 2 + ((key >> d) & 1)
        self.child[at], self.child[at ^ 1] = -leaf - 1, ref
        return leaf

    @property
    def nodes(self):
        return len(self.child) // 2


def src_of(ref):
    return 0 if ref == 0 else NODE << 30 | (ref - 1) if ref > 0 else LEAF << 30 | (-ref - 1)


def walk_model(sh, key, n_sib):
    """archive_walk restated: -> (status, depth, leaf, [source of depth d for d < min(depth, n_sib)])"""
    if key >> 48:
        return ABSENT, 0, 0, []
    ref, f, srcs = sh.root, 0, []
    while ref > 0:
        bit = (key >> f) & 1
        if f < n_sib:
            srcs.append(src_of(sh.child[(ref - 1) * 2 + (bit ^ 1)]))
        ref = sh.child[(ref - 1) * 2 + bit]
        f += 1
    if ref == 0 or sh.leaf_key[-ref - 1] != key:
        return ABSENT, f, 0, srcs
    return (DEEP if f >= n_sib else FOUND), f, -ref - 1, srcs


def met_of(sh, key):
    """what the walk for key ends at: None (an empty slot) or the key of the leaf it meets"""
    ref, f = sh.root, 0
    while ref > 0:
        ref = sh.child[(ref - 1) * 2 + ((key >> f) & 1)]
        f += 1
    return None if ref == 0 else sh.leaf_key[-ref - 1]


def digests(sh, value_of, hasher=None):
    """-> (digest of every node, hash of every leaf, the root's digest) with circomlib's hashes: a leaf is H(key, value, 1), a node H(l, r)"""
    h = hasher or B.host()
    leaf = [h.poseidon([k, value_of(k), 1]) for k in sh.leaf_key]
    node = [None] * sh.nodes

    def of(ref):
        if ref == 0:
            return 0
        if ref < 0:
            return leaf[-ref - 1]
        n = ref - 1
        if node[n] is None:
            node[n] = h.poseidon([of(sh.child[2 * n]), of(sh.child[2 * n + 1])])
        return node[n]
    return node, leaf, of(sh.root)


def digest_of(src, node, leaf):
    return 0 if src >> 30 == ZERO else (node if src >> 30 == NODE else leaf)[src & 0x3FFFFFFF]


def absent_keys(sh, lo, hi):
    """-> (a key in lo .. hi - 1 whose walk meets another key's leaf, one whose walk meets an empty slot); None where there is none"""
    at_leaf = at_empty = None
    held = set(sh.leaf_key)
    for key in range(lo, hi):
        if key in held:
            continue
        m = met_of(sh, key)
        if m is None and at_empty is None:
            at_empty = key
        if m is not None and at_leaf is None:
            at_leaf = key
    return at_leaf, at_empty


def check_lines(cases, e0s):
    """tests/native/exit_archive_check.cpp's input and the lines the model expects back. cases: [(Shape, [(key, n_sib)])]; e0s: [e0]"""
    lines, expect = [], []
    for sh, queries in cases:
        lines.append("t %d %d %d" % (sh.root, sh.nodes, len(sh.leaf_key)))
        lines.append(" ".join(["c"] + [str(c) for c in sh.child]))
        lines.append(" ".join(["k"] + ["%x" % k for k in sh.leaf_key]))
        for key, n_sib in queries:
            lines.append("q %x %d" % (key, n_sib))
            status, depth, leaf, srcs = walk_model(sh, key, n_sib)
            expect.append(" ".join(str(v) for v in ["q", status, depth, leaf] + srcs))
    for e0 in e0s:
        lines.append("e %x %x" % (e0 & 0xFFFFFFFF, (e0 >> 64) & 0xFFFFFFFF))
        expect.append("e %d %d" % (e0 & 0xFFFFFFFF, (e0 >> 72) & 1))
    return "\n".join(lines) + "\n", expect


def edge_key_lists():
    """{name: the exit keys of the named edge batch of ledger_exit_common, in operation order}"""
    sp = X.exit_state(6)
    return {name: X.plan_model(l1_txs, l2_txs, [1], [0])["exit_key"] for name, (l1_txs, l2_txs) in X.edge_batches(sp).items()}


# ---- the GPU side's expectations -----------------------------------------------------------------------------------------------------------
def expected_rows(view, idx, n_levels):
    """builder.withdraw_input of an exit leaf in hz_ledger_withdraw_rows' layout: {name: [32] bytes}, siblings_state [n_levels + 1, 32]"""
    inp, _ = B.withdraw_input(view, idx, n_levels)
    out = {name: C.to_bytes([inp[SIGNAL[name]]])[0] for name in ROWS}
    out["siblings_state"] = C.to_bytes(inp["siblingsState"])
    return out


def assert_row(got, i, exp, what=""):
    for name, val in exp.items():
        assert got[name][i].tobytes() == np.asarray(val).tobytes(), (what, name)


def assert_zero_row(got, i, what=""):
    for name in ROWS + ("siblings_state",):
        assert not got[name][i].any(), (what, name)
