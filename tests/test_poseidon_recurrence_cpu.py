"""Poseidon's partial rounds as a linear recurrence (poseidon.h, PoseidonCfg<T>::REC; derivation: tools/poseidon_sparse.py): the
generator's coefficients reproduce the dense permutation in Python integers for every width, the constant blocks it lays out do
so when they are evaluated the way the device evaluates them (Montgomery products, both sinks), the host build of poseidon.h agrees
with the host library's textbook permutation, and the committed constants are what the generator writes."""
import ctypes
import functools
import json
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_constants as GC      # noqa: E402
import poseidon_sparse as PS    # noqa: E402

P = PS.P
R = 1 << 261
RINV = pow(R, P - 2, P)
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "poseidon_kat.json")))
WIDTHS = [2, 3, 4, 5, 6, 7]


def inputs(t):
    """the upstream known answers of the width (with their digests), all-zero, all p - 1, seeded random inputs"""
    rng = random.Random(977 * t)
    kat = [([int(x) for x in v["in"]], int(v["out"])) for v in GOLD["upstream_kat"] if len(v["in"]) == t - 1]
    rows = [[0] * (t - 1), [P - 1] * (t - 1)] + [[rng.randrange(P) for _ in range(t - 1)] for _ in range(3)]
    return kat + [(x, None) for x in rows]


@functools.lru_cache(maxsize=None)
def dense(t, x):
    """(digest, S-box inputs in evaluation order) of the textbook permutation"""
    sb = []
    return PS.poseidon_naive(list(x), t, sb), sb


@pytest.mark.parametrize("t", WIDTHS)
def test_coefficients_reproduce_the_dense_permutation(t):
    rc = PS.recurrence_params(t)
    n = t - 1
    assert len(rc["alpha"]) == n and len(rc["gamma"]) == n + 1 and sorted(rc["e"]) == list(range(t, rc["rp"] + 1))
    assert len(rc["ex"]) == len(rc["ey"]) == len(rc["cexit"]) == n
    for x, out in inputs(t):
        want, want_sb = dense(t, tuple(x))
        assert out is None or want == out
        sb = []
        assert PS.poseidon_recurrence(x, rc, sb) == want, x
        assert sb == want_sb, x
        # the partial-round S-box inputs themselves: x_k of the recurrence against the dense evaluation's, k = t .. rp - 1
        part = want_sb[4 * t:4 * t + rc["rp"]]
        ys = [pow(v, 5, P) for v in part]
        for k in range(t, rc["rp"]):
            got = (sum(rc["alpha"][i - 1] * part[k - i] for i in range(1, n + 1))
                   + sum(rc["gamma"][j - 1] * ys[k - j] for j in range(1, n + 2)) + rc["e"][k]) % P
            assert got == part[k], (x, k)


def eval_block(K, t, witness, x):
    """poseidon_hash<T> of poseidon.h for a REC width on the integers of its constant block, statement by statement: every value in
    Montgomery form except (witness sink) the S-box outputs. Returns (canonical digest, canonical S-box inputs)."""
    n, rp = t - 1, PS.N_ROUNDS_P[t - 2]
    tail = 4 * t + 1 + (rp // 2) * (4 * t + 1) + (rp % 2) * 2 * t + n * n + n
    mo = tail + 3 * t
    part = mo + t * t          # the appended constants: entry rounds, recurrence row, addends, exit matrix, its constants
    rec = part + n * 2 * t - n
    eo = rec + 2 * t - 1
    dense_o = eo + rp - n
    cf = dense_o + 2 * n * n
    assert len(K) == cf + n
    M = K[mo:mo + t * t]
    sb = []

    def sbox(v):
        sb.append(v * RINV % P)
        a = v * RINV % P
        return pow(a, 5, P) if witness else pow(a, 5, P) * R % P

    def row(coef, st, addend):     # (sum coef * st + addend) / R
        return (sum(c * s for c, s in zip(coef, st)) + (addend or 0)) * RINV % P

    def mix_ark(st, Cn, nc):
        return [row(M[i * t:(i + 1) * t], st, Cn[i] if i < nc else None) for i in range(t)]
    st = [K[0]] + [(v * R + K[j + 1]) % P for j, v in enumerate(x)]
    for r in range(3):
        st = mix_ark([sbox(v) for v in st], K[t * (r + 1):t * (r + 2)], t)
    st = mix_ark([sbox(v) for v in st], K[4 * t:4 * t + 1], 1)
    w = [st[0]] * (2 * n + 1)
    S = part
    for r in range(n):
        st = [sbox(st[0])] + st[1:]
        w = w[1:n + 1] + [st[0]] + w[n + 1:]
        xn = row(K[S:S + t], st, K[S + t])
        w = w[:n + 1] + w[n + 2:] + [xn]
        if r + 1 < n:
            st = [st[0]] + [(K[S + t + j] * st[0] * RINV + st[j]) % P for j in range(1, t)]
        st = [xn] + st[1:]
        S += 2 * t
    for r in range(n, rp):
        w = w[1:n + 1] + [sbox(w[2 * n])] + w[n + 1:]
        w = w[:n + 1] + w[n + 2:] + [row(K[rec:rec + 2 * n + 1], w, K[eo + r - n])]
    st = [w[2 * n]] + [row(K[dense_o + i * 2 * n:dense_o + (i + 1) * 2 * n], w[1:], K[cf + i]) for i in range(n)]
    for r in range(3):
        st = mix_ark([sbox(v) for v in st], K[tail + t * r:tail + t * (r + 1)], t)
    st = [sbox(v) for v in st]
    return row(M[:t], st, None) * RINV % P, sb


@pytest.mark.parametrize("t", WIDTHS)
def test_constant_blocks_evaluate_to_the_dense_permutation(t):
    """both blocks of the width with the recurrence's constants appended (digest sink: K, canonical S-box sink: KW), whichever form
    the width is compiled with; what precedes them is the pair form's block unchanged"""
    for witness in (False, True):
        K = GC.poseidon_block(t, witness, rec=True)
        pair = GC.poseidon_block(t, witness, rec=False)
        assert K[:len(pair)] == pair
        assert all(0 <= c < P for c in K)
        for x, _ in inputs(t):
            want, want_sb = dense(t, tuple(x))
            got, sb = eval_block(K, t, witness, x)
            assert got == want, (witness, x)
            assert sb == want_sb, (witness, x)


def test_the_switch_is_read_from_the_header():
    rec = GC.recurrence_widths()
    assert 3 in rec and set(rec) <= set(WIDTHS)
    for t in WIDTHS:
        for witness in (False, True):
            assert GC.poseidon_block(t, witness) == GC.poseidon_block(t, witness, rec=t in rec)


def test_host_build_of_the_device_form_equals_the_host_library():
    """hzb_poseidon_dev9 is poseidon_hash<T> of poseidon.h compiled for the host (9 x 29-bit limbs, the compiled-in form of every
    width); hzb_poseidon is the textbook permutation on the host field. Every arity, the same inputs."""
    from circuits_amd import builder as B
    h = B.host()
    out = ctypes.create_string_buffer(32)
    for t in WIDTHS:
        for x, kat in inputs(t):
            buf = b"".join(v.to_bytes(32, "little") for v in x)
            assert h.c.hzb_poseidon_dev9(t - 1, buf, out) == 0
            got = int.from_bytes(out.raw, "little")
            assert got == h.poseidon(x), (t, x)
            assert got == dense(t, tuple(x))[0], (t, x)
            assert kat is None or got == kat


def test_committed_constants_are_what_the_generator_writes():
    prod, orac, hostc = GC.poseidon_inc_texts()
    for text, path in ((prod, "circuits_amd/csrc/gen/poseidon_consts.inc"), (hostc, "circuits_amd/csrc/gen/poseidon_consts_host.inc"),
                       (orac, "oracle/gen/poseidon_consts_canon.inc")):
        assert open(os.path.join(ROOT, path)).read() == text, "%s is stale: python tools/gen_constants.py" % path
