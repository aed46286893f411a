#!/usr/bin/env python3
"""Sparse form of the Poseidon partial rounds (product-side constants only).

The circuit (circomlib 0.5.2 poseidon.circom) evaluates every partial round as Ark (t constants),
one S-box on state[0], Mix (dense t x t MDS): t^2 constant products per round. The witness only
holds the S-box signals (in2, in4, out), so any evaluation order that reproduces the S-box INPUTS
is admissible. Two exact rewrites (both classic, cf. the Poseidon paper's appendix on optimised
implementations) bring a partial round down to 2t - 1 constant products:

1. constants: only state[0] passes through the S-box, so the constants of the other t-1 lanes are
   pushed through the linear layer into the next round: e_r = c_r + carry_r, only e_r[0] is added,
   carry_{r+1} = M * (0, e_r[1..]); what is left after the last partial round is added to the
   constants of the following full round.
2. linear layer: with N_0 = I, round r applies M * diag(1, N_r) = diag(1, Mh N_r) * S_r where
   S_r = [[m00, v^T N_r], [(Mh N_r)^-1 w, I]] is sparse (M = [[m00, v^T], [w, Mh]]), and
   N_{r+1} = Mh N_r stays pending on lanes 1..t-1 (it commutes with the S-box, which only touches
   lane 0). After the last partial round the pending N_RP is applied once (dense, (t-1)^2 products).

state[0] is never transformed, so the S-box inputs and outputs are bit-identical to the naive
evaluation; `check()` verifies this against tools/poseidon_params.py (the textbook permutation) for random inputs.

Linear recurrence (`recurrence_params`, the form poseidon.h evaluates for the widths whose PoseidonCfg says REC). Between the
first and the last partial round lanes 1..t-1 are a linear system driven by one scalar a round: with y_k the S-box output of partial
round k, x_k its input, h the hidden lanes, M = [[m00, r], [b, A]] and n = t - 1,
    h' = A h + b y + (constants),    x' = m00 y + r h + (constant).
By Cayley-Hamilton (alpha_i = the negated coefficients of A's characteristic polynomial) the hidden lanes drop out:
    x_k = sum_{i=1..n} alpha_i x_{k-i} + sum_{j=1..n+1} gamma_j y_{k-j} + e_k          for k >= t,
gamma_j = g_j - sum_{i<j} alpha_i g_{j-i}, g_1 = m00, g_j = r A^(j-2) b (the impulse response), e_k = the same combination of the
response to the round constants alone. That is 2t - 1 products and ONE lazily reduced sum per round, and nothing else. The first
t - 1 partial rounds stay in the sparse form above (they produce x_1..x_n and y_0..y_{n-1}); after the last one the lanes are
recovered from the last n inputs and outputs through the inverse of the observability matrix [r; rA; ..; rA^(n-1)], stepped n rounds
forward (`ex`, `ey`, `cexit`: an n x 2n matrix and a constant that take the place of `dense`). `check_recurrence()` verifies digest
and every S-box input against the textbook permutation.
"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from poseidon_params import P, N_ROUNDS_P, generate  # noqa: E402


def mat_mul(A, B):
    n, m, k = len(A), len(B[0]), len(B)
    return [[sum(A[i][x] * B[x][j] for x in range(k)) % P for j in range(m)] for i in range(n)]


def mat_vec(A, v):
    return [sum(a * b for a, b in zip(row, v)) % P for row in A]


def mat_inv(A):
    n = len(A)
    a = [list(r) + [1 if i == j else 0 for j in range(n)] for i, r in enumerate(A)]
    for c in range(n):
        piv = next(r for r in range(c, n) if a[r][c] % P)
        a[c], a[piv] = a[piv], a[c]
        inv = pow(a[c][c], P - 2, P)
        a[c] = [x * inv % P for x in a[c]]
        for r in range(n):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [(x - f * y) % P for x, y in zip(a[r], a[c])]
    return [r[n:] for r in a]


def sparse_params(t):
    """Returns dict: rp, e0[rp] (constant added to lane 0 before the S-box of partial round r),
    row[rp][t] (lane-0 row of S_r), col[rp][t-1], dense[(t-1)][(t-1)] = N_RP, and cfull: the constants of
    the first full round after the partial rounds with the leftover carry folded in."""
    C, M = generate(t)
    rp = N_ROUNDS_P[t - 2]
    m00, v, w = M[0][0], M[0][1:], [M[i][0] for i in range(1, t)]
    Mh = [M[i][1:] for i in range(1, t)]
    carry = [0] * t
    e0, row, col = [], [], []
    N = [[1 if i == j else 0 for j in range(t - 1)] for i in range(t - 1)]
    for r in range(rp):
        c = C[t * (4 + r): t * (5 + r)]
        e = [(c[j] + carry[j]) % P for j in range(t)]
        e0.append(e[0])
        carry = mat_vec(M, [0] + e[1:])
        vN = [sum(v[k] * N[k][j] for k in range(t - 1)) % P for j in range(t - 1)]
        MhN = mat_mul(Mh, N)
        col.append(mat_vec(mat_inv(MhN), w))
        row.append([m00] + vN)
        N = MhN
    cf = C[t * (4 + rp): t * (5 + rp)]
    cfull = [(cf[j] + carry[j]) % P for j in range(t)]
    return {"t": t, "rp": rp, "C": C, "M": M, "e0": e0, "row": row, "col": col, "dense": N, "cfull": cfull}


def poseidon_sparse(inputs, sp, sboxes=None):
    """Evaluation with the sparse partial rounds; appends every S-box input to `sboxes`."""
    t, rp, C, M = sp["t"], sp["rp"], sp["C"], sp["M"]
    st = [0] + [x % P for x in inputs]

    def full(st, c):
        st = [(a + b) % P for a, b in zip(st, c)]
        if sboxes is not None:
            sboxes.extend(st)
        st = [pow(x, 5, P) for x in st]
        return mat_vec(M, st)

    for r in range(4):
        st = full(st, C[t * r: t * (r + 1)])
    for r in range(rp):
        x = (st[0] + sp["e0"][r]) % P
        if sboxes is not None:
            sboxes.append(x)
        y = pow(x, 5, P)
        s0 = (sp["row"][r][0] * y + sum(a * b for a, b in zip(sp["row"][r][1:], st[1:]))) % P
        st = [s0] + [(st[1 + i] + sp["col"][r][i] * y) % P for i in range(t - 1)]
    st = [st[0]] + mat_vec(sp["dense"], st[1:])
    st = full(st, sp["cfull"])
    for r in range(5 + rp, 8 + rp):
        st = full(st, C[t * r: t * (r + 1)])
    return st[0]


def poseidon_naive(inputs, t, sboxes):
    C, M = generate(t)
    rp = N_ROUNDS_P[t - 2]
    st = [0] + [x % P for x in inputs]
    for r in range(8 + rp):
        st = [(st[j] + C[t * r + j]) % P for j in range(t)]
        if r < 4 or r >= 4 + rp:
            sboxes.extend(st)
            st = [pow(x, 5, P) for x in st]
        else:
            sboxes.append(st[0])
            st[0] = pow(st[0], 5, P)
        st = mat_vec(M, st)
    return st[0]


def check(t, n=5, seed=1):
    rng = random.Random(seed + t)
    sp = sparse_params(t)
    for _ in range(n):
        x = [rng.randrange(P) for _ in range(t - 1)]
        a, b = [], []
        assert poseidon_naive(x, t, a) == poseidon_sparse(x, sp, b)
        assert a == b, "S-box inputs differ"
    return sp


def char_poly_alpha(A):
    """alpha_1..alpha_n with A^n = sum_i alpha_i A^(n-i) (Faddeev-LeVerrier over the field)"""
    n = len(A)
    ident = [[1 if i == j else 0 for j in range(n)] for i in range(n)]
    Mk = [[0] * n for _ in range(n)]
    c = 1                      # coefficient of lambda^n
    alpha = []
    for k in range(1, n + 1):
        Mk = [[(x + c * e) % P for x, e in zip(ra, ri)] for ra, ri in zip(mat_mul(A, Mk), ident)]
        AM = mat_mul(A, Mk)
        c = (-sum(AM[i][i] for i in range(n)) * pow(k, P - 2, P)) % P     # coefficient of lambda^(n-k)
        alpha.append((-c) % P)
    return alpha


def recurrence_params(t):
    """sparse_params(t) plus: alpha[n], gamma[n+1] (index 0 = lag 1), e[k] for k = t..rp (e[rp] belongs to lane 0 of the full round
    after the partial rounds), ex[n][n] / ey[n][n] / cexit[n]: lanes 1.. of that full round (constants included) =
    ex . (x_{rp-n+1}..x_rp) + ey . (y_{rp-n}..y_{rp-1}) + cexit."""
    sp = sparse_params(t)
    C, M, rp, n = sp["C"], sp["M"], sp["rp"], t - 1
    m00, r, b = M[0][0], M[0][1:], [M[i][0] for i in range(1, t)]
    A = [M[i][1:] for i in range(1, t)]
    dot = lambda u, v: sum(x * y for x, y in zip(u, v)) % P   # noqa: E731
    alpha = char_poly_alpha(A)
    # impulse response g_1.. and the powers of A
    Apow = [[[1 if i == j else 0 for j in range(n)] for i in range(n)]]
    for _ in range(n):
        Apow.append(mat_mul(A, Apow[-1]))
    g = [None, m00] + [dot(r, mat_vec(Apow[j - 2], b)) for j in range(2, n + 2)]
    gamma = [(g[j] - sum(alpha[i - 1] * g[j - i] for i in range(1, j))) % P for j in range(1, n + 2)]
    # Cayley-Hamilton: the impulse response obeys the recurrence from lag n + 2 on
    g_next = dot(r, mat_vec(mat_mul(A, Apow[n - 1]), b)) if n else 0
    assert n == 0 or g_next == sum(alpha[i - 1] * g[n + 2 - i] for i in range(1, n + 1)) % P
    # response to the constants alone (every S-box output taken as 0); round rp = the full round that follows
    ck = lambda k: C[t * (4 + k): t * (5 + k)]                # noqa: E731
    xc, hc = [ck(0)[0]], [ck(0)[1:]]
    for k in range(rp):
        c = ck(k + 1)
        xc.append((dot(r, hc[k]) + c[0]) % P)
        hc.append([(u + v) % P for u, v in zip(mat_vec(A, hc[k]), c[1:])])
    e = {k: (xc[k] - sum(alpha[i - 1] * xc[k - i] for i in range(1, n + 1))) % P for k in range(t, rp + 1)}
    # exit: O h_k0 = X - G Y - (constants), k0 = rp - n; h_rp = A^n h_k0 + sum_j A^(n-1-j) b y_{k0+j} + (constants)
    O = [[sum(r[x] * Apow[i][x][j] for x in range(n)) % P for j in range(n)] for i in range(n)]
    Oinv = mat_inv(O)                                          # raises StopIteration when not observable
    assert mat_mul(O, Oinv) == Apow[0], "observability matrix not invertible"
    ex = mat_mul(Apow[n], Oinv)
    G = [[g[i - j + 1] if j <= i else 0 for j in range(n)] for i in range(n)]
    B = [[mat_vec(Apow[n - 1 - j], b)[i] for j in range(n)] for i in range(n)]
    exG = mat_mul(ex, G)
    ey = [[(B[i][j] - exG[i][j]) % P for j in range(n)] for i in range(n)]
    k0 = rp - n
    exX = mat_vec(ex, xc[k0 + 1: k0 + n + 1])
    cexit = [(hc[rp][i] - exX[i]) % P for i in range(n)]
    sp.update({"alpha": alpha, "gamma": gamma, "e": e, "ex": ex, "ey": ey, "cexit": cexit})
    return sp


def poseidon_recurrence(inputs, rc, sboxes=None):
    """Evaluation as poseidon.h does it for a REC width: n sparse rounds, then the recurrence, then the exit matrix."""
    t, rp, C, M = rc["t"], rc["rp"], rc["C"], rc["M"]
    n = t - 1
    st = [0] + [x % P for x in inputs]

    def full(st, c):
        st = [(a + b) % P for a, b in zip(st, c)]
        if sboxes is not None:
            sboxes.extend(st)
        st = [pow(x, 5, P) for x in st]
        return mat_vec(M, st)

    for r in range(4):
        st = full(st, C[t * r: t * (r + 1)])
    xs, ys = [(st[0] + rc["e0"][0]) % P], []
    lanes = st[1:]
    for r in range(n):                 # entry: x_1..x_n, y_0..y_{n-1}; the lanes are not needed after the last row
        y = pow(xs[r], 5, P)
        ys.append(y)
        nxt = rc["e0"][r + 1] if r + 1 < rp else rc["cfull"][0]
        xs.append((rc["row"][r][0] * y + sum(a * b for a, b in zip(rc["row"][r][1:], lanes)) + nxt) % P)
        lanes = [(lanes[i] + rc["col"][r][i] * y) % P for i in range(n)]
    for k in range(n, rp):
        ys.append(pow(xs[k], 5, P))
        xs.append((sum(rc["alpha"][i - 1] * xs[k + 1 - i] for i in range(1, n + 1))
                   + sum(rc["gamma"][j - 1] * ys[k + 1 - j] for j in range(1, n + 2)) + rc["e"][k + 1]) % P)
    if sboxes is not None:
        sboxes.extend(xs[:rp])
    X, Y = xs[rp - n + 1: rp + 1], ys[rp - n: rp]
    st = [xs[rp]] + [(a + b + c) % P for a, b, c in zip(mat_vec(rc["ex"], X), mat_vec(rc["ey"], Y), rc["cexit"])]
    for r in range(4 + rp, 8 + rp):    # the constants of round 4 + rp are in e[rp] and cexit already
        if r > 4 + rp:
            st = [(a + b) % P for a, b in zip(st, C[t * r: t * (r + 1)])]
        if sboxes is not None:
            sboxes.extend(st)
        st = mat_vec(M, [pow(x, 5, P) for x in st])
    return st[0]


def check_recurrence(t, n=5, seed=1, extra=()):
    rng = random.Random(seed + t)
    rc = recurrence_params(t)
    cases = [[0] * (t - 1), [P - 1] * (t - 1)] + [list(x) for x in extra] + [[rng.randrange(P) for _ in range(t - 1)] for _ in range(n)]
    for x in cases:
        a, b = [], []
        assert poseidon_naive(x, t, a) == poseidon_recurrence(x, rc, b), "digest differs"
        assert a == b, "S-box inputs differ"
    return rc


if __name__ == "__main__":
    for t in range(2, 8):
        check(t)
        check_recurrence(t)
        print("t=%d sparse == recurrence == naive (digest and every S-box input)" % t)
