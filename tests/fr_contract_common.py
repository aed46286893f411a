"""The contract of every routine of circuits_amd/csrc/fr.h, as a table: precondition, operands at the edges of the precondition, and
the requirement on the result. Python integers only -- nothing here is shared with fr.h; value(limbs) = sum v[i] * 2^(29 i).

tools/range_check.py proves that the callers stay inside these ranges and takes each routine's contract as an axiom ("operands in
the stated range -> result congruent, normalised, below the stated bound"). This table states the axioms, and two runners put them to
the routines themselves: tests/test_fr_contract.py on the device through hz_fr_raw_ops (both builds of the kernels), and
tests/test_fr_contract_cpu.py through the host compile tests/native/fr_contract_host.cpp. tests/test_fr_contract_cpu.py also ties the
table to range_check's models (same operand bounds accepted, no result bound above the model's).

The requirements are the contract, not today's representative: a correct rewrite of a routine passes unchanged.

  every Fr result            limbs 0..7 below 2^29
  reduced sums               congruent to the stated expression, below 2p (fr_cond_sub_4p: below 4p)
  lazy sums                  congruent, inside the interval that fr.h's comment states
  the Montgomery family      column sums worth T: r R = T (mod p) and r <= floor(T / R) + p -- the reduction returns (T + M p) / R with
                             M < R, the bound range_check.mont uses
  canonical forms            the exact value, the unique representative in [0, p)
  fr_is_zero, fr_eq          the exact boolean; 0 and p are both zero
  fr_inv, fr_inv_fermat      r a = R^2 (mod p), r = 0 (mod p) for a = 0 (mod p); below 2p
  fr_pow                     for a = x R: r = x^e R (mod p)
"""
import functools
import itertools
import random

import numpy as np

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R = 1 << 261
RINV = pow(R, -1, P)
R2 = R * R % P
M29 = (1 << 29) - 1
LIMIT = 1 << 257            # fr.h fr_mul: "inputs normalised with value < 2^257"
P_TOP = 0x30644E            # p's top limb (p >> 232)
TOP_EQ = (P_TOP << 232) | 5  # top limb equal to p's, value below p
assert TOP_EQ < P and P >> 232 == P_TOP

# The edge values of the issue; an operand takes those its precondition admits.
EDGES = [0, 1, 2, P - 1, P, P + 1, 2 * P - 1, 2 * P, 4 * P - 1, 4 * P, 8 * P - 1, LIMIT - 1, LIMIT - 2,
         (1 << 232) - 1, 1 << 232, (1 << 29) - 1, 1 << 29, TOP_EQ]
EDGES_U64 = [0, 1, 2, (1 << 29) - 1, 1 << 29, (1 << 32) - 1, 1 << 32, (1 << 58) - 1, (1 << 64) - 1]
EDGES_EXP = [0, 1, 2, 3, P - 2, P - 1, P, (1 << 255), (1 << 256) - 1, (1 << 32) - 1, 1 << 32]

CAP = 1 << 14
CAPS = {"fr_inv": 4096, "fr_pow": 4096, "fr_inv_fermat": 256}
EDGE_DRAWS = 2048           # seeded draws from the edges, for the ops whose cross product is too large to send whole


def limbs(x):
    """integer -> 9 words: limbs 0..7 of 29 bits, limb 8 the rest"""
    assert 0 <= x < 1 << (232 + 32)
    return [(x >> (29 * i)) & M29 for i in range(8)] + [x >> 232]


def value(w):
    return sum(int(v) << (29 * i) for i, v in enumerate(w))


def words32(x, n=8):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def pack(kind, x):
    if kind == "fr":
        return limbs(x)
    if kind == "fc":      # a 256-bit integer as 8 x u32 in words 0..7
        assert 0 <= x < 1 << 256
        return words32(x) + [0]
    assert kind == "u64" and 0 <= x < 1 << 64
    return words32(x, 2) + [0] * 7


def in_p(x):
    return "%.6f p" % (x / P) if x > 1 << 200 else "%d" % x


# ---- requirements: each returns None or the name of the requirement that failed ------------------------------------------------------
def _normalised(w):
    return all(int(v) <= M29 for v in w[:8])


def req_sum(expr, bound):
    """reduced sum: normalised, congruent to expr(t), below bound(t)"""
    def check(t, w):
        if not _normalised(w):
            return "limbs 0..7 below 2^29"
        r = value(w)
        if (r - expr(t)) % P:
            return "congruent to the stated expression mod p"
        if not r < bound(t):
            return "result %s below %s" % (in_p(r), in_p(bound(t)))
    return check


def req_lazy(expr, bound, positive):
    """lazy sum: normalised, congruent, in (0, bound) or [0, bound)"""
    inner = req_sum(expr, bound)

    def check(t, w):
        e = inner(t, w)
        if e is None and positive and value(w) == 0:
            return "result above 0"
        return e
    return check


def mont_bound(T):
    return T // R + P + 1   # exclusive


def req_mont(T):
    """r R = T (mod p), r <= floor(T / R) + p, normalised"""
    def check(t, w):
        if not _normalised(w):
            return "limbs 0..7 below 2^29"
        r = value(w)
        if (r * R - T(t)) % P:
            return "r R congruent to the column sums T mod p"
        if not r < mont_bound(T(t)):
            return "result %s at most floor(T / R) + p = %s" % (in_p(r), in_p(mont_bound(T(t)) - 1))
    return check


def req_exact_limbs(expr):
    """the exact value in normalised limbs (one encoding per integer)"""
    def check(t, w):
        if not _normalised(w):
            return "limbs 0..7 below 2^29"
        if value(w) != expr(t):
            return "exactly %s (got %s)" % (in_p(expr(t)), in_p(value(w)))
    return check


def req_exact_fc(expr):
    def check(t, w):
        if int(w[8]) != 0:
            return "word 8 of an Fc result is zero"
        got = sum(int(v) << (32 * i) for i, v in enumerate(w[:8]))
        if got != expr(t):
            return "exactly %s (got %s)" % (in_p(expr(t)), in_p(got))
    return check


def req_bool(expr):
    def check(t, w):
        if any(int(v) for v in w[1:]) or int(w[0]) != int(bool(expr(t))):
            return "exactly the boolean %d (got words %s)" % (bool(expr(t)), [int(v) for v in w])
    return check


def _req_inv(t, w):
    if not _normalised(w):
        return "limbs 0..7 below 2^29"
    r, a = value(w), t[0]
    if a % P == 0:
        if r % P:
            return "inverse(0) = 0 mod p"
    elif (r * a - R2) % P:
        return "r a congruent to R^2 mod p"
    if not r < 2 * P:
        return "result %s below 2p" % in_p(r)


def _req_pow(t, w):
    if not _normalised(w):
        return "limbs 0..7 below 2^29"
    a, e = t
    if (value(w) - pow(a * RINV % P, e, P) * R) % P:
        return "r congruent to x^e R mod p for a = x R"


# ---- the table ---------------------------------------------------------------------------------------------------------------------
class Op:
    """name / code: the routine and its HZ_FRR_* code; kinds: "fr" | "fc" | "u64" per operand; ubs: the exclusive bound of each operand
    alone; joint: the part of the precondition that ties operands together; check: the requirement; extra: tuples always sent;
    points: for the tie to tools/range_check.py, corners of the precondition (exclusive operand bounds) at which the model is evaluated;
    bound: the exclusive bound the requirement puts on the result for given operands (None: no numeric bound / not an Fr)"""

    def __init__(self, name, code, kinds, ubs, check, joint=None, extra=(), points=None, bound=None, edges=None, positive=False):
        self.name, self.code, self.kinds, self.ubs, self.check = name, code, tuple(kinds), tuple(ubs), check
        self.joint, self.extra, self.bound, self.positive = joint, [tuple(x) for x in extra], bound, positive
        self.points = [tuple(p) for p in (points or [ubs])]
        self.edge_lists = edges or [self._edges(k, u) for k, u in zip(self.kinds, self.ubs)]

    @staticmethod
    def _edges(kind, ub):
        if kind == "u64":
            return list(EDGES_U64)
        if kind == "fc":
            return [e for e in EDGES if e < 1 << 256] + [(1 << 256) - 1, (1 << 256) - 2]
        return [e for e in EDGES if e < ub]

    def pre(self, t):
        """the precondition, as fr.h's comment and range_check's need(...) state it"""
        return len(t) == len(self.ubs) and all(0 <= x < u for x, u in zip(t, self.ubs)) and (self.joint is None or self.joint(t))

    def cap(self):
        return CAPS.get(self.name, CAP)

    def edge_product(self):
        """every admissible tuple of the operands' admissible edges"""
        return [t for t in itertools.product(*self.edge_lists) if self.pre(t)]

    def all_max(self):
        return tuple(u - 1 for u in self.ubs)


def _draw(rng, ub, edges):
    mode = rng.randrange(4)
    if mode == 0:
        return rng.randrange(ub)
    if mode == 1:     # limbs of zeros, ones and noise: the carry chains
        x = 0
        for i in range(9):
            x |= rng.choice((0, M29, M29, rng.getrandbits(29), 1, 1 << 28)) << (29 * i)
        return x % ub
    if mode == 2:     # beside an edge
        return min(max(rng.choice(edges) + rng.randrange(-3, 4), 0), ub - 1)
    return rng.randrange(1 << rng.randrange(1, ub.bit_length() + 1)) % ub


def _seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name)) + 0xF29


@functools.lru_cache(maxsize=None)
def operands(name):
    """The list of operand tuples of an op -- the same list, from the same seed, for every runner. Edges first (the full cross product
    for up to three operands; seeded draws from the edges and the all-maximal tuple beyond), then a seeded random fill up to the cap."""
    op = OPS[name]
    rng = random.Random(_seed(name))
    out = list(op.extra)
    if len(op.kinds) <= 3:
        out += op.edge_product()
    else:
        if op.pre(op.all_max()):
            out.append(op.all_max())
        while len(out) < EDGE_DRAWS:
            t = tuple(rng.choice(e) for e in op.edge_lists)
            if op.pre(t):
                out.append(t)
    assert len(out) <= op.cap(), (name, len(out))
    while len(out) < op.cap():
        t = tuple(_draw(rng, u, e) for u, e in zip(op.ubs, op.edge_lists))
        if op.pre(t):
            out.append(t)
    for t in out:
        assert op.pre(t), (name, t)     # nothing outside the contract is ever sent
    return tuple(out)


def pack_operands(op, tuples):
    """uint32[n_operands][n][9] (pack(), a column at a time)"""
    n = len(tuples)
    a = np.zeros((len(op.kinds), n, 9), dtype=np.uint32)
    for t in tuples:
        assert op.pre(t), (op.name, t)
    for k, kind in enumerate(op.kinds):
        if kind != "fr":
            a[k] = np.frombuffer(b"".join(t[k].to_bytes(36, "little") for t in tuples), dtype="<u4").reshape(n, 9)
            continue
        q = np.frombuffer(b"".join(t[k].to_bytes(40, "little") for t in tuples), dtype="<u8").reshape(n, 5)
        for i in range(9):
            w, sh = divmod(29 * i, 64)
            v = q[:, w] >> np.uint64(sh)
            if sh > 64 - 32:
                v = v | (q[:, w + 1] << np.uint64(64 - sh))
            a[k, :, i] = (v & np.uint64(M29 if i < 8 else 0xFFFFFFFF)).astype(np.uint32)
    if n:      # the vectorised cut against pack() itself
        for i in {0, n // 2, n - 1}:
            for k, kind in enumerate(op.kinds):
                assert list(a[k, i]) == pack(kind, tuples[i][k]), (op.name, i, k)
    return a


@functools.lru_cache(maxsize=None)
def packed(name):
    return pack_operands(OPS[name], operands(name))


def judge(op, tuples, out, who):
    """every element against the op's requirement; the message names op, build, element, lane, operands in units of p, requirement"""
    assert out.shape == (len(tuples), 9), "%s %s: %d results for %d tuples" % (op.name, who, len(out), len(tuples))
    bad = []
    for i, (t, w) in enumerate(zip(tuples, out)):
        e = op.check(t, w)
        if e is not None:
            bad.append("%s [%s] element %d (lane %d of wavefront %d): operands (%s): required: %s" % (
                op.name, who, i, i % 64, i // 64, ", ".join(in_p(x) for x in t), e))
    assert not bad, "%d of %d elements fail\n" % (len(bad), len(tuples)) + "\n".join(bad[:12])


def _dot_T(n, add):
    def T(t):
        return sum(t[2 * i] * t[2 * i + 1] for i in range(n)) + (t[2 * n] if add else 0)
    return T


def _mont_op(name, code, kinds, ubs, T, **kw):
    return Op(name, code, kinds, ubs, req_mont(T), bound=lambda t: mont_bound(T(t)), **kw)


def _sum_op(name, code, ubs, expr, bound=2 * P, **kw):
    return Op(name, code, ["fr"] * len(ubs), ubs, req_sum(expr, lambda t: bound), bound=lambda t: bound, **kw)


def _lazy_op(name, code, ubs, expr, bound, positive, **kw):
    return Op(name, code, ["fr"] * len(ubs), ubs, req_lazy(expr, bound, positive), bound=bound, positive=positive, **kw)


def _build():
    names = ["fr_add", "fr_sub", "fr_neg", "fr_dbl", "fr_sub_lazy", "fr_dbl_lazy", "fr_add_lazy", "fr_sub2_lazy", "fr_3a_b_c_lazy", "fr_sub3",
             "fr_sub_a_2x", "fr_cond_sub_2p", "fr_cond_sub_4p", "fr_cond_sub_p", "fr_cond_sub_p_rare", "fr_is_zero", "fr_eq", "fr_mul", "fr_sqr",
             "fr_muladd", "fr_muladd2"] + ["fr_dot%d" % n for n in range(1, 7)] + ["fr_dot%d_add" % n for n in range(1, 7)] + [
             "fr_from_canon", "fr_from_u64", "fr_to_canon", "fr_canon_limbs", "fr_pack_canon", "fr_inv", "fr_inv_fermat", "fr_pow"]
    C = {n: i for i, n in enumerate(names)}    # the HZ_FRR_* codes of include/hermez_witness.h, in its order
    A = LIMIT   # the free operand of a lazy sum ("a in [0, A)"): as large as a product takes it
    ops = [
        # fr_add: the sum goes through fr_cond_sub_2p ("t < 4p"); range_check: a + b below 4p
        _sum_op("fr_add", C["fr_add"], (4 * P, 4 * P), lambda t: t[0] + t[1], joint=lambda t: t[0] + t[1] < 4 * P,
                points=[(2 * P, 2 * P), (4 * P, 1), (1, 4 * P), (3 * P, P), (P, 3 * P)]),
        _sum_op("fr_sub", C["fr_sub"], (2 * P, 2 * P), lambda t: t[0] - t[1]),
        _sum_op("fr_neg", C["fr_neg"], (2 * P,), lambda t: -t[0]),
        _sum_op("fr_dbl", C["fr_dbl"], (2 * P,), lambda t: 2 * t[0]),
        # "a - b + 2p in (0, A + 2p) for a in [0, A), b in [0, 2p)": for the operand a itself the interval is (0, a + 2p]
        _lazy_op("fr_sub_lazy", C["fr_sub_lazy"], (A, 2 * P), lambda t: t[0] - t[1], lambda t: t[0] + 2 * P + 1, True),
        _lazy_op("fr_dbl_lazy", C["fr_dbl_lazy"], (A,), lambda t: 2 * t[0], lambda t: 2 * t[0] + 1, False),
        _lazy_op("fr_add_lazy", C["fr_add_lazy"], (A, A), lambda t: t[0] + t[1], lambda t: t[0] + t[1] + 1, False),
        # "a - b - c + 4p in (0, A + 4p) for a in [0, A), b + c < 4p"
        _lazy_op("fr_sub2_lazy", C["fr_sub2_lazy"], (A, 4 * P, 4 * P), lambda t: t[0] - t[1] - t[2], lambda t: t[0] + 4 * P + 1, True,
                 joint=lambda t: t[1] + t[2] < 4 * P, points=[(A, 2 * P, 2 * P), (A, 4 * P, 1), (A, 1, 4 * P), (A, 3 * P, P), (A, P, 3 * P)]),
        _lazy_op("fr_3a_b_c_lazy", C["fr_3a_b_c_lazy"], (A, A, A), lambda t: 3 * t[0] + t[1] + t[2], lambda t: 3 * t[0] + t[1] + t[2] + 1, False),
        # "m in [0, 2p), a, b, c in [0, 2p) with a + b + c < 4p"
        _sum_op("fr_sub3", C["fr_sub3"], (2 * P,) * 4, lambda t: t[0] - t[1] - t[2] - t[3], joint=lambda t: t[1] + t[2] + t[3] < 4 * P,
                extra=[(2 * P - 1, 2 * P - 1, 2 * P - 1, 0), (0, 2 * P - 1, 2 * P - 1, 0), (0, 0, 2 * P - 1, 2 * P - 1), (2 * P - 1, 2 * P - 1, 0, 2 * P - 1),
                       (2 * P - 1, 0, 0, 0), (0, 2 * P - 1, P, P), (0, P, P, 2 * P - 1)],
                points=[(2 * P, 2 * P, 2 * P, 1), (2 * P, 2 * P, 1, 2 * P), (2 * P, 1, 2 * P, 2 * P), (2 * P, 2 * P, P, P), (2 * P, P, 2 * P, P),
                        (2 * P, P, P, 2 * P)]),
        _sum_op("fr_sub_a_2x", C["fr_sub_a_2x"], (2 * P,) * 3, lambda t: t[0] - t[1] - 2 * t[2]),
        _sum_op("fr_cond_sub_2p", C["fr_cond_sub_2p"], (4 * P,), lambda t: t[0]),
        _sum_op("fr_cond_sub_4p", C["fr_cond_sub_4p"], (8 * P,), lambda t: t[0], bound=4 * P),
        Op("fr_cond_sub_p", C["fr_cond_sub_p"], ["fr"], (2 * P,), req_exact_limbs(lambda t: t[0] % P), bound=lambda t: P),
        Op("fr_cond_sub_p_rare", C["fr_cond_sub_p_rare"], ["fr"], (2 * P,), req_exact_limbs(lambda t: t[0] % P), bound=lambda t: P),
        Op("fr_is_zero", C["fr_is_zero"], ["fr"], (2 * P,), req_bool(lambda t: t[0] % P == 0)),
        Op("fr_eq", C["fr_eq"], ["fr", "fr"], (2 * P, 2 * P), req_bool(lambda t: (t[0] - t[1]) % P == 0)),
        _mont_op("fr_mul", C["fr_mul"], ["fr"] * 2, (LIMIT, LIMIT), lambda t: t[0] * t[1]),
        _mont_op("fr_sqr", C["fr_sqr"], ["fr"], (LIMIT,), lambda t: t[0] * t[0]),
        # "a < p, b and s normalised with b < 2^257, s < 8p"
        _mont_op("fr_muladd", C["fr_muladd"], ["fr"] * 3, (P, LIMIT, 8 * P), lambda t: t[0] * t[1] + t[2] * R),
        _mont_op("fr_muladd2", C["fr_muladd2"], ["fr"] * 5, (P, LIMIT, P, LIMIT, 8 * P), lambda t: t[0] * t[1] + t[2] * t[3] + t[4] * R),
    ]
    for n in range(1, 7):     # every operand of every product below 2^257; the all-maximal tuple of fr_dot<6> is the tightest accumulator
        ops.append(_mont_op("fr_dot%d" % n, C["fr_dot%d" % n], ["fr"] * (2 * n), (LIMIT,) * (2 * n), _dot_T(n, False),
                            extra=[(LIMIT - 1,) * (2 * n)]))
    for n in range(1, 7):     # "`addend` is a value < p in 29-bit limbs"
        ops.append(_mont_op("fr_dot%d_add" % n, C["fr_dot%d_add" % n], ["fr"] * (2 * n + 1), (LIMIT,) * (2 * n) + (P,), _dot_T(n, True),
                            extra=[(LIMIT - 1,) * (2 * n) + (P - 1,)]))
    ops += [
        # "also accepts any 256-bit integer": T = c R^2
        _mont_op("fr_from_canon", C["fr_from_canon"], ["fc"], (1 << 256,), lambda t: t[0] * R2),
        _mont_op("fr_from_u64", C["fr_from_u64"], ["u64"], (1 << 64,), lambda t: t[0] * R2),
        # "(a + m p)/R <= p": holds for a <= R, the range range_check states for fr_canon_limbs; fr_to_canon is the same reduction
        Op("fr_to_canon", C["fr_to_canon"], ["fr"], (LIMIT,), req_exact_fc(lambda t: t[0] * RINV % P)),
        Op("fr_canon_limbs", C["fr_canon_limbs"], ["fr"], (LIMIT,), req_exact_limbs(lambda t: t[0] * RINV % P), bound=lambda t: P),
        Op("fr_pack_canon", C["fr_pack_canon"], ["fr"], (P,), req_exact_fc(lambda t: t[0])),
        # "value of a (< 2p, normalised)"
        Op("fr_inv", C["fr_inv"], ["fr"], (2 * P,), _req_inv, bound=lambda t: 2 * P),
        Op("fr_inv_fermat", C["fr_inv_fermat"], ["fr"], (2 * P,), _req_inv, bound=lambda t: 2 * P),
        # a is a multiplicand: below 2^257; "a public 256-bit exponent given as 8 LE limbs"
        Op("fr_pow", C["fr_pow"], ["fr", "fc"], (LIMIT, 1 << 256), _req_pow, edges=[[e for e in EDGES if e < LIMIT], list(EDGES_EXP)]),
    ]
    assert [o.code for o in ops] == list(range(len(names))) and [o.name for o in ops] == names
    return {o.name: o for o in ops}


OPS = _build()
N_OPS = len(OPS)    # HZ_FRR_COUNT


# ---- wavefront scenarios (device only): whole launches whose element -> lane mapping matters -----------------------------------------
def _below_top(rng):
    """a value whose top limb is below p's: no lane of such a wavefront can be >= p"""
    return rng.randrange(P_TOP << 232)


@functools.lru_cache(maxsize=None)
def wave_scenarios(name):
    """[(label, tuples)]: each is one launch, element i on lane i % 64 of wavefront i // 64"""
    rng = random.Random(_seed(name) + 1)
    sc = []
    if name in ("fr_cond_sub_p_rare", "fr_canon_limbs"):
        # what the routine is given so that the value BEFORE its conditional subtraction is x (below its top limb / >= p / beside p)
        if name == "fr_cond_sub_p_rare":
            low, at_p, top_eq = (lambda: _below_top(rng)), [P, P + 1, 2 * P - 1, P + (1 << 232)], [TOP_EQ, P - 1, P - (1 << 29)]
        else:   # the reduction gives a / R mod p, and exactly p for a multiple of p other than 0
            low, at_p, top_eq = (lambda: _below_top(rng) * R % P), [P, 2 * P, 4 * P, 8 * P], [x * R % P for x in (TOP_EQ, P - 1, P - (1 << 29))]
        sc.append(("skip taken: 4 wavefronts, every top limb below p's", [(low(),) for _ in range(256)]))
        for lane in (0, 17, 63):
            for v in at_p:
                w = [(low(),) for _ in range(192)]
                w[64 + lane] = (v,)
                sc.append(("one lane at or above p (%s) on lane %d of wavefront 1" % (in_p(v), lane), w))
        for v in top_eq:
            w = [(low(),) for _ in range(128)]
            w[64 + 29] = (v,)
            sc.append(("one lane with p's top limb, below p: branch entered, nothing subtracted", w))
        for n in (129, 191):     # ragged tails: n = 1 and 63 mod 64
            w = [(low(),) for _ in range(n)]
            sc.append(("ragged tail n = %d, skip taken" % n, list(w)))
            w[n - 1] = (at_p[0],)
            sc.append(("ragged tail n = %d, its last lane at p" % n, w))
        sc.append(("a whole wavefront at or above p", [(at_p[i % len(at_p)],) for i in range(64)]))
    if name == "fr_inv":
        sc.append(("a whole wavefront of 0 and p: g = 0 from the first batch", [((0, P)[i & 1],) for i in range(64)]))
        sc.append(("a whole wavefront of 0", [(0,)] * 64))
        mix = [0, P, 1, P - 1, P + 1, 2 * P - 1] + [1 << k for k in range(1, 254)]
        w = []
        for i in range(512):
            w.append((mix[(i * 7) % len(mix)] if i % 3 else rng.randrange(2 * P),))
        sc.append(("lanes that finish early beside lanes that have not", w))
        w = [(rng.randrange(2 * P),) for _ in range(64)]
        for lane, v in ((0, 0), (17, P), (63, 1), (31, 1 << 253)):
            w[lane] = (v,)
        sc.append(("random lanes with 0, p, 1, 2^253 among them", w))
        sc.append(("ragged tail n = 65 of powers of two", [(1 << (i * 3 % 254),) for i in range(65)]))
        sc.append(("one wavefront of a single repeated random value", [(rng.randrange(P),)] * 64))
    for label, tuples in sc:
        for t in tuples:
            assert OPS[name].pre(t), (name, label, t)
    return tuple((label, tuple(t)) for label, t in sc)


# ---- the host runner -------------------------------------------------------------------------------------------------------------------
def build_host_runner(exe, src=None, flags=("-O2",)):
    import os
    import subprocess
    src = src or os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "fr_contract_host.cpp")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wno-unknown-pragmas", src, "-o", exe])
    return exe


def run_host(exe, op, arr):
    """arr: uint32[n_operands][n][9] -> uint32[n][9] through the host compile of the same dispatch"""
    import subprocess
    head = np.array([op.code, arr.shape[1], arr.shape[0]], dtype="<u4").tobytes()
    r = subprocess.run([exe], input=head + arr.astype("<u4").tobytes(), capture_output=True)
    assert r.returncode == 0, "%s: host runner exit %d: %s" % (op.name, r.returncode, r.stderr.decode()[-2000:])
    return np.frombuffer(r.stdout, dtype="<u4").reshape(-1, 9)
