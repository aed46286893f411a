"""HashInputs (csrc/fee_kernels.hip: k_hi_prep, k_sha_chain / k_sha_chain_w, k_sha_expand) as `component main`, at the block counts and
launch sizes at which the sequential SHA-256 chain takes each of its paths, against a reference that shares nothing with the project:
the message of reference src/hash-inputs.circom put together in Python and hashed by hashlib.

Which kernel form a launch of B instances of a message of `nblocks` SHA-256 blocks runs (ctx_step.hip enqueue_hash_inputs over the launchers of fee_kernels.hip):

  B <= 16            k_sha_chain_w: workgroups of 8 batches (B = 9: a partial second workgroup, B = 16: a full one)
  B >= 17            k_sha_chain: workgroups of 64 batches (17 of 64 lanes, 64: exactly one workgroup, 65: a second one of one batch,
                     130: a third of two), k_sha_expand with cooperative half-wavefront stores where B % 32 == 0 (32, 64)
  nblocks > 8        more than one chunk of 8 blocks: the LDS double buffer of both chain kernels (9: a tail of one block, 17: two flips)
  nblocks >= 64      the launch is split into eight piped groups of per = ceil(nblocks / 8) blocks, each group's chain kernel starting
                     from the chaining value the one before left (64: per = 8, one chunk each; 65: per = 9, groups off the chunk grid, a
                     last group of 2 blocks; 73: per = 10, a last group of 3)

and the two padding edges of nblocks = (totalBits + 64) / 512 + 1 (include/hz_layout.h, shared by the oracle and the HIP path):
totalBits mod 512 = 447 (the last length at which the `1` bit and the 64-bit length fit the message's last block; 440 is the last one
that is a whole number of bytes) and 448 (the first that appends a block holding the length alone).

hashlib hashes whole bytes. The one shape here whose message is not a whole number of bytes, (15, 17, 3, 1) with 4 031 bits, is hashed
by `sha256_of_bits` below, SHA-256 as FIPS 180-4 states it, with its constants derived from the primes as the standard defines them;
test_python_sha256_equals_hashlib holds it to hashlib on every message here that hashlib can take."""
import functools
import hashlib
import math
import random

import numpy as np
import pytest

import fuzz_common as FZ
from oracle_binding import OracleCtx

P = FZ.P
SHA_BLOCK_SIGNALS = 30952   # stored signals of one SHA-256 block of the witness, 0.99 MB per instance
# (nTx, nLevels, maxL1Tx, maxFeeTx): (bits of the message, bits mod 512, SHA-256 blocks)
SHAPES = {
    (13, 22, 3, 2): (4024, 440, 8),       # the last whole-byte length with `1` bit and length in the message's last block
    (15, 17, 3, 1): (4031, 447, 8),       # one full chunk; the last length with `1` bit and length in the last block
    (23, 16, 2, 2): (4032, 448, 9),       # chunk of 8, then a tail of 1; the appended length-only block
    (37, 9, 1, 6): (4032, 448, 9),        # the same edge at an odd nLevels
    (75, 16, 2, 2): (8192, 0, 17),        # chunks 8, 8, 1: the double buffer flips twice
    (375, 16, 2, 2): (32192, 448, 64),    # piped: 8 groups of exactly one chunk
    (382, 16, 2, 2): (32752, 496, 65),    # piped: per = 9, groups start off the chunk grid, the last group is 2 blocks
    (433, 16, 2, 2): (36832, 480, 73),    # piped: per = 10 (a chunk of 8 and a tail of 2 in every group), the last group is 3 blocks
}
PIPED = [s for s, v in SHAPES.items() if v[2] >= 64]
LAUNCHES = (1, 8, 9, 16, 17, 32, 64, 65, 130)
FIRST_SHA_SIGNAL = "main.inputsHasher.sha256compression[%d].sigmaPlus[0].sigma0.xor3.mid[0]"


# ---- the reference: reference src/hash-inputs.circom's message, hashlib's SHA-256 ------------------------------------------------
def message_bits(shape, d):
    L = shape[1]

    def be(v, n):
        return [(v >> (n - 1 - k)) & 1 for k in range(n)]
    bits = be(d["oldLastIdx"], 48) + be(d["newLastIdx"], 48) + be(d["oldStateRoot"], 256) + be(d["newStateRoot"], 256) + be(d["newExitRoot"], 256)
    bits += list(d["L1TxsFullData"]) + list(d["L1L2TxsData"])
    for v in d["feeTxsData"]:
        bits += be(v, L)
    return bits + be(d["globalChainID"], 16) + be(d["currentNumBatch"], 32)


def _primes(n):
    out, k = [], 2
    while len(out) < n:
        if all(k % q for q in out):
            out.append(k)
        k += 1
    return out


def _icbrt(v):
    r = int(round(v ** (1.0 / 3)))
    while r * r * r > v:
        r -= 1
    while (r + 1) ** 3 <= v:
        r += 1
    return r


SHA_H0 = [math.isqrt(q << 64) & 0xFFFFFFFF for q in _primes(8)]    # first 32 bits of the fractional parts of the square roots
SHA_K = [_icbrt(q << 96) & 0xFFFFFFFF for q in _primes(64)]        # ... of the cube roots


def sha256_of_bits(bits):
    """SHA-256 (FIPS 180-4) of a message of any number of bits -> 32 bytes"""
    def rotr(x, n):
        return ((x >> n) | (x << (32 - n))) & 0xFFFFFFFF
    n = len(bits)
    padded = list(bits) + [1] + [0] * ((447 - n) % 512) + [(n >> (63 - k)) & 1 for k in range(64)]
    words = np.packbits(np.array(padded, dtype=np.uint8)).view(">u4").astype(np.uint64).tolist()
    h = list(SHA_H0)
    for b0 in range(0, len(words), 16):
        w = words[b0:b0 + 16]
        for t in range(16, 64):
            s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)
            s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)
            w.append((w[t - 16] + s0 + w[t - 7] + s1) & 0xFFFFFFFF)
        a, b, c, d, e, f, g, hh = h
        for t in range(64):
            t1 = (hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + SHA_K[t] + w[t]) & 0xFFFFFFFF
            t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & 0xFFFFFFFF
            a, b, c, d, e, f, g, hh = (t1 + t2) & 0xFFFFFFFF, a, b, c, (d + t1) & 0xFFFFFFFF, e, f, g
        h = [(x + y) & 0xFFFFFFFF for x, y in zip(h, (a, b, c, d, e, f, g, hh))]
    return b"".join(x.to_bytes(4, "big") for x in h)


def reference_hash(shape, d):
    bits = message_bits(shape, d)
    assert len(bits) == SHAPES[shape][0]
    if len(bits) % 8:
        return int.from_bytes(sha256_of_bits(bits), "big") % P
    return int(hashlib.sha256(np.packbits(np.array(bits, dtype=np.uint8)).tobytes()).hexdigest(), 16) % P


# ---- inputs: every instance of a launch its own, some with all-zero and some with all-one data bits --------------------------------
def _make(shape, n, seed):
    rng = random.Random(seed)
    out = []
    for k in range(n):
        d = FZ.hash_inputs_valid(rng, shape, fill={3: 0, 5: 1}.get(k % 8))
        if k % 8 == 6:   # every scalar at the top of its range as well
            L = shape[1]
            d.update(oldLastIdx=(1 << L) - 1, newLastIdx=(1 << L) - 1 - k, oldStateRoot=P - 1, newStateRoot=P - 1 - k, newExitRoot=P - 2,
                     feeTxsData=[(1 << L) - 1] * shape[3], globalChainID=(1 << 16) - 1, currentNumBatch=(1 << 32) - 1)
        out.append(d)
    return out


@functools.lru_cache(maxsize=None)
def _cases(shape, seed=1):
    """(inputs of 130 instances, their reference hashes): computed once per shape and step, shared by every launch size"""
    cases = _make(shape, max(LAUNCHES), 1000 * seed + sum(shape))
    ref = [reference_hash(shape, d) for d in cases]
    assert len(set(ref)) == len(ref)
    return cases, ref


def _nblocks(ctx):
    """SHA-256 blocks of a hash-inputs context, from the names and the length of its layout"""
    first = ctx.lookup(FIRST_SHA_SIGNAL % 0)
    n, rem = divmod(ctx.witness_len() - first, SHA_BLOCK_SIGNALS)
    assert rem == 0 and ctx.lookup(FIRST_SHA_SIGNAL % (n - 1)) == first + (n - 1) * SHA_BLOCK_SIGNALS
    with pytest.raises(KeyError):
        ctx.lookup(FIRST_SHA_SIGNAL % n)
    return n


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_python_sha256_equals_hashlib():
    assert SHA_H0[0] == 0x6A09E667 and SHA_K[0] == 0x428A2F98 and SHA_K[63] == 0xC67178F2
    rng = random.Random(5)
    for nbytes in (0, 1, 55, 56, 63, 64, 119, 120, 503, 504, 1000):
        msg = bytes(rng.randrange(256) for _ in range(nbytes))
        assert sha256_of_bits(np.unpackbits(np.frombuffer(msg, dtype=np.uint8)).tolist()) == hashlib.sha256(msg).digest()
    for shape, (total, _, _) in SHAPES.items():
        if total % 8 == 0 and total < 10000:
            bits = message_bits(shape, _cases(shape)[0][0])
            assert sha256_of_bits(bits) == hashlib.sha256(np.packbits(np.array(bits, dtype=np.uint8)).tobytes()).digest()


@pytest.mark.parametrize("shape", list(SHAPES), ids=str)
def test_oracle_equals_hashlib_and_block_count(shape):
    """the oracle's hashInputsOut == the reference for several instances (random, all-zero, all-one, top of every range), and the block
    count of the layout the oracle and the HIP path share == the table's, which was worked out from the padding rule of FIPS 180-4"""
    total, mod, nb = SHAPES[shape]
    assert total % 512 == mod and nb == -(-(total + 1 + 64) // 512)
    cases, ref = _cases(shape)
    n = 8 if nb < 64 else 3
    pick = list(range(n)) if nb < 64 else [0, 3, 5]
    o = OracleCtx("hash-inputs", *shape, n_instances=n)
    assert _nblocks(o) == nb
    for k, c in enumerate(pick):
        o.set_inputs(cases[c], instance=k)
    assert o.run() is None
    assert [o.get("main.hashInputsOut", k) for k in range(n)] == [ref[c] for c in pick]


@pytest.mark.parametrize("shape", [(70, 16, 2, 6), (9, 16, 1, 6)], ids=str)
def test_oracle_on_garbage_threads_equal_serial(shape):
    """fuzz_common.hash_inputs_cases makes the mix it claims, the oracle survives it, threads == one thread"""
    n = 96
    cases = FZ.hash_inputs_cases(n, shape, 16)
    parts = FZ.run_oracle_threads("hash-inputs", shape, cases, n_threads=4)
    one = FZ.run_oracle_threads("hash-inputs", shape, cases, n_threads=1)
    fa, fb = FZ.oracle_failures(parts), FZ.oracle_failures(one)
    assert fa == fb and 0 < len(fa) < n
    assert {FZ.constraint_name(v[1]) for v in fa.values()} == {"hashInputs: Num2Bits sum", "hashInputs: index padding === 0"}
    assert all(v[0] == 0 for v in fa.values())
    # the generator's own count of failing elements agrees with the oracle's verdict, instance by instance
    assert {k for k, d in enumerate(cases) if FZ.hash_inputs_lowest_failures(d, shape)} == set(fa)
    o1 = one[0][0]
    for o, lo, cnt in parts:
        for k in (0, cnt - 1):
            assert o.read_bytes(0, o.witness_len(), k) == o1.read_bytes(0, o1.witness_len(), lo + k)
        assert o.unwritten()[0] == 0   # a rejected witness is still complete
    # the mix over as many cases as the GPU test draws: more than half rejected, at least a tenth double failures with equal keys
    many = FZ.hash_inputs_cases(2048, shape, 17)
    counts = [FZ.hash_inputs_lowest_failures(d, shape) for d in many]
    assert sum(c > 0 for c in counts) > 1024 and sum(c == 0 for c in counts) > 100 and sum(c >= 2 for c in counts) >= 205


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _launch(hz, shape, B, cases, g=None):
    g = g or hz.ctx("hash-inputs", nTx=shape[0], nLevels=shape[1], maxL1Tx=shape[2], maxFeeTx=shape[3], n_instances=B)
    FZ.set_all_inputs(g, cases[:B])
    g.run()
    return g


def _digests(g, B):
    row = g.lookup("main.hashInputsOut")   # physical layout [signal][instance]
    raw = g.read_raw_bytes(row * B, B)
    return [int.from_bytes(raw[32 * k:32 * k + 32], "little") for k in range(B)]


def _compare_instances(g, shape, cases, which):
    """the whole witness of the instances `which` of a launch against an oracle context that holds just those"""
    o = OracleCtx("hash-inputs", *shape, n_instances=len(which))
    for j, k in enumerate(which):
        o.set_inputs(cases[k], instance=j)
    assert o.run() is None
    wl = o.witness_len()
    assert wl == g.witness_len()
    for j, k in enumerate(which):
        for first in range(0, wl, 1 << 18):
            c = min(1 << 18, wl - first)
            assert g.read_bytes(first, c, k) == o.read_bytes(first, c, j), "instance %d, elements from %d" % (k, first)


# witness bytes of a launch: drop what would need more than about 2.5 GB (the piped shapes at B >= 64)
DIGEST_ROWS = [(s, B) for s in SHAPES for B in LAUNCHES if SHAPES[s][2] * B * SHA_BLOCK_SIGNALS * 32 < 2.5e9]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,B", DIGEST_ROWS, ids=lambda v: str(v).replace(" ", ""))
def test_hip_digest_equals_hashlib(hz, shape, B):
    """main.hashInputsOut of EVERY instance of the launch == hashlib's SHA-256 of the circuit's message, mod r"""
    assert all((s, B) in DIGEST_ROWS for s in PIPED for B in (17, 32))
    cases, ref = _cases(shape)
    g = _launch(hz, shape, B, cases)
    assert g.sha_blocks() == SHAPES[shape][2] == _nblocks(g)
    assert _digests(g, B) == ref[:B]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,B,which", [
    ((23, 16, 2, 2), 65, None),
    ((15, 17, 3, 1), 64, None),
    ((75, 16, 2, 2), 33, None),
    ((382, 16, 2, 2), 17, (0, 15, 16)),        # (lane 16 is the last)
    ((375, 16, 2, 2), 32, (0, 15, 16, 31)),    # piped, with k_sha_expand's cooperative stores
], ids=lambda v: str(v).replace(" ", ""))
def test_hip_whole_buffer_equals_oracle(hz, shape, B, which):
    """the whole physical buffer bit for bit -- chain[] at every block, through k_sha_expand: every instance of the three unpiped rows, the
    instances in lanes 0, 15, 16 and the last of the two piped ones"""
    cases, ref = _cases(shape)
    g = _launch(hz, shape, B, cases)
    assert _digests(g, B) == ref[:B] and g.failures() == []
    if which is None:
        parts = FZ.run_oracle_threads("hash-inputs", shape, cases[:B])
        assert all(o.run_result is None for o, _, _ in parts)
        FZ.compare_instanced(g, parts, B)
    else:
        _compare_instances(g, shape, cases, which)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,B,which", [((75, 16, 2, 2), 33, (0, 3, 5, 15, 16, 32)), ((382, 16, 2, 2), 17, (0, 3, 5, 16))], ids=lambda v: str(v).replace(" ", ""))
def test_hip_second_step_through_one_context(hz, shape, B, which):
    """A second step with other inputs through the context of the first: k_hi_prep ORs the message into a buffer that every step must
    have cleared, so the instances whose data bits were all one in the first step (k % 8 == 5) are all zero in the second and the
    other way round (the first step's cases reversed, B - 1 a multiple of 8: lane 3 <-> lane B - 1 - 3 = 5 mod 8)."""
    assert (B - 1) % 8 == 0
    cases, ref = _cases(shape)
    g = _launch(hz, shape, B, cases)
    assert _digests(g, B) == ref[:B]
    cases2, ref2 = cases[:B][::-1], ref[:B][::-1]
    fresh, fref = _cases(shape, seed=2)
    for k in range(0, B, 2):   # and half of the lanes get inputs the context has not seen
        cases2[k], ref2[k] = fresh[k], fref[k]
    assert all(set(cases[k]["L1L2TxsData"]) == {1} and set(cases2[k]["L1L2TxsData"]) == {0} for k in (5,))
    g = _launch(hz, shape, B, cases2, g)
    assert _digests(g, B) == ref2 and g.failures() == []
    _compare_instances(g, shape, cases2, which)


def _fuzz_hash_inputs(hz, shape, n_total, chunk, whole_every):
    """hash_inputs_cases through one context, `chunk` instances a step. Every instance: the first failure (unit, constraint, lhs, rhs) and
    every signal outside the SHA-256 blocks (inputs, Num2Bits outputs, the digest) == the oracle's; every `whole_every`-th instance: the SHA-256
    blocks as well (16 MB each at (70, 16, 2, 6) -- the blocks of all of them are the cost of the oracle and of the compare, and
    test_hip_whole_buffer_equals_oracle has them for every instance of its launches). The oracle runs 256 instances at a time."""
    from circuits_amd import ConstraintError
    g = hz.ctx("hash-inputs", nTx=shape[0], nLevels=shape[1], maxL1Tx=shape[2], maxFeeTx=shape[3], n_instances=chunk)
    head, wl = g.lookup(FIRST_SHA_SIGNAL % 0), g.witness_len()
    rejected, cids, doubles = 0, set(), 0
    for c0 in range(0, n_total, chunk):
        cases = FZ.hash_inputs_cases(chunk, shape, 21000 + c0)
        doubles += sum(FZ.hash_inputs_lowest_failures(d, shape) >= 2 for d in cases)
        packed = [FZ.pack_case(d) for d in cases]
        FZ.set_all_packed(g, packed)
        err = None
        try:
            g.run()
        except ConstraintError as e:
            err = e
        a = np.frombuffer(g.read_raw_bytes(0, head * chunk), dtype=np.uint8).reshape(head, chunk, 32)
        recorded = []
        for s0 in range(0, chunk, 256):
            cnt = min(256, chunk - s0)
            parts = FZ.run_oracle_threads("hash-inputs", shape, cases[s0:s0 + cnt], set_case=lambda o, i, k, s0=s0: FZ.set_packed_case(o, packed[s0 + i], k))
            fails = FZ.oracle_failures(parts)
            recorded.append((_Recorded(fails), s0, cnt))
            for o, lo, n in parts:
                b = np.frombuffer(o.read_raw_bytes(0, head * n), dtype=np.uint8).reshape(head, n, 32)
                assert np.array_equal(a[:, s0 + lo:s0 + lo + n, :], b), "signals before the SHA-256 blocks differ, instances %d..%d" % (c0 + s0 + lo, c0 + s0 + lo + n - 1)
                for k in range(n):
                    if (s0 + lo + k) % whole_every == 0:
                        for first in range(head, wl, 1 << 18):
                            c = min(1 << 18, wl - first)
                            assert g.read_bytes(first, c, s0 + lo + k) == o.read_bytes(first, c, k), "instance %d, elements from %d" % (c0 + s0 + lo + k, first)
        rejected += FZ.check_failures(g, recorded, err)
        cids |= {FZ.constraint_name(v[1]) for r, _, _ in recorded for v in r.fails.values()}
    return rejected, cids, doubles


class _Recorded:
    """the first failures of a slice of oracle instances, kept after the slice's contexts are gone (fuzz_common.oracle_failures reads them)"""

    def __init__(self, fails):
        self.fails = fails

    def failure_of(self, k):
        return self.fails.get(k)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,whole_every", [((70, 16, 2, 6), 32), ((9, 16, 1, 6), 8)], ids=["79-lanes", "17-lanes"])
def test_hip_adversarial_fuzz_hash_inputs(hz, shape, whole_every):
    """Garbage and deliberate double failures through the standalone main, 2 048 instances in two steps of one context. (70, 16, 2, 6):
    79 lanes of k_hi_prep per instance, the header lane and the fee lanes of an instance in different wavefronts; (9, 16, 1, 6): 17 lanes,
    mostly in one. Among the elements of an instance that fail the same constraint the reported operands are those of the first in the
    template's order -- oldLastIdx, newLastIdx, the fee slots, globalChainID, currentNumBatch."""
    n_total = 2048
    rejected, cids, doubles = _fuzz_hash_inputs(hz, shape, n_total, n_total // 2, whole_every)
    assert n_total // 2 < rejected < n_total
    assert cids == {"hashInputs: Num2Bits sum", "hashInputs: index padding === 0"}
    assert doubles * 10 >= n_total


# ---- the same double failures through RollupMain, in each of its schedules ---------------------------------------------------------
MAIN_SHAPE = (64, 16, 8, 4)


@functools.lru_cache(maxsize=None)
def _main_cases():
    """[(label, RollupMain input)]: a valid synthetic batch with two or three of {globalChainID, fee indices of the slots from 1 up} out of
    range. In every one of them the first failure of the batch is a HashInputs constraint (test_rollup_main_double_failures_oracle); the
    other range-checked elements cannot be used for that: an oldLastIdx out of range is rejected by decodeTx.idxChecker of transaction 0,
    a currentNumBatch by its decodeTx.isMaxNumBatchOk and the fee index of slot 0 by feeTx.processor.checkOldInput of that slot, which
    are all unit 0 with a lower constraint id; newLastIdx is computed."""
    from circuits_amd import builder as B
    base = B.synthetic_batch(*MAIN_SHAPE, n_accounts=12, exits=2, seed=77).get_input()
    big, pad = 1 << 48, 1 << 20
    chain = base["globalChainID"]
    edits = [
        ("fee 1 >= 2^48, chainID >= 2^16", {"feeIdxs": {1: 3 * big + 1}, "globalChainID": chain + (5 << 16)}),
        ("fee 1, fee 3 >= 2^48", {"feeIdxs": {1: big + 5, 3: 2 * big + 7}}),
        ("fee 1, fee 2 padding", {"feeIdxs": {1: pad | 3, 2: 7 * pad | 5}}),
        ("fee 1 padding, fee 3 >= 2^48, chainID >= 2^16", {"feeIdxs": {1: 3 * pad | 1, 3: big + 9}, "globalChainID": chain + (1 << 20)}),
    ]
    out = [("valid", base)]
    for label, e in edits:
        d = {k: FZ._copy(v) for k, v in base.items()}
        for k, v in e.items():
            if isinstance(v, dict):
                for j, x in v.items():
                    d[k][j] = x
            else:
                d[k] = v
        out.append((label, d))
    return out


@functools.lru_cache(maxsize=None)
def _main_oracle():
    cases = [d for _, d in _main_cases()]
    o = OracleCtx("rollup-main", *MAIN_SHAPE, n_instances=len(cases))
    for k, d in enumerate(cases):
        o.set_inputs(d, instance=k)
    o.run_result = o.run()
    return o


def test_rollup_main_double_failures_oracle():
    """the cases are what they are meant to be: the valid batch passes, every other one is rejected first by HashInputs (unit 0)"""
    o = _main_oracle()
    assert o.failure_of(0) is None
    names = set()
    for k, (label, _) in enumerate(_main_cases()):
        if k:
            f = o.failure_of(k)
            assert f is not None and f[0] == 0 and FZ.constraint_name(f[1]).startswith("hashInputs: "), (label, f and FZ.constraint_name(f[1]))
            names.add(FZ.constraint_name(f[1]))
    assert len(names) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, 2, 2 | 4], ids=["plain", "latency", "latency-solo"])
def test_hip_rollup_main_double_failures(hz, flags):
    """two or three out-of-range public scalars / fee indices in one batch, through a plain context, one with HZ_FLAG_LATENCY (the header
    lane of k_hi_prep is then a launch of its own, after the fee lanes') and one with HZ_FLAG_LATENCY | HZ_FLAG_SOLO: first failure and
    whole witness of every batch == the oracle's"""
    from circuits_amd import ConstraintError
    o = _main_oracle()
    cases = [d for _, d in _main_cases()]
    g = hz.ctx("rollup-main", nTx=MAIN_SHAPE[0], nLevels=MAIN_SHAPE[1], maxL1Tx=MAIN_SHAPE[2], maxFeeTx=MAIN_SHAPE[3], n_instances=len(cases), flags=flags)
    try:
        FZ.set_all_inputs(g, cases)
        err = None
        try:
            g.run()
        except ConstraintError as e:
            err = e
        assert FZ.check_failures(g, [(o, 0, len(cases))], err) == len(cases) - 1
        wl = o.witness_len()
        assert g.total() == o.total()
        for k in range(len(cases)):
            for first in range(0, wl, 1 << 18):
                c = min(1 << 18, wl - first)
                assert g.read_bytes(first, c, k) == o.read_bytes(first, c, k), "batch %d (%s), elements from %d" % (k, _main_cases()[k][0], first)
    finally:
        g.close()   # flagged contexts one after the other: how many are alive decides the form of their chain kernel
