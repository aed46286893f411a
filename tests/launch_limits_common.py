"""Shared by tests/test_launch_limits.py (GPU) and tests/test_launch_limits_cpu.py: inputs, references and the audit table of every
launch cap, grid.y cut and chunk constant of circuits_amd/csrc (NOTES lesson 26: a size switch in a launcher needs a test on each side).

One technique keeps a launch of half a million elements as cheap to check as one of a thousand: the inputs are PERIODIC with a prime
period that is no multiple of the wavefront -- row i holds case i % period, PERIOD_FR = 1009 for rows of field elements, PERIOD_INST =
1013 for instances -- so the expected result is the reference's answer for the `period` distinct cases, tiled (tile / tile_index: numpy
or torch indexing, never a Python loop over instances), and the comparison covers EVERY element of the large launch. A kernel that
skips, repeats or misplaces part of its range puts case j where case k belongs, and j != k (mod period) for every displacement that
is no multiple of the period -- in particular for a multiple of 64, 256 or 2048 * 256 below it."""
import os
import random
import re

import numpy as np

import fuzz_common as FZ
from oracle_binding import OracleCtx, P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "circuits_amd", "csrc")

PERIOD_FR, PERIOD_INST = 1009, 1013
CAP = 2048 * 256                      # the element-wise launchers: 2048 workgroups of 256 lanes, a grid-stride loop beyond
N_AT_CAP, N_PAST_CAP = CAP, CAP + 256 + 1   # no second pass; a whole workgroup and one ragged lane in the second pass
N_FR = CAP + 257
GRID_Y = 65535                        # scatter_staged_inputs (the head of enqueue_impl) cuts a run of staged instances here
B_STAGE = 2 * GRID_Y + 7              # runs of 65535, 65535 and 7
EXPORT_CH = 32768                     # hz_witness_export_range_dev's chunk of instances
B_EXPORT = 2 * EXPORT_CH + 5
MUX_B = (2048, 2049, 2052)            # in[256]: 524288 elements (one pass), then a second pass of 256 and of 1024 elements
FILL = 0xA5                           # 0xA5A5...A5 is no field element: a slot nobody wrote cannot pass for a value
NSBOX = {t: 8 * t + [56, 57, 56, 60, 60, 63][t - 2] for t in range(2, 8)}
GIB16 = 16 << 30

# every context the GPU file creates: (template, shape keywords, instances). hz_template_device_bytes of each stays below 16 GiB
# (test_launch_limits_cpu.py; no device needed).
CONTEXTS = [("mux256", {}, b) for b in MUX_B] + [("decode-float", {}, B_STAGE), ("hash-state", {}, B_EXPORT), ("hash-state", {}, EXPORT_CH)]
# Withdraw past k_transpose32's cap: siblingsState is (nLevels + 1) * B elements, so B = 524288 / (nLevels + 1) + 1 instances of 2.4 MB
# each (the SHA-256 bit witness of hashGlobalInputs, whatever nLevels) -- 24.6 GiB at nLevels = 48 and still 19.7 GiB at nLevels = 63,
# the deepest the template takes. No shape crosses the cap below 16 GiB, so there is no such test; Mux256 crosses the same transpose.
WITHDRAW_PAST_CAP = [(48, 10703), (63, 8193)]


# ---- tiling ------------------------------------------------------------------------------------------------------------------------------
def tile_index(n, period, shift=0):
    """which case element i of a launch of n holds: (i + shift) % period"""
    return (np.arange(n, dtype=np.int64) + shift) % period


def tile(a, n, shift=0):
    """a[period, ...] -> [n, ...], row i = a[(i + shift) % period]"""
    return np.ascontiguousarray(a[tile_index(n, len(a), shift)])


def fr_rows(vals):
    """integers -> uint8[n, 32], little endian, reduced mod P"""
    return np.frombuffer(b"".join(int(v % P).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


def raw_rows(vals):
    """integers below 2^256 as they are (an element >= r among them) -> uint8[n, 32]"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


def row_int(r):
    return int.from_bytes(np.asarray(r, dtype=np.uint8).tobytes(), "little")


EDGES = (0, P - 1, (1 << 253) + 5, 1, 2, P - 2, (P - 1) // 2, (P + 1) // 2, 1 << 253, (1 << 253) - 1, (1 << 29) - 1, (1 << 232) - 1)


def field_cases(period, seed, width=1):
    """`period` rows of `width` field elements: every edge in every column at once, one edge in one column of a random row, then
    fuzz_common.garbage over random elements"""
    rng = random.Random(seed)
    rows = [[e] * width for e in EDGES]
    for e in EDGES[:4]:
        for j in range(width):
            r = [rng.randrange(P) for _ in range(width)]
            r[j] = e
            rows.append(r)
    while len(rows) < period:
        rows.append([FZ.garbage(rng, rng.randrange(P)) if rng.random() < 0.3 else rng.randrange(P) for _ in range(width)])
    return rows[:period]


# ---- 1: element-wise kernels ---------------------------------------------------------------------------------------------------------------
def poseidon_reference(oracle, t, witness):
    """(inputs uint8[1009, t - 1, 32], digests uint8[1009, 32], S-box signals uint8[3 nsbox, 1009, 32] or None) from the oracle"""
    rows = field_cases(PERIOD_FR, 0x11C0 + t, t - 1)
    dig, wit = oracle.poseidon_batch(t, rows, witness=witness)
    w = np.frombuffer(wit, dtype=np.uint8).reshape(3 * NSBOX[t], PERIOD_FR, 32).copy() if witness else None
    return fr_rows([x for r in rows for x in r]).reshape(PERIOD_FR, t - 1, 32), fr_rows(dig), w


HZ_FR_MUL, HZ_FR_INV, HZ_FR_MULADD, HZ_FR_SQRT = 2, 4, 5, 7
HALF = (P - 1) // 2


def _sqrt_required(x):
    """test_hip_field_ops_against_python_bigints' requirement, which names one value: the root <= (r - 1) / 2, 0 for a non-residue"""
    r = FZ.fr_sqrt(x)
    if r is None:
        return 0
    r = min(r, P - r)
    assert r * r % P == x % P and r <= HALF
    return r


FR_OPS = {
    "mul": (HZ_FR_MUL, True, lambda x, y: x * y % P),
    "muladd": (HZ_FR_MULADD, True, lambda x, y: (x * y + x + y) % P),
    "inv": (HZ_FR_INV, False, lambda x, y: pow(x, P - 2, P)),
    "sqrt": (HZ_FR_SQRT, False, lambda x, y: _sqrt_required(x)),
}


def fr_ops_reference(name):
    """(a uint8[1009, 32], b or None, expected uint8[1009, 32]) for one hz_fr_ops operation, Python integers"""
    rows = field_cases(PERIOD_FR, 0xF0 + FR_OPS[name][0], 2)
    if name == "sqrt":   # half of the operands squares, with the edges among the rest
        rows = [[r[0] * r[0] % P if i % 2 else r[0], 0] for i, r in enumerate(rows)]
    _, two, f = FR_OPS[name]
    return fr_rows([r[0] for r in rows]), fr_rows([r[1] for r in rows]) if two else None, fr_rows([f(r[0], r[1]) for r in rows])


def fr_raw_reference(name="fr_mul"):
    """(op, the first 1009 operand tuples of fr_contract_common's list -- the cross product of the edges first --, packed uint32[k, 1009, 9])"""
    import fr_contract_common as FC
    op = FC.OPS[name]
    tuples = FC.operands(name)[:PERIOD_FR]
    return op, tuples, FC.pack_operands(op, tuples)


def judge_raw_tiled(op, tuples, out, who):
    """every element of a tiled launch against the op's requirement: element i ran tuple i % period, and the distinct (tuple, result)
    pairs of the whole output are judged one by one (a deterministic routine leaves `period` of them)"""
    import fr_contract_common as FC
    n = len(out)
    keyed = np.concatenate([tile_index(n, len(tuples)).astype(np.uint32)[:, None], out], axis=1)
    pairs = np.unique(keyed, axis=0)
    assert len(pairs) >= len(tuples)
    FC.judge(op, [tuples[int(k)] for k in pairs[:, 0]], pairs[:, 1:], who)
    return len(pairs)


# ---- 2, 3, 4: instanced mains ------------------------------------------------------------------------------------------------------------
def mux256_cases():
    return FZ.mux256_cases(PERIOD_INST, 0x256)


def decode_float_cases():
    return FZ.decode_float_cases(PERIOD_INST, 0xDF)


def hash_state_cases():
    return FZ.hash_state_cases(PERIOD_INST, 0x45)


class MainTile:
    """the oracle over the `period` cases of one main, one instance each: the raw buffer as uint8[signals, period, 32], the first
    failure of every rejected case, and the cases' inputs as uint8[period, flat length, 32] per input signal"""

    def __init__(self, template, cases, kw=None):
        kw = kw or {}
        self.template, self.cases, self.n = template, cases, len(cases)
        self.o = o = OracleCtx(template, kw.get("nTx", 0), kw.get("nLevels", 0), kw.get("maxL1Tx", 0), kw.get("maxFeeTx", 0), n_instances=self.n)
        self.inputs = {}
        for name in cases[0]:
            flat = [FZ.flatten(c[name]) for c in cases]
            self.inputs[name] = fr_rows([x for f in flat for x in f]).reshape(self.n, len(flat[0]), 32)
            assert o.o.c.orc_set_input(o.h, -1, name.encode(), self.inputs[name].tobytes(), self.n * len(flat[0])) == 0
        self.first = o.run()
        self.wl = o.witness_len()
        assert o.total() == self.wl * self.n
        self.raw = np.frombuffer(o.read_raw_bytes(), dtype=np.uint8).reshape(self.wl, self.n, 32).copy()
        # hz_error's members per case; `failed` marks the cases that have one
        self.fail = np.zeros(self.n, dtype=ERR_DTYPE)
        self.failed = np.zeros(self.n, dtype=bool)
        for k in range(self.n):
            f = o.failure_of(k)
            if f is not None:
                self.failed[k] = True
                self.fail[k] = (0, f[0], f[1], list(f[2].to_bytes(32, "little")), list(f[3].to_bytes(32, "little")))

    def expected_raw(self, which):
        """the physical buffer of a launch whose instance k holds case which[k]: signal s of instance k at s * B + k
        (hermez_witness.h, "The physical buffer") -> uint8[signals, B, 32]"""
        return self.raw[:, which, :]

    def expected_failures(self, which):
        """hz_witness_failures' records of that launch: one per rejected instance, in instance order (the unit counts within the instance)"""
        which = np.asarray(which)
        inst = np.nonzero(self.failed[which])[0]
        out = self.fail[which[inst]].copy()
        out["instance"] = inst
        return out


ERR_DTYPE = np.dtype([("instance", "<i4"), ("unit", "<i4"), ("constraint_id", "<i4"), ("lhs", "u1", (32,)), ("rhs", "u1", (32,))])
assert ERR_DTYPE.itemsize == 76   # capi.hz_error


def physical_layout(values, B):
    """the numpy statement of the layout for ONE input signal set for every instance: values uint8[B, flat, 32] (instance-major, as
    hz_set_input takes them) -> uint8[flat, B, 32], element j of instance k at (first signal + j) * B + k"""
    assert values.shape[0] == B
    return np.ascontiguousarray(values.transpose(1, 0, 2))


def mix_per_window(failed, window=64):
    """(fewest, most) rejected cases over every `window` consecutive instances of the tiled sequence (cyclic: a window may span the
    seam between two periods)"""
    f = np.asarray(failed, dtype=np.int64)
    c = np.concatenate([[0], np.cumsum(np.concatenate([f, f[:window]]))])
    counts = c[window:window + len(f)] - c[:len(f)]
    return int(counts.min()), int(counts.max())


# ---- 5: hz_poseidon_dag --------------------------------------------------------------------------------------------------------------------
DAG_UNUSED = 0xFFFFFFFF
PATTERN = np.full(32, FILL, dtype=np.uint8)


class Dag:
    """a table and its segments for hz_poseidon_dag: vals uint8[n, 32], job_in uint32[jobs, 6], job_out uint32[jobs], segments"""

    def __init__(self, vals, job_in, job_out, segs):
        self.vals = np.ascontiguousarray(vals, dtype=np.uint8)
        self.job_in = np.ascontiguousarray(job_in, dtype=np.uint32).reshape(-1, 6)
        self.job_out = np.ascontiguousarray(job_out, dtype=np.uint32)
        self.seg_t = np.array([s[0] for s in segs], dtype=np.uint32)
        self.seg_first = np.array([s[1] for s in segs], dtype=np.uint64)
        self.seg_count = np.array([s[2] for s in segs], dtype=np.uint64)

    def well_formed(self):
        """what the kernel needs of a segment whose jobs run at once: distinct outputs, and no job reads another job's output"""
        n = len(self.vals)
        for t, first, count in zip(self.seg_t, self.seg_first, self.seg_count):
            first, count, t = int(first), int(count), int(t)
            assert 2 <= t <= 7 and first + count <= len(self.job_out)
            ins, outs = self.job_in[first:first + count, :t - 1], self.job_out[first:first + count]
            assert ins.max(initial=0) < n and outs.max(initial=0) < n and len(set(outs.tolist())) == count
            mine = np.repeat(outs[:, None], t - 1, axis=1)
            assert not np.isin(ins[ins != mine], outs).any()
        return True

    def reference(self, oracle):
        """oracle.poseidon_batch job by job, in segment order, over a copy of the table -> uint8[n, 32]"""
        v = self.vals.copy()
        for t, first, count in zip(self.seg_t, self.seg_first, self.seg_count):
            first, count, t = int(first), int(count), int(t)
            if not count:
                continue
            ins = self.job_in[first:first + count, :t - 1]
            rows = [[row_int(v[j]) for j in r] for r in ins]
            dig, _ = oracle.poseidon_batch(t, rows)
            v[self.job_out[first:first + count]] = fr_rows(dig)
        return v


def dag_pool(rng, n):
    """n known values: 0, p - 1, 2^253 + 5, then random elements"""
    return [0, P - 1, (1 << 253) + 5][:n] + [rng.randrange(P) for _ in range(max(0, n - 3))]


DAG_COUNTS = (1, 63, 64, 65, 129)
DAG_FIRSTS = (0, 77)


def dag_single(t, count, first, seed):
    """one segment of width t: jobs first .. first + count - 1 read a pool of known values (0 and p - 1 among them, one job with one
    value in every input) and write a slot each; the `first` jobs in front of it are whole, valid jobs of their own slots that NO
    segment names: their slots keep the pattern. The unused columns of the segment's jobs hold 0xFFFFFFFF."""
    rng = random.Random(seed)
    n_pool, n_jobs = 24, first + count
    vals = np.concatenate([fr_rows(dag_pool(rng, n_pool)), np.tile(PATTERN, (n_jobs, 1))])
    job_in = np.array([[rng.randrange(n_pool) for _ in range(6)] for _ in range(n_jobs)], dtype=np.uint32)
    job_in[first] = 0 if count == 1 else 1             # 0 (or p - 1) in every input
    if count > 2:
        job_in[first + 1], job_in[first + 2] = 0, 5    # 0 everywhere; one random value repeated in every input
    job_in[first:, t - 1:] = DAG_UNUSED
    return Dag(vals, job_in, n_pool + np.arange(n_jobs), [(t, first, count)])


def dag_chain(seed, n_segs=40):
    """`n_segs` segments of mixed widths and sizes; every job of segment g reads digests segment g - 1 wrote (segment 0: the pool).
    Segment 5's job 0 writes the slot it alone reads; segment 12's job 1 writes the slot segment 10's job 0 wrote, which segment 13 reads."""
    rng = random.Random(seed)
    n_pool = 16
    counts = [rng.choice((1, 3, 17, 63, 64, 65, 100, 130)) for _ in range(n_segs)]
    if n_segs > 12:
        counts[10] = counts[12] = 65
    widths = [2 + (g * 5 + 3) % 6 for g in range(n_segs)]
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n_jobs = int(first[-1])
    slot0 = n_pool
    job_in = np.full((n_jobs, 6), DAG_UNUSED, dtype=np.uint32)
    job_out = (slot0 + np.arange(n_jobs)).astype(np.uint32)
    prev = list(range(n_pool))
    for g in range(n_segs):
        t, f0 = widths[g], int(first[g])
        src = list(prev)
        own = src.pop(0) if g == 5 and len(src) > 1 else None   # nobody else in segment 5 reads it
        for i in range(counts[g]):
            job_in[f0 + i, :t - 1] = [rng.choice(src) for _ in range(t - 1)]
        if own is not None:
            job_in[f0, 0] = job_out[f0] = own
        if g == 12:
            job_out[f0 + 1] = job_out[int(first[10])]
        if g == 13:
            job_in[f0, 0] = job_out[int(first[10])]   # what segment 12 left there
        prev = [int(s) for s in job_out[f0:int(first[g + 1])]]
    vals = np.concatenate([fr_rows(dag_pool(rng, n_pool)), np.tile(PATTERN, (n_jobs, 1))])
    return Dag(vals, job_in, job_out, [(widths[g], int(first[g]), counts[g]) for g in range(n_segs)])


def dag_small(seed):
    """a table of 8 values: 5 known ones, 3 jobs in two segments"""
    rng = random.Random(seed)
    vals = np.concatenate([fr_rows([rng.randrange(P) for _ in range(5)]), np.tile(PATTERN, (3, 1))])
    job_in = np.full((3, 6), DAG_UNUSED, dtype=np.uint32)
    job_in[0, :2], job_in[1, :1], job_in[2, :4] = [0, 1], [2], [5, 6, 3, 4]
    return Dag(vals, job_in, [5, 6, 7], [(3, 0, 1), (2, 1, 1), (5, 2, 1)])


DAG_BIG = 1 << 18


def dag_big(oracle):
    """a table of 2^18 values: the first 2^17 periodic with period 1009, job i hashes values i and i + 1 into slot 2^17 + i
    -> (Dag, expected table): the digests are the oracle's 1009 distinct ones, tiled"""
    half = DAG_BIG // 2
    base = field_cases(PERIOD_FR, 0xDA6, 1)
    known = fr_rows([r[0] for r in base])
    n_jobs = half - 1
    vals = np.concatenate([tile(known, half), np.tile(PATTERN, (half, 1))])
    i = np.arange(n_jobs, dtype=np.uint32)
    job_in = np.full((n_jobs, 6), DAG_UNUSED, dtype=np.uint32)
    job_in[:, 0], job_in[:, 1] = i, i + 1
    d = Dag(vals, job_in, half + i, [(3, 0, n_jobs)])
    dig, _ = oracle.poseidon_batch(3, [[base[r][0], base[(r + 1) % PERIOD_FR][0]] for r in range(PERIOD_FR)])
    exp = vals.copy()
    exp[half:half + n_jobs] = tile(fr_rows(dig), n_jobs)
    return d, exp


def dag_thread_tables(caller, n_calls=16):
    """the tables of one of the two callers: short chains, every one different"""
    return [dag_chain(0x7C00 + 97 * caller + k, n_segs=3 + (k + caller) % 4) for k in range(n_calls)]


def dag_via_hasher(oracle, leaves):
    """a small binary tree through builder.DagHasher (the batch builders' route): its evaluate() hands over a table, which this module's
    reference evaluates -> (root by the reference, root hashed directly with the oracle)"""
    from circuits_amd import builder as B

    def evaluate(vals, job_in, job_out, seg_t, seg_first, seg_count):
        d = Dag(np.frombuffer(bytes(vals), dtype=np.uint8).reshape(-1, 32), job_in, job_out, list(zip(seg_t, seg_first, seg_count)))
        assert d.well_formed()
        vals[:] = d.reference(oracle).tobytes()
        return None
    h = B.DagHasher(evaluate)
    level = list(leaves)
    direct = list(leaves)
    while len(level) > 1:
        level = [h.poseidon([level[i], level[i + 1]]) for i in range(0, len(level), 2)]
        direct = oracle.poseidon_batch(3, [[direct[i], direct[i + 1]] for i in range(0, len(direct), 2)])[0]
    return h.resolve()(level[0]), direct[0]


# ---- 6: the audit table ------------------------------------------------------------------------------------------------------------------
AUDIT_PATTERNS = [r"blocks > [0-9]", r"std::min<[^>]*>\([^;]*,\s*(2048|4096)\)", r"\b65535u?\b", r"\b32768\b", r"1u << 21\b", r"1u << 22\b", r"block_cap\(\)"]
_T = "tests/test_launch_limits.py::"
# one row per source line that holds a launch cap or a chunk constant: (file, text found in that line, the limit, the test that stands
# on the far side of it -- or the reason none does)
AUDIT = [
    ("poseidon_kernels.hip", "if (blocks > 256 * 8) blocks = 256 * 8;", "launch_poseidon: 2048 x 256 lanes, grid-stride beyond 524288 permutations",
     _T + "test_poseidon_digests_past_the_grid_cap, test_poseidon_witness_past_the_grid_cap"),
    ("poseidon_kernels.hip", "if (blocks > 2048) blocks = 2048;", "hz_fr_ops (fr_ops_kernel): 524288 elements a pass", _T + "test_fr_ops_past_the_grid_cap"),
    ("eddsa_kernels.hip", "if (blocks > 2048) blocks = 2048;", "launch_fr_sqrt: 524288 elements a pass", _T + "test_fr_ops_past_the_grid_cap[sqrt]"),
    ("fr_raw_ops.h", "if (blocks > 2048) blocks = 2048;", "hz_fr_raw_ops: 524288 elements a pass, both forms", _T + "test_fr_raw_ops_past_the_grid_cap"),
    ("ctx.hip", "const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 2048);",
     "k_transpose32, twice. instance = -1 (n = B * outer * inner): 524288 elements a pass. instance >= 0 (n = outer * inner of ONE instance)",
     _T + "test_mux256_inputs_from_the_device for instance = -1. The per-instance transpose is UNREACHABLE at any shape the project runs: its "
     "largest input is RollupMain's siblings, nTx * (nLevels + 1) elements, which passes 524288 only from nTx ~ 15 900 at nLevels = 32 "
     "(the headline shape is nTx = 2048). Withdraw at instance = -1: no shape below 16 GiB (WITHDRAW_PAST_CAP)"),
    ("ctx.hip", "while (e < lo.n_inst && c->staged[e] && e - b < 65535u)", "enqueue_impl -> scatter_staged_inputs -> launch_unpack: a run of staged instances is cut at grid.y = 65535",
     _T + "test_stage_range_across_the_grid_y_cut, test_second_step_stages_a_run_across_the_cut, test_range_check_across_the_cut"),
    ("ctx.hip", "const uint64_t chunk = std::min<uint64_t>(count, 1u << 22);", "hz_witness_read: gathers of 2^22 elements",
     "NOT CROSSED: every whole-buffer read of the suite stays below 2^22 elements per instance. It is the suite's own read path: an error "
     "there shows as false failures, not hidden ones"),
    ("ctx.hip", "hipLaunchKernelGGL(k_gather_virtual, dim3((unsigned)std::min<uint64_t>((g.count + 255) / 256, 4096))", "k_gather_virtual: 4096 x 256 lanes a chunk, grid-stride to 2^22",
     "NOT CROSSED by this file: part of hz_witness_read, the suite's own read path (an error shows as false failures); multi-instance reads of the "
     "suite stay below 2^20 elements an instance"),
    ("ctx.hip", "const uint64_t chunk = std::min<uint64_t>(std::max<uint64_t>(count, 1), 1u << 21);", "hz_witness_gather: 2^21 indices a chunk",
     "NOT CROSSED: no caller gathers more than 2^21 elements at once; the suite's own read path, as hz_witness_read"),
    ("ctx.hip", "hipLaunchKernelGGL(k_gather_index, dim3((unsigned)std::min<uint64_t>((g.count + 255) / 256, 4096))", "k_gather_index: 4096 x 256 lanes a chunk, grid-stride to 2^21",
     "NOT CROSSED by this file: part of hz_witness_gather, the suite's own read path, as k_gather_virtual"),
    ("export.hip", "static uint64_t block_cap() {", "2^16 workgroups a launch (HZ_EXPORT_BLOCKS lowers it for experiments)", "definition"),
    ("export.hip", "static unsigned grid_for(uint64_t n, unsigned block)", "k_export_singles_x4 / k_export_dvars / k_phys_index: 2^16 x 256 lanes, the kernels loop beyond",
     "NOT CROSSED: wants a list of more than 2^24 variables; the headline map (tests/test_export_dev.py) has 1.2 x 10^8 variables in several lists, "
     "HashState here 1 886. HZ_EXPORT_BLOCKS is a setting for experiments, not a shape"),
    ("export.hip", "const uint64_t cap = std::max<uint64_t>(3, block_cap() == (1u << 16)", "k_export_stored's shares of 2^16 workgroups", "as grid_for: NOT CROSSED below 2^24 list entries"),
    ("export.hip", "ninst <= 32768", "export_chunk's contract (a comment)", _T + "test_export_across_the_instance_chunk"),
    ("export.hip", "const uint32_t CH = 32768;", "hz_witness_export_range_dev: chunks of 32768 instances", _T + "test_export_across_the_instance_chunk"),
    ("export.hip", "if (instance < 0 && g.n_inst > 32768)", "hz_witness_derive_dev refuses instance = -1 above 32768 instances",
     _T + "test_derive_dev_refuses_more_than_a_chunk, test_derive_dev_at_exactly_a_chunk"),
    ("ledger_l1.h", "balances [8][1024] u32 = 32768 B", "an LDS size in a comment", "no launch limit"),
    ("ledger_select.h", "the want word: 0 .. 65535, or NONE", "a value range of hz_ledger_select_batch", "no launch limit (tests/test_ledger_select.py covers the range)"),
    ("ledger_select.h", "where that lies in 0 .. 65535", "the same range, in a comment", "no launch limit"),
]


def audit_scan():
    """[(file, line number, stripped line)] of every line of a source file in circuits_amd/csrc (generated tables aside) that matches
    one of AUDIT_PATTERNS"""
    pats = [re.compile(p) for p in AUDIT_PATTERNS]
    out = []
    for dirpath, _, files in os.walk(CSRC):
        if os.path.basename(dirpath) in ("gen", "build"):
            continue
        for f in sorted(files):
            if not f.endswith((".hip", ".h", ".cpp")):
                continue
            path = os.path.join(dirpath, f)
            for i, line in enumerate(open(path, encoding="utf-8", errors="replace"), 1):
                if any(p.search(line) for p in pats):
                    out.append((os.path.relpath(path, CSRC), i, line.strip()))
    return out


def audit_unmatched(table=None, scan=None):
    """(source lines no row covers, rows no source line holds)"""
    table = AUDIT if table is None else table
    scan = audit_scan() if scan is None else scan
    loose = [(f, i, line) for f, i, line in scan if not any(r[0] == f and r[1] in line for r in table)]
    stale = [r for r in table if not any(r[0] == f and r[1] in line for f, _, line in scan)]
    return loose, stale
