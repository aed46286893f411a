"""Parity on the FAR side of every grid cap, grid.y cut and instance chunk of the element-wise and plumbing kernels (NOTES lesson 26; the
audit table in tests/launch_limits_common.py names, per source line, the test here that crosses it).

Every launch is tiled from about a thousand distinct cases (period 1009 / 1013, launch_limits_common) and compared bit for bit, EVERY
element, with the reference's answer for those cases: the CPU oracle for Poseidon and the mains, Python integers for the field
operations, fr_contract_common's requirement for the raw routine, the literal route of export_derived_common for derived variables.
Expectations are index-selected tiles, on the device where the launch is large. Every launch is in bounds by construction; the only
refusals exercised are argument and input checks."""
import ctypes
import threading
import time

import numpy as np
import pytest

import launch_limits_common as LL
from oracle_binding import P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64   # rows behind every output that must keep the fill


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _idx(n, period, shift=0):
    import torch
    return (torch.arange(n, device=DEV, dtype=torch.int64) + shift) % period


def _first_diff(got, want):
    """(index of the first differing row, got, want) of two [n, 32] device tensors"""
    import torch
    bad = torch.nonzero((got != want).any(dim=-1).reshape(-1))
    i = int(bad[0])
    g, w = got.reshape(-1, 32)[i].cpu().numpy(), want.reshape(-1, 32)[i].cpu().numpy()
    return i, LL.row_int(g), LL.row_int(w), int(bad.numel())


# ---- 1: element-wise kernels past the grid cap -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [2, 3, 4, 5, 6, 7])
def test_poseidon_digests_past_the_grid_cap(hz, oracle, t):
    """hz_poseidon_batch_dev, digests: n = 524288 (the cap: one pass) and 524288 + 256 + 1 (a whole workgroup and one ragged lane in the
    second pass); every digest against the oracle's tile"""
    import torch
    ins, dig, _ = LL.poseidon_reference(oracle, t, False)
    d_ins, d_dig = _dev(ins), _dev(dig)
    for n in (LL.N_AT_CAP, LL.N_PAST_CAP):
        idx = _idx(n, LL.PERIOD_FR)
        d_in = d_ins[idx].contiguous()
        out = torch.full((n + GUARD, 32), LL.FILL, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        hz.poseidon_batch_dev(t, n, d_in.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        want = d_dig[idx]
        assert torch.equal(out[:n], want), "t = %d, n = %d: digest %d is %d, the oracle's %d (%d differ)" % ((t, n) + _first_diff(out[:n], want))
        assert bool((out[n:] == LL.FILL).all()), "t = %d, n = %d: written behind the last digest" % (t, n)


@pytest.mark.parametrize("t", [3, 7])
def test_poseidon_witness_past_the_grid_cap(hz, oracle, t):
    """the witness form ([3 nsbox][n], the layout bench.py's Poseidon figures are measured on) for the recurrence form (t = 3) and the
    widest pair form (t = 7) at the same two n: every S-box signal and every digest against the oracle's tile, in slabs of signal rows"""
    import torch
    ins, dig, wit = LL.poseidon_reference(oracle, t, True)
    d_ins, d_dig, d_wit = _dev(ins), _dev(dig), _dev(wit)
    rows = 3 * LL.NSBOX[t]
    for n in (LL.N_AT_CAP, LL.N_PAST_CAP):
        idx = _idx(n, LL.PERIOD_FR)
        d_in = d_ins[idx].contiguous()
        out = torch.full((n, 32), LL.FILL, dtype=torch.uint8, device=DEV)
        w = torch.full((rows * n + GUARD, 32), LL.FILL, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        hz.poseidon_batch_dev(t, n, d_in.data_ptr(), out.data_ptr(), w.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(out, d_dig[idx]), "t = %d, n = %d, witness form: digest %d is %d, the oracle's %d (%d differ)" % ((t, n) + _first_diff(out, d_dig[idx]))
        got = w[:rows * n].view(rows, n, 32)
        for r0 in range(0, rows, 32):
            want = d_wit[r0:r0 + 32][:, idx]
            if not torch.equal(got[r0:r0 + 32], want):
                i, g, e, cnt = _first_diff(got[r0:r0 + 32], want)
                raise AssertionError("t = %d, n = %d: S-box signal row %d of permutation %d is %d, the oracle's %d (%d differ in the slab)" % (t, n, r0 + i // n, i % n, g, e, cnt))
            del want
        assert bool((w[rows * n:] == LL.FILL).all())
        del w, got


@pytest.mark.parametrize("name", list(LL.FR_OPS))
def test_fr_ops_past_the_grid_cap(hz, name):
    """hz_fr_ops at n = 524288 + 257 against Python integers on the tile (fr_ops_kernel's loop; launch_fr_sqrt's for sqrt)"""
    op = LL.FR_OPS[name][0]
    a, b, exp = LL.fr_ops_reference(name)
    n = LL.N_FR
    ta, tb = LL.tile(a, n), (LL.tile(b, n) if b is not None else None)
    out = np.full((n + GUARD, 32), LL.FILL, dtype=np.uint8)
    hz._check(hz.c.hz_fr_ops(0, op, n, ta.ctypes.data_as(ctypes.c_char_p), tb.ctypes.data_as(ctypes.c_char_p) if tb is not None else None,
                             out.ctypes.data_as(ctypes.c_char_p)))
    want = LL.tile(exp, n)
    bad = np.nonzero((out[:n] != want).any(axis=1))[0]
    assert not bad.size, "%s: element %d (case %d) is %d, Python says %d; %d differ" % (
        name, bad[0], bad[0] % LL.PERIOD_FR, LL.row_int(out[bad[0]]), LL.row_int(want[bad[0]]), bad.size)
    assert (out[n:] == LL.FILL).all()


@pytest.mark.parametrize("form", [0, 1], ids=["inline", "out-of-line"])
def test_fr_raw_ops_past_the_grid_cap(hz, form):
    """hz_fr_raw_ops, fr_mul in both forms at the same n: every element against fr_contract_common's requirement for the op"""
    op, tuples, packed = LL.fr_raw_reference("fr_mul")
    n = LL.N_FR
    operands = np.ascontiguousarray(packed[:, LL.tile_index(n, LL.PERIOD_FR), :])
    out = hz.fr_raw_ops(op.code, form, operands)
    LL.judge_raw_tiled(op, tuples, out, "device, form %d, n = %d" % (form, n))


# ---- 2: hz_set_input_dev, every instance at once ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mux_tile():
    return LL.MainTile("mux256", LL.mux256_cases())


@pytest.mark.parametrize("B", LL.MUX_B)
def test_mux256_inputs_from_the_device(hz, mux_tile, B):
    """Mux256 x B, `in` (256 elements an instance) and `s` set with instance = -1 from device tensors: 524288 elements are one pass of
    k_transpose32, 2049 and 2052 instances add a second pass of 256 and of 1024 elements. The input region read back == the numpy
    statement of the layout; after run() the whole buffer == the oracle's tile."""
    import torch
    m = mux_tile
    which = LL.tile_index(B, m.n)
    idx = _idx(B, m.n)
    g = hz.ctx("mux256", n_instances=B)
    keep = []
    for name in ("in", "s"):
        d = _dev(m.inputs[name])[idx].contiguous()
        keep.append(d)
        torch.cuda.synchronize()
        g.set_input_dev(name, d.data_ptr(), B * m.inputs[name].shape[1], instance=-1)
    torch.cuda.synchronize()
    for name, first in (("in", "main.in[0]"), ("s", "main.s[0]")):
        s, width = g.lookup(first), m.inputs[name].shape[1]
        got = np.frombuffer(g.read_raw_bytes(s * B, width * B), dtype=np.uint8).reshape(width, B, 32)
        want = LL.physical_layout(m.inputs[name][which], B)
        bad = np.argwhere((got != want).any(axis=2))
        assert not len(bad), "B = %d: element %d of `%s` of instance %d is %d, set %d (%d differ)" % (
            B, bad[0][0], name, bad[0][1], LL.row_int(got[tuple(bad[0])]), LL.row_int(want[tuple(bad[0])]), len(bad))
    g.run()
    got = np.frombuffer(g.read_raw_bytes(), dtype=np.uint8).reshape(m.wl, B, 32)
    assert np.array_equal(got, m.expected_raw(which))
    g.close()


# ---- 3: bulk staging across the 16-bit grid limit ----------------------------------------------------------------------------------------------
def _failures(hz, g):
    """hz_witness_failures into a numpy record array (no Python object per instance)"""
    n = ctypes.c_size_t(0)
    hz._check(hz.c.hz_witness_failures(g.h, None, 0, ctypes.byref(n)))
    out = np.zeros(max(n.value, 1), dtype=LL.ERR_DTYPE)
    if n.value:
        from circuits_amd.capi import hz_error
        hz._check(hz.c.hz_witness_failures(g.h, ctypes.cast(out.ctypes.data, ctypes.POINTER(hz_error)), n.value, ctypes.byref(n)))
    return out[:n.value]


def _run_and_compare(hz, g, m, which, what):
    """run(): the first failing instance raises; failures() == the oracle's tile, in instance order; the whole buffer == the oracle's tile"""
    from circuits_amd import ConstraintError
    exp = m.expected_failures(which)
    assert len(exp)
    with pytest.raises(ConstraintError) as e:
        g.run()
    f0 = exp[0]
    assert (e.value.instance, e.value.unit, e.value.constraint_id, e.value.lhs, e.value.rhs) == (
        int(f0["instance"]), int(f0["unit"]), int(f0["constraint_id"]), LL.row_int(f0["lhs"]), LL.row_int(f0["rhs"])), what
    got = _failures(hz, g)
    assert len(got) == len(exp), "%s: %d failing instances, the oracle's tile has %d" % (what, len(got), len(exp))
    bad = np.nonzero(got != exp)[0]
    assert not bad.size, "%s: failure record %d is %r, the oracle's %r (%d differ)" % (what, bad[0], got[bad[0]], exp[bad[0]], bad.size)
    B = len(which)
    for r0 in range(0, m.wl, 16):
        rows = min(16, m.wl - r0)
        a = np.frombuffer(g.read_raw_bytes(r0 * B, rows * B), dtype=np.uint8).reshape(rows, B, 32)
        b = m.raw[r0:r0 + rows][:, which]
        if not np.array_equal(a, b):
            r, k = np.argwhere((a != b).any(axis=2))[0]
            raise AssertionError("%s: signal row %d of instance %d (case %d) is %d, the oracle's %d" % (what, r0 + r, k, which[k], LL.row_int(a[r, k]), LL.row_int(b[r, k])))


@pytest.fixture(scope="module")
def decode_float():
    return LL.MainTile("decode-float", LL.decode_float_cases())


@pytest.fixture(scope="module")
def staged(hz, decode_float):
    """DecodeFloat x 131077 and its packed staging buffer (one 32-byte input an instance: 4 MB), in pinned host memory"""
    m = decode_float
    B = LL.B_STAGE
    g = hz.ctx("decode-float", n_instances=B)
    total, sigs = g.packed_layout()
    assert total == 32 and [(nm, off, w, ln) for nm, off, w, ln in sigs] == [("in", 0, 32, 1)]
    which = LL.tile_index(B, m.n)
    packed = np.ascontiguousarray(m.inputs["in"][which].reshape(B, 32))
    pin = hz.host_alloc(B * 32)
    ctypes.memmove(pin, packed.ctypes.data, B * 32)
    yield g, m, which, packed, pin
    hz.host_free(pin)
    g.close()


@pytest.mark.parametrize("source", ["device", "pinned"])
def test_stage_range_across_the_grid_y_cut(hz, staged, source):
    """one hz_inputs_stage_range(0, B) from one contiguous buffer, B = 131077: enqueue scatters runs of 65535, 65535 and 7 instances.
    Accepted and rejected instances mixed on both sides of 65535 and of 131070 (asserted on the case list in the CPU file)."""
    import torch
    g, m, which, packed, pin = staged
    B = LL.B_STAGE
    if source == "device":
        d = _dev(packed)
        torch.cuda.synchronize()
        g.stage_range(0, B, d.data_ptr(), 32)
    else:
        g.stage_range(0, B, pin, 32)
    _run_and_compare(hz, g, m, which, "DecodeFloat x %d staged from %s memory" % (B, source))


def test_second_step_stages_a_run_across_the_cut(hz, staged):
    """the next step through the same context: the list rotated by 37, and only instances 65530 .. 65541 staged -- a run that starts
    below the cut of the step before and ends above it; every other instance keeps its inputs"""
    g, m, which, packed, pin = staged
    B = LL.B_STAGE
    g.stage_range(0, B, pin, 32)
    _run_and_compare(hz, g, m, which, "the step before")
    w2 = which.copy()
    w2[65530:65542] = LL.tile_index(B, m.n, 37)[65530:65542]
    rot = np.ascontiguousarray(m.inputs["in"][w2[65530:65542]].reshape(12, 32))
    pin2 = hz.host_alloc(12 * 32)
    ctypes.memmove(pin2, rot.ctypes.data, 12 * 32)
    try:
        g.stage_range(65530, 12, pin2, 32)
        _run_and_compare(hz, g, m, w2, "instances 65530 .. 65541 staged anew")
    finally:
        hz.host_free(pin2)


def test_range_check_across_the_cut(hz, staged):
    """an element >= r at instance 65534, 65535, 65536 and at the last one, one at a time: the next check answers HZ_ERR_INPUT naming the
    input, and the step after a clean re-stage is the accepted-and-rejected launch again"""
    from circuits_amd import HzError
    g, m, which, packed, pin = staged
    B = LL.B_STAGE
    bad = hz.host_alloc(B * 32)
    try:
        for k in (LL.GRID_Y - 1, LL.GRID_Y, LL.GRID_Y + 1, B - 1):
            ctypes.memmove(bad, packed.ctypes.data, B * 32)
            ctypes.memmove(bad + 32 * k, LL.raw_rows([P + (k & 7)]).ctypes.data, 32)
            g.stage_range(0, B, bad, 32)
            with pytest.raises(HzError) as e:
                g.run()
            assert e.value.status == 4 and "input in[0]" in str(e.value), (k, str(e.value))
            g.stage_range(0, B, pin, 32)
            exp = m.expected_failures(which)
            with pytest.raises(HzError) as e:
                g.run()
            assert e.value.status == 3 and e.value.instance == int(exp[0]["instance"]), (k, str(e.value))
            assert np.array_equal(_failures(hz, g), exp), k
        _run_and_compare(hz, g, m, which, "after the clean re-stages")
    finally:
        hz.host_free(bad)


# ---- 4: export across the instance chunk -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hash_state_ref():
    """the literal reference of every variable of HashState's map for the 1013 cases -> (names, sym, rows uint8[1013, nvars, 32], MainTile)"""
    import export_derived_common as X
    cases = LL.hash_state_cases()
    names, refs, o = X.reference_set("hash-state", {}, cases)
    sym = X.Sym(names, 0x1E)
    rows = np.zeros((len(cases), sym.nvars, 32), dtype=np.uint8)
    for k, ref in enumerate(refs):
        want, lit = sym.expected(ref)
        assert lit.all()   # HashState has no constraint-pinned component input: every variable has a literal value
        rows[k] = want
    assert sym.nvars * 32 * LL.B_EXPORT < 4 << 30
    kinds = {X.KIND_NAMES[k]: int((names.kind == k).sum()) for k in range(6)}
    assert kinds["stored"] > 300 and kinds["Poseidon"] > 1000 and kinds["form"] > 0 and kinds["product"] and kinds["quotient"], kinds
    return names, sym, rows, LL.MainTile("hash-state", cases)


class _Export:
    def __init__(self, hz, ref, B):
        import torch
        self.hz, self.B = hz, B
        self.names, self.sym, rows, m = ref
        self.which = LL.tile_index(B, m.n)
        self.g = g = hz.ctx("hash-state", n_instances=B)
        idx = _idx(B, m.n)
        self.keep = []
        for name, vals in m.inputs.items():
            d = _dev(vals)[idx].contiguous()
            self.keep.append(d)
            torch.cuda.synchronize()
            g.set_input_dev(name, d.data_ptr(), B * vals.shape[1], instance=-1)
        g.run()
        got = np.frombuffer(g.read_raw_bytes(), dtype=np.uint8).reshape(m.wl, B, 32)
        assert np.array_equal(got, m.expected_raw(self.which))
        self.mp = g.import_sym(self.sym.text, self.sym.r1cs)
        assert self.mp.unresolved() == [] and self.mp.nvars() == self.sym.nvars and self.mp.derived() > 1000
        self.rows = _dev(rows)
        self.idx = idx

    def check(self, first, count):
        """instances [first, first + count) (first = -1: all, through instance = -1): every variable of every instance"""
        import torch
        nv = self.sym.nvars
        n = self.B if first < 0 else count
        out = torch.full((n + 1, nv, 32), LL.FILL, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        if first < 0:
            self.mp.export_dev(out.data_ptr(), -1)
        else:
            self.hz._check(self.hz.c.hz_witness_export_range_dev(self.g.h, self.mp.h, first, count, out.data_ptr(), None))
        torch.cuda.synchronize()
        f = max(first, 0)
        want = self.rows[self.idx[f:f + n]]
        if not torch.equal(out[:n], want):
            bad = torch.nonzero((out[:n] != want).any(dim=2))
            j, v = int(bad[0][0]), int(bad[0][1])
            ent = {int(x): int(e) for e, x in zip(self.sym.keep, self.sym.var)}
            raise AssertionError("export (%d, %d) of %d instances: variable %d (%s) of instance %d is %d, the reference's %d; %d values of %d instances differ" % (
                first, count, self.B, v, self.names.names[ent[v]] if v else "one", f + j, LL.row_int(out[j, v].cpu().numpy()), LL.row_int(want[j, v].cpu().numpy()),
                int(bad.shape[0]), int(torch.unique(bad[:, 0]).numel())))
        assert bool((out[n] == LL.FILL).all()), "export (%d, %d): written behind the last instance" % (first, count)
        return out


@pytest.fixture(scope="module")
def export65541(hz, hash_state_ref):
    e = _Export(hz, hash_state_ref, LL.B_EXPORT)
    yield e
    e.g.close()


@pytest.mark.parametrize("first,count", [(-1, LL.B_EXPORT), (32760, 16), (65530, 11), (32764, 32772), (3, 65536)],
                         ids=["all-3-chunks-plain", "range-32760+16-x4", "range-65530+11-plain", "range-32764+32772-x4-then-x4", "range-3+65536-x4"])
def test_export_across_the_instance_chunk(export65541, first, count):
    """HashState x 65541 (chunks of 32768, 32768 and 5): instance = -1, ranges that straddle an instance numbered 32768 or 65536, and
    ranges of more than one chunk whose output must advance -- counts that are multiples of 4 (k_export_singles_x4) and not. Stored
    variables are the oracle's tile, derived ones the literal route; every variable of every instance."""
    export65541.check(first, count)


def test_derive_dev_refuses_more_than_a_chunk(hz, export65541):
    e = export65541
    p = ctypes.c_void_p()
    assert hz.c.hz_witness_derive_dev(e.g.h, e.mp.h, -1, ctypes.byref(p), None) == 1   # HZ_ERR_ARG, before any launch
    assert b"32768" in hz.c.hz_last_error()
    assert e.mp.derive_dev(instance=65540)   # one instance is fine


def test_derive_dev_at_exactly_a_chunk(hz, hash_state_ref):
    """a context of 32768 instances: hz_witness_derive_dev(instance = -1) succeeds, slot = instance; every derived variable read through
    hz_symmap_dev_index's table equals the exported vector (which equals the reference)"""
    import torch
    B = LL.EXPORT_CH
    e = _Export(hz, hash_state_ref, B)
    out = e.check(-1, B)
    nv = e.sym.nvars
    from test_export_dev import _DevArr, _d2h
    d_phys, _, D = e.mp.dev_index()
    phys = _d2h(d_phys, nv, "<i8").view(np.uint64)
    p = e.mp.derive_dev(instance=-1)
    torch.cuda.synchronize()
    dval = torch.as_tensor(_DevArr(p, B * D * 32, "|u1"), device=DEV).view(B, D, 32)   # slot = instance
    derived = np.nonzero(phys >> np.uint64(63))[0]
    slots = (phys[derived] & np.uint64((1 << 63) - 1)).astype(np.int64)
    assert len(derived) == e.mp.derived() > 1000 and slots.max() < D   # (two variables of one value may share a slot)
    slot = _dev(slots)
    assert torch.equal(dval[:, slot], out[:B][:, _dev(derived.astype(np.int64))])
    e.g.close()


# ---- 5: hz_poseidon_dag, directly --------------------------------------------------------------------------------------------------------------
def _dag_run(hz, d, with_ms=True):
    """-> the table after the call, uint8[n, 32]"""
    vals = bytearray(d.vals.tobytes())
    if with_ms:
        ms = hz.poseidon_dag(vals, d.job_in, d.job_out, d.seg_t, d.seg_first, d.seg_count)
        assert ms >= 0.0
    else:
        buf = (ctypes.c_char * len(vals)).from_buffer(vals)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        hz._check(hz.c.hz_poseidon_dag(0, buf, len(vals) // 32, p(d.job_in), p(d.job_out), ctypes.c_uint64(len(d.job_out)), p(d.seg_t), p(d.seg_first),
                                       p(d.seg_count), ctypes.c_uint32(len(d.seg_t)), None))
    return np.frombuffer(bytes(vals), dtype=np.uint8).reshape(-1, 32)


def _dag_same(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not bad.size, "%s: table entry %d is %d, the reference's %d (%d differ)" % (what, bad[0], LL.row_int(got[bad[0]]), LL.row_int(want[bad[0]]), bad.size)


@pytest.mark.parametrize("t", [2, 3, 4, 5, 6, 7])
def test_dag_single_segments(hz, oracle, t):
    """one segment of every width at 1, 63, 64, 65 and 129 jobs, starting at job 0 and at job 77: the jobs in front of `first` stay
    untouched (their slots keep the pattern), the unused columns of job_in hold 0xFFFFFFFF"""
    for count in LL.DAG_COUNTS:
        for first in LL.DAG_FIRSTS:
            d = LL.dag_single(t, count, first, 100 * t + count + first)
            _dag_same(_dag_run(hz, d), d.reference(oracle), "t = %d, %d jobs from job %d" % (t, count, first))


def test_dag_chain_of_40_segments(hz, oracle):
    d = LL.dag_chain(0xC4A1)
    _dag_same(_dag_run(hz, d), d.reference(oracle), "chain of 40 segments")


def test_dag_resident_buffers_grow_and_are_reused(hz, oracle):
    """8 values, then 2^18, then 8 again with other values: the resident buffers only grow, nothing stale may show. Then no segments,
    no jobs, with and without device_ms: the table comes back as it went in."""
    a, c = LL.dag_small(1), LL.dag_small(2)
    big, big_exp = LL.dag_big(oracle)
    _dag_same(_dag_run(hz, a), a.reference(oracle), "8 values")
    _dag_same(_dag_run(hz, big), big_exp, "2^18 values")
    _dag_same(_dag_run(hz, c), c.reference(oracle), "8 values after 2^18")
    _dag_same(_dag_run(hz, a, with_ms=False), a.reference(oracle), "8 values, no device_ms")
    none = np.zeros(0, dtype=np.uint32)
    for with_ms in (True, False):
        no_segs = LL.Dag(a.vals, a.job_in, a.job_out, [])
        _dag_same(_dag_run(hz, no_segs, with_ms), a.vals, "n_segs = 0")
        no_jobs = LL.Dag(a.vals, none.reshape(0, 6), none, [(3, 0, 0)])
        _dag_same(_dag_run(hz, no_jobs, with_ms), a.vals, "n_jobs = 0")


def test_dag_two_callers_at_once(hz, oracle):
    """two threads, 16 calls each with different tables (ctypes releases the interpreter lock inside the call), so both resident sets of
    the device serve; every call's table is checked"""
    tables = [LL.dag_thread_tables(c) for c in (0, 1)]
    want = [[d.reference(oracle) for d in ts] for ts in tables]
    got = [[None] * 16, [None] * 16]
    errs = []
    gate = threading.Barrier(2)

    def work(c):
        try:
            gate.wait(timeout=30)
            for k, d in enumerate(tables[c]):
                got[c][k] = _dag_run(hz, d, with_ms=bool(k % 2))
        except Exception as e:   # pragma: no cover
            errs.append(e)
    ths = [threading.Thread(target=work, args=(c,)) for c in (0, 1)]
    t0 = time.time()
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errs, errs
    for c in (0, 1):
        for k in range(16):
            _dag_same(got[c][k], want[c][k], "caller %d, call %d" % (c, k))
    assert time.time() - t0 < 60
