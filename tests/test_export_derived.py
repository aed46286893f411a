"""The DERIVED half of the device export (circuits_amd/csrc/export.hip: k_derive_poseidon<T>, k_derive_forms, k_export_dvars) on launches
of many instances, ranges that do not start at instance 0, maps that name only some variables, and rejected instances.

tests/test_export_dev.py runs these kernels with one instance, instance 0, one valid input; its multi-instance tests use maps without a
derived variable. Here every launch has several DIFFERENT inputs, so a value taken from the wrong instance is a wrong value, and every
variable of every exported instance is compared, bit for bit, with
  * the literal reference of tests/export_derived_common.py (the oracle's witness for stored variables; circomlib's Poseidon template and
    the reference's `<==` lines over the oracle's witness for derived ones; the template's own constraint for IsZero / Num2Bits inputs),
    one oracle run per distinct input;
  * the library's host evaluator (hz_witness_read_sym in pieces of at most 4 096 variables, the route of SymMap.read_small), which
    works on 4 x 64-bit limbs on the CPU where the kernels work on 9 x 29-bit limbs -- accepted and rejected instances alike.
The maps are synthetic .sym files of an unreduced compile, as tests/test_derived_signals.py builds them, in a seeded random variable
order (and by name for the host evaluator, whose cost per piece grows with the components a piece touches). A .sym alone never makes
the library evaluate one derived variable from another, so every full map carries an .r1cs as well that defines 112 variables over
derived ones (export_derived_common.Names.add_solved: linear chains, products, quotients with a divisor that is 0 in some instances):
drv_operand's derived branch, DV_PRODUCT and DV_QUOTIENT, and several dependency levels of k_derive_forms."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import export_derived_common as X   # noqa: E402
from test_export_dev import _d2h   # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xA5   # the output buffer before an export: 0xA5A5...A5 is not a field element, so a variable nobody wrote cannot pass for a value


class Launch:
    """one context with its inputs set and run, the maps of its main and the reference of each distinct input"""

    def __init__(self, hz, template, kw, ref, n, which=None):
        from circuits_amd import ConstraintError
        self.hz, self.template, self.kw, self.n = hz, template, kw, n
        self.names, self.refs, self.inputs, self.sym, self.sym_by_name = ref
        self.which = [k % len(self.inputs) for k in range(n)] if which is None else which
        self.g = hz.ctx(template, n_instances=n, **kw)
        for k, w in enumerate(self.which):
            self.g.set_inputs(self.inputs[w], instance=k)
        try:
            self.g.run()
        except ConstraintError:
            pass
        self.mp = self.g.import_sym(self.sym.text, self.sym.r1cs)
        assert self.mp.unresolved() == [], self.mp.unresolved()[:5]
        assert self.mp.nvars() == self.sym.nvars and self.mp.derived() > 0
        self._by_name = None

    def ref_of(self, k):
        return self.refs[self.which[k]]

    def export(self, first, count, mp=None):
        """instances [first, first + count) -> [count][nvars][32]; first = -1: every instance through instance = -1"""
        import torch
        mp = self.mp if mp is None else mp
        n = self.n if first < 0 else count
        out = torch.full((n * mp.nvars() * 32,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        if first < 0:
            mp.export_dev(out.data_ptr(), -1)
        elif count == 1:
            mp.export_dev(out.data_ptr(), first)
        else:
            self.hz._check(self.hz.c.hz_witness_export_range_dev(self.g.h, mp.h, first, count, out.data_ptr(), None))
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(n, mp.nvars(), 32)

    def check(self, first, count, what):
        """export and compare every variable of every instance with the reference of that instance's own input"""
        got = self.export(first, count)
        for j in range(got.shape[0]):
            k = max(first, 0) + j
            X.compare(self.sym, self.ref_of(k), got[j], k, what)
        return got

    def host_rows(self, k):
        """instance k through the HOST evaluator, rows in the order of self.sym's variables. Read through a second map of the same names
        numbered by name: a piece of 4 096 variables then lies in a few components instead of in all of them."""
        if self._by_name is None:
            self._by_name = self.g.import_sym(self.sym_by_name.text, self.sym_by_name.r1cs)
            assert self._by_name.unresolved() == [] and self._by_name.derived() == self.mp.derived()
        mp, nv = self._by_name, self.sym.nvars
        buf = np.full((nv, 32), FILL, dtype=np.uint8)
        for f in range(0, nv, 4096):
            self.hz._check(self.hz.c.hz_witness_read_sym(self.g.h, mp.h, k, f, min(4096, nv - f), buf.ctypes.data + 32 * f))
        rows = np.empty_like(buf)
        rows[0] = buf[0]
        rows[self.sym.var] = buf[self.sym_by_name.var]   # (both maps keep every entry: entry i is sym.var[i] here, sym_by_name.var[i] there)
        return rows


def _ref(template, kw, inputs, seed):
    names, refs, o = X.reference_set(template, kw, inputs)
    return (names, refs, inputs, X.Sym(names, seed), X.Sym(names, seed, order="by name")), o


@pytest.fixture(scope="module")
def main_ref():
    ref, o = _ref("rollup-main", X.MAIN_KW, X.main_batches(), 0xD1)
    assert all(o.failure_of(k) is None for k in range(X.N_MAIN_BATCHES))
    return ref


@pytest.fixture(scope="module")
def main8(hz, main_ref):
    """RollupMain(8,16,4,4) x 8 instances, three distinct batches cycled"""
    return Launch(hz, "rollup-main", X.MAIN_KW, main_ref, 8)


@pytest.fixture(scope="module")
def main5(hz, main_ref):
    """the same x 5 instances: not a multiple of 4"""
    return Launch(hz, "rollup-main", X.MAIN_KW, main_ref, 5)


@pytest.fixture(scope="module")
def wd_ref():
    ref, o = _ref("withdraw", dict(nLevels=16), X.withdraw_inputs(), 0xD3)
    assert len(ref[2]) >= 3 and all(o.failure_of(k) is None for k in range(len(ref[2])))
    return ref


@pytest.fixture(scope="module")
def wd37(hz, wd_ref):
    return Launch(hz, "withdraw", dict(nLevels=16), wd_ref, X.WD_N)


@pytest.fixture(scope="module")
def rtx48(hz):
    """RollupTx(16,2) x 48 garbage cases, one oracle instance per case -> (launch, instances the oracle rejects)"""
    ref, o = _ref("rollup-tx", X.RTX_KW, X.rollup_tx_cases(), 0xD4)
    rejected = [k for k in range(X.RTX_N) if o.failure_of(k) is not None]
    assert len(rejected) >= 8 and X.RTX_N - len(rejected) >= 8
    ln = Launch(hz, "rollup-tx", X.RTX_KW, ref, X.RTX_N)
    assert sorted({f[0] for f in ln.g.failures()}) == rejected
    return ln, rejected


# ---- 1, 2: RollupMain, every path of export_chunk ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,count", [(0, 1), (3, 1), (7, 1), (-1, 8), (1, 4), (2, 3)],
                         ids=["instance0", "instance3", "instance7", "all-x4", "range1+4-x4", "range2+3-plain"])
def test_main_x8_every_variable_of_every_instance(main8, first, count):
    main8.check(first, count, "RollupMain x 8, export (%d, %d)" % (first, count))


@pytest.mark.parametrize("first", [0, 4])
def test_main_x8_device_equals_host_evaluator(main8, first):
    """every instance through the host evaluator == the device export of all instances at once (four instances a test)"""
    got = main8.export(-1, 8)
    for k in range(first, first + 4):
        X.compare_rows(got[k], main8.host_rows(k), main8.sym, k, "RollupMain x 8, device export / host evaluator")


@pytest.mark.parametrize("first,count", [(-1, 5), (1, 3)], ids=["all-plain", "range1+3"])
def test_main_x5(main5, first, count):
    main5.check(first, count, "RollupMain x 5, export (%d, %d)" % (first, count))


# ---- 3: the unit is the instance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,count", [(-1, 37), (1, 36), (17, 1)], ids=["all37-plain", "range1+36-x4", "instance17"])
def test_withdraw_x37(wd37, first, count):
    got = wd37.check(first, count, "Withdraw x 37, export (%d, %d)" % (first, count))
    if count == 36:
        for j in (0, 18, 35):
            X.compare_rows(got[j], wd37.host_rows(1 + j), wd37.sym, 1 + j, "Withdraw x 37, device export / host evaluator")


# ---- 4: accepted and rejected instances inside one wavefront of the derive kernels -----------------------------------------------------------
def test_rollup_tx_garbage_all_at_once(rtx48):
    """48 mutated transactions, accepted and rejected mixed: the derived values of a rejected instance are defined all the same (an
    IsZero input from inv = 0, x^5 / x^4 at x = 0), and both evaluators must give them"""
    ln, rejected = rtx48
    got = ln.check(-1, X.RTX_N, "RollupTx x 48 garbage, all at once")
    for k in range(X.RTX_N):
        X.compare_rows(got[k], ln.host_rows(k), ln.sym, k, "RollupTx x 48 garbage (%s), device export / host evaluator" % ("rejected" if k in rejected else "accepted"))


def test_rollup_tx_garbage_single_instances(rtx48):
    ln, rejected = rtx48
    accepted = [k for k in range(X.RTX_N) if k not in rejected]
    picks = [accepted[len(accepted) // 2], rejected[len(rejected) // 2], X.RTX_N - 1]
    assert picks[0] > 0 and picks[1] > 0
    for k in picks:
        ln.check(k, 1, "RollupTx x 48 garbage, instance %d alone" % k)


# ---- 5: maps that name only some of the variables -------------------------------------------------------------------------------------------
def test_partial_maps(main8):
    """one entry in five / one derived entry in two (every stored entry in exactly one of the two): pos_emit on a sparse list of slots,
    the `used` closure of build_plan on a part of the derived variables; every named variable of every instance == the reference == the
    full map's value for the same name"""
    full = main8.export(-1, 8)
    for label, keep in zip(("one in five", "one in two"), X.partial_keeps(main8.names, 0xD5)):
        sym = X.Sym(main8.names, 0xD6, keep=keep)
        assert sym.r1cs is None
        mp = main8.g.import_sym(sym.text)
        assert mp.unresolved() == [] and mp.nvars() == sym.nvars
        assert 0 < mp.derived() < main8.mp.derived()
        got = main8.export(-1, 8, mp)
        for k in range(8):
            X.compare(sym, main8.ref_of(k), got[k], k, "partial map (%s), all at once" % label)
            assert (sym.by_entry(got[k]) == main8.sym.by_entry(full[k])[keep]).all(), (label, k)
        for first, count in ((5, 1), (1, 4)):
            part = main8.export(first, count, mp)
            for j in range(count):
                X.compare(sym, main8.ref_of(first + j), part[j], first + j, "partial map (%s), export (%d, %d)" % (label, first, count))


# ---- 6: indirection instead of a copy ------------------------------------------------------------------------------------------------------
def _through_the_index(ln, exported):
    """hz_symmap_dev_index + hz_witness_derive_dev name the same values as the exported vector"""
    import torch
    from circuits_amd import HzError
    g, mp, n, nv = ln.g, ln.mp, ln.n, ln.sym.nvars
    p0, stride, nd = mp.dev_index()
    assert nd > 0
    phys0 = _d2h(p0, nv, "<i8").view(np.uint64)
    istr = _d2h(stride, nv, "<i4").astype(np.int64)
    derived = (phys0 >> np.uint64(63)) == 1
    slot = (phys0 & np.uint64(X.DERIVED_BIT - 1)).astype(np.int64)
    assert int(derived.sum()) == mp.derived() and slot[derived].max() < nd and (istr[derived] == 0).all()
    raw = np.frombuffer(g.read_raw_bytes(), dtype=np.uint8).reshape(-1, 32)

    def vector(buf, inst_slot, k):
        out = np.empty((nv, 32), dtype=np.uint8)
        out[~derived] = raw[slot[~derived] + k * istr[~derived]]
        out[derived] = buf[inst_slot * nd + slot[derived]]
        return out

    def check_all():
        ptr = mp.derive_dev(-1)
        torch.cuda.synchronize()
        buf = _d2h(ptr, n * nd * 32, "|u1").reshape(-1, 32)
        for k in (0, n // 2, n - 1):
            X.compare_rows(vector(buf, k, k), exported[k], ln.sym, k, "%s: dev_index + derive_dev(-1)" % ln.template)

    def check_one(k):
        ptr = mp.derive_dev(k)
        torch.cuda.synchronize()
        buf = _d2h(ptr, nd * 32, "|u1").reshape(-1, 32)
        X.compare_rows(vector(buf, 0, k), exported[k], ln.sym, k, "%s: dev_index + derive_dev(%d)" % (ln.template, k))
    check_all()
    check_one(0)
    check_one(n - 1)
    # argument errors, and a valid call right after each
    out = torch.full((nv * 32,), FILL, dtype=torch.uint8, device="cuda:0")
    for bad in (lambda: mp.derive_dev(n), lambda: mp.derive_dev(-2),
                lambda: ln.hz._check(ln.hz.c.hz_witness_export_range_dev(g.h, mp.h, n - 1, 2, out.data_ptr(), None)),
                lambda: ln.hz._check(ln.hz.c.hz_witness_export_range_dev(g.h, mp.h, n, 1, out.data_ptr(), None))):
        with pytest.raises(HzError):
            bad()
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == FILL).all()
        check_one(n - 1)
    check_all()
    X.compare_rows(ln.export(n - 1, 1)[0], exported[n - 1], ln.sym, n - 1, "%s: export after the argument errors" % ln.template)


def test_dev_index_and_derive_dev_main(main8):
    _through_the_index(main8, main8.check(-1, 8, "RollupMain x 8, all at once"))


def test_dev_index_and_derive_dev_rollup_tx_garbage(rtx48):
    ln, _ = rtx48
    _through_the_index(ln, ln.check(-1, X.RTX_N, "RollupTx x 48 garbage, all at once"))


# ---- 7: few workgroups, many loop iterations ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worker_jobs(tmp_path_factory, main_ref, wd_ref):
    """the inputs and the .sym of cases 1 and 3 as files, written once for the four worker runs"""
    d = tmp_path_factory.mktemp("export_derived")
    jobs = {}
    for key, template, kw, ref, n, exports in (("main", "rollup-main", X.MAIN_KW, main_ref, 8, ["all", [7, 1]]),
                                              ("withdraw", "withdraw", dict(nLevels=16), wd_ref, X.WD_N, ["all", [1, 36]])):
        sym = ref[3]
        with open(str(d / (key + ".sym")), "w") as f:
            f.write(sym.text)
        with open(str(d / (key + ".r1cs")), "wb") as f:
            f.write(sym.r1cs)
        jobs[key] = (dict(template=template, kw=kw, n_instances=n, inputs=ref[2], which=[k % len(ref[2]) for k in range(n)], sym=str(d / (key + ".sym")), r1cs=str(d / (key + ".r1cs")), exports=exports), ref)
    return jobs


@pytest.mark.parametrize("blocks", [3, 24])
@pytest.mark.parametrize("key", ["main", "withdraw"])
def test_capped_grids(worker_jobs, tmp_path, key, blocks):
    """HZ_EXPORT_BLOCKS = 3 and 24 (read once per process: a fresh child): with 8 instances both leave k_export_stored three
    workgroups per instance, so every one of its lists, k_export_singles_x4 and k_export_dvars walk their grid-stride loops several
    times (1.3 x 10^6 variables through 3 or 24 workgroups of 256); the worker only writes what it exported."""
    job, ref = worker_jobs[key]
    names, refs, inputs, sym, _ = ref
    job = dict(job, out=str(tmp_path))
    with open(str(tmp_path / "job.json"), "w") as f:
        json.dump(job, f)
    env = dict(os.environ, HZ_EXPORT_BLOCKS=str(blocks))
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "export_derived_worker.py"), str(tmp_path / "job.json")],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-600:] + r.stderr[-1200:]
    for i, ex in enumerate(job["exports"]):
        first, count = (0, job["n_instances"]) if ex == "all" else ex
        got = np.load(str(tmp_path / ("export_%d.npy" % i)))
        assert got.shape == (count, sym.nvars, 32)
        for j in range(count):
            X.compare(sym, refs[job["which"][first + j]], got[j], first + j, "%s with HZ_EXPORT_BLOCKS=%d, export %r" % (key, blocks, ex))
        os.remove(str(tmp_path / ("export_%d.npy" % i)))


# ---- 8: which k_derive_poseidon<T> these maps reach ---------------------------------------------------------------------------------------------
def test_poseidon_widths_reached(main_ref, wd_ref, rtx48):
    """t over the components whose internals the maps above name. No main of this library holds a Poseidon of one input, so
    k_derive_poseidon<2> is reached by no map; its host statement, derived.h pos_trace(2), is held to the literal template in
    tests/test_derived_signals.py::test_poseidon_trace_from_sbox_signals_on_the_host."""
    assert main_ref[0].widths() == {3, 4, 5, 6, 7}
    assert wd_ref[0].widths() == {3, 4, 5}
    assert rtx48[0].names.widths() == {3, 4, 5, 6}
