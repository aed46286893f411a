"""Garbage parity for the twelve mains the adversarial fuzz never reached: DecodeTx (k_dec_main), FeeTx (k_fee_front / k_smt /
k_fee_back), HashState (k_hash_state_main), the eight templates of k_gadget<..> and AySign2Ax (k_ay_sign_2_ax_main) as `component
main`, on inputs outside every range the enclosing RollupTx feeds them (tests/fuzz_common.py, tests/standalone_fuzz_common.py; the
CPU half is tests/test_standalone_fuzz_cpu.py). These kernels are not the code RollupMain runs -- k_main_front fuses the same
statements -- so the garbage of rollup_main_cases / rollup_tx_cases never executes them.

Requirement per instance, as in tests/test_adversarial_fuzz.py: the whole physical witness AND the first violated constraint (unit,
constraint id, lhs, rhs) equal the oracle's; and the verdict equals the reference's own recorded constraint system. What only garbage
reaches: compute_fee_ld_dev's two paths chosen per wavefront (the lists lay whole wavefronts out: all selectors bits with feeSel and
amount out of range, one non-bit at lane 0 / 17 / 63, none a bit), BalanceUpdater's 193-bit sum wrapping mod P, the low bits of a
value whose Num2Bits failed, selectors that are field elements, AySign2Ax without a point / with x = 0, and the order of the reports
where several constraints fail at once."""
import pytest

import declared_forms as DF
import fuzz_common as FZ
import standalone_fuzz_common as SF

pytestmark = pytest.mark.gpu


def _run(g):
    from circuits_amd import ConstraintError
    try:
        g.run()
    except ConstraintError as e:
        return e
    return None


@pytest.mark.parametrize("key", SF.MAINS)
def test_hip_one_launch_whole_buffer_and_first_failures(hz, key):
    """n instances in one launch (449: seven wavefronts and a lane; DecodeTx 193; FeeTx 129, k_smt's latency form)"""
    cases, parts, failures = SF.full_list(key)
    n = len(cases)
    assert n == SF.N_GPU[key]
    SF.check_mix(key, n, failures)
    g = hz.ctx(key, n_instances=n, **SF.kw_of(key))
    FZ.set_all_inputs(g, cases)
    err = _run(g)
    FZ.compare_instanced(g, parts, n)
    assert FZ.check_failures(g, parts, err) == len(failures)
    if key in SF.NEVER_FAIL:
        assert err is None and g.failures() == []
        assert 2 * sum(SF.out_of_range(key, d) for d in cases) >= n


@pytest.mark.parametrize("key", SF.MAINS)
def test_hip_two_steps_through_one_context_rotated(hz, key):
    """the same list again, rotated by 37 instances: every lane meets another case, and the wavefronts of ComputeFee's two paths trade
    places over a buffer the other path wrote"""
    cases, parts, failures = SF.full_list(key)
    n = len(cases)
    g = hz.ctx(key, n_instances=n, **SF.kw_of(key))
    for shift in (0, SF.ROTATE):
        which = [(k + shift) % n for k in range(n)]
        FZ.set_all_inputs(g, [cases[d] for d in which])
        err = _run(g)
        FZ.compare_replicated(g, parts, n, n, which)
        assert FZ.check_failures(g, parts, err, which=which) == len(failures)


@pytest.mark.parametrize("key", SF.MAINS)
def test_hip_one_instance_alone(hz, key):
    """n = 1: the first rejected case and the first accepted one (the mains that cannot fail: the first and the last case)"""
    cases, parts, failures = SF.full_list(key)
    n = len(cases)
    if key in SF.NEVER_FAIL:
        picks = [0, n - 1]
    else:
        picks = [min(failures), min(k for k in range(n) if k not in failures)]
    for d in picks:
        g = hz.ctx(key, n_instances=1, **SF.kw_of(key))
        g.set_inputs(cases[d])
        err = _run(g)
        FZ.compare_replicated(g, parts, 1, n, [d])
        assert FZ.check_failures(g, parts, err, which=[d]) == (1 if d in failures else 0)
        assert (err is not None) == (d in failures)


def test_hip_fee_tx_throughput_form(hz):
    """FeeTx above HZ_SMT_LAT_MAX instances (csrc/kernels.h), a whole number of wavefronts and one lane: k_smt's throughput form on the
    same 129 cases, replicated on the device; sampled instances whole against the oracle, every instance's first failure"""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "circuits_amd", "csrc", "kernels.h")).read()
    lat_max = int(re.search(r"#define\s+HZ_SMT_LAT_MAX\s+(\d+)u?\b", text).group(1))
    n = (lat_max // FZ.WAVE + 1) * FZ.WAVE + 1
    assert n > lat_max and n % FZ.WAVE == 1
    cases, parts, failures = SF.full_list("fee-tx")
    m = len(cases)
    g = hz.ctx("fee-tx", n_instances=n, **SF.kw_of("fee-tx"))
    which = [(k + 5 * (k // m)) % m for k in range(n)]   # (each repetition shifted: a lane does not meet the same case twice)
    FZ.place_replicas(g, cases, which)
    err = _run(g)
    assert FZ.check_failures(g, parts, err, which=which) == sum(d in failures for d in which)
    wl = g.witness_len()
    ref = {}
    for o, lo, cnt in parts:
        for k in range(cnt):
            ref[lo + k] = o.read_bytes(0, wl, k)
    for k in list(range(0, n, 13)) + [n - 1, n - 2, n - 64, n - 65]:
        assert g.read_bytes(0, wl, k) == ref[which[k]], (k, which[k])


@pytest.mark.parametrize("key", SF.MAINS)
def test_hip_verdict_equals_the_recorded_system(hz, key):
    """the served witness of every instance through the reference's own constraints (.sym + .r1cs of the recorded system): nothing
    unresolved, and a violated constraint exactly in the instances the kernels reject"""
    cases, parts, failures = SF.full_list(key)
    n = len(cases)
    m = DF.load(key)
    g = hz.ctx(key, n_instances=n, **SF.kw_of(key))
    sym, r1cs, _ = DF.sym_and_r1cs(m)
    mp = g.import_sym(sym, r1cs)
    assert mp.unresolved() == []
    FZ.set_all_inputs(g, cases)
    _run(g)
    rejected = {f[0] for f in g.failures()}
    assert rejected == set(failures)
    for k in range(n):
        n_bad, _ = mp.check_r1cs(instance=k, cap=1)
        assert (n_bad > 0) == (k in rejected), (key, k, n_bad)
