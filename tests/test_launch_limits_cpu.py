"""The CPU half of tests/test_launch_limits.py: the tiling helpers and references of tests/launch_limits_common.py against the oracle at
small sizes, the case lists (period, accepted and rejected cases within every 64 consecutive instances, distinct failures), the device
memory of every context the GPU file creates, and the audit table of launch caps and chunk constants against the sources."""
import numpy as np
import pytest

import launch_limits_common as LL
from oracle_binding import OracleCtx, P


# ---- tiling ------------------------------------------------------------------------------------------------------------------------------
def test_periods_are_prime_and_no_multiple_of_a_wavefront():
    for p in (LL.PERIOD_FR, LL.PERIOD_INST):
        assert all(p % d for d in range(2, int(p ** 0.5) + 1)) and p % 64
    # a displacement by a workgroup, a whole grid pass, a grid.y run or an export chunk lands on another case
    for step in (64, 256, LL.CAP, LL.GRID_Y, LL.EXPORT_CH, 37):
        assert step % LL.PERIOD_FR and step % LL.PERIOD_INST
    assert LL.N_AT_CAP == 524288 and LL.N_PAST_CAP == 524288 + 257 and LL.N_FR == 524288 + 257
    assert LL.B_STAGE == 131077 and LL.B_EXPORT == 65541 and [b * 256 - LL.CAP for b in LL.MUX_B] == [0, 256, 1024]


def test_tile_is_the_plain_statement():
    a = np.arange(7 * 3, dtype=np.uint8).reshape(7, 3)
    for n, shift in ((1, 0), (7, 0), (8, 0), (23, 0), (23, 5)):
        t = LL.tile(a, n, shift)
        assert t.shape == (n, 3) and all((t[i] == a[(i + shift) % 7]).all() for i in range(n))
    assert LL.row_int(LL.fr_rows([P + 5])[0]) == 5 and LL.row_int(LL.raw_rows([P])[0]) == P


def test_field_cases_hold_the_edges():
    for width in (1, 2, 6):
        rows = LL.field_cases(LL.PERIOD_FR, 3, width)
        assert len(rows) == LL.PERIOD_FR and all(len(r) == width and all(0 <= x < P for x in r) for r in rows)
        for e in (0, P - 1, (1 << 253) + 5):
            assert [e] * width in rows
        assert len({tuple(r) for r in rows}) > 800   # (garbage repeats 0, 1, 2 and p - 1)


# ---- references --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [2, 3, 7])
def test_poseidon_reference_is_the_oracle_row_by_row(oracle, t):
    ins, dig, wit = LL.poseidon_reference(oracle, t, True)
    assert ins.shape == (LL.PERIOD_FR, t - 1, 32) and dig.shape == (LL.PERIOD_FR, 32) and wit.shape == (3 * LL.NSBOX[t], LL.PERIOD_FR, 32)
    for r in (0, 1, 2, 500, LL.PERIOD_FR - 1):   # one row alone gives the same digest and the same column of S-box signals
        d1, w1 = oracle.poseidon_batch(t, [[LL.row_int(x) for x in ins[r]]], witness=True)
        assert LL.row_int(dig[r]) == d1[0] and wit[:, r, :].tobytes() == w1


def test_fr_ops_references():
    for name, (_, two, f) in LL.FR_OPS.items():
        a, b, exp = LL.fr_ops_reference(name)
        assert a.shape == exp.shape == (LL.PERIOD_FR, 32) and (b is not None) == two
        vals = [LL.row_int(r) for r in a]
        assert 0 in vals and P - 1 in vals
        for i in (0, 1, 2, 3, 77, 1008):
            assert LL.row_int(exp[i]) == f(vals[i], LL.row_int(b[i]) if two else 0)
    a, _, exp = LL.fr_ops_reference("sqrt")
    roots = nones = 0
    for x, r in zip(map(LL.row_int, a), map(LL.row_int, exp)):   # the requirement of test_hip_field_ops_against_python_bigints
        if pow(x, (P - 1) // 2, P) in (0, 1):
            assert r * r % P == x and r <= (P - 1) // 2
            roots += 1
        else:
            assert r == 0
            nones += 1
    assert roots > 500 and nones > 200


def test_fr_raw_reference_and_the_tiled_judge():
    import fr_contract_common as FC
    op, tuples, packed = LL.fr_raw_reference()
    assert op.name == "fr_mul" and packed.shape == (2, LL.PERIOD_FR, 9) and len(tuples) == LL.PERIOD_FR
    assert any(t == (0, 0) for t in tuples) and any(max(t) >= FC.LIMIT - 2 for t in tuples)   # the edges' cross product comes first
    n = 3 * LL.PERIOD_FR + 5
    good = np.array([FC.limbs(a * b * FC.RINV % P) for a, b in tuples], dtype=np.uint32)
    assert LL.judge_raw_tiled(op, tuples, LL.tile(good, n), "model") == LL.PERIOD_FR
    bad = LL.tile(good, n)
    assert (good[500] != good[501]).any()
    bad[2 * LL.PERIOD_FR + 500] = good[501]   # one element of the third period holds its neighbour's product
    with pytest.raises(AssertionError):
        LL.judge_raw_tiled(op, tuples, bad, "model")


# ---- case lists ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decode_float():
    return LL.MainTile("decode-float", LL.decode_float_cases())


def test_decode_float_cases_mix_within_every_64_instances(decode_float):
    m = decode_float
    assert m.n == LL.PERIOD_INST and m.first is not None
    lo, hi = LL.mix_per_window(m.failed)
    assert lo >= 4 and hi <= 60, (lo, hi)     # accepted AND rejected cases in every 64 consecutive instances, seams included
    recs = {(int(r["constraint_id"]), r["lhs"].tobytes(), r["rhs"].tobytes()) for r in m.fail[m.failed]}
    assert len(recs) >= 100                    # distinct failures: a record of the wrong instance is a wrong record
    which = LL.tile_index(LL.B_STAGE, m.n)
    exp = m.expected_failures(which)
    inst = exp["instance"]
    assert (np.diff(inst) > 0).all() and len(inst) == int(m.failed[which].sum())
    for cut in (LL.GRID_Y, 2 * LL.GRID_Y):     # failing instances on both sides of 65535 and of 131070, close to them
        assert ((inst >= cut - 16) & (inst < cut)).any() and ((inst >= cut) & (inst < cut + 7)).any(), cut
    assert inst[-1] >= LL.B_STAGE - 7
    k = int(inst[len(inst) // 2])
    assert exp[len(inst) // 2]["lhs"].tobytes() == m.fail[k % m.n]["lhs"].tobytes()
    # the rotated second step: instances 65530 .. 65541 hold case (k + 37) % 1013, and that changes their verdicts
    w2 = which.copy()
    w2[65530:65542] = LL.tile_index(LL.B_STAGE, m.n, 37)[65530:65542]
    assert (m.failed[w2[65530:65542]] != m.failed[which[65530:65542]]).any()
    assert (m.raw[:, w2[65530:65542]] != m.raw[:, which[65530:65542]]).any(axis=(0, 2)).all()


def test_expected_raw_is_the_oracles_layout(decode_float):
    """the numpy statement of the physical buffer (signal s of instance k at s * B + k) against OracleCtx.read_raw_bytes of a launch
    laid out the same way"""
    m = decode_float
    B = 2 * m.n + 9
    which = LL.tile_index(B, m.n, 5)
    o = OracleCtx("decode-float", n_instances=B)
    vals = m.inputs["in"][which]
    assert o.o.c.orc_set_input(o.h, -1, b"in", vals.tobytes(), B) == 0
    o.run()
    assert o.read_raw_bytes() == m.expected_raw(which).tobytes()
    s = o.lookup("main.in")
    assert o.read_raw_bytes(s * B, B) == LL.physical_layout(vals, B).tobytes()
    assert [o.failure_of(int(k)) is not None for k in range(B)] == m.failed[which].tolist()


def test_mux256_cases_and_layout():
    cases = LL.mux256_cases()
    m = LL.MainTile("mux256", cases)
    assert m.n == LL.PERIOD_INST and m.first is None and not m.failed.any()   # no constraint of this main can fail
    assert m.inputs["in"].shape == (m.n, 256, 32) and m.inputs["s"].shape == (m.n, 8, 32)
    outs = m.raw[m.o.lookup("main.out")]
    assert len({r.tobytes() for r in outs}) > 300
    B = 70
    which = LL.tile_index(B, m.n)
    o = OracleCtx("mux256", n_instances=B)
    for k in range(B):
        o.set_inputs(cases[k], instance=k)
    assert o.run() is None and o.read_raw_bytes() == m.expected_raw(which).tobytes()
    s = o.lookup("main.in[0]")
    assert o.lookup("main.in[255]") == s + 255
    assert o.read_raw_bytes(s * B, 256 * B) == LL.physical_layout(m.inputs["in"][which], B).tobytes()


def test_hash_state_cases():
    m = LL.MainTile("hash-state", LL.hash_state_cases())
    assert m.n == LL.PERIOD_INST and m.first is None and not m.failed.any()   # the template packs and hashes
    assert len({r.tobytes() for r in m.raw[m.o.lookup("main.out")]}) > 900


def test_withdraw_past_the_cap_has_no_shape_below_16_gib():
    """the written reason there is no Withdraw test at instance = -1 past k_transpose32's cap"""
    from circuits_amd import lib
    L = lib()
    for n_levels, b in LL.WITHDRAW_PAST_CAP:
        assert (n_levels + 1) * b > LL.CAP
        assert L.template_device_bytes("withdraw", nLevels=n_levels, n_instances=b) > LL.GIB16


# ---- the DAG reference -----------------------------------------------------------------------------------------------------------------------
def test_dag_reference_against_the_dag_hasher(oracle):
    import random
    rng = random.Random(4)
    leaves = [rng.randrange(P) for _ in range(16)]
    via, direct = LL.dag_via_hasher(oracle, leaves)
    assert via == direct


def test_dag_tables_are_well_formed(oracle):
    for t in range(2, 8):
        for count in LL.DAG_COUNTS:
            for first in LL.DAG_FIRSTS:
                d = LL.dag_single(t, count, first, 100 * t + count + first)
                assert d.well_formed() and (d.job_in[first:, t - 1:] == LL.DAG_UNUSED).all() and d.job_in[:first].max(initial=0) < len(d.vals)
                pool = [LL.row_int(r) for r in d.vals[:24]]
                assert pool[0] == 0 and pool[1] == P - 1
    d = LL.dag_single(4, 65, 77, 1)
    ref = d.reference(oracle)
    assert (ref[24:24 + 77] == LL.PATTERN).all() and not (ref[24 + 77:] == LL.PATTERN).all(axis=1).any()
    assert LL.row_int(ref[24 + 77 + 1]) == oracle.poseidon_batch(4, [[0, 0, 0]])[0][0]
    c = LL.dag_chain(0xC4A1)
    assert c.well_formed() and len(c.seg_t) == 40 and set(c.seg_t.tolist()) == {2, 3, 4, 5, 6, 7}
    f = c.seg_first.astype(int)
    assert c.job_out[f[5]] in c.job_in[f[5], :int(c.seg_t[5]) - 1]                     # a job that writes one of its own inputs
    assert c.job_out[f[12] + 1] == c.job_out[f[10]] and c.job_in[f[13], 0] == c.job_out[f[10]]   # one slot, two writers, a later reader
    ref = c.reference(oracle)
    assert not (ref[c.job_out] == LL.PATTERN).all(axis=1).any()
    assert LL.dag_small(1).well_formed() and len(LL.dag_small(1).vals) == 8
    tabs = LL.dag_thread_tables(0) + LL.dag_thread_tables(1)
    assert all(x.well_formed() for x in tabs) and len({x.vals.tobytes() for x in tabs}) == 32
    big, exp = LL.dag_big(oracle)
    assert len(big.vals) == LL.DAG_BIG and big.well_formed()
    sub = LL.Dag(big.vals, big.job_in, big.job_out, [(3, 2000, 50)])                # the tiled expectation against the reference on a part
    lo = LL.DAG_BIG // 2 + 2000
    assert (sub.reference(oracle)[lo:lo + 50] == exp[lo:lo + 50]).all()


# ---- device memory -------------------------------------------------------------------------------------------------------------------------
def test_every_context_stays_below_16_gib(capsys):
    from circuits_amd import lib
    L = lib()
    for template, kw, b in LL.CONTEXTS:
        n = L.template_device_bytes(template, n_instances=b, **kw)
        with capsys.disabled():
            print("\n  %s x %d: %.3f GiB" % (template, b, n / 2 ** 30), end="")
        assert 0 < n < LL.GIB16, (template, b, n)


# ---- the audit table -----------------------------------------------------------------------------------------------------------------------
def test_every_launch_cap_in_the_sources_has_a_row():
    loose, stale = LL.audit_unmatched()
    assert not loose, "a launch cap or chunk constant without a row in launch_limits_common.AUDIT (add the row AND its test):\n" + "\n".join("%s:%d: %s" % x for x in loose)
    assert not stale, "rows of launch_limits_common.AUDIT that no source line holds any more:\n" + "\n".join("%s: %s" % (r[0], r[1]) for r in stale)
    for f, text, limit, where in LL.AUDIT:
        assert limit and where, (f, text)


def test_the_audit_notices_a_deleted_row_and_a_new_cap():
    scan = LL.audit_scan()
    for i in range(len(LL.AUDIT)):
        loose, _ = LL.audit_unmatched(LL.AUDIT[:i] + LL.AUDIT[i + 1:], scan)
        assert loose, LL.AUDIT[i][:2]
    new = scan + [("state.hip", 1, "if (blocks > 1024) blocks = 1024;")]
    loose, _ = LL.audit_unmatched(LL.AUDIT, new)
    assert loose == [new[-1]]
    import re
    for line in ("blocks = std::min<size_t>((n + 255) / 256, 4096);", "e - b < 65535u", "n > 32768)", "count, 1u << 22);", "grid_for(n, block_cap())"):
        assert any(re.search(p, line) for p in LL.AUDIT_PATTERNS), line
    assert not any(re.search(p, "  32768ull,") or re.search(p, "0x05632768u") for p in LL.AUDIT_PATTERNS)


def test_the_tests_the_table_names_exist():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_launch_limits.py")).read()
    defined = set(re.findall(r"^def (test_\w+)", text, re.M))
    named = set()
    for _, _, _, where in LL.AUDIT:
        if "test_launch_limits.py::" in where:
            named |= set(re.findall(r"\b(test_[a-z0-9_]+)", where.split("tests/test_launch_limits.py::", 1)[1]))
    named = {n for n in named if not n.startswith(("test_witness", "test_export_dev", "test_ledger"))}
    assert named and named <= defined, sorted(named - defined)
