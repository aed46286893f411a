"""The CPU half of tests/test_export_derived.py: the literal reference and the inputs of its launches held to their claims without a GPU
(tests/export_derived_common.py)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import declared_forms as DF   # noqa: E402
import export_derived_common as X   # noqa: E402


@pytest.fixture(scope="module")
def main_set():
    return X.reference_set("rollup-main", X.MAIN_KW, X.main_batches())


@pytest.fixture(scope="module")
def rtx_set():
    return X.reference_set("rollup-tx", X.RTX_KW, X.rollup_tx_cases())


@pytest.fixture(scope="module")
def wd_set():
    return X.reference_set("withdraw", dict(nLevels=16), X.withdraw_inputs())


def test_literal_reference_equals_the_recorded_system(rtx_set):
    """a second reference for the first: on the accepted RollupTx(16,2) cases the literal values == what follows from the ORACLE's
    stored signals through the reference's own recorded constraints (tests/declared_forms.py, Poseidon by the host library)"""
    from circuits_amd import builder as B
    names, refs, o = rtx_set
    m = DF.load("rollup-tx")
    assert tuple(m["args"]) == (X.RTX_KW["nLevels"], X.RTX_KW["maxFeeTx"])
    accepted = [k for k in range(X.RTX_N) if o.failure_of(k) is None]
    stored_names = [n for n in DF.all_names(m) if n in names.index]
    assert len(stored_names) > 20000
    n_checked = 0
    for k in accepted:
        ref = refs[k]
        known = {n: ref.get(n) for n in stored_names}
        val, unknown = DF.solve_with_hashes(m, known, lambda xs: B.host().poseidon(xs))
        assert not unknown, (k, unknown[:5])
        for e in range(len(names.names)):
            nm = names.names[e]
            if names.kind[e] == X.STORED or nm not in val:
                continue
            n_checked += 1
            if ref.literal[e]:
                assert ref.value(e) == val[nm], (k, nm, X.KIND_NAMES[names.kind[e]])
            else:
                assert names.checks[nm](val[nm], ref.get), (k, nm)
    derived = int((names.kind != X.STORED).sum())
    assert n_checked >= len(accepted) * derived * 9 // 10   # (the recorded system names nearly every variable of the synthetic compile)


@pytest.mark.parametrize("case", ["main", "withdraw", "rollup-tx"])
def test_neighbouring_instances_differ_in_every_kind(request, case):
    """instance k of a launch holds input k mod (number of inputs): every two neighbours (the wrap-around included, and 8 -> 5
    instances keeps the cycle) differ in at least one derived variable of each kind present -- Poseidon-internal, linear form, IsZero
    input, product, quotient -- so a kernel that drops or doubles the
    instance term cannot pass. Products and quotients are the variables the maps' .r1cs defines over derived ones (Names.add_solved)."""
    names, refs, _ = request.getfixturevalue({"main": "main_set", "withdraw": "wd_set", "rollup-tx": "rtx_set"}[case])
    n = len(refs)
    assert n >= 3
    kinds = {X.KIND_NAMES[k] for k in (X.POSEIDON, X.FORM, X.ISZERO, X.PRODUCT, X.QUOTIENT) if (names.kind == k).any()}
    assert kinds == {"Poseidon", "form", "IsZero", "product", "quotient"}
    pairs = [(a, (a + 1) % n) for a in range(n)]
    if case == "withdraw":
        pairs.append(((X.WD_N - 1) % n, 0))
    for a, b in pairs:
        if a == b:
            continue
        d = X.neighbours_differ(names, refs[a], refs[b])
        assert set(d) == kinds and all(v > 0 for v in d.values()), (case, a, b, d)


def test_garbage_shares(rtx_set):
    """at least 8 accepted and 8 rejected among the 48, decided by the oracle alone; and the rejected ones not all by one constraint"""
    _, _, o = rtx_set
    fails = [o.failure_of(k) for k in range(X.RTX_N)]
    rejected = [f for f in fails if f is not None]
    assert len(rejected) >= 8 and X.RTX_N - len(rejected) >= 8
    assert len({f[1] for f in rejected}) >= 3
    # both kinds inside the first wavefront's first and second half, and in every block of 16 lanes
    for lo in range(0, X.RTX_N, 16):
        blk = fails[lo:lo + 16]
        assert any(f is None for f in blk) and any(f is not None for f in blk), lo


def test_solved_variables_read_derived_ones(main_set, wd_set, rtx_set):
    """the variables the maps' .r1cs defines: each reads at least one derived variable, three linear ones in four read the one before
    (dependency levels), the .r1cs exists for a full map and not for a map without them; among the garbage cases a quotient's divisor
    is 0 for some instances and not for others"""
    for names, refs, _ in (main_set, wd_set, rtx_set):
        assert len(names.solved) == sum(X.N_SOLVED) and len(names.names) == names.n_base + len(names.solved)
        for i, forms in enumerate(names.solved):
            read = [e for f in forms if f for _, e in f[1]]
            assert all(e < names.n_base + i for e in read) and any(names.kind[e] != X.STORED for e in read)
            if i < X.N_SOLVED[0] and i % 4:
                assert names.n_base + i - 1 in read
        assert X.Sym(names, 1).r1cs[:4] == b"r1cs" and X.Sym(names, 1, keep=range(names.n_base)).r1cs is None
    names, refs, _ = rtx_set
    zero = [sum(r.form_value(fb) == 0 for r in refs) for fa, fb, fc in names.solved if fa is None]
    assert any(0 < z < len(refs) for z in zero), zero


def test_partial_map_subsets(main_set):
    names, _, _ = main_set
    fifth, half = X.partial_keeps(names, 0xD5)
    n = names.n_base
    assert 0.18 * n < len(fifth) < 0.22 * n
    st = names.kind == X.STORED
    in_fifth, in_half = set(map(int, fifth)), set(map(int, half))
    for e in map(int, st.nonzero()[0]):
        assert (e in in_fifth) != (e in in_half)
    n_der = int((~st[:n]).sum())
    assert 0.45 * n_der < sum(1 for e in in_half if not st[e]) < 0.55 * n_der
    per = X.named_per_component(names, fifth)
    assert len(per) == len(names.blocks)
    assert sum(1 for a, b in per.values() if 1 < a < b) > len(per) // 2      # some but not all slots named
    assert sum(1 for a, b in per.values() if a == 1) >= 2                      # a single slot named
    # two variables that name ONE slot of a component's trace are in the full map (sigmaF[0][j].in is ark[0].out[j]) and in `half`
    pairs = [(c + ".sigmaF[0][1].in", c + ".ark[0].out[1]") for c in sorted(names.blocks)]
    assert all(a in names.entry and b in names.entry for a, b in pairs)
    assert sum(1 for a, b in pairs if names.entry[a] in in_half and names.entry[b] in in_half) >= 10


def test_names_are_the_same_for_every_input_and_all_kinds_present(main_set, wd_set, rtx_set):
    for names, refs, _ in (main_set, wd_set, rtx_set):
        assert len(names.names) == len(set(names.names))
        for r in refs:
            assert r.rows.shape == (len(names.names), 32) and r.literal.sum() + len(names.checks) == len(names.names)
    assert main_set[0].widths() == {3, 4, 5, 6, 7} and wd_set[0].widths() == {3, 4, 5} and rtx_set[0].widths() == {3, 4, 5, 6}
