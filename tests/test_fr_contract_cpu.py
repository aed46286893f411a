"""The contract table of fr.h (tests/fr_contract_common.py) without a GPU: the table is what it says it is, the host compile of
fr.h keeps every contract (tests/native/fr_contract_host.cpp: Python integers as the reference, not fr.h against fr.h), and the
table, fr.h's comments and the models of tools/range_check.py agree about every range."""
import os
import re
import sys

import pytest

import fr_contract_common as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import range_check as RC  # noqa: E402

P, R = FC.P, FC.R


def _header_codes():
    """the HZ_FRR_* enumerators of include/hermez_witness.h, evaluated"""
    text = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    body = re.search(r"enum \{ (HZ_FRR_ADD.*?)\};", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    codes, nxt = {}, 0
    for item in (x.strip() for x in body.split(",")):
        if not item:
            continue
        if "=" in item:
            name, expr = (s.strip() for s in item.split("="))
            nxt = eval(expr, {}, dict(codes))
        else:
            name = item
        codes[name] = nxt
        nxt += 1
    return codes


def test_the_table_names_the_headers_op_codes():
    H = _header_codes()
    assert H["HZ_FRR_COUNT"] == FC.N_OPS == len({o.code for o in FC.OPS.values()})
    for name, op in FC.OPS.items():
        m = re.fullmatch(r"fr_dot(\d)(_add)?", name)
        want = H["HZ_FRR_DOT1_ADD" if m.group(2) else "HZ_FRR_DOT1"] + int(m.group(1)) - 1 if m else H["HZ_FRR_" + name[3:].upper()]
        assert op.code == want, name


def test_the_table_sends_its_edges_and_drops_nothing():
    for name, op in FC.OPS.items():
        sent = FC.operands(name)
        assert len(sent) == op.cap() <= FC.CAP and FC.packed(name).shape == (len(op.kinds), len(sent), 9), name
        assert all(op.pre(t) for t in sent), name
        have = set(sent)
        for k, edges in enumerate(op.edge_lists):       # every admissible edge of the issue's list reaches every operand
            want = [e for e in (FC.EDGES if op.kinds[k] == "fr" else edges) if e < op.ubs[k]]
            assert want and set(want) <= {t[k] for t in sent}, (name, k)
        if len(op.kinds) <= 3:                          # the full cross product of the admissible edges
            prod = op.edge_product()
            assert prod and set(prod) <= have, name
            n_free = 1
            for e in op.edge_lists:
                n_free *= len(e)
            assert len(prod) == n_free or op.joint is not None, name
        else:                                           # seeded draws from the edges and the all-maximal tuple
            assert len(sent) >= FC.EDGE_DRAWS and set(op.extra) <= have, name
        # the same list for every runner: regenerated from the seed, it is identical
        assert FC.operands.__wrapped__(name) == sent, name
        # what is packed is what was generated: limbs back to integers
        arr = FC.packed(name)
        for i in (0, len(sent) // 2, len(sent) - 1):
            for k, kind in enumerate(op.kinds):
                back = FC.value(arr[k, i]) if kind == "fr" else sum(int(v) << (32 * j) for j, v in enumerate(arr[k, i]))
                assert back == sent[i][k], (name, i, k)
    assert FC.operands("fr_dot6")[0] == (FC.LIMIT - 1,) * 12      # the tightest column accumulator of the file
    for name in ("fr_cond_sub_p_rare", "fr_canon_limbs", "fr_inv"):
        sc = FC.wave_scenarios(name)
        assert sc and FC.wave_scenarios.__wrapped__(name) == sc
        assert {len(t) % 64 for _, t in sc} >= ({0, 1, 63} if name != "fr_inv" else {0, 1})


def test_the_requirements_reject_wrong_results():
    """the judge is not vacuous: a representative outside the bound, a wrong limb, an unnormalised limb and a wrong boolean fail"""
    import numpy as np
    op = FC.OPS["fr_add"]
    t = (1 << 29, 5)
    FC.judge(op, [t], np.array([FC.limbs(sum(t))], dtype=np.uint32), "self")
    unnormalised = [sum(t)] + [0] * 8                      # the right integer, limb 0 not below 2^29
    for wrong in (FC.limbs(sum(t) + 2 * P), FC.limbs(sum(t) + 1), unnormalised):
        with pytest.raises(AssertionError, match="fr_add .self. element 0 .lane 0"):
            FC.judge(op, [t], np.array([wrong], dtype=np.uint32), "self")
    mul = FC.OPS["fr_mul"]
    a, b = P - 1, FC.LIMIT - 1
    FC.judge(mul, [(a, b)], np.array([FC.limbs(a * b * FC.RINV % P)], dtype=np.uint32), "self")
    with pytest.raises(AssertionError, match="floor"):
        FC.judge(mul, [(1, 1)], np.array([FC.limbs(FC.RINV + P)], dtype=np.uint32), "self")     # congruent, but above floor(T / R) + p
    with pytest.raises(AssertionError, match="boolean"):
        FC.judge(FC.OPS["fr_is_zero"], [(P,)], np.zeros((1, 9), dtype=np.uint32), "self")
    with pytest.raises(AssertionError, match="exactly"):
        FC.judge(FC.OPS["fr_cond_sub_p"], [(P,)], np.array([FC.limbs(P)], dtype=np.uint32), "self")
    with pytest.raises(AssertionError, match="above 0"):
        FC.judge(FC.OPS["fr_sub_lazy"], [(0, 0)], np.zeros((1, 9), dtype=np.uint32), "self")


@pytest.fixture(scope="module")
def host_runner(tmp_path_factory):
    return FC.build_host_runner(str(tmp_path_factory.mktemp("fr_contract") / "fr_contract_host"))


@pytest.mark.parametrize("name", list(FC.OPS))
def test_host_fr_routine_keeps_its_contract(host_runner, name):
    op = FC.OPS[name]
    FC.judge(op, FC.operands(name), FC.run_host(host_runner, op, FC.packed(name)), "host")


# ---- the tie to the proof ------------------------------------------------------------------------------------------------------------
def _dot_model(n, add):
    return lambda *v: RC.fr_dot(list(v[0:2 * n:2]), list(v[1:2 * n:2]), v[2 * n] if add else None)


MODELS = {
    "fr_add": RC.fr_add, "fr_sub": RC.fr_sub, "fr_neg": lambda a: RC.fr_sub(RC.const(0, "zero"), a), "fr_dbl": RC.fr_dbl,
    "fr_sub_lazy": RC.fr_sub_lazy, "fr_dbl_lazy": RC.fr_dbl_lazy, "fr_add_lazy": RC.fr_add_lazy, "fr_sub2_lazy": RC.fr_sub2_lazy,
    "fr_3a_b_c_lazy": RC.fr_3a_b_c_lazy, "fr_sub3": RC.fr_sub3, "fr_sub_a_2x": RC.fr_sub_a_2x, "fr_cond_sub_2p": RC.fr_cond_sub_2p,
    "fr_cond_sub_4p": RC.fr_cond_sub_4p, "fr_cond_sub_p": RC.fr_cond_sub_p, "fr_cond_sub_p_rare": RC.fr_cond_sub_p_rare,
    "fr_is_zero": RC.fr_is_zero, "fr_mul": RC.fr_mul, "fr_sqr": RC.fr_sqr, "fr_muladd": RC.fr_muladd, "fr_muladd2": RC.fr_muladd2,
    "fr_canon_limbs": RC.fr_canon_limbs, "fr_inv": RC.fr_inv,
    # conversions are products with the constant R^2 (fr.h: fr_mul(fr_unpack(c), r2))
    "fr_from_canon": lambda c: RC.fr_mul(c, RC.const(FC.R2, "R^2")), "fr_from_u64": lambda c: RC.fr_mul(c, RC.const(FC.R2, "R^2")),
}
for _n in range(1, 7):
    MODELS["fr_dot%d" % _n] = _dot_model(_n, False)
    MODELS["fr_dot%d_add" % _n] = _dot_model(_n, True)
# no model in tools/range_check.py: fr_eq (fr_sub then fr_is_zero), fr_to_canon, fr_pack_canon, fr_inv_fermat, fr_pow
UNMODELLED = {"fr_eq", "fr_to_canon", "fr_pack_canon", "fr_inv_fermat", "fr_pow"}


def _tie_points(op):
    """operand bounds (exclusive) at which the model is evaluated: the corners of the precondition; where the precondition ties
    operands together, every admissible tuple of edges as its own corner as well"""
    pts = list(op.points)
    if op.joint is not None:
        pts += [tuple(x + 1 for x in t) for t in op.edge_product()] if len(op.kinds) <= 3 else [tuple(x + 1 for x in t) for t in FC.operands(op.name)[:FC.EDGE_DRAWS]]
    return pts


@pytest.mark.parametrize("name", list(FC.OPS))
def test_the_table_and_the_proof_state_the_same_ranges(name):
    op = FC.OPS[name]
    if name in UNMODELLED:
        assert name not in MODELS
        return
    model = MODELS[name]
    for ubs in _tie_points(op):
        top = tuple(u - 1 for u in ubs)
        assert op.pre(top), (name, ubs)                      # the corner is inside the table's precondition ...
        res = model(*[RC.V(u, name="operand %d" % k) for k, u in enumerate(ubs)])   # ... and the model accepts it: no RangeError
        if op.bound is None:
            continue
        table_ub = op.bound(top)                             # the requirement's bound is monotone in the operands: worst at the corner
        if name == "fr_inv":
            # The contract says "below 2p"; the model states what today's fr_inv gives (a product with R^3, 1.0x p). The proof must
            # not lean on the difference: the callers' bounds are re-proved below with the contract's 2p in the model's place.
            assert res.ub <= table_ub
            continue
        assert table_ub <= res.ub, "%s: the table admits results up to %s, the proof assumes below %s" % (name, FC.in_p(table_ub), FC.in_p(res.ub))
    # one step outside the table's precondition the model refuses too, wherever it states a limit of its own
    for k, u in enumerate(op.ubs):
        if op.kinds[k] != "fr" or (name, k) in FREE_OPERANDS:
            continue
        out = [RC.V(1 if op.joint is not None and j != k else x, name="operand") for j, x in enumerate(op.points[0])]
        out[k] = RC.V(u + 1, name="outside")
        with pytest.raises(RC.RangeError):
            model(*out)


# operands whose range the routine leaves open ("a in [0, A)": the table sends them up to 2^257, the model takes any A)
FREE_OPERANDS = {("fr_sub_lazy", 0), ("fr_dbl_lazy", 0), ("fr_add_lazy", 0), ("fr_add_lazy", 1), ("fr_sub2_lazy", 0), ("fr_3a_b_c_lazy", 0),
                 ("fr_3a_b_c_lazy", 1), ("fr_3a_b_c_lazy", 2),
                 ("fr_canon_limbs", 0)} | {   # (fr_canon_limbs: the model takes a up to R, the table stops at a multiplicand's 2^257)
                ("fr_dot%d_add" % n, 2 * n) for n in range(1, 7)}


def test_the_callers_hold_with_the_contracts_bound_for_the_inverse(monkeypatch):
    """fr_inv's contract is "below 2p"; range_check models the tighter figure of the present routine. With 2p in its place every
    caller that uses an inverse (batch_inv, the signature ladders, the doubling chain) still stays inside its ranges."""
    def contract_inv(a):
        RC.need(a.ub <= 2 * P, "fr_inv: %r not below 2p" % a)
        return RC.V(2 * P, name="fr_inv (contract)")
    monkeypatch.setattr(RC, "fr_inv", contract_inv)
    for G in (1, 2, 3, 4):
        RC.seg_any_step(G)
    for G in (1, 8):
        RC.seg_fix_step(G)
    RC.ed_dbl_proj_chain(147)
