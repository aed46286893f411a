"""Adversarial differential fuzz of the HIP path against the oracle (VERDICT r3 "parity gaps" 1a): >= 10 000 seeded instances each of
SMTProcessor(33), SMTVerifier(33), RollupTx(32, 64), Withdraw(32), and RollupMain batches, with inputs no builder makes (tests/fuzz_common.py).
Requirement per instance: the whole physical witness AND the first violated constraint (unit, constraint id, lhs, rhs) equal the
oracle's -- the calculator of the reference defines both for arbitrary field elements (reference test/rollup-tx.test.js:911-918,
test/rollup-main.test.js:868-877, test/withdraw.test.js:159-171). The CPU half checks the generators and the oracle's threading."""
import pytest

import fuzz_common as FZ
from oracle_binding import OracleCtx


# ---- CPU: the generators make what they claim, the oracle survives it, threads == one thread -------------------------------------
@pytest.mark.parametrize("template,shape,gen", [
    ("smt-processor", (0, 33, 0, 0), lambda n: FZ.smt_processor_cases(n, 33, 11)),
    ("smt-verifier", (0, 33, 0, 0), lambda n: FZ.smt_verifier_cases(n, 33, 12)),
    ("rollup-tx", (0, 16, 0, 4), lambda n: FZ.rollup_tx_cases(n, 16, 4, 13)),
    ("withdraw", (0, 16, 0, 0), lambda n: FZ.withdraw_cases(n, 16, 14)),
    ("rollup-main", (4, 16, 2, 2), lambda n: FZ.rollup_main_cases(n, (4, 16, 2, 2), 15)),
])
def test_oracle_on_garbage_threads_equal_serial(template, shape, gen):
    n = 96
    cases = gen(n)
    parts = FZ.run_oracle_threads(template, shape, cases, n_threads=4)
    one = FZ.run_oracle_threads(template, shape, cases, n_threads=1)
    fa, fb = FZ.oracle_failures(parts), FZ.oracle_failures(one)
    assert fa == fb
    # the mix: some instances stay valid, most are rejected, and not all by the same constraint
    assert 0 < len(fa) < n
    assert len({v[1] for v in fa.values()}) >= (2 if template == "withdraw" else 3)
    o1 = one[0][0]
    for o, lo, cnt in parts:
        for k in (0, cnt - 1):
            assert o.read(0, o.witness_len(), k) == o1.read(0, o1.witness_len(), lo + k)
        assert o.unwritten()[0] == 0   # a rejected witness is still complete


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _fuzz(hz, template, shape, gen, n_total, chunk, ctx_kw, flags=0):
    from circuits_amd import ConstraintError
    g = hz.ctx(template, n_instances=chunk, flags=flags, **ctx_kw)
    rejected = 0
    cids = set()
    for c0 in range(0, n_total, chunk):
        cases = gen(chunk, c0)
        FZ.set_all_inputs(g, cases)
        err = None
        try:
            g.run()
        except ConstraintError as e:
            err = e
        parts = FZ.run_oracle_threads(template, shape, cases)
        rejected += FZ.check_failures(g, parts, err)
        cids |= {v[1] for v in FZ.oracle_failures(parts).values()}
        if template == "rollup-main":
            total = g.total()
            assert total == sum(o.total() for o, _, _ in parts)
            for o, lo, cnt in parts:
                wl = o.witness_len()
                for k in range(cnt):
                    for first in range(0, wl, 1 << 17):
                        c = min(1 << 17, wl - first)
                        assert g.read_bytes(first, c, lo + k) == o.read_bytes(first, c, k), "instance %d, elements from %d" % (c0 + lo + k, first)
        else:
            FZ.compare_instanced(g, parts, chunk)
    if flags:
        g.close()   # flagged contexts one after the other: how many are alive decides the form of their chain kernel (ctx_step.hip enqueue_smt_chain)
    return rejected, cids


@pytest.mark.gpu
@pytest.mark.parametrize("template,shape,n_total,chunk", [
    ("smt-processor", (0, 33, 0, 0), 6144, 6144),
    ("smt-processor", (0, 33, 0, 0), 4096, 2048),    # contexts small enough for the latency form of the chain kernel (ctx.hip hz_ctx_create: its default here)
    ("smt-verifier", (0, 33, 0, 0), 10240, 10240),
    # (two chunks through ONE context each: the second step meets the first one's buffer -- constant marks, persistent scratch;
    #  10 240 instances of these two took a minute of a ten-minute suite for the same two kernel forms)
    ("withdraw", (0, 32, 0, 0), 4096, 2048),
    ("rollup-tx", (0, 32, 0, 64), 4096, 2048),
])
def test_hip_adversarial_fuzz(hz, template, shape, n_total, chunk):
    L, F = shape[1], shape[3]
    gen = {"smt-processor": lambda n, s: FZ.smt_processor_cases(n, L, 7000 + s),
           "smt-verifier": lambda n, s: FZ.smt_verifier_cases(n, L, 8000 + s),
           "withdraw": lambda n, s: FZ.withdraw_cases(n, L, 9000 + s),
           "rollup-tx": lambda n, s: FZ.rollup_tx_cases(n, L, F, 10000 + s)}[template]
    kw = {"nLevels": L}
    if template == "rollup-tx":
        kw["maxFeeTx"] = F
    rejected, cids = _fuzz(hz, template, shape, gen, n_total, chunk, kw)
    assert n_total // 2 < rejected < n_total and len(cids) >= (2 if template == "withdraw" else 4)


@pytest.mark.gpu
def test_hip_adversarial_fuzz_rollup_main(hz):
    """whole batches with garbage anywhere (transactions, fee slots, intermediate signals, key bits that are not bits): the front
    kernel's copied L1TxFullData rows, the early last-transaction chains, the fee chain and HashInputs on rejected batches"""
    shape = (4, 16, 2, 2)
    rejected, cids = _fuzz(hz, "rollup-main", shape, lambda n, s: FZ.rollup_main_cases(n, shape, 11000 + s), 1024, 512,
                           dict(nTx=4, nLevels=16, maxL1Tx=2, maxFeeTx=2))
    assert 450 < rejected < 1024 and len(cids) >= 6


def _with_signature_edges(cases, edges, seed):
    """`cases` with the first len(edges) of them replaced by the signature edges, in a seeded order"""
    import random
    assert len(edges) < len(cases) // 2
    out = list(edges) + cases[len(edges):]
    random.Random(seed).shuffle(out)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [2, 2 | 4], ids=["latency", "latency-solo"])
@pytest.mark.parametrize("template,shape,n_total", [("rollup-tx", (0, 32, 0, 64), 2048), ("rollup-main", (4, 16, 2, 2), 512)], ids=["rollup-tx", "rollup-main"])
def test_hip_adversarial_fuzz_flagged(hz, template, shape, n_total, flags):
    """Garbage and the signature edges (fuzz_common.signature_edge_cases) through contexts created with HZ_FLAG_LATENCY (2) and
    HZ_FLAG_LATENCY | HZ_FLAG_SOLO (6, include/hermez_witness.h), one launch each, the same requirements as the plain rows above.
    Which kernels that selects (ctx.hip hz_ctx_create / ctx_step.hip enqueue_smt_chain; the profile names do not tell the forms apart, so the
    rule is stated here): a RollupMain context with HZ_FLAG_LATENCY runs its chains on four CU-masked streams -- the split signature
    kernels (k_eddsa_pre_a beside the front kernel, k_eddsa_pre_b, k_eddsa_ladder<1>, k_eddsa_fix<1>, k_eddsa_final), k_main_feeacc
    behind the fixed-base kernel -- and, with at most 2 048 transactions per launch (512 x 4 here) and at most two such contexts alive
    on the device, k_smt<true> (a quad of lanes per chain); HZ_FLAG_SOLO keeps k_smt<true> whatever else is alive. A RollupTx
    context has no partition: HZ_FLAG_LATENCY alone leaves it the plain schedule, HZ_FLAG_SOLO gives it k_smt<true> (2 048
    instances: the limit). Every context here is closed before the next one is made."""
    nTx, L, m1, F = shape
    if template == "rollup-tx":
        def gen(n, s):
            labels, cases = FZ.signature_form_tx_cases(L, F, 12000 + s, n_bases=4, n_garbage=n)
            edges = [d for lb, d in zip(labels, cases) if lb.startswith("tx ")]
            return _with_signature_edges(cases[len(cases) - n:], edges, 12500 + s)
        kw = {"nLevels": L, "maxFeeTx": F}
    else:
        def gen(n, s):
            from circuits_amd import builder as B
            edges = []
            for b in range(4):
                inp = B.synthetic_batch(nTx, L, m1, F, n_accounts=4 + b, exits=1, seed=13500 + s + b).get_input()
                edges += [d for _, d in FZ.rollup_main_signature_edges(inp)]
            return _with_signature_edges(FZ.rollup_main_cases(n, shape, 13000 + s), edges, 13900 + s)
        kw = dict(nTx=nTx, nLevels=L, maxL1Tx=m1, maxFeeTx=F)
    rejected, cids = _fuzz(hz, template, shape, gen, n_total, n_total, kw, flags=flags)
    assert n_total // 2 < rejected < n_total and len(cids) >= (4 if template == "rollup-tx" else 6)
