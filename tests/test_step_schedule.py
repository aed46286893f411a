"""The schedule of a step (csrc/ctx_step.hip): every way a context can order the same kernels -- the throughput schedule (early tail), the
CU-partitioned one (HZ_FLAG_LATENCY, with and without HZ_FLAG_SOLO), profiling on, profiling exclusive (every stream role on the launch
stream, nothing piped), a caller's stream instead of the context's own, a tx-sharded step with either tail -- leaves the same witness
buffer and reports the same first failure; the profile records of every schedule come in a pinned order; and what the constant marks
left in place is subtracted from the record of the chain that left it.

Shapes. RollupMain with two instances:
  MAIN_SMALL (4, 16, 2, 2)    6 SHA-256 blocks: HashInputs in one chain launch and one expansion. nTx = 4: the last transaction's early
                              launch has one unit per instance and the `skip_mod` of the main launch leaves three. No shape of nTx = 4
                              reaches 64 blocks (maxL1Tx <= nTx: at most 912 + 4 * 624 + 4 * 144 + 64 * 48 = 7 056 bits, 14 blocks).
  MAIN_PIPED (48, 16, 48, 2)  68 blocks (912 + 48 * 624 + 48 * 80 + 2 * 16 = 34 736 bits): from 64 blocks the expansion is piped over a second
                              stream in eight groups of 9 blocks, the last of 5.
(blocks = (bits + 64) // 512 + 1, bits = 912 + maxL1Tx * 624 + nTx * (2 * nLevels + 48) + maxFeeTx * nLevels: include/hz_layout.h; the
test asserts hz_sha_blocks() on either side of 64.) Standalone templates: the instances tests/test_gadget_mains.py runs."""
import json
import os

import pytest

import fuzz_common as FZ
from oracle_binding import OracleCtx

pytestmark = pytest.mark.gpu

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MAIN_SMALL = (4, 16, 2, 2)
MAIN_PIPED = (48, 16, 48, 2)
LATENCY, SOLO = 2, 4
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "step_profile_order.json")


def sha_blocks(shape):
    n_tx, n_levels, max_l1, max_fee = shape
    return (912 + max_l1 * 624 + n_tx * (2 * n_levels + 48) + max_fee * n_levels + 64) // 512 + 1


def _main_inputs(shape):
    """two batches of one shape (the two instances), and the same pair with one input of instance 1 deliberately unsatisfied: garbage
    siblings under transaction 1's first processor, so its root check fails"""
    from circuits_amd import builder as B
    n_tx, n_levels, max_l1, max_fee = shape
    exits = 1 if n_tx - max_l1 > 1 else 0
    good = [B.synthetic_batch(n_tx, n_levels, max_l1, max_fee, n_accounts=4 + 3 * b, exits=exits, seed=0x5C4ED + b).get_input() for b in range(2)]
    bad1 = dict(good[1])
    sib = [list(r) for r in bad1["siblings1"]]
    sib[1] = [(7 * j + 11) % P for j in range(len(sib[1]))]
    bad1["siblings1"] = sib
    return good, [good[0], bad1]


def _oracle(shape, pair):
    o = OracleCtx("rollup-main", *shape, n_instances=2)
    for b, inp in enumerate(pair):
        o.set_inputs(inp, instance=b)
    return o, o.run()


@pytest.fixture(scope="module", params=[MAIN_SMALL, MAIN_PIPED], ids=str)
def main_case(request):
    """inputs and the oracle's buffers and first failure: computed once per shape, shared by every schedule, never changed"""
    shape = request.param
    good, bad = _main_inputs(shape)
    og, rg = _oracle(shape, good)
    ob, rb = _oracle(shape, bad)
    assert rg is None and rb is not None and rb[0] == 1, (rg, rb)
    return {"shape": shape, "good": good, "bad": bad, "good_buf": og.read_raw_bytes(), "bad_buf": ob.read_raw_bytes(),
            "failure": (rb[0], rb[1], rb[2], rb[4], rb[5])}


def _ctx(hz, shape, flags=0, n_instances=2):
    return hz.ctx("rollup-main", nTx=shape[0], nLevels=shape[1], maxL1Tx=shape[2], maxFeeTx=shape[3], n_instances=n_instances, flags=flags)


def _step(g, pair, stream):
    """one step of both instances -> the first failure, or None"""
    from circuits_amd import ConstraintError
    for b, inp in enumerate(pair):
        g.set_inputs(inp, instance=b)
    try:
        if stream is None:
            g.run()
        else:
            g.enqueue(stream)
            g.check()
    except ConstraintError as e:
        return (e.instance, e.unit, e.constraint_id, e.lhs, e.rhs)
    return None


# (flags, profiling: 0 off / 1 on / 2 exclusive, through a caller's stream)
SCHEDULES = {
    "plain": (0, 0, False),
    "latency": (LATENCY, 0, False),
    "latency-solo": (LATENCY | SOLO, 0, False),
    "profiled": (0, 1, False),
    "exclusive": (0, 2, False),
    "latency-exclusive": (LATENCY, 2, False),
    "caller-stream": (0, 0, True),
    "latency-caller-stream": (LATENCY, 0, True),
}


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_every_schedule_gives_the_same_buffer(hz, main_case, schedule):
    """Three steps through ONE context of each schedule: the valid pair (a fresh buffer), the pair with the unsatisfied input (the marks of
    step one in place), and -- after hz_clear_inputs, which makes the next step clear the marks first -- the valid pair again. After every
    step the WHOLE physical buffer equals the oracle's, which is one buffer for all schedules; the failure of step two is the oracle's,
    instance, unit, constraint and operands."""
    import torch
    flags, prof, own_stream = SCHEDULES[schedule]
    shape = main_case["shape"]
    g = _ctx(hz, shape, flags)
    assert (g.sha_blocks() >= 64) == (shape == MAIN_PIPED) and g.sha_blocks() == sha_blocks(shape)
    if prof:
        g.set_profiling(True, exclusive=prof == 2)
    s = torch.cuda.Stream().cuda_stream if own_stream else None
    assert _step(g, main_case["good"], s) is None
    assert g.read_raw_bytes() == main_case["good_buf"], "step 1"
    assert _step(g, main_case["bad"], s) == main_case["failure"]
    assert g.read_raw_bytes() == main_case["bad_buf"], "step 2"
    g.clear_inputs()
    assert _step(g, main_case["good"], s) is None
    assert g.read_raw_bytes() == main_case["good_buf"], "step 3"
    g.close()


@pytest.mark.parametrize("tail", ["tail", "tail_chain"])
def test_sharded_step_with_either_tail_gives_the_same_buffer(hz, main_case, tail):
    """one context as the only rank of a tx-sharded step (its shard: every transaction), the tail on a caller's stream: the whole
    HashInputs, or message and chain alone with the expansion through hz_sha_expand -- two steps, the buffer of instance 0's batch"""
    import torch
    shape = main_case["shape"]
    o = OracleCtx("rollup-main", *shape)
    o.set_inputs(main_case["good"][0])
    assert o.run() is None
    g = _ctx(hz, shape, n_instances=1)
    g.set_shard(0, shape[0], True)
    g.set_inputs(main_case["good"][0])
    s = torch.cuda.Stream().cuda_stream
    for step in range(2):
        g.enqueue(s)
        if tail == "tail":
            g.enqueue_tail(s)
        else:
            g.enqueue_tail_chain(s)
            g.sha_expand(0, g.sha_blocks(), None, s)
        g.check()
        assert g.read_raw_bytes() == o.read_raw_bytes(), step
    g.close()


def _standalone_cases():
    import test_gadget_mains as GM
    return GM.all_cases()


@pytest.mark.parametrize("case", _standalone_cases(), ids=lambda c: c.template)
def test_standalone_mains_under_every_stream_resolution(hz, case):
    """the gadget mains at the instances of tests/test_gadget_mains.py: own stream, profiling, profiling exclusive, a caller's stream --
    two steps each, the whole buffer against the oracle"""
    import torch
    import test_gadget_mains as GM
    good = [i for i, e in case.items if not isinstance(e, str)]
    n = len(good)
    o = OracleCtx(case.template, n_instances=n, **GM._oracle_kw(case.params))
    for k, inp in enumerate(good):
        o.set_inputs(inp, instance=k)
    assert o.run() is None
    ref = o.read_raw_bytes()
    for prof, own_stream in ((0, False), (1, False), (2, False), (0, True)):
        g = hz.ctx(case.template, n_instances=n, **case.params)
        if prof:
            g.set_profiling(True, exclusive=prof == 2)
        for k, inp in enumerate(good):
            g.set_inputs(inp, instance=k)
        s = torch.cuda.Stream().cuda_stream if own_stream else None
        for step in range(2):
            g.enqueue(s)
            g.check()
            assert g.read_raw_bytes() == ref, (prof, own_stream, step)
        g.close()


def _small_inputs(template):
    """(context parameters, inputs of one instance) of the standalone templates hz_witness_enqueue handles besides the gadget mains"""
    from circuits_amd import builder as B
    import random
    if template == "rollup-tx":
        bb = B.synthetic_batch(8, 16, 2, 2, n_accounts=6, exits=1, seed=5)
        return dict(nLevels=16, maxFeeTx=2), bb.get_single_tx_input(3)[0]
    if template == "decode-tx":
        return dict(nLevels=16), FZ.decode_tx_bases(16)[0]
    if template == "fee-tx":
        return dict(nLevels=16), FZ.fee_tx_cases(1, 16, 3)[0]
    if template == "hash-state":
        return dict(), FZ.hash_state_cases(1, 3)[0]
    if template == "withdraw":
        fx = B.ExitTreeFixture(8, seed=3)
        return dict(nLevels=16), B.withdraw_input(fx, sorted(fx.exit_leaves)[0], 16)[0]
    if template == "hash-inputs":
        return dict(nTx=4, nLevels=16, maxL1Tx=2, maxFeeTx=2), FZ.hash_inputs_valid(random.Random(3), MAIN_SMALL)
    if template == "hash-inputs piped":   # (64 blocks or more: the expansion piped over the fee stream -- the launch stream itself under exclusive)
        return dict(nTx=48, nLevels=16, maxL1Tx=48, maxFeeTx=2), FZ.hash_inputs_valid(random.Random(4), MAIN_PIPED)
    if template == "smt-processor":
        return dict(nLevels=16), FZ.smt_processor_cases(1, 16, 3)[0]
    if template == "smt-verifier":
        return dict(nLevels=16), FZ.smt_verifier_cases(1, 16, 3)[0]
    raise KeyError(template)


SMALL_TEMPLATES = ["rollup-tx", "decode-tx", "fee-tx", "hash-state", "withdraw", "hash-inputs", "smt-processor", "smt-verifier"]


@pytest.mark.parametrize("template", SMALL_TEMPLATES + ["hash-inputs piped"])
def test_standalone_templates_under_every_stream_resolution(hz, template):
    """the standalone templates whose steps use the stream roles -- RollupTx (signature and fixed-base streams, joined by ev_ed),
    Withdraw (the SHA part on the signature stream), HashInputs below and from 64 blocks (piped over the fee stream), FeeTx and
    SMTProcessor (the fee chain) -- and the other one-launch mains: own stream, profiling, profiling exclusive, a caller's stream --
    two steps each, the whole buffer and the first failure against the oracle"""
    import torch
    from circuits_amd import ConstraintError
    params, inp = _small_inputs(template)
    name = template.split()[0]
    o = OracleCtx(name, **params)
    o.set_inputs(inp)
    r = o.run()
    failure = None if r is None else (r[0], r[1], r[2], r[4], r[5])
    ref = o.read_raw_bytes()
    for prof, own_stream in ((0, False), (1, False), (2, False), (0, True)):
        g = hz.ctx(name, **params)
        if template.endswith("piped"):
            assert g.sha_blocks() >= 64
        if prof:
            g.set_profiling(True, exclusive=prof == 2)
        g.set_inputs(inp)
        s = torch.cuda.Stream().cuda_stream if own_stream else None
        for step in range(2):
            got = None
            try:
                g.enqueue(s)
                g.check()
            except ConstraintError as e:
                got = (e.instance, e.unit, e.constraint_id, e.lhs, e.rhs)
            assert got == failure, (prof, own_stream, step)
            assert g.read_raw_bytes() == ref, (prof, own_stream, step)
        g.close()


# ---- 2: the order of the profile records ----------------------------------------------------------------------------------------------
def profile_orders(hz):
    """{label: [[name, units], ...]} of Ctx.profile() after one step, for every template hz_witness_enqueue handles and RollupMain in
    each of its schedules. tools or tests with another library behind HZ_WITNESS_LIB record the same table from it."""
    from circuits_amd import ConstraintError, HzError
    out = {}

    def order(g):
        return [[name, units] for name, _ms, _bytes, units in g.profile()]

    def run(g):
        try:   # (some generated cases are garbage by design: the records do not depend on what the kernels find)
            g.run()
        except (ConstraintError, HzError):
            pass

    import test_gadget_mains as GM
    seen = set()
    for case in GM.all_cases():
        if case.template in seen:
            continue
        seen.add(case.template)
        g = hz.ctx(case.template, **case.params)
        g.set_profiling(True)
        g.set_inputs(case.items[0][0])
        run(g)
        out[case.template] = order(g)
        g.close()
    for template in SMALL_TEMPLATES:
        params, inp = _small_inputs(template)
        g = hz.ctx(template, **params)
        g.set_profiling(True)
        g.set_inputs(inp)
        run(g)
        out[template] = order(g)
        g.close()
    good, _ = _main_inputs(MAIN_SMALL)
    for label, flags, exclusive in (("rollup-main plain", 0, False), ("rollup-main latency", LATENCY, False), ("rollup-main latency-solo", LATENCY | SOLO, False),
                                    ("rollup-main exclusive", 0, True), ("rollup-main latency exclusive", LATENCY, True)):
        g = _ctx(hz, MAIN_SMALL, flags)
        g.set_profiling(True, exclusive=exclusive)
        for b, inp in enumerate(good):
            g.set_inputs(inp, instance=b)
        run(g)
        out[label] = order(g)
        g.close()
    for tail in ("tail", "tail_chain"):
        g = _ctx(hz, MAIN_SMALL, n_instances=1)
        g.set_profiling(True)
        g.set_shard(0, MAIN_SMALL[0], True)
        g.set_inputs(good[0])
        g.enqueue()
        if tail == "tail":
            g.enqueue_tail()
        else:
            g.enqueue_tail_chain()
            g.sha_expand(0, g.sha_blocks())
        g.check()
        out["rollup-main sharded + " + tail] = order(g)
        g.close()
    return out


def test_profile_record_order_is_pinned(hz):
    """the (name, units) of every profile record, in order, equal what the library of the commit named in the fixture produced"""
    golden = json.load(open(GOLDEN))
    got = profile_orders(hz)
    assert sorted(got) == sorted(golden["orders"])
    for label in golden["orders"]:
        assert got[label] == golden["orders"][label], label


# ---- 3: skip accounting follows the chain ---------------------------------------------------------------------------------------------
def _chain_bytes(g, name="smt"):
    return [by for nm, _ms, by, _units in g.profile() if nm == name]


def test_standalone_smt_processor_subtracts_what_its_launch_left_in_place(hz):
    """The standalone SMTProcessor's chain launch is named "smt" and keeps the fee chain's marks and counter (its scratch is the fee
    scratch). Two profiled steps on the same inputs: on the second every empty level is left in place, and the record's
    algorithmic_bytes must say so. (Before the record remembered its chain, hz_profile_get subtracted the transaction chain's counter
    for every record named "smt", and no block of this template was attributed to the chain launch at all: both steps reported the same
    bytes, 0.)"""
    from circuits_amd import ConstraintError
    n = 64
    cases = FZ.smt_processor_cases(n, 16, 77)
    g = hz.ctx("smt-processor", nLevels=16, n_instances=n)
    g.set_profiling(True)
    FZ.set_all_inputs(g, cases)
    seen = []
    for _ in range(2):
        try:
            g.run()
        except ConstraintError:   # mutated proofs violate constraints; the records are what is read here
            pass
        by = _chain_bytes(g)
        assert len(by) == 1
        seen.append(by[0])
    assert seen[1] < seen[0], seen
    g.close()


def test_throughput_main_subtracts_the_early_launch_of_the_last_transactions(hz, main_case, monkeypatch):
    """Throughput RollupMain: the transaction chain's record stands for the main launch AND the early launch of the last transaction of
    every batch. The second step on the same inputs leaves the empty levels of both in place: its "smt" bytes drop, and by no less than
    the drop of a context that evaluates every transaction in ONE launch with one counter (a CU-partitioned context has no early tail;
    the same kernel form for both: HZ_SMT_LATENCY_FORM=0). With the main launch's counter alone -- what hz_profile_get used to subtract
    -- the throughput context's drop lacks the last transactions' levels and falls short of it."""
    monkeypatch.setenv("HZ_SMT_LATENCY_FORM", "0")
    shape = main_case["shape"]
    g = _ctx(hz, shape)
    g.set_profiling(True)
    for b, inp in enumerate(main_case["good"]):
        g.set_inputs(inp, instance=b)
    seen = []
    for _ in range(2):
        g.run()
        by = _chain_bytes(g)
        assert len(by) == 1
        seen.append(by[0])
    assert seen[1] < seen[0], seen
    h = _ctx(hz, shape, LATENCY)
    h.set_profiling(True)
    for b, inp in enumerate(main_case["good"]):
        h.set_inputs(inp, instance=b)
    whole = []
    for _ in range(2):
        h.run()
        whole.append(_chain_bytes(h)[0])
    print("smt algorithmic_bytes, steps 1 and 2: throughput %r, one launch %r" % (seen, whole))
    assert whole[1] < whole[0] and seen[0] - seen[1] >= whole[0] - whole[1], (seen, whole)
    g.close()
    h.close()
