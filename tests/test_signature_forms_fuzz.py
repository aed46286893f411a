"""Garbage and signature edges through EVERY form of the signature kernels, against the oracle.

The signature check (EdDSAPoseidonVerifier inside RollupTx / RollupMain) runs in one of two kernel forms chosen by the size of the
launch (eddsa_kernels.hip eddsa_split_form, launch_eddsa_ladder / launch_eddsa_fix: the split form up to HZ_ED_SPLIT_MAX = 16 384 signatures, the throughput
form -- k_eddsa_seg<4>, k_eddsa_fix<8>, what bench.py measures -- above), and flagged contexts (HZ_FLAG_LATENCY, HZ_FLAG_SOLO) run a
third schedule around the split kernels. Which test covers which input class in which form -- a form that is added shows up here as a
row of empty cells:

  form                      | valid builder output                            | garbage (fuzz_common.mutate)                 | signature edges (fuzz_common.signature_edge_cases)
  --------------------------+-------------------------------------------------+----------------------------------------------+---------------------------------------------------
  split, RollupTx           | test_witness_gpu::test_rollup_tx_config2_*      | test_adversarial_fuzz::test_hip_adversarial_ | test_adversarial_fuzz::test_hip_adversarial_fuzz_
                            |                                                 | fuzz[rollup-tx]                              | flagged[rollup-tx-*] (plain schedule: see there)
  split, RollupMain         | test_witness_gpu::test_rollup_main_small_bit_   | test_adversarial_fuzz::test_hip_adversarial_ | test_adversarial_fuzz::test_hip_adversarial_fuzz_
  (k_eddsa_pre_a / _pre_b)  | exact, test_config4_*                           | fuzz_rollup_main                             | flagged[rollup-main-*] (same kernels)
  throughput, RollupTx      | test_witness_gpu::test_throughput_signature_    | test_throughput_form_garbage_rollup_tx       | test_throughput_form_garbage_rollup_tx;
                            | kernels_bit_exact                               |                                              | test_throughput_signature_kernels_bit_exact (s + l)
  throughput, RollupMain    | test_witness_gpu::test_throughput_rollup_main_  | test_throughput_form_garbage_rollup_main     | test_throughput_form_garbage_rollup_main
                            | many_batches, test_headline_launch_whole_buffer |                                              |
  flagged (LATENCY / SOLO)  | test_witness_gpu::test_latency_scheduling_flag_ | test_adversarial_fuzz::test_hip_adversarial_ | test_adversarial_fuzz::test_hip_adversarial_fuzz_
                            | bit_exact, test_constant_marks                  | fuzz_flagged                                 | flagged
  oracle alone (CPU)        | test_witness_cpu                                | test_adversarial_fuzz::test_oracle_on_       | test_signature_edge_cases_on_the_oracle
                            |                                                 | garbage_threads_equal_serial                 |

Lane -> signature mapping of the throughput kernels (k_eddsa_seg<G> and k_eddsa_fix<G>, `mk_io`): with n signatures and
nl = ceil(n / G) lanes, lane li holds units li, li + nl, ..., li + (G - 1) nl: slot g of every lane is the g-th stretch of nl units, a
lane's signatures are NOT neighbours in the launch, and a slot past the end repeats the lane's first unit (fuzz_common.lane_units).
The composition conditions below are stated on that mapping."""
import random

import pytest

import fuzz_common as FZ

S_RANGE = "rollupTx.sigVerifier: compConstant.out*enabled === 0"
S_N2B = "rollupTx.sigVerifier.snum2bits: Num2Bits(253) sum"


# ---- CPU: the oracle's side of the signature edges ---------------------------------------------------------------------------------
def test_signature_edge_cases_on_the_oracle():
    """Pins the inputs of the GPU tests: the valid base passes, every s in [l, 2^253) is rejected by CompConstant and by nothing
    before it (s + k l is the same point S * B8: both equality checks would pass), s >= 2^253 by the Num2Bits line before it, a
    rejected witness is complete, and the variants reach at least five different first constraints. With the verifier disabled
    (fromIdx = 0, onChain = 1) it reports nothing below 2^253."""
    from circuits_amd import builder as B
    bb = B.synthetic_batch(40, 16, 6, 4, n_accounts=12, exits=3, seed=4242)
    ins = [bb.get_single_tx_input(i)[0] for i in range(bb.nTx)]
    l2 = [i for i, d in enumerate(ins) if not d["onChain"] and d["fromIdx"]]
    l1c = [i for i, d in enumerate(ins) if d["onChain"] and d["newAccount"]]
    edges = FZ.signature_edge_cases(ins[l2[0]], ins[l2[1]], ins[l1c[0]])
    labels = [lb for lb, _ in edges]
    parts = FZ.run_oracle_threads("rollup-tx", (0, 16, 0, 4), [d for _, d in edges], n_threads=4)
    fails = FZ.oracle_failures(parts)
    first = {lb: (FZ.constraint_name(fails[i][1]) if i in fails else None) for i, lb in enumerate(labels)}
    assert labels[0] == "valid" and first["valid"] is None
    l, s = B.SUBORDER, ins[l2[0]]["s"]
    assert 0 < s < l
    in_range = 0
    for lb, d in edges:
        if " & " in lb or lb.startswith("create") or lb == "valid":   # verifier disabled / another transaction
            if " & " in lb and d["s"] < (1 << 253):
                assert first[lb] is None or "sigVerifier" not in first[lb], (lb, first[lb])
            continue
        if l <= d["s"] < (1 << 253):
            assert first[lb] == S_RANGE, (lb, first[lb])
            in_range += 1
        elif d["s"] >= (1 << 253):
            assert first[lb] == S_N2B, (lb, first[lb])
        else:
            assert first[lb] is not None and first[lb] != S_RANGE, (lb, first[lb])   # s itself is the only accepted value below l
    assert in_range >= 4 and first["s=s+1l"] == S_RANGE and first["s=l"] == S_RANGE and first["s=2^253-1"] == S_RANGE
    assert first["s=2^253"] == S_N2B and first["s=p-1"] == S_N2B
    assert len({v for v in first.values() if v is not None}) >= 5, sorted({str(v) for v in first.values()})
    for o, _, _ in parts:
        assert o.unwritten()[0] == 0


def _tx_table(n, rejected, accepted, seed):
    """which[] of the RollupTx launch: states first (forced slots of the ragged lanes, an accepted case in every lane of four and of
    eight, the rest rejected with probability 0.85), then the cases: every rejected case once in each of the four slot stretches"""
    rng = random.Random(seed)
    l4, l8 = FZ.lane_units(n, 4), FZ.lane_units(n, 8)
    state = [None] * n   # True: accepted
    ragged = [lane for lanes in (l4, l8) for lane in lanes if len(lane) < len(lanes[0])]   # lanes with padding slots
    for lane in ragged:
        state[lane[0]] = False   # the unit the padding repeats
    for lane in ragged:
        for u in lane[1:]:
            if state[u] is None:   # (unit 4 112 is the first of the ragged lane of four AND slot 1 of a ragged lane of eight: rejected)
                state[u] = True
    for lanes in (l4, l8):
        for lane in lanes:
            if not any(state[u] is True for u in lane):
                state[rng.choice([u for u in lane if state[u] is None])] = True
    for u in range(n):
        if state[u] is None:
            state[u] = rng.random() >= 0.85
    which = [None] * n
    nl = len(l4)
    for g in range(4):
        slots = [u for u in range(g * nl, min((g + 1) * nl, n)) if not state[u]]
        assert len(slots) >= len(rejected)
        rng.shuffle(slots)
        for j, u in enumerate(slots):
            which[u] = rejected[j] if j < len(rejected) else rng.choice(rejected)
    slots = [u for u in range(n) if state[u]]
    rng.shuffle(slots)
    for j, u in enumerate(slots):
        which[u] = accepted[j] if j < len(accepted) else rng.choice(accepted)
    return which


def _assert_tx_table(n, which, rejected):
    """the conditions the launch is built for, from the table itself"""
    rej, firsts = set(rejected), set()
    for per_lane in (4, 8):
        lanes = FZ.lane_units(n, per_lane)
        assert sorted(u for lane in lanes for u in lane) == list(range(n))
        assert all(any(which[u] not in rej for u in lane) for lane in lanes), "a lane of %d without an accepted signature" % per_lane
        assert 2 * sum(any(which[u] in rej for u in lane) for lane in lanes) >= len(lanes)
        ragged = [lane for lane in lanes if len(lane) < per_lane]
        assert ragged, "no lane with a padding slot"
        firsts |= {lane[0] for lane in ragged}
    for per_lane in (4, 8):
        for lane in FZ.lane_units(n, per_lane):
            if len(lane) < per_lane:   # first unit rejected, the others accepted (but a unit that is another ragged lane's first)
                assert which[lane[0]] in rej and all(which[u] not in rej for u in lane[1:] if u not in firsts)
                assert sum(u in firsts for u in lane[1:]) <= 1
    seen = {(which[u], g) for lane in FZ.lane_units(n, 4) for g, u in enumerate(lane)}
    assert all((d, g) in seen for d in rej for g in range(4)), "a rejected case that misses a slot of the lanes of four"
    assert n // 2 < sum(which[u] in rej for u in range(n)) < n


def _run(g):
    from circuits_amd import ConstraintError
    try:
        g.run()
    except ConstraintError as e:
        return e
    return None


@pytest.mark.gpu
def test_throughput_form_garbage_rollup_tx(hz):
    """RollupTx(16, 4) x 16 451 instances in one launch: the THROUGHPUT form (k_eddsa_pre, k_eddsa_seg<4>, k_eddsa_fix<8>,
    k_eddsa_final). About 1 300 distinct cases (fuzz_common.signature_form_tx_cases: 40 valid transactions, the signature edges of
    eight of them, 500 mutated ones), each evaluated once by the oracle and replicated by a seeded table which, asserted from the
    table on the real lane -> unit mapping (module docstring):
      * puts an accepted signature into every lane of four (k_eddsa_seg) and of eight (k_eddsa_fix) and a rejected one into at least half of them --
        the shared Montgomery inversion with its zero-divisor patches decides about accepted neighbours of hostile signatures;
      * has every rejected case in each of the four slots of some lane of four;
      * makes the first unit of every lane with a padding slot (16 451 = 4 x 4 113 - 1 = 8 x 2 057 - 5: one lane of four, five of
        eight) a rejected one -- the padding repeats it and must not report again -- and its other units accepted ones (but unit
        4 112, which is the first of the ragged lane of four and slot 1 of lane 2 055 of eight: rejected).
    Compared for EVERY instance: the whole physical buffer and the first-failure record against the oracle's for which[k], and the
    launch-wide error against the lowest failing instance. Then the table is rotated by one instance, the inputs are placed again
    and the same context runs again: whatever a rejected signature left in LDS, the lane buffer of the fixed-base kernel or the
    inter-kernel scratch meets another neighbour."""
    L, F, N = 16, 4, 16384 + 67
    labels, cases = FZ.signature_form_tx_cases(L, F, 4242, n_bases=8, n_garbage=500)
    D = len(cases)
    assert 1000 <= D <= 2000
    parts = FZ.run_oracle_threads("rollup-tx", (0, L, 0, F), cases)
    fails = FZ.oracle_failures(parts)
    rejected, accepted = sorted(fails), [d for d in range(D) if d not in fails]
    names = {labels[d]: FZ.constraint_name(fails[d][1]) for d in rejected}
    assert len({fails[d][1] for d in rejected}) >= 8 and sum(v == S_RANGE for v in names.values()) >= 8 * 4
    which = _tx_table(N, rejected, accepted, seed=20261)
    _assert_tx_table(N, which, rejected)
    g = hz.ctx("rollup-tx", nLevels=L, maxFeeTx=F, n_instances=N)
    for step in range(2):
        FZ.place_replicas(g, cases, which)
        err = _run(g)
        FZ.compare_replicated(g, parts, N, D, which)
        n_rej = FZ.check_failures(g, parts, err, which=which)
        assert N // 2 < n_rej < N
        which = which[-1:] + which[:-1]


def _main_cases(shape, seed):
    """(labels, cases, builder hash or None): valid batches, batches with one signature edge in an L2 transaction, mutated batches"""
    from circuits_amd import builder as B
    bbs = [B.synthetic_batch(*shape, n_accounts=6 + b, exits=b % 3, seed=seed + b) for b in range(6)]
    out = [("valid batch %d" % b, bb.get_input(), bb.get_hash_inputs()) for b, bb in enumerate(bbs)]
    for b in range(4):
        out += [("batch %d, %s" % (b, lb), d, None) for lb, d in FZ.rollup_main_signature_edges(bbs[b].get_input(), ("s=s+1l", "ay1=2", "r8=(0,1)"))]
    out += [("garbage %d" % k, d, None) for k, d in enumerate(FZ.rollup_main_cases(24, shape, seed + 100))]
    return [x[0] for x in out], [x[1] for x in out], [x[2] for x in out]


@pytest.mark.gpu
def test_throughput_form_garbage_rollup_main(hz):
    """RollupMain(8, 16, 3, 4) x 2 060 batches in one set of launches (16 480 transactions: the throughput form, every ladder lane
    holds transactions of four DIFFERENT batches, every lane of the fixed-base kernel of eight). 42 distinct batches -- six valid,
    twelve with one signature edge (s + l, an ay1 without a point, R8 = (0, 1)) in an L2 transaction, 24 mutated anywhere -- replicated by a
    seeded table. Per instance: the first-failure record and hashGlobalInputs against the oracle's for which[k] (valid batches: the
    builder's hash as well -- the accepted neighbours of a rejected batch in the same lanes); the launch-wide error; the complete
    logical witness of every distinct batch's first replica and of the first, a middle and the last instance. Then the table
    rotated by one batch, on the same context."""
    shape, N = (8, 16, 3, 4), 2060
    labels, cases, hashes = _main_cases(shape, 900)
    D = len(cases)
    assert 24 <= D <= 48
    parts = FZ.run_oracle_threads("rollup-main", shape, cases)
    fails = FZ.oracle_failures(parts)
    part_of = {lo + k: (o, k) for o, lo, cnt in parts for k in range(cnt)}
    valid = [d for d in range(D) if hashes[d] is not None]
    assert not any(d in fails for d in valid) and len(fails) >= D // 2 and len({v[1] for v in fails.values()}) >= 6
    for lb, want in (("s=s+1l", S_RANGE), ("ay1=2", "rollupTx.getAx.b2Point.babyCheck")):
        assert all(FZ.constraint_name(fails[d][1]) == want for d in range(D) if labels[d].endswith(lb))
    rng = random.Random(20262)
    which = list(range(D)) + [rng.choice(valid) if rng.random() < 0.3 else rng.choice(sorted(fails)) for _ in range(N - D)]
    rng.shuffle(which)
    # transaction u = 8 k + t of the launch belongs to batch k: lanes that hold transactions of a rejected batch beside a valid batch's
    nTx = shape[0]
    for per_lane in (4, 8):
        lanes = FZ.lane_units(N * nTx, per_lane)
        assert all(len(lane) == per_lane for lane in lanes)
        mixed = sum(any(which[u // nTx] in fails for u in lane) and any(which[u // nTx] in valid for u in lane) for lane in lanes)
        assert 2 * mixed >= len(lanes)
    g = hz.ctx("rollup-main", nTx=shape[0], nLevels=shape[1], maxL1Tx=shape[2], maxFeeTx=shape[3], n_instances=N)
    wl = g.witness_len()
    sig = g.lookup("main.hashGlobalInputs")
    for step in range(2):
        FZ.place_replicas(g, cases, which)
        err = _run(g)
        n_rej = FZ.check_failures(g, parts, err, which=which)
        assert N // 2 < n_rej < N
        assert all(o.witness_len() == wl for o, _, _ in parts) and g.total() * D == sum(o.total() for o, _, _ in parts) * N
        for k in range(N):
            o, j = part_of[which[k]]
            h = g.read(sig, 1, k)[0]
            assert h == o.read(sig, 1, j)[0], "hashGlobalInputs of instance %d (%s)" % (k, labels[which[k]])
            if hashes[which[k]] is not None:
                assert h == hashes[which[k]]
        whole = {which.index(d) for d in range(D)} | {0, N // 2 + 1, N - 1}
        for k in sorted(whole):
            o, j = part_of[which[k]]
            for first in range(0, wl, 1 << 17):
                cnt = min(1 << 17, wl - first)
                assert g.read_bytes(first, cnt, k) == o.read_bytes(first, cnt, j), "instance %d (%s), elements from %d" % (k, labels[which[k]], first)
        which = which[-1:] + which[:-1]
