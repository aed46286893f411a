"""Poseidon's partial rounds as a linear recurrence on the device (poseidon.h, PoseidonCfg<T>::REC): hz_poseidon_batch_dev for every
width, digest-only and witness form, on 130 permutations -- two whole wavefronts and a ragged one: the wave-uniform skip of
fr_cond_sub_p_rare decides per wavefront, a single lane proves nothing -- against the oracle's dense Poseidon: every stored S-box
signal and the digest. Inputs: the upstream known answers, all-zero, all p - 1, values at the top of the field, seeded random rows.
(The whole-buffer suites test_smt_kat / test_witness_gpu / test_constant_marks / test_poseidon are the parity yardstick of k_smt, k_hash4
and the signature prologue, which run the same poseidon_hash<T>.)"""
import json
import os
import random

import pytest

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "poseidon_kat.json")))
NSBOX = {t: 8 * t + [56, 57, 56, 60, 60, 63][t - 2] for t in range(2, 8)}
N = 130


def rows_for(t):
    rng = random.Random(4001 * t)
    rows = [[rng.randrange(P) for _ in range(t - 1)] for _ in range(N)]
    special = [[int(x) for x in v["in"]] for v in GOLD["upstream_kat"] if len(v["in"]) == t - 1]
    special += [[0] * (t - 1), [P - 1] * (t - 1), [P - 2] * (t - 1), [(1 << 253) + 1] * (t - 1), [1] * (t - 1)]
    # one of each in every wavefront (lanes 0.., 64.., 128..: the ragged one takes what fits)
    for base in (0, 64, 128):
        for i, r in enumerate(special):
            if base + i < N:
                rows[base + i] = r
    return rows


@pytest.fixture(scope="module")
def reference(oracle):
    """the oracle's digests and S-box witness of the rows of every width, computed once"""
    out = {}
    for t in range(2, 8):
        rows = rows_for(t)
        dig, wit = oracle.poseidon_batch(t, rows, witness=True)
        out[t] = (rows, dig, wit)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("t", [2, 3, 4, 5, 6, 7])
def test_batch_dev_digest_and_every_sbox_signal(hz, reference, t):
    import torch
    rows, dig, wit = reference[t]
    assert len(wit) == 96 * NSBOX[t] * N
    for v in GOLD["upstream_kat"]:
        if len(v["in"]) == t - 1:
            assert str(dig[rows.index([int(x) for x in v["in"]])]) == v["out"]
    flat = b"".join(x.to_bytes(32, "little") for r in rows for x in r)
    d_in = torch.frombuffer(bytearray(flat), dtype=torch.uint8).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    want = b"".join(x.to_bytes(32, "little") for x in dig)
    # digest only: Montgomery S-box, constant block K
    d_out = torch.zeros(32 * N, dtype=torch.uint8, device="cuda")
    hz.poseidon_batch_dev(t, N, d_in.data_ptr(), d_out.data_ptr(), None, stream)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == want
    # witness: canonical S-box, constant block KW; every in2 / in4 / out of every S-box of every permutation
    d_out.zero_()
    d_wit = torch.zeros(len(wit), dtype=torch.uint8, device="cuda")
    hz.poseidon_batch_dev(t, N, d_in.data_ptr(), d_out.data_ptr(), d_wit.data_ptr(), stream)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == want
    got = d_wit.cpu().numpy().tobytes()
    if got != wit:
        bad = next(i for i in range(len(wit) // 32) if got[32 * i:32 * i + 32] != wit[32 * i:32 * i + 32])
        pytest.fail("t=%d: S-box signal %d of S-box %d differs at permutation %d" % (t, (bad // N) % 3, bad // (3 * N), bad % N))
