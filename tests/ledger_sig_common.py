"""Shared by tests/test_ledger_sig.py (GPU) and tests/test_ledger_sig_cpu.py: a plain Python restatement of the ledger's signature check
(hz_ledger_apply_l2_signed / hz_ledger_verify_l2) on integers -- the message of decode-tx.circom, AySign2Ax,
EdDSAPoseidonVerifier as a group-law statement --, signing of ledger_common's transfers with the base's keys, and fuzz_common's signature
edges lifted onto a ledger batch."""
import functools

import numpy as np

import fuzz_common as F
import ledger_common as C
from circuits_amd import builder as B

P, L_ORDER = B.P, B.SUBORDER
CHAIN_ID = 1
SIG_FIELDS = ("s", "r8x", "r8y")


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def message(t, chain_id=CHAIN_ID):
    """(txCompressedData, txCompressedDataV2, M) of a transaction dictionary; {} is the padding NOP"""
    return B.build_tx_compressed_data(t, chain_id), B.build_tx_compressed_data_v2(t), B.build_hash_sig(t, chain_id)


def recover_ax(ay, sign):
    """AySign2Ax: the root of (1 - ay^2) / (a - d ay^2) above (P - 1) / 2 iff sign; None where the circuit finds none"""
    x = F.bjj_x_of(ay)
    if x is None or (x == 0 and sign):
        return None
    if x and (x > (P - 1) // 2) != bool(sign):
        x = P - x
    return x


def verify(s, r8x, r8y, ay, sign, msg):
    """EdDSAPoseidonVerifier's verdict: S < l, hm the full integer, 8 A with x != 0, BabyAdd(R8, hm 8A) == S B8 by the affine formula on
    R8 as given, both denominators nonzero"""
    if s >= L_ORDER:
        return False
    ax = recover_ax(ay, sign)
    if ax is None:
        return False
    hm = B.host().poseidon([r8x, r8y, ax, ay, msg])
    q8 = F.bjj_mul((ax, ay), 8)
    if q8[0] == 0:
        return False
    x2, y2 = F.bjj_mul(q8, hm)
    t = F.BJJ_D * r8x * x2 * r8y * y2 % P
    if (1 + t) % P == 0 or (1 - t) % P == 0:
        return False
    x3 = (r8x * y2 + r8y * x2) * pow(1 + t, -1, P) % P
    y3 = (r8y * y2 - F.BJJ_A * r8x * x2) * pow(1 - t, -1, P) % P
    return (x3, y3) == F.bjj_mul(B.BASE8, s)


def verdict(t, ay, sign, current_num_batch=1, chain_id=CHAIN_ID):
    """0, 7 (signature rejected) or 8 (maxNumBatch expired); 7 wins over 8, a NOP is 0"""
    if not t.get("fromIdx", 0):
        return 0
    if not verify(t.get("s", 0), t.get("r8x", 0), t.get("r8y", 0), ay, sign, message(t, chain_id)[2]):
        return 7
    mb = t.get("maxNumBatch", 0)
    return 8 if mb and mb < current_num_batch else 0


def key_of(cols, first_idx, idx):
    """(ay, sign) of account idx in loaded columns (e0, balance, ay, ethAddr as [N, 32])"""
    return C.to_int(cols[2][idx - first_idx]), (C.to_int(cols[0][idx - first_idx]) >> 72) & 1


def verdicts(txs, cols, first_idx, current_num_batch=1, chain_id=CHAIN_ID):
    return [verdict(t, *key_of(cols, first_idx, t["fromIdx"]), current_num_batch, chain_id) if t.get("fromIdx", 0) else 0 for t in txs]


def expected_sig_arrays(txs, chain_id=CHAIN_ID):
    rows = [message(t, chain_id) for t in txs]
    return {name: C.to_bytes([r[j] for r in rows]) for j, name in enumerate(("tx_compressed_data", "tx_compressed_data_v2", "sig_l2_hash"))}


# ---- signing ----------------------------------------------------------------------------------------------------------------------------
def signer(base, idx):
    return base.keys()[int(base.key_idx[idx - base.first_idx])]


def sign(base, t, chain_id=CHAIN_ID):
    """the transfer with s, r8x, r8y of its sender's key over its message (in place, returned)"""
    if t.get("fromIdx", 0):
        t.update(signer(base, t["fromIdx"]).sign_msg(B.build_hash_sig(t, chain_id)))
    return t


def signed_batch(base, m, seed, pool=None, n_tx=None, chain_id=CHAIN_ID):
    rng = np.random.default_rng(seed ^ 0x5167)
    txs = C.draw_batch(base, m, seed, pool=pool, n_tx=n_tx)
    for t in txs:
        if t:   # the fields only the signature covers, drawn as well
            t["toEthAddr"] = int(rng.integers(0, 1 << 62)) << 90 if rng.integers(0, 2) else 0
            t["toBjjAy"] = int(rng.integers(1, 1 << 62)) ** 4 % P if rng.integers(0, 2) else 0
            t["toBjjSign"] = int(rng.integers(0, 2))
            t["maxNumBatch"] = int(rng.integers(0, 3)) * 1000
            sign(base, t, chain_id)
    return txs


def forge(t, how):
    """a copy of a signed transfer with a signature the verifier rejects, of one of four causes"""
    t = dict(t)
    if how == "s":
        t["s"] = (t["s"] + 1) % L_ORDER
    elif how == "r8":
        t["r8x"], t["r8y"] = B.BASE8
    elif how == "malleable":
        t["s"] += L_ORDER
    elif how == "stale":   # signed, then changed
        t["userFee"] = (t.get("userFee", 0) + 1) % 256
    else:
        raise ValueError(how)
    return t


# ---- fuzz_common's edges on a ledger batch -------------------------------------------------------------------------------------------
NOT_LEDGER_INPUTS = ("sign1=2",)   # and every " & fromIdx=0" / " & onChain=1" gate


@functools.lru_cache(maxsize=None)
def edge_state():
    """64 accounts at indices 0 .. 63: the state a circuit of nLevels = 6 can hold (decode-tx wants every index below 2^nLevels).
    Index 0 is the NOP and 1 the exit account: transfers use 2 .. 63."""
    return B.DenseState.build(6, first_idx=0)


def edge_batches(base, chain_id=CHAIN_ID):
    """[(label, txs, cols)]: a batch of three signed transfers between distinct accounts whose transaction 1 carries one of
    signature_edge_cases' edges. s and r8 edits change the transaction; key edits change the loaded ay / e0 columns of its sender
    (cols: what Ledger.load takes). The first entry is the unmodified batch."""
    f0 = base.first_idx
    txs = [sign(base, C.tx(f0 + 2 + 2 * i, f0 + 3 + 2 * i, 1000 + i, 100, nonce=0), chain_id) for i in range(3)]
    cols0 = [np.array(c) for c in base.leaf_fields()]
    ay, sg = key_of(cols0, f0, txs[1]["fromIdx"])
    single = dict({k: txs[1][k] for k in SIG_FIELDS}, ay1=ay, sign1=sg, onChain=0, fromIdx=txs[1]["fromIdx"])
    other = {k: txs[2][k] for k in SIG_FIELDS}
    out = []
    for label, e in F.signature_edge_cases(single, other):
        if " & " in label or label in NOT_LEDGER_INPUTS:
            continue
        batch = [dict(t) for t in txs]
        batch[1].update({k: e[k] for k in SIG_FIELDS})
        cols = [np.array(c) for c in cols0]
        row = txs[1]["fromIdx"] - f0
        cols[2][row] = C.to_bytes([e["ay1"]])[0]
        cols[0][row] = C.to_bytes([C.to_int(cols[0][row]) & ~(1 << 72) | (e["sign1"] << 72)])[0]
        out.append((label, batch, cols))
    return out


def check_lines(cases, chain_id=CHAIN_ID):
    """cases: [(transaction, ay, sign, current_num_batch)] -> the lines tests/native/ledger_sig_check.cpp reads, expectations from the model"""
    lines = []
    for t, ay, sg, cur in cases:
        tcd, v2, msg = message(t, chain_id)
        f = [chain_id, cur, t["fromIdx"], t["toIdx"], t.get("amountF", 0), t.get("nonce", 0), t.get("tokenID", 0), t.get("userFee", 0), t.get("toBjjSign", 0),
             t.get("maxNumBatch", 0), t.get("toEthAddr", 0), t.get("toBjjAy", 0), t["s"], t["r8x"], t["r8y"], ay, sg, verdict(t, ay, sg, cur, chain_id), msg, tcd, v2]
        lines.append(" ".join("%x" % v for v in f))
    return "\n".join(lines) + "\n"
