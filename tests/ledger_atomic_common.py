"""Shared by tests/test_ledger_atomic.py (GPU) and tests/test_ledger_atomic_cpu.py: atomic transactions on the ledger
(hz_ledger_apply_batch_atomic). A plain Python model of the link check -- the row an rqOffset names, the link fields of a
row, the verdict --, small batches of transfers over a dense state with their nonces, the derivation of the rq fields a signer commits
to (BatchBuilder.build's, extended to the targets whose link fields are zero), signing, and the checker: BatchBuilder's inputs for the same
rows handed to the oracle's rollup-main."""
import ledger_common as C
import ledger_sig_common as S
from circuits_amd import builder as B

REASON = 13
RQ_FIELDS = ("rqTxCompressedDataV2", "rqToEthAddr", "rqToBjjAy")
P = B.P


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def target_row(r, k, n_l1, n_rows):
    """the row transaction r is compared with, or -1 for zeros: offset 0, a position outside the batch, an L1 row (a NOP: link_target)"""
    if k == 0:
        return -1
    t = r + k if k <= 3 else r - (8 - k)
    return t if n_l1 <= t < n_rows else -1


def link_fields(t):
    """(txCompressedDataV2, toEthAddr, toBjjAy) as signed; zeros for an L2 NOP"""
    if not t.get("fromIdx", 0):
        return (0, 0, 0)
    return (B.build_tx_compressed_data_v2(t), t.get("toEthAddr", 0), t.get("toBjjAy", 0))


def link_target(n_l1, l2_txs, i):
    """the row L2 transaction i is compared with, -1 where that is zeros (a NOP target, and a NOP's own entry, included)"""
    t = l2_txs[i]
    if not t.get("fromIdx", 0):
        return -1
    row = target_row(n_l1 + i, t.get("rqOffset", 0), n_l1, n_l1 + len(l2_txs))
    return row if row >= 0 and l2_txs[row - n_l1].get("fromIdx", 0) else -1


def verdicts(n_l1, l2_txs):
    """0 or 13 per L2 transaction: its three rq fields against its target's link fields, as integers"""
    out = []
    for i, t in enumerate(l2_txs):
        if not t.get("fromIdx", 0):
            out.append(0)
            continue
        row = link_target(n_l1, l2_txs, i)
        want = link_fields(l2_txs[row - n_l1]) if row >= 0 else (0, 0, 0)
        out.append(0 if tuple(t.get(f, 0) for f in RQ_FIELDS) == want else REASON)
    return out


def first_refusal(n_l1, l2_txs):
    """(row, 13) of the lowest broken link, or None"""
    v = verdicts(n_l1, l2_txs)
    return (n_l1 + v.index(REASON), REASON) if REASON in v else None


def derive(n_l1, l2_txs):
    """copies of the transactions; one with rqOffset and no explicit rq fields gets its target's link fields (zeros where the target has
    none), before it is signed"""
    out = [dict(t) for t in l2_txs]
    for i, t in enumerate(out):
        if t.get("rqOffset", 0) and RQ_FIELDS[0] not in t:
            row = link_target(n_l1, out, i)
            t.update(zip(RQ_FIELDS, link_fields(out[row - n_l1]) if row >= 0 else (0, 0, 0)))
    return out


def sign_all(base, l2_txs):
    """every active transaction signed by its sender's key over its message, rq fields included"""
    return [S.sign(base, dict(t)) for t in l2_txs]


# ---- batches -----------------------------------------------------------------------------------------------------------------------------
def transfers(base, n, start=0, amount=3, offsets=None, signed_dest=False):
    """n small transfers around the accounts of the base, nonces counted per sender; offsets: {i: rqOffset}; signed_dest: every transfer
    also signs a toEthAddr, a toBjjAy and a toBjjSign of its own (by index they only enter the message), consecutive ones a few apart, so a
    link field read from the wrong neighbour, or off by one, is another value"""
    f0, N = base.first_idx, base.N
    nonce, out = {}, []
    for i in range(n):
        f, t = f0 + (start + i) % N, f0 + (start + i + 1) % N
        tx = C.tx(f, t, amount + i % 5, 0, nonce=nonce.get(f, 0))
        nonce[f] = nonce.get(f, 0) + 1
        if offsets and i in offsets:
            tx["rqOffset"] = offsets[i]
        if signed_dest:
            tx.update(toEthAddr=(0xA11CE << 140) + 3 * i + 2, toBjjAy=P - 5 - 3 * i, toBjjSign=i & 1)
        out.append(tx)
    return out


def deposits(base, n):
    """n L1 deposits of the accounts' own owners: rows that change balances and carry no link fields"""
    import ledger_l1_common as L1
    return [L1.own(base, base.first_idx + j, 0, 0, 7 + j) for j in range(n)]


def off_by_one(t, field):
    """the transaction with one rq field changed by one, staying below r"""
    v = t.get(field, 0)
    return dict(t, **{field: v - 1 if v else 1})


# ---- the checker -------------------------------------------------------------------------------------------------------------------------
def builder_inputs(base, l1_txs, l2_txs, shape, plan=(1,), idxs=(0,)):
    """BatchBuilder's RollupMain inputs for the rows, the rq fields kept as given and the transactions signed by their owners over the
    message that holds them -> the dictionary"""
    n_tx, n_levels, max_l1, max_fee = shape
    txs = [dict(t, onChain=1) for t in l1_txs] + [dict(t, signer=S.signer(base, t["fromIdx"])) if t.get("fromIdx", 0) else {} for t in l2_txs]
    txs += [{} for _ in range(n_tx - len(txs))]
    plan, idxs = list(plan) + [0] * (max_fee - len(plan)), list(idxs) + [0] * (max_fee - len(idxs))
    _, bb = C.builder_batch(base, txs, plan, idxs, n_levels, max_l1=max_l1)
    return bb.get_input()


def oracle_accepts(inp, shape):
    from oracle_binding import OracleCtx
    o = OracleCtx("rollup-main", *shape)
    o.set_inputs(inp)
    return o.run() is None


# ---- tests/native/ledger_atomic_check.cpp's input ----------------------------------------------------------------------------------------
def check_lines(n_l1=3, n_rows=12):
    """t r k n_l1 n_rows expect (decimal; expect -1: zeros) for r = 0, 3, n_rows - 1 and all eight offsets; m a b expect (hex) for
    rq_fields_match with the field at position a / b of the six replaced -- pairs that differ in the top limb only among them"""
    lines = []
    for n1 in (0, n_l1):
        for r in (0, 3, n_rows - 1):
            for k in range(8):
                lines.append("t %d %d %d %d %d" % (r, k, n1, n_rows, target_row(r, k, n1, n_rows)))
    low = 0x1234567890ABCDEF
    for a, b in ((low, low), (low, low | 1 << 255), (low | 1 << 224, low), (low | 1 << 255, low | 1 << 255), (0, 1 << 224), (P - 1, P - 1), (P - 1, (P - 1) ^ (1 << 252))):
        for pos in range(3):
            lines.append("m %d %x %x %d" % (pos, a, b, 1 if a == b else 0))
    return "\n".join(lines) + "\n"


def message_lines(txs):
    """s records: the fields of each transaction dictionary, its three rq fields and M = build_hash_sig at chain_id 1, in hex"""
    lines = []
    for t in txs:
        vals = [t.get(k, 0) for k in ("fromIdx", "toIdx", "amountF", "nonce", "tokenID", "userFee", "toBjjSign", "maxNumBatch", "toEthAddr", "toBjjAy") + RQ_FIELDS]
        lines.append("s " + " ".join("%x" % v for v in vals) + " %x" % B.build_hash_sig(t, 1))
    return "\n".join(lines) + "\n"
