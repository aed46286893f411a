"""Shared by tests/test_ledger_main_inputs.py (GPU) and tests/test_ledger_main_inputs_cpu.py: RollupMain's input signals as the reference
declares them (tests/golden/rollup_main_inputs.json), packed layouts made of that list, the descriptor table hz_ledger_main_inputs must make
of a layout -- restated from the builder's own tables of where the ledger leaves each signal --, the cases of the host program, and the
batches the GPU tests apply."""
import json
import os

from circuits_amd import builder as B
from circuits_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollup_main_inputs.json")
NEW_SYMBOLS = ["hz_ledger_main_inputs", "hz_ledger_main_inputs_ms", "hz_ledger_plan_main_inputs"]
FLAGS = {"sigs": capi.MI_SIGS, "rq": capi.MI_RQ, "exits": capi.MI_EXITS, "creates": capi.MI_CREATES, "aux": capi.MI_AUX, "growing": capi.MI_GROWING}
NEEDS_SIGS = ("toBjjAy", "toEthAddr", "maxNumBatch", "s", "r8x", "r8y")
NEEDS_RQ = B.RQ_SIGNALS
FROM_ROWS = ("txCompressedData", "txCompressedDataV2", "amountF", "fromIdx", "toIdx", "onChain", "newAccount", "loadAmountF", "fromEthAddr")
P = B.P


def signal_list():
    """[(name, [dimension words])] in the reference's declaration order"""
    with open(GOLDEN) as f:
        return [(n, d) for n, d in json.load(f)["signals"]]


def dims(words, shape):
    n_tx, n_levels, _, max_fee = shape
    val = {"nTx": n_tx, "nTx-1": n_tx - 1, "maxFeeTx": max_fee, "maxFeeTx-1": max_fee - 1, "nLevels+1": n_levels + 1, "256": 256}
    return [val[w] for w in words]


def layout(shape, order=None):
    """(total bytes, [(name, offset, width, flat length)]) over the reference's signals in `order` (default: as declared): every signal
    32-byte aligned, bit signals one byte an element -- the rule of hz_inputs_upload's format"""
    sigs = signal_list()
    if order is not None:
        by_name = dict(sigs)
        sigs = [(n, by_name[n]) for n in order]
    out, off = [], 0
    for name, words in sigs:
        flat = 1
        for d in dims(words, shape):
            flat *= d
        width = 1 if name == "fromBjjCompressed" else 32
        off = (off + 31) & ~31
        out.append((name, off, width, flat))
        off += flat * width
    return (off + 31) & ~31, out


def expected_plan(shape, flags):
    """{signal: (kind, source, first row, rows)} as the issue's list of sources says, from the builder's own tables"""
    n_tx, _, _, max_fee = shape
    has = {k: bool(flags & v) for k, v in FLAGS.items()}
    exp = {"oldLastIdx": ("copy", "globals", 0, 1), "globalChainID": ("copy", "globals", 1, 1), "currentNumBatch": ("copy", "globals", 2, 1),
           "feeIdxs": ("copy", "fee_idxs", 0, max_fee), "feePlanTokens": ("copy", "fee_plan_tokens", 0, max_fee),
           "imOnChain": ("onChain", "rows", 0, n_tx - 1), "fromBjjCompressed": ("fromBjjCompressed", "from_bjj", 0, n_tx)}
    for name, (arr, first, rows) in B.l2_state_signals(n_tx, max_fee).items():
        exp[name] = ("copy", arr, first, rows)
    for name, (arr, first, rows) in B.exit_signals(n_tx).items():
        exp[name] = ("copy", arr, first, rows) if has["exits"] else ("zero", None, 0, rows)
    for name, (arr, first, rows) in B.create_signals(n_tx).items():
        exp[name] = ("copy", arr, first, rows) if has["creates"] else ("zero", None, 0, rows)
    if not has["creates"]:
        exp["imOutIdx"] = ("broadcast", "globals", 0, n_tx - 1)   # old_last_idx in every row
    exp["auxToIdx"] = ("copy", "auxToIdx", 0, n_tx) if has["aux"] else ("zero", None, 0, n_tx)
    for name in FROM_ROWS:
        exp[name] = (name, "rows", 0, n_tx)
    for name in NEEDS_SIGS:
        exp[name] = (name, "rows", 0, n_tx) if has["sigs"] else ("zero", None, 0, n_tx)
    for name in NEEDS_RQ:
        exp[name] = (name, "rows", 0, n_tx) if has["rq"] else ("zero", None, 0, n_tx)
    return exp


def first_difference(lay, got, exp):
    """the first signal and element at which two packed buffers differ, as words; None when they are equal"""
    if got == exp:
        return None
    total, sigs = lay
    if len(got) != len(exp):
        return "lengths %d and %d" % (len(got), len(exp))
    for name, off, width, flat in sorted(sigs, key=lambda s: s[1]):
        for e in range(flat):
            a, b = got[off + e * width:off + (e + 1) * width], exp[off + e * width:off + (e + 1) * width]
            if a != b:
                return "signal %s, element %d: %#x, not %#x" % (name, e, int.from_bytes(a, "little"), int.from_bytes(b, "little"))
    at = next(i for i in range(total) if got[i] != exp[i])
    return "byte %d, in no signal's range: %#x, not %#x" % (at, got[at], exp[at])


# ---- the host program's cases ----------------------------------------------------------------------------------------------------------
EDGE_L1 = {"chain": 0xFFFF, "from": (1 << 48) - 3, "to": (1 << 48) - 2, "token": 0x80000001, "amountF": (1 << 40) - 1, "loadAmountF": (1 << 40) - 1,
           "eth": (1 << 160) - 1}
EDGE_L2 = {"fromIdx": (1 << 48) - 3, "toIdx": (1 << 48) - 2, "amountF": (1 << 40) - 1, "nonce": (1 << 40) - 2, "tokenID": 0x80000001, "userFee": 255, "toBjjSign": 1,
           "maxNumBatch": (1 << 32) - 1, "toEthAddr": (1 << 160) - 1, "toBjjAy": P - 1, "s": P - 1, "r8x": P - 2, "r8y": (1 << 253) + 5, "rqOffset": 7,
           "rqTxCompressedDataV2": (1 << 217) - 1, "rqToEthAddr": (1 << 160) - 1, "rqToBjjAy": P - 3}
SMALL_L2 = {"fromIdx": 300, "toIdx": 301, "amountF": 17, "nonce": 0, "tokenID": 1, "userFee": 0, "toBjjSign": 0, "maxNumBatch": 0, "toEthAddr": 0, "toBjjAy": 0, "s": 1,
            "r8x": 2, "r8y": 3, "rqOffset": 0, "rqTxCompressedDataV2": 0, "rqToEthAddr": 0, "rqToBjjAy": 0}
BIT_KEYS = [0, (1 << 256) - 1] + [1 << b for b in (0, 31, 32, 254, 255)] + [(P - 1) | 1 << 254 | 1 << 255]


def l1_expected(kind, c, create):
    frm = 0 if create else c["from"]
    return {"txCompressedData": B.CONST_SIG | (c["chain"] << 32) | (frm << 48) | (c["to"] << 96) | (c["token"] << 144), "amountF": c["amountF"], "fromIdx": frm,
            "toIdx": c["to"], "onChain": 1, "newAccount": 1 if create else 0, "loadAmountF": c["loadAmountF"], "fromEthAddr": c["eth"]}.get(kind, 0)


def l2_expected(kind, t, chain, have_rq):
    """what the builder writes for the transaction dictionary t ({} for a NOP): _ledger_batch_inputs' L2 branch"""
    if not t.get("fromIdx", 0):
        t = {}
    vals = {"txCompressedData": B.build_tx_compressed_data(t, chain), "amountF": t.get("amountF", 0), "txCompressedDataV2": B.build_tx_compressed_data_v2(t),
            "fromIdx": t.get("fromIdx", 0), "toIdx": t.get("toIdx", 0), "toBjjAy": t.get("toBjjAy", 0), "toEthAddr": t.get("toEthAddr", 0),
            "maxNumBatch": t.get("maxNumBatch", 0), "s": t.get("s", 0), "r8x": t.get("r8x", 0), "r8y": t.get("r8y", 0)}
    if have_rq:
        vals.update({k: t.get(k, 0) for k in B.RQ_SIGNALS})
    return vals.get(kind, 0)


def check_lines():
    """the cases of tests/native/ledger_main_inputs_check.cpp, the expectation of each by the builder's formulas in Python integers"""
    lines = []
    kinds = {name: i for i, name in enumerate(capi.MI_KINDS)}
    small_l1 = {"chain": 1, "from": 256, "to": 0, "token": 1, "amountF": 0, "loadAmountF": 5, "eth": 0xABC}
    for c in (EDGE_L1, small_l1):
        for create in (0, 1):
            for kind, k in kinds.items():
                if k < 3 or kind == "fromBjjCompressed":
                    continue
                lines.append("1 %x %x %x %x %x %x %x %x %x %x" % (k, c["chain"], c["from"], c["to"], c["token"], c["amountF"], c["loadAmountF"], c["eth"], create,
                                                                    l1_expected(kind, c, create)))
    for t, chain in ((EDGE_L2, 0xFFFF), (SMALL_L2, 1), (dict(EDGE_L2, fromIdx=0), 0xFFFF)):
        for have_rq in (0, 1):
            for kind, k in kinds.items():
                if k < 3 or kind == "fromBjjCompressed":
                    continue
                lines.append("2 %x %x " % (k, chain) + " ".join("%x" % t[f] for f in ("fromIdx", "toIdx", "amountF", "nonce", "tokenID", "userFee", "toBjjSign", "maxNumBatch",
                                                                                      "toEthAddr", "toBjjAy", "s", "r8x", "r8y", "rqOffset") + B.RQ_SIGNALS[1:]) +
                             " %x %x" % (have_rq, l2_expected(kind, t, chain, have_rq)))
    for key in BIT_KEYS:
        for g in range(16):
            lines.append("b %x %x %s" % (key, g, bytes((key >> (16 * g + b)) & 1 for b in range(16)).hex()))
    return "\n".join(lines) + "\n"
