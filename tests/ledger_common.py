"""Shared by tests/test_ledger.py (GPU) and tests/test_ledger_cpu.py: transfer batches drawn over a DenseState, the checker -- the Python
BatchBuilder over the same state with host hashing --, its results lifted into hz_ledger_apply_l2's output layout, and a plain Python
model of the ledger's scheme (events, grouped prefix sums over signed deltas, the fee scan, the lowest-failure rule)."""
import numpy as np

from circuits_amd import builder as B
from device_state_common import base_state, to_bytes, to_int  # noqa: F401

LEAF = ("tokenID", "nonce", "sign", "balance", "ay", "ethAddr")
SELECTORS = (0, 1, 100, 176, 191, 192, 193)   # both sides of 192, and 0


def tx(frm, to, amount, fee=0, token=1, nonce=None):
    t = {"fromIdx": frm, "toIdx": to, "amountF": B.fix2float(amount), "tokenID": token, "userFee": fee, "onChain": 0}
    if nonce is not None:
        t["nonce"] = nonce
    return t


def draw_batch(base, m, seed, pool=None, n_tx=None):
    """m valid transfers over `pool` accounts of the base (repeats, self-transfers, zero amounts, every selector of SELECTORS), explicit
    nonces, padded with NOPs to n_tx -> list of transaction dictionaries"""
    rng = np.random.default_rng(seed)
    accounts = min(base.N, pool or base.N)
    off = int(rng.integers(0, base.N - accounts + 1))
    bal, nonce, txs = {}, {}, []
    for _ in range(m):
        f, t = (base.first_idx + off + int(x) for x in rng.integers(0, accounts, size=2))
        b = bal.get(f, base.state(f)["balance"])
        amount = 0 if rng.integers(0, 8) == 0 else B.float2fix(B.floor_fix2float(b // int(rng.integers(8, 40))))
        sel = SELECTORS[int(rng.integers(0, len(SELECTORS)))]
        txs.append(tx(f, t, amount, sel, nonce=nonce.get(f, 0)))
        bal[f] = b - amount - B.compute_fee(amount, sel)
        nonce[f] = nonce.get(f, 0) + 1
        if amount:
            bal[t] = bal.get(t, base.state(t)["balance"]) + amount
    return txs + [{} for _ in range((n_tx or m) - m)]


def builder_batch(base, txs, plan_tokens, fee_idxs, n_levels, db=None, max_l1=0):
    """the checker: the same batch through RollupDB(base=...).build_batch with host hashing -> (db, built BatchBuilder)"""
    db = db or B.RollupDB(chain_id=1, base=base)
    bb = db.build_batch(len(txs), n_levels, max_l1, len(plan_tokens))
    for t in txs:
        bb.add_tx(dict(t) if t else {"onChain": 0})
    bb.fee_tokens, bb.fee_idxs = list(plan_tokens), list(fee_idxs)
    bb.build()
    return db, bb


def _rows(vals):
    if vals and isinstance(vals[0], list):
        return np.stack([to_bytes(r) for r in vals])
    return to_bytes(vals)


def expected_arrays(bb):
    """the builder's input dictionary in hz_ledger_apply_l2's output layout (name -> uint8 array)"""
    inp = bb.get_input()
    out = {f + n: _rows(inp[f + n]) for n in "123" for f in LEAF + ("siblings",)}
    out["state_root_after"] = _rows(inp["imStateRoot"] + [inp["imInitStateRootFee"]])
    out["acc_fee_after"] = _rows(inp["imAccFeeOut"] + [inp["imFinalAccFee"]])
    out["state_root_after_fee"] = _rows(inp["imStateRootFee"] + [bb.new_state_root])
    out["final_acc_fee"] = _rows(inp["imFinalAccFee"])
    out["old_root"] = _rows([inp["oldStateRoot"]])
    out["new_root"] = _rows([bb.new_state_root])
    return out


def assert_same(got, exp, names=None):
    for name in names or exp:
        g, e = got[name], exp[name]
        assert g.shape == e.shape, (name, g.shape, e.shape)
        bad = np.flatnonzero((g != e).reshape(g.shape[0], -1).any(axis=1))
        assert bad.size == 0, "%s differs at rows %s" % (name, bad[:8].tolist())


def leaf_rows(db, idxs):
    """the builder's leaves of the accounts idxs as hz_ledger_accounts returns them: [n, 4, 32]"""
    return np.stack([to_bytes(B.leaf_fields(db.leaves[i])) for i in idxs])


def touched(txs, fee_idxs):
    return sorted({t[k] for t in txs if t.get("fromIdx") for k in ("fromIdx", "toIdx")} | {i for i in fee_idxs if i})


# ---- a plain restatement of the planner and of the scheme -----------------------------------------------------------------------------
def plan_model(txs, plan_tokens, fee_idxs):
    m = len(txs)
    out = {"ev_sender": [-1] * m, "ev_receiver": [-1] * m, "fee_slot": [-1] * m, "last_event": [-1] * m, "account": [], "prev_same": [], "unit": [], "kind": []}
    last = {}

    def event(acct, unit, kind):
        out["account"].append(acct)
        out["prev_same"].append(last.get(acct, -1))
        out["unit"].append(unit)
        out["kind"].append(kind)
        last[acct] = len(out["account"]) - 1
        return last[acct]
    for i, t in enumerate(txs):
        if t.get("fromIdx", 0):
            out["ev_sender"][i] = event(t["fromIdx"], i, 0)
            if t.get("amountF", 0) & ((1 << 35) - 1):
                out["ev_receiver"][i] = event(t["toIdx"], i, 1)
            tok = t.get("tokenID", 0)
            out["fee_slot"][i] = list(plan_tokens).index(tok) if tok in plan_tokens else -1
        out["last_event"][i] = len(out["account"]) - 1
    out["ev_fee"] = [event(a, m + j, 2) if a else -1 for j, a in enumerate(fee_idxs)]
    return out


def scheme_model(leaf_of, txs, plan_tokens, fee_idxs):
    """The ledger's scheme on Python integers, the way the kernels do it: per-transaction amounts and fees; the fee scan; then, account
    by account (NOT transaction by transaction), a prefix sum over the signed deltas of the account's events that checks token, nonce,
    underflow and overflow and lowers one failure word. -> ("refused", unit, reason) or ("ok", leaf fields by name, acc_fee_after, final)"""
    m, F = len(txs), len(plan_tokens)
    p = plan_model(txs, plan_tokens, fee_idxs)
    M = len(p["account"])
    delta, acc, rows, over = [0] * M, [0] * F, [], []
    for i, t in enumerate(txs):
        if t.get("fromIdx", 0):
            amount = B.float2fix(t.get("amountF", 0))
            fee = B.compute_fee(amount, t.get("userFee", 0))
            if fee >> 128:   # reason 16: the circuit rejects such a fee (src/compute-fee.circom:89-91); only a charged row has one
                over.append((i, 16))
            delta[p["ev_sender"][i]] = -(amount + fee)
            if p["ev_receiver"][i] >= 0:
                delta[p["ev_receiver"][i]] = amount
            if p["fee_slot"][i] >= 0:
                acc[p["fee_slot"][i]] += fee
        rows.append(list(acc))
    for j in range(F):
        if p["ev_fee"][j] >= 0:
            delta[p["ev_fee"][j]] = acc[j]
    groups = {}
    for e, a in enumerate(p["account"]):
        groups.setdefault(a, []).append(e)
    fail = min(over) if over else None
    before = [None] * M
    for a in sorted(groups, reverse=True):   # any order of the groups must give the same answer
        leaf = dict(leaf_of(a))
        for e in groups[a]:
            before[e] = dict(leaf)
            unit, kind = p["unit"][e], p["kind"][e]
            bad = []
            tok = plan_tokens[unit - m] if kind == 2 else txs[unit].get("tokenID", 0)
            if leaf["tokenID"] != tok:
                bad.append((1, 4, 6)[kind])
            if kind == 0:
                if leaf["nonce"] != txs[unit].get("nonce", 0):
                    bad.append(2)
                if leaf["nonce"] == (1 << 40) - 1:   # reason 12: nonce + 1 is not a leaf field, and the circuit does not wrap
                    bad.append(12)
                leaf["nonce"] += 1
            leaf["balance"] += delta[e]
            if leaf["balance"] < 0:
                bad.append(3)
            elif leaf["balance"] >= 1 << 192:
                bad.append(5)
            for r in bad:
                fail = min(fail, (unit, r)) if fail else (unit, r)
    if fail:
        return ("refused",) + fail
    zero = dict.fromkeys(LEAF, 0)
    out = {f + n: [] for n in "123" for f in LEAF}
    for i, t in enumerate(txs):
        s1 = before[p["ev_sender"][i]] if p["ev_sender"][i] >= 0 else zero
        s2 = before[p["ev_receiver"][i]] if p["ev_receiver"][i] >= 0 else dict(zero, tokenID=t.get("tokenID", 0) if t.get("fromIdx", 0) else 0)
        for f in LEAF:
            out[f + "1"].append(s1[f])
            out[f + "2"].append(s2[f])
    for j in range(F):
        s3 = before[p["ev_fee"][j]] if p["ev_fee"][j] >= 0 else zero
        for f in LEAF:
            out[f + "3"].append(s3[f])
    return "ok", out, rows, acc
