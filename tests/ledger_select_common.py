"""Shared by tests/test_ledger_select.py (GPU) and tests/test_ledger_select_cpu.py: a batch selected from a pool
(hz_ledger_select_batch). A plain Python model of the procedure -- the running index and the new leaves of
ledger_create_common, the L1 run with ledger_exit_common's static part (ledger_l1_common.l1_run's recurrence, with forceExits), the
builder's fee formula, ledger_atomic_common's link fields, ledger_create_common's lookup, ledger_sig_common's verdict --, the retry loop a
caller writes without the call, pool generators and tests/native/ledger_select_check.cpp's input."""
import numpy as np

import ledger_addr_common as A
import ledger_atomic_common as Q
import ledger_common as C
import ledger_create_common as CR
import ledger_exit_common as X
import ledger_l1_common as L1
import ledger_sig_common as S
from circuits_amd import builder as B

PARTNER, FULL, FEE_OVERFLOW = 14, 15, 16
NONCE_MAX = (1 << 40) - 1
LIMIT = 1 << 192
Refused = CR.Refused


def offset_of(d):
    """the rqOffset that names a row d rows away, 0: none does"""
    return d if 1 <= d <= 3 else 8 + d if -4 <= d <= -1 else 0


def partners(pool):
    return [t.get("partner", -1) if t.get("fromIdx", 0) and t.get("partner") is not None else -1 for t in pool]


def closure(pool_active, partner, kept):
    """the closure step alone over kept flags -> (forced flags, offsets): a kept transaction whose partner is not kept, or stands where no
    offset reaches, is forced out"""
    row, n = {}, 0
    for i, k in enumerate(kept):
        if k and pool_active[i]:
            row[i] = n
            n += 1
    forced, off = [0] * len(kept), [0] * len(kept)
    for i, p in enumerate(partner):
        if p >= 0 and i in row:
            off[i] = offset_of(row[p] - row[i]) if p in row else 0
            forced[i] = int(off[i] == 0)
    return forced, off


def model(acc, l1_txs, pool, current_num_batch=1, max_keep=None, verify=False, chain_id=S.CHAIN_ID, capacity=1 << 12):
    """the procedure of DESIGN.md 8j on Python integers. acc: ledger_create_common.Accounts. -> ("refused", L1 row, 5) or {"verdict",
    "kept", "rq_offset", "aux_to_idx", "rounds"}; Refused for the argument errors"""
    f0, m = acc.first_idx, len(pool)
    max_keep = m if max_keep is None else max_keep
    aux, _ = CR.running_index(f0, acc.n, capacity, l1_txs)
    slots = {a: CR.new_leaf(t) for a, t in zip(aux, l1_txs) if a}
    count = acc.n + len(slots)
    leaf_of = lambda i: slots[i] if i in slots else acc.state(i)   # noqa: E731
    eff_l1 = [dict(t, fromIdx=a) if a else t for a, t in zip(aux, l1_txs)]
    for t in pool:
        if t.get("fromIdx", 0) and not f0 <= t["fromIdx"] < f0 + count:
            raise Refused("outside the state")
        if t.get("fromIdx", 0) and t.get("toIdx", 0) > CR.EXIT and not f0 <= t["toIdx"] < f0 + count:
            raise Refused("outside the state")
    partner = partners(pool)
    for i, p in enumerate(partner):
        if pool[i].get("fromIdx", 0) and pool[i].get("partner") is not None and not -1 <= pool[i]["partner"] < m:
            raise Refused("outside the pool")
        if p == i:
            raise Refused("the transaction itself")
    # ---- the static verdicts: nothing the walk changes
    static, receiver, aux_to = [], [], []
    for i, t in enumerate(pool):
        if not t.get("fromIdx", 0):
            static.append(set())
            receiver.append(0)
            aux_to.append(0)
            continue
        s, bad = leaf_of(t["fromIdx"]), set()
        asks = A.is_to_addr(t) and L1.has_amount(t)
        found = CR.lookup(leaf_of, f0, count, t) if asks else 0
        aux_to.append(found)
        r = 0 if not L1.has_amount(t) or X.is_exit(t) else found if asks else t["toIdx"]
        receiver.append(r)
        if asks and not found:
            bad.add(9)
        if t.get("tokenID", 0) != s["tokenID"]:
            bad.add(1)
        if r and leaf_of(r)["tokenID"] != t.get("tokenID", 0):
            bad.add(4)
        if verify:
            bad.add(S.verdict(t, s["ay"], s["sign"], current_num_batch, chain_id))
        want = Q.link_fields(pool[partner[i]]) if partner[i] >= 0 else (0, 0, 0)
        if tuple(t.get(f, 0) for f in Q.RQ_FIELDS) != want:
            bad.add(13)
        if B.compute_fee(L1.amount_of(t), t.get("userFee", 0)) >> 128:   # amount and selector alone: the highest-numbered reason
            bad.add(FEE_OVERFLOW)
        static.append(bad - {0})
    active = [bool(t.get("fromIdx", 0)) for t in pool]
    forced, rounds = set(), 0
    while True:
        rounds += 1
        bal, nonce = {}, {}
        get = lambda a: bal[a] if a in bal else leaf_of(a)["balance"]   # noqa: E731
        for i, t in enumerate(eff_l1):   # ledger_l1_common.l1_run's recurrence, by account
            eff_load, eff2, _ = X.static_part(leaf_of, t)
            s = t["fromIdx"]
            eff3 = eff2 if get(s) + eff_load - eff2 >= 0 else 0
            bal[s] = get(s) + eff_load - eff3
            over = bal[s] >= LIMIT
            if L1.has_amount(t) and not X.is_exit(t):
                bal[t["toIdx"]] = get(t["toIdx"]) + eff3
                over = over or bal[t["toIdx"]] >= LIMIT
            if over:
                return ("refused", i, 5)
        verdict, kept = [0] * m, []
        for i, t in enumerate(pool):
            if not active[i]:
                continue
            if i in forced:
                verdict[i] = PARTNER
                continue
            s, r, bad = t["fromIdx"], receiver[i], set(static[i])
            cur = nonce.get(s, leaf_of(s)["nonce"])
            amount = L1.amount_of(t)
            debit = amount + B.compute_fee(amount, t.get("userFee", 0))
            if t.get("nonce", 0) != cur:
                bad.add(2)
            if cur == NONCE_MAX:
                bad.add(12)
            if get(s) < debit:
                bad.add(3)
            elif r and (get(s) - debit if r == s else get(r)) + amount >= LIMIT:
                bad.add(5)
            if bad:
                verdict[i] = 9 if 9 in bad else min(bad)
            elif len(kept) >= max_keep:
                verdict[i] = FULL
            else:
                kept.append(i)
                nonce[s] = cur + 1
                bal[s] = get(s) - debit
                if r:
                    bal[r] = get(r) + amount
        now, off = closure(active, partner, [int(i in kept) for i in range(m)])
        if not any(now):
            return {"verdict": verdict, "kept": kept, "rq_offset": off, "aux_to_idx": aux_to, "rounds": rounds}
        forced |= {i for i, f in enumerate(now) if f}


def compact(pool, res):
    """the kept transactions as rows to apply: the rqOffset of the compacted batch, no `partner` key"""
    return [{k: v for k, v in dict(pool[i], rqOffset=res["rq_offset"][i]).items() if k != "partner"} for i in res["kept"]]


def retry_reference(apply, l1_txs, pool):
    """the loop a caller writes without the call: apply the whole list, drop the row the refusal names, repeat. apply(l1_txs, l2_txs) ->
    None, or (L2 transaction, reason) of the refusal. -> (kept pool indices, reason per pool index, refusals)"""
    alive, reasons, refusals = list(range(len(pool))), [0] * len(pool), 0
    while True:
        r = apply(l1_txs, [pool[i] for i in alive])
        if r is None:
            return alive, reasons, refusals
        refusals += 1
        reasons[alive.pop(r[0])] = r[1]


def model_apply(acc):
    """retry_reference's apply over ledger_create_common.model: the refusal contract of hz_ledger_apply_batch_creates, no fee slots"""
    def apply(l1_txs, l2_txs):
        res = CR.model(acc, l1_txs, l2_txs, [], [])
        return (res[1] - len(l1_txs), res[2]) if isinstance(res, tuple) else None
    return apply


# ---- pools -------------------------------------------------------------------------------------------------------------------------------
def accounts(base, edit=None):
    """ledger_create_common.Accounts over the base's leaves, some of them edited: {offset: {field: value}}"""
    leaves = [dict(base.state(base.first_idx + j)) for j in range(base.N)]
    for j, fields in (edit or {}).items():
        leaves[j].update(fields)
    return CR.Accounts(leaves, base.first_idx) if edit else CR.Accounts.of(base)


def valid_pool(acc, m, seed, senders=None):
    """m transfers that are all applicable in order: nonces counted per sender, amounts a small share of what the sender holds"""
    rng = np.random.default_rng(seed)
    f0, n = acc.first_idx, acc.n
    senders = senders or list(range(n))
    bal, nonce, out = {}, {}, []
    for _ in range(m):
        f = f0 + senders[int(rng.integers(0, len(senders)))]
        t = f0 + int(rng.integers(0, n))
        leaf = acc.state(f)
        b = bal.get(f, leaf["balance"])
        amount = 0 if rng.integers(0, 8) == 0 else B.float2fix(B.floor_fix2float(b // int(rng.integers(8, 40))))
        sel = C.SELECTORS[int(rng.integers(0, len(C.SELECTORS)))]
        out.append(C.tx(f, t, amount, sel, token=leaf["tokenID"], nonce=nonce.get(f, leaf["nonce"])))
        bal[f] = b - amount - B.compute_fee(amount, sel)
        nonce[f] = nonce.get(f, leaf["nonce"]) + 1
        if amount:
            bal[t] = bal.get(t, acc.state(t)["balance"]) + amount
    return out


SPOILS = ("stale", "ahead", "overdraft", "unknown", "token")


def spoil(acc, t, how):
    """a copy of a transfer the circuit rejects: a nonce already used / not yet reached (2), more than the sender can hold (3), a
    destination nobody holds (9), a token that is not the sender's (1)"""
    t = dict(t)
    if how == "stale":
        t["nonce"] = t.get("nonce", 0) - 1 if t.get("nonce", 0) else 7
    elif how == "ahead":
        t["nonce"] = t.get("nonce", 0) + 3
    elif how == "overdraft":
        t["amountF"] = B.fix2float(((1 << 35) - 1) * 10 ** 25)
    elif how == "unknown":
        t.update(toIdx=0, toEthAddr=0xDEAD << 100, amountF=t["amountF"] or B.fix2float(1))
    elif how == "token":
        t["tokenID"] = t.get("tokenID", 0) + 5
    else:
        raise ValueError(how)
    return t


def spoilt_pool(acc, m, seed, share=4, senders=None):
    """valid_pool with about one transaction in `share` spoilt: every later transaction of a spoilt one's sender, and everything funded
    by it, then depends on the drop"""
    rng = np.random.default_rng(seed ^ 0x5E1)
    pool = valid_pool(acc, m, seed, senders)
    return [spoil(acc, t, SPOILS[int(rng.integers(0, len(SPOILS)))]) if rng.integers(0, share) == 0 else t for t in pool]


def link(pool, i, p):
    """transaction i requires transaction p: the rq fields its signer commits to are p's link fields (in place)"""
    pool[i].update(zip(Q.RQ_FIELDS, Q.link_fields(pool[p])), partner=p)


# ---- tests/native/ledger_select_check.cpp's input ----------------------------------------------------------------------------------------
def check_lines():
    """s bal kept debit tx_nonce resident expect: select_want then select_step; c to amount ok new: select_credit; o d expect:
    select_offset; l partner_kept row partner_row expect: select_link; t flags token tok_s tok_r sig expect: select_static (hex)"""
    lines = []
    bal = 5 * 10 ** 30 + 12345
    for debit, exp in ((bal - 1, 0), (bal, 0), (bal + 1, 3), ((1 << 204) - 1, 3), (0, 0)):
        lines.append("s %x %x %x %x %x %x" % (bal, 2, debit, 9, 7, exp))
    lines.append("s %x %x %x %x %x %x" % (LIMIT - 1, 0, LIMIT - 1, 0, 0, 0))
    lines.append("s %x %x %x %x %x %x" % (0, 0, 1, 0, 0, 3))
    for resident, nonce, kept, exp in ((5, 5, 0, 0), (5, 5, 1, 2), (5, 5 + 65535, 65535, 0), (5, 5 + 65535, 65534, 2), (5, 5 + 65536, 65535, 2), (5, 5 + 65536, 0, 2),
                                       (5, 4, 0, 2), (5, 4, 65535, 2), (0, 1 << 40, 0, 2), (NONCE_MAX, NONCE_MAX, 0, 12), (NONCE_MAX - 1, NONCE_MAX, 1, 12),
                                       (NONCE_MAX - 1, NONCE_MAX, 0, 2), (NONCE_MAX - 1, NONCE_MAX - 1, 0, 0), (NONCE_MAX, 1 << 40, 1, 2), (NONCE_MAX, (1 << 64) - 1, 0, 2)):
        lines.append("s %x %x %x %x %x %x" % (bal, kept, 1, nonce, resident, exp))
    lines.append("s %x %x %x %x %x %x" % (3, 0, 4, NONCE_MAX, NONCE_MAX, 3))   # 3 is lower than 12
    for to, amount in ((LIMIT - 2, 1), (LIMIT - 1, 0), (LIMIT - 1, 1), (LIMIT - 1, 2), (0, LIMIT - 1), (1, LIMIT - 1), (LIMIT - 1, ((1 << 35) - 1) * 10 ** 31),
                       (7, 0), ((1 << 160) + 5, (1 << 128) - 5)):
        ok = to + amount < LIMIT
        lines.append("c %x %x %x %x" % (to, amount, int(ok), to + amount if ok else to))
    for d in range(-7, 8):
        lines.append("o %x %x" % (d & 0xFFFFFFFF, offset_of(d)))
    for kept_p, row, prow in ((1, 0, 1), (1, 0, 3), (1, 0, 4), (1, 4, 0), (1, 5, 0), (1, 5, 4), (0, 0, 1), (0, 5, 4), (1, 4000, 4003), (1, 4095, 4091), (1, 4095, 4090)):
        lines.append("l %x %x %x %x" % (kept_p, row, prow, offset_of(prow - row) if kept_p else 0))
    for flags, token, tok_s, tok_r, sig, exp in ((1, 1, 1, 0, 0, 0), (1, 1, 2, 0, 0, 1), (9, 1, 1, 2, 0, 4), (1, 1, 1, 2, 0, 0), (9, 1, 1, 1, 7, 7), (9, 1, 1, 2, 7, 4),
                                                 (9, 1, 1, 2, 13, 4), (1, 1, 1, 0, 13, 13), (1, 1, 1, 0, 8, 8), (5, 1, 2, 0, 7, 9), (5, 1, 1, 0, 0, 9), (9, 2, 1, 1, 7, 1)):
        lines.append("t %x %x %x %x %x 0 %x" % (flags, token, tok_s, tok_r, sig, exp))
        lines.append("t %x %x %x %x %x 1 %x" % (flags, token, tok_s, tok_r, sig, exp or FEE_OVERFLOW))   # every other reason is lower
    return "\n".join(lines) + "\n" + fee_lines()


def fee_lines():
    """g float40 selector fee over: ledger_fee and ledger_fee_overflows on l1_float40's amount, over the whole float40 table of
    fee_bound_common (both check programs read this record)"""
    import fee_bound_common as FB
    lines = []
    for sel, below, above in FB.float40_table():
        for f in (below, above):
            if f is not None:
                fee = FB.fee_of(f, sel)
                lines.append("g %x %x %x %x" % (f, sel, fee, fee >> 128 != 0))
    return "\n".join(lines) + "\n"
