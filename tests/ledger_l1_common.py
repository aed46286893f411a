"""Shared by tests/test_ledger_l1.py (GPU) and tests/test_ledger_l1_cpu.py: L1 transactions on the device-resident ledger
(hz_ledger_apply_batch). A plain Python model of the scheme -- static nullifiers from the leaves before the batch, the
serial recurrence over the local slots' balances, then ledger_common's grouped prefix sums over rows --, the planner restated with the
L1 slots, the batch drawer biased towards every nullifier cause, the causes read back from BatchBuilder's own results, the named edge
batches and tests/native/ledger_l1_check.cpp's input."""
import functools

import numpy as np

import ledger_addr_common as A
import ledger_common as C
from circuits_amd import builder as B

LEAF = C.LEAF
MANT = (1 << 35) - 1
NULL_LOAD, NULL_AMOUNT = 1, 2          # bits of the static flags, and of the flag bytes (bit 1 there: isAmountNullified)
CAUSES = ("tok1", "load", "eth", "tok2", "underflow", "chain")


def l1(frm, to, amount=0, load=0, token=1, eth=0):
    """an L1 transaction on existing accounts: deposit (to = 0, amount = 0), depositTransfer, forceTransfer (load = 0)"""
    return {"onChain": 1, "fromIdx": frm, "toIdx": to, "amountF": B.fix2float(amount), "loadAmountF": B.fix2float(load), "tokenID": token, "fromEthAddr": eth}


def own(state, frm, to, amount=0, load=0, token=None, eth=None):
    """l1() with the sender's own token and address unless given"""
    leaf = state.state(frm)
    return l1(frm, to, amount, load, leaf["tokenID"] if token is None else token, leaf["ethAddr"] if eth is None else eth)


def amount_of(t):
    return B.float2fix(t.get("amountF", 0))


def load_of(t):
    return B.float2fix(t.get("loadAmountF", 0))


def has_amount(t):
    return bool(t.get("amountF", 0) & MANT)


# ---- the planner, restated ---------------------------------------------------------------------------------------------------------------
def plan_model(l1_txs, l2_txs, plan_tokens, fee_idxs):
    """ledger_common.plan_model over rows (L1 first; kinds 3 and 4 are the L1 sender and receiver), plus the local slots of the L1 run:
    the accounts it touches numbered by first appearance, sender before receiver"""
    n_l1, R = len(l1_txs), len(l1_txs) + len(l2_txs)
    out = {"ev_sender": [-1] * R, "ev_receiver": [-1] * R, "fee_slot": [-1] * R, "last_event": [-1] * R, "account": [], "prev_same": [], "unit": [], "kind": [],
           "l1_slot_sender": [], "l1_slot_receiver": [], "slot_account": []}
    last = {}

    def event(acct, unit, kind):
        out["account"].append(acct)
        out["prev_same"].append(last.get(acct, -1))
        out["unit"].append(unit)
        out["kind"].append(kind)
        last[acct] = len(out["account"]) - 1
        return last[acct]

    def slot(acct):
        if acct not in out["slot_account"]:
            out["slot_account"].append(acct)
        return out["slot_account"].index(acct)
    for i, t in enumerate(l1_txs + l2_txs):
        on = i < n_l1
        if t.get("fromIdx", 0):
            out["ev_sender"][i] = event(t["fromIdx"], i, 3 if on else 0)
            if on:
                out["l1_slot_sender"].append(slot(t["fromIdx"]))
                out["l1_slot_receiver"].append(slot(t["toIdx"]) if has_amount(t) else -1)
            if has_amount(t):
                out["ev_receiver"][i] = event(t["toIdx"], i, 4 if on else 1)
            if not on:
                tok = t.get("tokenID", 0)
                out["fee_slot"][i] = list(plan_tokens).index(tok) if tok in plan_tokens else -1
        out["last_event"][i] = len(out["account"]) - 1
    out["ev_fee"] = [event(a, R + j, 2) if a else -1 for j, a in enumerate(fee_idxs)]
    return out


# ---- the scheme --------------------------------------------------------------------------------------------------------------------------
def static_part(leaf_of, t):
    """(eff_load, eff2, flags) of an L1 transaction from the leaves as they are before the batch"""
    s = leaf_of(t["fromIdx"])
    amount, load, token = amount_of(t), load_of(t), t.get("tokenID", 0)
    null_tok1 = token != s["tokenID"]
    null_load = null_tok1 and load != 0
    null_eth = amount != 0 and t.get("fromEthAddr", 0) != s["ethAddr"]
    null_tok2 = amount != 0 and token != leaf_of(t["toIdx"])["tokenID"]
    null_amount = null_eth or null_tok2 or (null_tok1 and amount != 0)
    return 0 if null_load else load, 0 if null_amount else amount, (NULL_LOAD if null_load else 0) | (NULL_AMOUNT if null_amount else 0)


def l1_run(leaf_of, l1_txs, p):
    """the device's L1 kernel: phase 1 (static parts, the slots' balances), phase 2 (the recurrence in order over the slots), phase 3
    (deltas by event, flag bytes) -> (delta {event: value}, flags, eff3 per transaction, final balance per slot)"""
    stat = [static_part(leaf_of, t) for t in l1_txs]
    bal = [leaf_of(a)["balance"] for a in p["slot_account"]]
    delta, flags, eff3s = {}, [], []
    for i, (eff_load, eff2, fl) in enumerate(stat):
        s, r = p["l1_slot_sender"][i], p["l1_slot_receiver"][i]
        ok = bal[s] + eff_load - eff2 >= 0
        eff3 = eff2 if ok else 0
        bal[s] += eff_load - eff3
        if r >= 0:
            bal[r] += eff3
        delta[p["ev_sender"][i]] = eff_load - eff3
        if p["ev_receiver"][i] >= 0:
            delta[p["ev_receiver"][i]] = eff3
        flags.append((fl & NULL_LOAD) | (0 if (not fl & NULL_AMOUNT and ok) else NULL_AMOUNT))
        eff3s.append(eff3)
    return delta, flags, eff3s, bal


def scheme_model(leaf_of, l1_txs, l2_txs, plan_tokens, fee_idxs):
    """The ledger's scheme over a whole batch on Python integers, the way the kernels do it: the L1 run leaves its events' deltas, the L2
    rows and the fee scan theirs, and then every account's events are walked as one group. An L1 event checks neither token nor nonce;
    reason 3 cannot arise on it (asserted); reason 5 can. -> ("refused", row, reason) or
    ("ok", leaf fields by name, acc_fee_after, final, flags, {account: leaf after the batch})"""
    n_l1, R, F = len(l1_txs), len(l1_txs) + len(l2_txs), len(plan_tokens)
    rows_tx = list(l1_txs) + list(l2_txs)
    p = plan_model(l1_txs, l2_txs, plan_tokens, fee_idxs)
    M = len(p["account"])
    l1_delta, flags, _, slot_bal = l1_run(leaf_of, l1_txs, p)
    delta, acc, rows, over = [0] * M, [0] * F, [], []
    for e, v in l1_delta.items():
        delta[e] = v
    for i, t in enumerate(rows_tx):
        if i >= n_l1 and t.get("fromIdx", 0):
            amount = amount_of(t)
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
    fail, before, after = min(over) if over else None, [None] * M, {}
    for a in sorted(groups, reverse=True):
        leaf = dict(leaf_of(a))
        for e in groups[a]:
            before[e] = dict(leaf)
            unit, kind = p["unit"][e], p["kind"][e]
            bad = []
            if kind < 3:
                tok = plan_tokens[unit - R] if kind == 2 else rows_tx[unit].get("tokenID", 0)
                if leaf["tokenID"] != tok:
                    bad.append((1, 4, 6)[kind])
            if kind == 0:
                if leaf["nonce"] != rows_tx[unit].get("nonce", 0):
                    bad.append(2)
                if leaf["nonce"] == (1 << 40) - 1:   # reason 12: nonce + 1 is not a leaf field, and the circuit does not wrap
                    bad.append(12)
                leaf["nonce"] += 1
            leaf["balance"] += delta[e]
            if leaf["balance"] < 0:
                assert kind < 3, "reason 3 on an L1 event"
                bad.append(3)
            elif leaf["balance"] >= 1 << 192:
                bad.append(5)
            for r in bad:
                fail = min(fail, (unit, r)) if fail else (unit, r)
        after[a] = leaf
    # the balances the serial phase carried are the ones the grouped walk reaches after the account's last L1 event
    for q, a in enumerate(p["slot_account"]):
        last_l1 = [e for e in groups[a] if p["kind"][e] >= 3][-1]
        assert leaf_of(a)["balance"] + sum(delta[e] for e in groups[a] if e <= last_l1) == slot_bal[q]
    if fail:
        return ("refused",) + fail
    zero = dict.fromkeys(LEAF, 0)
    out = {f + n: [] for n in "123" for f in LEAF}
    for i, t in enumerate(rows_tx):
        s1 = before[p["ev_sender"][i]] if p["ev_sender"][i] >= 0 else zero
        s2 = before[p["ev_receiver"][i]] if p["ev_receiver"][i] >= 0 else dict(zero, tokenID=t.get("tokenID", 0) if i >= n_l1 and t.get("fromIdx", 0) else 0)
        for f in LEAF:
            out[f + "1"].append(s1[f])
            out[f + "2"].append(s2[f])
    for j in range(F):
        s3 = before[p["ev_fee"][j]] if p["ev_fee"][j] >= 0 else zero
        for f in LEAF:
            out[f + "3"].append(s3[f])
    return "ok", out, rows, acc, flags, after


# ---- the checker -------------------------------------------------------------------------------------------------------------------------
def builder_batch(state, l1_txs, l2_txs, plan_tokens, fee_idxs, n_levels, n_tx=None, db=None, max_l1=None):
    """BatchBuilder over the same state with host hashing; the L2 transactions get their auxToIdx as in ledger_addr_common"""
    n_tx = n_tx or len(l1_txs) + len(l2_txs)
    txs = [dict(t) for t in l1_txs] + list(l2_txs) + [{} for _ in range(n_tx - len(l1_txs) - len(l2_txs))]
    return A.builder_batch(state, txs, plan_tokens, fee_idxs, n_levels, db=db, max_l1=len(l1_txs) if max_l1 is None else max_l1)


def builder_flags(bb, n_l1):
    """the flag bytes from the builder's own results: nullifyLoadAmount is read off the leaves (a load that did not arrive)"""
    inp, out = bb.get_input(), []
    for i in range(n_l1):
        load_nullified = inp["tokenID1"][i] != (inp["txCompressedData"][i] >> 144) & 0xFFFFFFFF and inp["loadAmountF"][i] & MANT != 0
        out.append((NULL_LOAD if load_nullified else 0) | (NULL_AMOUNT if bb.tx_meta[i]["isAmountNullified"] else 0))
    return out


def builder_causes(bb, n_l1):
    """which nullifier causes a built batch holds, by the builder's results alone (its before-leaves and isAmountNullified): tok1, load,
    eth, tok2; underflow: nullified with no static cause; chain: an underflow that would not have happened had an earlier transfer into
    that sender, itself nullified by underflow, gone through"""
    inp, found, missed = bb.get_input(), set(), {}
    for i in range(n_l1):
        token = (inp["txCompressedData"][i] >> 144) & 0xFFFFFFFF
        amount, load = B.float2fix(inp["amountF"][i]), B.float2fix(inp["loadAmountF"][i])
        tok1 = token != inp["tokenID1"][i]
        eth = amount != 0 and inp["fromEthAddr"][i] != inp["ethAddr1"][i]
        tok2 = amount != 0 and token != inp["tokenID2"][i]
        found |= {name for name, hit in (("tok1", tok1), ("load", tok1 and load), ("eth", eth), ("tok2", tok2)) if hit}
        if bb.tx_meta[i]["isAmountNullified"] and not (tok1 and amount) and not eth and not tok2:
            found.add("underflow")
            frm = inp["fromIdx"][i]
            if inp["balance1"][i] + load + missed.get(frm, 0) >= amount:
                found.add("chain")
            missed[inp["toIdx"][i]] = missed.get(inp["toIdx"][i], 0) + amount
    return found


def expected_arrays(bb, l2_txs, n_l1):
    """the builder's dictionary in hz_ledger_apply_batch's output layout, with the zero-amount rows of L2 transfers to an address as
    ledger_addr_common specifies them"""
    exp = C.expected_arrays(bb)
    exp["auxToIdx"] = C.to_bytes(bb.get_input()["auxToIdx"])
    for i, row in A.zero_amount_rows(l2_txs).items():
        for name, v in row.items():
            exp[name][n_l1 + i] = C.to_bytes([v])[0]
    return exp


def touched(l1_txs, l2_txs, fee_idxs, aux=()):
    acc = set()
    for t in list(l1_txs) + list(l2_txs):
        if t.get("fromIdx"):
            acc |= {t["fromIdx"]} | ({t["toIdx"]} if t.get("toIdx") else set())
    return sorted(acc | {i for i in fee_idxs if i} | {a for a in aux if a})


# ---- batches -----------------------------------------------------------------------------------------------------------------------------
def float_floor(x):
    return B.float2fix(B.floor_fix2float(x))


def draw_batch(state, seed, n_l1=8, m=8):
    """n_l1 L1 transactions biased towards the nullifier causes (a foreign token with and without a load, a foreign address, a receiver of
    another token, amounts above the balance, a sender that counts on the transfer just before it), then m valid L2 transfers on the
    balances the L1 run leaves -> (l1_txs, l2_txs)"""
    rng = np.random.default_rng(seed)
    f0, N = state.first_idx, state.N
    leaf = {i: state.state(i) for i in range(f0, f0 + N)}
    bal = {i: leaf[i]["balance"] for i in leaf}
    by_token = {}
    for i in leaf:
        by_token.setdefault(leaf[i]["tokenID"], []).append(i)
    pool = [f0 + int(x) for x in rng.choice(N, size=min(N, 6), replace=False)]
    l1_txs, prev, chain_next = [], None, False
    for _ in range(n_l1):
        kind = 9 if chain_next else int(rng.integers(0, 10))
        chain_next = kind in (5, 6) and rng.integers(0, 2) == 0
        frm = pool[int(rng.integers(0, len(pool)))]
        if kind == 9 and prev is not None:
            frm = prev["toIdx"] or frm          # the receiver of the transfer before, whatever became of it
        same = [i for i in pool if leaf[i]["tokenID"] == leaf[frm]["tokenID"]] or [frm]
        to = same[int(rng.integers(0, len(same)))]
        if kind == 3:
            other = [i for i in pool if leaf[i]["tokenID"] != leaf[frm]["tokenID"]]
            to = other[int(rng.integers(0, len(other)))] if other else to
        token = leaf[frm]["tokenID"] if kind not in (1, 2) else 3 - leaf[frm]["tokenID"]
        eth = leaf[frm]["ethAddr"] if kind != 4 else leaf[frm]["ethAddr"] ^ 1
        load = float_floor(int(rng.integers(1, 1 << 60))) if kind in (0, 1, 5) or rng.integers(0, 3) == 0 else 0
        amount = float_floor(bal[frm] // int(rng.integers(2, 9)))
        if kind in (5, 6, 9):
            amount = float_floor(2 * (bal[frm] + load) + 1000)      # above what the sender holds
            if kind == 9 and prev is not None and amount_of(prev):
                amount = float_floor(bal[frm] + amount_of(prev) // 2)   # covered only if the transfer before arrived
        if kind == 0:
            amount, to = 0, 0                     # a plain deposit
        if kind == 7:
            to = frm                              # a self-transfer
        t = l1(frm, to, amount, load, token, eth)
        l1_txs.append(t)
        # follow the balances as the circuit does, so that later draws know what the accounts hold
        eff_load, eff2, _ = static_part(lambda a: leaf[a], t)
        eff3 = eff2 if bal[frm] + eff_load - eff2 >= 0 else 0
        bal[frm] += eff_load - eff3
        if amount_of(t):
            bal[to] += eff3
        prev = t
    nonce, l2_txs = {}, []
    for _ in range(m):
        f = pool[int(rng.integers(0, len(pool)))] if rng.integers(0, 2) else f0 + int(rng.integers(0, N))
        same = by_token[leaf[f]["tokenID"]]
        t = same[int(rng.integers(0, len(same)))]
        amount = 0 if rng.integers(0, 8) == 0 else float_floor(bal[f] // int(rng.integers(8, 40)))
        sel = C.SELECTORS[int(rng.integers(0, len(C.SELECTORS)))]
        l2_txs.append(C.tx(f, t, amount, sel, token=leaf[f]["tokenID"], nonce=nonce.get(f, 0)))
        bal[f] -= amount + B.compute_fee(amount, sel)
        nonce[f] = nonce.get(f, 0) + 1
        if amount:
            bal[t] += amount
    return l1_txs, l2_txs


SEEDS = (1, 2, 3, 4, 5, 6)      # with the states of seeded_batches: every cause of CAUSES occurs (asserted on the CPU, by the builder)


def seeded_batches():
    """[(k, state, l1_txs, l2_txs)]: 16 to 64 accounts, at most 8 + 8 transactions"""
    out = []
    for n, seed in enumerate(SEEDS):
        k = 4 + n % 3
        st = A.mixed_state(k)
        l1_txs, l2_txs = draw_batch(st, seed, n_l1=8 - n % 2, m=8 - n % 3)
        out.append((k, st, l1_txs, l2_txs))
    return out


def fee_accounts(st):
    tok = [st.state(st.first_idx + j)["tokenID"] for j in range(st.N)]
    return [st.first_idx + tok.index(1), st.first_idx + tok.index(2), 0, 0]


def edge_batches(sp):
    """the named edges on ledger_addr_common.special_state(k >= 5): {name: (l1_txs, l2_txs)}. Accounts f0 + 1 .. f0 + 8 hold token 1
    (except those special_state edits), f0 + 9 holds token 2"""
    f0, leaf = sp.first_idx, sp.state
    a, b, c, d = f0 + 1, f0 + 3, f0 + 4, f0 + 6
    assert all(leaf(x)["tokenID"] == 1 for x in (a, b, c, d)) and leaf(f0 + 9)["tokenID"] == 2
    bal = lambda x: leaf(x)["balance"]   # noqa: E731
    big = float_floor(2 * bal(a) + 10)
    return {
        # A -> B underflows; B -> C counted on it and is nullified too; C -> D does not and goes through
        "underflow_chain": ([own(sp, a, b, big), own(sp, b, c, float_floor(bal(b) + big // 2)), own(sp, c, d, float_floor(bal(c) // 2))], []),
        # the amount is covered only by the load of the same transaction
        "deposit_transfer_spends_its_load": ([own(sp, a, b, float_floor(3 * bal(a) // 2), load=float_floor(bal(a)))], []),
        # a foreign token nullifies the load (and the amount); the same sender then cannot cover what the load would have
        "load_nullified_then_underflow": ([own(sp, a, b, 0, load=float_floor(4 * bal(a)), token=2), own(sp, a, b, float_floor(3 * bal(a)))], []),
        "self_transfer": ([own(sp, a, a, float_floor(bal(a) // 2), load=77), own(sp, a, a, float_floor(3 * bal(a)))], []),
        "from_eth_addr_mismatch": ([own(sp, a, b, 1000, load=50, eth=leaf(a)["ethAddr"] ^ 2), own(sp, a, b, 0, load=60, eth=12345)], []),
        "receiver_token_mismatch": ([own(sp, a, f0 + 9, 1000, load=50)], []),
        "zero_amount_deposit": ([own(sp, a, 0, 0, load=123000), own(sp, b, c, 0, load=5)], []),
        "one_account_pair": ([own(sp, a, b, float_floor(bal(a) // 3)), own(sp, b, a, float_floor(bal(b) // 5), load=9), own(sp, a, b, big),
                              own(sp, b, a, 100), own(sp, a, b, 200, load=7, token=2), own(sp, a, b, 0, load=1), own(sp, b, a, float_floor(bal(b) // 7)),
                              own(sp, a, b, 300)], []),
        # the deposit funds an L2 transfer the resident balance could not
        "l2_funded_by_l1_deposit": ([own(sp, a, 0, 0, load=float_floor(8 * bal(a)))], [C.tx(a, b, float_floor(5 * bal(a)), 176, nonce=0)]),
    }


@functools.lru_cache(maxsize=None)
def rich_state(k=6):
    """special_state with account f0 + 1 at 2^192 - 1000: a load of 1000 or more is reason 5"""
    def edit(cols):
        cols[1][1] = C.to_bytes([(1 << 192) - 1000])[0]
    return A.with_planes(A.special_state(k), edit)


def refused_after_nullified(sp):
    """A -> B is nullified by underflow; the L2 transfer from B that counted on it is refused with reason 3 at its own row"""
    f0, leaf = sp.first_idx, sp.state
    a, b, c = f0 + 1, f0 + 3, f0 + 4
    big = float_floor(2 * leaf(a)["balance"] + 10)
    return [own(sp, a, b, big)], [C.tx(c, a, 10, 0, nonce=0), C.tx(b, c, float_floor(leaf(b)["balance"] + big // 2), 0, nonce=0)]


# ---- tests/native/ledger_l1_check.cpp's input --------------------------------------------------------------------------------------------
def check_lines(cases):
    """cases: [(leaf_of, l1_txs)]; every case is one run of the recurrence: its slots' balances, its transactions with what the model
    expects of each (eff3, flag byte, the sender's delta in two's complement), the balances afterwards"""
    lines = []
    for leaf_of, txs in cases:
        p = plan_model(txs, [], [], [])
        _, flags, eff3s, bal = l1_run(leaf_of, txs, p)
        lines.append("r %x" % len(p["slot_account"]))
        for q, a in enumerate(p["slot_account"]):
            lines.append("b %x %x" % (q, leaf_of(a)["balance"]))
        for i, t in enumerate(txs):
            s = leaf_of(t["fromIdx"])
            tok_r = leaf_of(t["toIdx"])["tokenID"] if has_amount(t) else 0
            eff_load = static_part(leaf_of, t)[0]
            lines.append("t %x %x %x %x %x %x %x %x %x %x %x %x" % (
                p["l1_slot_sender"][i], p["l1_slot_receiver"][i] & 0xFFFF, t["amountF"], t["loadAmountF"], t["tokenID"], t["fromEthAddr"], s["tokenID"],
                s["ethAddr"], tok_r, eff3s[i], flags[i], (eff_load - eff3s[i]) % (1 << 256)))
        for q in range(len(bal)):
            lines.append("e %x %x" % (q, bal[q]))
    return "\n".join(lines) + "\n"
