"""Shared by tests/test_ledger_exit.py (GPU) and tests/test_ledger_exit_cpu.py: exits on the device-resident ledger
(hz_ledger_apply_batch_exits). The planner restated in plain Python with the second list of exit operations; a model of the
scheme -- the L1 run with forceExits, the grouped walk over the state events, the exit scan over the operations of every exit key --; the
checker's results lifted into the call's output layout; a batch drawer that mixes every row kind; the named edge batches and
tests/native/ledger_exit_check.cpp's input."""
import functools

import numpy as np

import ledger_addr_common as A
import ledger_common as C
import ledger_l1_common as L1
from circuits_amd import builder as B

LEAF = C.LEAF
EXIT = B.EXIT_IDX
EXIT_ARRAYS = ("new_exit", "is_old0_2", "old_key2", "old_value2", "exit_root_after", "new_exit_root")
MAX_AMOUNT = ((1 << 35) - 1) * 10 ** 31   # the largest float40


def is_exit(t):
    return bool(t.get("fromIdx", 0)) and t.get("toIdx", 0) == EXIT


def x2(frm, amount, fee=0, token=1, nonce=None):
    """an L2 exit"""
    return C.tx(frm, EXIT, amount, fee, token=token, nonce=nonce)


def fx(state, frm, amount, load=0, token=None, eth=None):
    """an L1 forceExit with the sender's own token and address unless given"""
    return L1.own(state, frm, EXIT, amount, load, token, eth)


# ---- the planner, restated ---------------------------------------------------------------------------------------------------------------
def plan_model(l1_txs, l2_txs, plan_tokens, fee_idxs):
    """ledger_l1_common.plan_model where a row with toIdx == 1 makes no receiver event: with an amount it makes an operation on the exit
    tree at key fromIdx instead. The operations in row order are a second list (exit_row, exit_key); exit_prev is the previous
    operation on the same key (-1: this one inserts the key), exit_perm the operations grouped by key, groups by first appearance"""
    n_l1, R = len(l1_txs), len(l1_txs) + len(l2_txs)
    out = {"ev_sender": [-1] * R, "ev_receiver": [-1] * R, "fee_slot": [-1] * R, "last_event": [-1] * R, "account": [], "prev_same": [], "unit": [], "kind": [],
           "l1_slot_sender": [], "l1_slot_receiver": [], "slot_account": [], "ev_exit": [-1] * R, "last_exit": [-1] * R, "exit_row": [], "exit_key": [],
           "exit_prev": []}
    last, last_x = {}, {}

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
    for i, t in enumerate(list(l1_txs) + list(l2_txs)):
        on = i < n_l1
        if t.get("fromIdx", 0):
            out["ev_sender"][i] = event(t["fromIdx"], i, 3 if on else 0)
            receiver = L1.has_amount(t) and not is_exit(t)
            if on:
                out["l1_slot_sender"].append(slot(t["fromIdx"]))
                out["l1_slot_receiver"].append(slot(t["toIdx"]) if receiver else -1)
            if receiver:
                out["ev_receiver"][i] = event(t["toIdx"], i, 4 if on else 1)
            elif L1.has_amount(t):
                out["ev_exit"][i] = len(out["exit_row"])
                out["exit_prev"].append(last_x.get(t["fromIdx"], -1))
                last_x[t["fromIdx"]] = len(out["exit_row"])
                out["exit_row"].append(i)
                out["exit_key"].append(t["fromIdx"])
            if not on:
                tok = t.get("tokenID", 0)
                out["fee_slot"][i] = list(plan_tokens).index(tok) if tok in plan_tokens else -1
        out["last_event"][i] = len(out["account"]) - 1
        out["last_exit"][i] = len(out["exit_row"]) - 1
    out["ev_fee"] = [event(a, R + j, 2) if a else -1 for j, a in enumerate(fee_idxs)]
    order = []
    for key in out["exit_key"]:
        if key not in order:
            order.append(key)
    out["exit_perm"] = [x for key in order for x, k2 in enumerate(out["exit_key"]) if k2 == key]
    return out


def tree_plan_model(keys):
    """what circomlib's tree does with ordered inserts of keys into the empty tree, by the key set alone: (insert, is_old0, old_key, depth of
    the new leaf) per operation. A key is alone at the shallowest depth where no other held key shares its low bits"""
    held, out = [], []
    for key in keys:
        if key in held:
            out.append((0, 0, key, None))
            continue
        f = 0   # the find depth: the walk descends while more than one held key shares the prefix
        while sum(1 for h in held if (h ^ key) & ((1 << f) - 1) == 0) > 1:
            f += 1
        met = [h for h in held if (h ^ key) & ((1 << f) - 1) == 0]
        if not met:
            out.append((1, 1, key, f))
        else:
            d = f
            while not ((met[0] ^ key) >> d) & 1:
                d += 1
            out.append((1, 0, met[0], d + 1))
        held.append(key)
    return out


# ---- the scheme --------------------------------------------------------------------------------------------------------------------------
def static_part(leaf_of, t):
    """ledger_l1_common.static_part, where the receiver's token of a forceExit is the sender's: null_tok2 adds nothing"""
    if not is_exit(t):
        return L1.static_part(leaf_of, t)
    s = leaf_of(t["fromIdx"])
    amount, load, token = L1.amount_of(t), L1.load_of(t), t.get("tokenID", 0)
    null_tok1 = token != s["tokenID"]
    null_load = null_tok1 and load != 0
    null_eth = amount != 0 and t.get("fromEthAddr", 0) != s["ethAddr"]
    null_amount = null_eth or (null_tok1 and amount != 0)
    return 0 if null_load else load, 0 if null_amount else amount, (L1.NULL_LOAD if null_load else 0) | (L1.NULL_AMOUNT if null_amount else 0)


def l1_run(leaf_of, l1_txs, p):
    """ledger_l1_common.l1_run with forceExits: no receiver slot, eff3 left for the exit operation -> (delta, flags, eff3s)"""
    bal = [leaf_of(a)["balance"] for a in p["slot_account"]]
    delta, flags, eff3s = {}, [], []
    for i, t in enumerate(l1_txs):
        eff_load, eff2, fl = static_part(leaf_of, t)
        s, r = p["l1_slot_sender"][i], p["l1_slot_receiver"][i]
        ok = bal[s] + eff_load - eff2 >= 0
        eff3 = eff2 if ok else 0
        bal[s] += eff_load - eff3
        if r >= 0:
            bal[r] += eff3
        delta[p["ev_sender"][i]] = eff_load - eff3
        if p["ev_receiver"][i] >= 0:
            delta[p["ev_receiver"][i]] = eff3
        flags.append((fl & L1.NULL_LOAD) | (0 if (not fl & L1.NULL_AMOUNT and ok) else L1.NULL_AMOUNT))
        eff3s.append(eff3)
    return delta, flags, eff3s


def exit_scan(leaf_of, p, amounts):
    """the device's exit scan: key by key (NOT row by row), the operations of a key in order. The first inserts {tokenID, sign, ay, ethAddr}
    of the sender's leaf as it is before the batch, nonce 0, balance eff3; the later ones add. -> (the leaf before every operation,
    None for an insert; the leaf after it; the lowest (row, 5) where a new balance reaches 2^192, or None)"""
    X = len(p["exit_row"])
    before, after, fail = [None] * X, [None] * X, None
    groups = {}
    for x in p["exit_perm"]:
        groups.setdefault(p["exit_key"][x], []).append(x)
    for key in sorted(groups, reverse=True):   # any order of the keys must give the same answer
        s = leaf_of(key)
        leaf = None
        for x in groups[key]:
            before[x] = dict(leaf) if leaf else None
            leaf = dict(leaf) if leaf else {"tokenID": s["tokenID"], "nonce": 0, "sign": s["sign"], "balance": 0, "ay": s["ay"], "ethAddr": s["ethAddr"]}
            leaf["balance"] += amounts[x]
            if leaf["balance"] >= 1 << 192:
                fail = min(fail, (p["exit_row"][x], 5)) if fail else (p["exit_row"][x], 5)
            after[x] = dict(leaf)
    return before, after, fail


def scheme_model(leaf_of, l1_txs, l2_txs, plan_tokens, fee_idxs):
    """ledger_l1_common.scheme_model over rows that may be exits. -> ("refused", row, reason) or ("ok", leaf fields by name, acc_fee_after,
    final, flags, {account: leaf after}, newExit per row, {key: exit leaf after the batch})"""
    n_l1, R, F = len(l1_txs), len(l1_txs) + len(l2_txs), len(plan_tokens)
    rows_tx = list(l1_txs) + list(l2_txs)
    p = plan_model(l1_txs, l2_txs, plan_tokens, fee_idxs)
    M, X = len(p["account"]), len(p["exit_row"])
    l1_delta, flags, eff3s = l1_run(leaf_of, l1_txs, p)
    delta, acc, rows, amounts, over = [0] * M, [0] * F, [], [0] * X, []
    for e, v in l1_delta.items():
        delta[e] = v
    for i, t in enumerate(rows_tx):
        if i >= n_l1 and t.get("fromIdx", 0):
            amount = L1.amount_of(t)
            fee = B.compute_fee(amount, t.get("userFee", 0))
            if fee >> 128:   # reason 16: the circuit rejects such a fee (src/compute-fee.circom:89-91); only a charged row has one
                over.append((i, 16))
            delta[p["ev_sender"][i]] = -(amount + fee)
            if p["ev_receiver"][i] >= 0:
                delta[p["ev_receiver"][i]] = amount
            if p["fee_slot"][i] >= 0:
                acc[p["fee_slot"][i]] += fee
        if p["ev_exit"][i] >= 0:
            amounts[p["ev_exit"][i]] = eff3s[i] if i < n_l1 else L1.amount_of(t)
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
                if leaf["nonce"] == (1 << 40) - 1:
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
    x_before, x_after, x_fail = exit_scan(leaf_of, p, amounts)
    if x_fail:
        fail = min(fail, x_fail) if fail else x_fail
    if fail:
        return ("refused",) + fail
    zero = dict.fromkeys(LEAF, 0)
    out = {f + n: [] for n in "123" for f in LEAF}
    new_exit = []
    for i, t in enumerate(rows_tx):
        s1 = before[p["ev_sender"][i]] if p["ev_sender"][i] >= 0 else zero
        if p["ev_exit"][i] >= 0:
            s2 = x_before[p["ev_exit"][i]] or zero
            new_exit.append(0 if x_before[p["ev_exit"][i]] else 1)
        else:
            s2 = before[p["ev_receiver"][i]] if p["ev_receiver"][i] >= 0 else dict(zero, tokenID=t.get("tokenID", 0) if i >= n_l1 and t.get("fromIdx", 0) else 0)
            new_exit.append(0)
        for f in LEAF:
            out[f + "1"].append(s1[f])
            out[f + "2"].append(s2[f])
    for j in range(F):
        s3 = before[p["ev_fee"][j]] if p["ev_fee"][j] >= 0 else zero
        for f in LEAF:
            out[f + "3"].append(s3[f])
    exit_leaves = {p["exit_key"][x]: x_after[x] for x in range(X)}   # (row order: the last operation of a key stays)
    return "ok", out, rows, acc, flags, after, new_exit, exit_leaves


# ---- the checker -------------------------------------------------------------------------------------------------------------------------
builder_batch = L1.builder_batch


def expected_arrays(bb, l2_txs, n_l1):
    """ledger_l1_common.expected_arrays plus the six exit arrays from the builder's dictionary"""
    exp = L1.expected_arrays(bb, l2_txs, n_l1)
    inp = bb.get_input()
    exp.update(new_exit=C.to_bytes(inp["newExit"]), is_old0_2=C.to_bytes(inp["isOld0_2"]), old_key2=C.to_bytes(inp["oldKey2"]),
               old_value2=C.to_bytes(inp["oldValue2"]), exit_root_after=C.to_bytes(inp["imExitRoot"] + [bb.new_exit_root]),
               new_exit_root=C.to_bytes([bb.new_exit_root]))
    return exp


def exit_leaf_rows(bb, keys):
    """the builder's exit leaves as hz_ledger_exit_accounts returns them: [n, 4, 32]"""
    return np.stack([C.to_bytes(B.leaf_fields(bb.exit_leaves[i])) for i in keys])


def touched(state, l1_txs, l2_txs, fee_idxs):
    acc = set()
    for t in list(l1_txs) + list(l2_txs):
        if t.get("fromIdx"):
            acc |= {t["fromIdx"]} | ({t["toIdx"]} if t.get("toIdx", 0) > EXIT else set())
    return sorted(acc | {i for i in fee_idxs if i} | {a for a in A.aux_list(state, l2_txs) if a})


# ---- batches -----------------------------------------------------------------------------------------------------------------------------
def draw_batch(state, seed, n_l1=8, m=10):
    """every row kind in one batch: deposits, depositTransfers, forceTransfers and forceExits (valid, with a foreign token or address, above
    the balance, of zero amount), then valid L2 transfers (some to an address), L2 exits (repeated on one account, of zero amount,
    after a forceExit of the same account) on the balances the L1 run leaves -> (l1_txs, l2_txs)"""
    rng = np.random.default_rng(seed)
    f0, N = state.first_idx, state.N
    leaf = {i: state.state(i) for i in range(f0, f0 + N)}
    bal = {i: leaf[i]["balance"] for i in leaf}
    by_token = {}
    for i in leaf:
        by_token.setdefault(leaf[i]["tokenID"], []).append(i)
    pool = [f0 + int(x) for x in rng.choice(N, size=min(N, 5), replace=False)]
    l1_txs = []
    for _ in range(n_l1):
        kind = int(rng.integers(0, 8))
        frm = pool[int(rng.integers(0, len(pool)))]
        same = [i for i in pool if leaf[i]["tokenID"] == leaf[frm]["tokenID"]]
        to = EXIT if rng.integers(0, 2) else same[int(rng.integers(0, len(same)))]
        token = leaf[frm]["tokenID"] if kind != 1 else 3 - leaf[frm]["tokenID"]
        eth = leaf[frm]["ethAddr"] if kind != 2 else leaf[frm]["ethAddr"] ^ 1
        load = L1.float_floor(int(rng.integers(1, 1 << 60))) if kind in (0, 4) else 0
        amount = L1.float_floor(bal[frm] // int(rng.integers(2, 9)))
        if kind == 3:
            amount = L1.float_floor(2 * (bal[frm] + load) + 1000)
        if kind == 0:
            amount, to = 0, (EXIT if to == EXIT else 0)     # a deposit, or a forceExit of nothing
        t = L1.l1(frm, to, amount, load, token, eth)
        l1_txs.append(t)
        eff_load, eff2, _ = static_part(lambda a: leaf[a], t)
        eff3 = eff2 if bal[frm] + eff_load - eff2 >= 0 else 0
        bal[frm] += eff_load - eff3
        if L1.amount_of(t) and to != EXIT:
            bal[to] += eff3
    nonce, l2_txs = {}, []
    for _ in range(m):
        f = pool[int(rng.integers(0, len(pool)))] if rng.integers(0, 3) else f0 + int(rng.integers(0, N))
        same = by_token[leaf[f]["tokenID"]]
        to = same[int(rng.integers(0, len(same)))]
        amount = 0 if rng.integers(0, 8) == 0 else L1.float_floor(bal[f] // int(rng.integers(8, 40)))
        sel = C.SELECTORS[int(rng.integers(0, len(C.SELECTORS)))]
        t = C.tx(f, to, amount, sel, token=leaf[f]["tokenID"], nonce=nonce.get(f, 0))
        r = int(rng.integers(0, 5))
        if r < 2:
            t["toIdx"] = to = EXIT
        elif r == 2:
            t = A.to_addr(t, leaf[to])
            to = A.brute_force(state, t)
        l2_txs.append(t)
        bal[f] -= amount + B.compute_fee(amount, sel)
        nonce[f] = nonce.get(f, 0) + 1
        if amount and to != EXIT:
            bal[to] += amount
    return l1_txs, l2_txs


SEEDS = (11, 12, 13, 14, 15, 16)
KINDS = ("deposit", "l1_transfer", "force_exit", "force_exit_zero", "force_exit_nullified", "l2_transfer", "l2_to_addr", "l2_exit", "l2_exit_zero",
         "l2_exit_update", "l2_exit_after_force_exit")


def seeded_batches():
    """[(k, state, l1_txs, l2_txs)]: 16 to 64 accounts, at most 8 + 10 rows"""
    out = []
    for n, seed in enumerate(SEEDS):
        k = 4 + n % 3
        st = A.mixed_state(k)
        out.append((k, st) + draw_batch(st, seed, n_l1=8 - n % 2, m=10 - n % 3))
    return out


def kinds_of(bb, l1_txs, l2_txs):
    """which row kinds of KINDS a built batch holds, by the builder's results"""
    inp, found, seen = bb.get_input(), set(), set()
    for i, t in enumerate(list(l1_txs) + list(l2_txs)):
        on, amount = i < len(l1_txs), L1.has_amount(t)
        if is_exit(t):
            if on:
                found.add("force_exit" if amount else "force_exit_zero")
                if amount and bb.tx_meta[i]["isAmountNullified"]:
                    found.add("force_exit_nullified")
            else:
                found.add("l2_exit" if amount else "l2_exit_zero")
                if amount and not inp["newExit"][i]:
                    found.add("l2_exit_update")
                    if t["fromIdx"] in seen:
                        found.add("l2_exit_after_force_exit")
            if on and amount:
                seen.add(t["fromIdx"])
        elif on:
            found.add("l1_transfer" if amount else "deposit")
        elif t.get("fromIdx", 0):
            found.add("l2_to_addr" if A.is_to_addr(t) else "l2_transfer")
    return found


WHOLE = 10 ** 18    # an exit of exactly this amount with selector 176 takes the whole balance of exit_state's account f0 + 6


@functools.lru_cache(maxsize=None)
def exit_state(k=6):
    """special_state with account f0 + 6 holding exactly WHOLE + its fee at selector 176"""
    def edit(cols):
        cols[1][6] = C.to_bytes([WHOLE + B.compute_fee(WHOLE, 176)])[0]
    return A.with_planes(A.special_state(k), edit)


EDGES = ("first_exit_into_empty_tree", "second_key_meets_a_leaf", "keys_sharing_low_bits", "same_account_twice", "zero_amount_exit",
         "exit_whole_balance_with_fee", "transfer_in_then_exit_funded_by_it", "exit_then_transfer_same_sender", "force_exit_nullified_by_eth_addr",
         "force_exit_nullified_by_token", "force_exit_nullified_by_underflow", "force_exit_then_l2_exit_same_idx", "nullified_force_exit_then_l2_exit")


def edge_batches(sp):
    """the named edges on exit_state(6): {name: (l1_txs, l2_txs)}"""
    f0, leaf = sp.first_idx, sp.state
    a, b, c, w, far = f0 + 1, f0 + 3, f0 + 4, f0 + 6, f0 + 33
    assert all(leaf(x)["tokenID"] == 1 for x in (a, b, c, w, far))
    bal = lambda x: leaf(x)["balance"]   # noqa: E731
    part = lambda x, d=3: L1.float_floor(bal(x) // d)   # noqa: E731
    big = L1.float_floor(2 * bal(a) + 10)
    assert B.float2fix(B.fix2float(WHOLE)) == WHOLE and bal(w) == WHOLE + B.compute_fee(WHOLE, 176)
    return {
        "first_exit_into_empty_tree": ([], [x2(a, part(a), 100, nonce=0)]),
        "second_key_meets_a_leaf": ([], [x2(a, part(a), nonce=0), x2(b, part(b), 176, nonce=0)]),
        "keys_sharing_low_bits": ([], [x2(a, part(a), nonce=0), x2(far, part(far), nonce=0)]),
        "same_account_twice": ([], [x2(a, part(a), 1, nonce=0), C.tx(b, c, 5, nonce=0), x2(a, part(a, 4), 192, nonce=1)]),
        "zero_amount_exit": ([fx(sp, a, 0, load=5)], [x2(b, 0, 100, nonce=0)]),
        "exit_whole_balance_with_fee": ([], [x2(w, WHOLE, 176, nonce=0)]),
        "transfer_in_then_exit_funded_by_it": ([], [C.tx(b, a, part(b, 2), nonce=0), x2(a, L1.float_floor(bal(a) + part(b, 2) // 2), nonce=0)]),
        "exit_then_transfer_same_sender": ([], [x2(a, part(a), 100, nonce=0), C.tx(a, b, part(a, 4), 100, nonce=1)]),
        "force_exit_nullified_by_eth_addr": ([fx(sp, a, 1000, eth=leaf(a)["ethAddr"] ^ 2)], []),
        "force_exit_nullified_by_token": ([fx(sp, a, 1000, token=2)], []),
        "force_exit_nullified_by_underflow": ([fx(sp, a, big)], []),
        "force_exit_then_l2_exit_same_idx": ([fx(sp, a, part(a))], [x2(a, part(a, 5), 100, nonce=0)]),
        "nullified_force_exit_then_l2_exit": ([fx(sp, a, big)], [x2(a, part(a, 5), 100, nonce=0)]),
    }


# ---- tests/native/ledger_exit_check.cpp's input ------------------------------------------------------------------------------------------
def check_lines(groups):
    """groups: [(the sender's e0, [amounts])]: one exit key each, its operations in order. Expectations are plain Python: the exit leaf's
    e0 (tokenID | sign << 72, the nonce dropped), the four leaf-2 rows before every operation, the balance after it and whether that is
    still a leaf field (below 2^192)"""
    lines = []
    for e0_s, amounts in groups:
        e0 = (e0_s & 0xFFFFFFFF) | ((e0_s >> 72) & 1) << 72
        lines.append("g %x %x" % (e0_s, e0))
        bal = 0
        for amt in amounts:
            new = bal + amt
            lines.append("o %x %x %x %x %x %x %x" % (amt, e0 & 0xFFFFFFFF, 0, e0 >> 72, bal, new % (1 << 256), 1 if new < 1 << 192 else 0))
            bal = new
    for flags in range(4):
        lines.append("r %x %x" % (flags, 1 if flags == 1 else 0))
    return "\n".join(lines) + "\n"
