"""Shared by tests/test_ledger_addr.py (GPU) and tests/test_ledger_addr_cpu.py: receivers named by address or key (hz_ledger_apply_l2_addr,
DESIGN.md 8e). A plain Python model of the match rule and of the query table (csrc/ledger_resolve.h's hash, restated), states with
several tokens, "any"-address accounts and unique addresses, the batch drawer, the checker wrapper that hands BatchBuilder its auxToIdx,
and ledger_common's scheme model extended with reasons 9 - 11 and the zero-amount rows."""
import functools

import numpy as np

import device_state_common as D
import ledger_common as C
from circuits_amd import builder as B

ANY = (1 << 160) - 1
M32 = 0xFFFFFFFF


# ---- the match rule, brute force ------------------------------------------------------------------------------------------------------
def matches(leaf, token, to_eth, to_ay, to_sign):
    if leaf["tokenID"] != token:
        return False
    if to_eth != ANY:
        return leaf["ethAddr"] == to_eth
    return leaf["ethAddr"] == ANY and leaf["ay"] == to_ay and leaf["sign"] == to_sign


def brute_force(state, t):
    """the lowest index whose leaf (before the batch) holds t's signed destination and token, or 0"""
    for i in range(state.first_idx, state.first_idx + state.N):
        if matches(state.state(i), t.get("tokenID", 0), t.get("toEthAddr", 0), t.get("toBjjAy", 0), t.get("toBjjSign", 0)):
            return i
    return 0


# ---- the table, restated ---------------------------------------------------------------------------------------------------------------
def key_words(token, eth, ay, sign):
    """ResolveKey: [kind, token, eight 32-bit limbs of the address, or of ay under the "any" address]"""
    any_ = eth == ANY
    v = ay if any_ else eth
    return [(2 | (sign & 1)) if any_ else 1, token & M32] + [(v >> (32 * i)) & M32 for i in range(8)]


def hash_words(w):
    h = 0x811C9DC5
    for x in w:
        h = ((h ^ x) * 0x01000193) & M32
    return h ^ (h >> 15)


def slots_for(queries):
    s = 2
    while s < 2 * queries:
        s <<= 1
    return s


class Table:
    def __init__(self, slots):
        assert slots & (slots - 1) == 0
        self.slots, self.keys, self.longest = slots, [None] * slots, 0

    def insert(self, w):
        """the slot of w (entered when new); the longest probe chain is kept: 1 is a direct hit"""
        s = hash_words(w) & (self.slots - 1)
        for step in range(self.slots):
            if self.keys[s] is None or self.keys[s] == w:
                self.keys[s] = list(w)
                self.longest = max(self.longest, step + 1)
                return s
            s = (s + 1) & (self.slots - 1)
        return -1

    def probe(self, w):
        s = hash_words(w) & (self.slots - 1)
        for _ in range(self.slots):
            if self.keys[s] is None:
                return -1
            if self.keys[s] == w:
                return s
            s = (s + 1) & (self.slots - 1)
        return -1


def wants_lookup(t, skip_zero):
    return bool(t.get("fromIdx", 0)) and t.get("toIdx", 0) == 0 and not (skip_zero and not (t.get("amountF", 0) & ((1 << 35) - 1)))


def resolve_model(state, txs, skip_zero=False):
    """the device's scheme: distinct queries into the table, every account probes it, the lowest hit per slot -> (receivers, table)"""
    todo = [i for i, t in enumerate(txs) if wants_lookup(t, skip_zero)]
    out = [0] * len(txs)
    if not todo:
        return out, None
    table = Table(slots_for(len(todo)))
    slot = {i: table.insert(key_words(txs[i].get("tokenID", 0), txs[i].get("toEthAddr", 0), txs[i].get("toBjjAy", 0), txs[i].get("toBjjSign", 0))) for i in todo}
    result = [None] * table.slots
    for a in range(state.N):
        lf = state.state(state.first_idx + a)
        s = table.probe(key_words(lf["tokenID"], lf["ethAddr"], lf["ay"], lf["sign"]))
        if s >= 0 and (result[s] is None or a < result[s]):
            result[s] = a
    for i in todo:
        if result[slot[i]] is not None:
            out[i] = state.first_idx + result[slot[i]]
    return out, table


# ---- states -----------------------------------------------------------------------------------------------------------------------------
class PlaneState(B.DenseState):
    """a DenseState whose leaf fields are explicit planes (e0, balance, ay, ethAddr as [N, 32]): several tokens, "any"-address accounts,
    unique addresses. Keys (ay, sign) stay the base's, so its signers still sign."""

    def __init__(self, base, cols):
        levels, value = D.rebuild_levels(base.k, base.first_idx, cols)
        super().__init__(base.k, base.first_idx, base.seed, base.n_keys, base.key_idx, base.mant, base.expo, levels, value)
        self.cols = [np.array(c) for c in cols]

    def state(self, idx):
        j = idx - self.first_idx
        e0 = D.to_int(self.cols[0][j])
        return {"tokenID": e0 & M32, "nonce": (e0 >> 32) & ((1 << 40) - 1), "sign": (e0 >> 72) & 1, "balance": D.to_int(self.cols[1][j]),
                "ay": D.to_int(self.cols[2][j]), "ethAddr": D.to_int(self.cols[3][j])}

    def leaf_fields(self):
        return tuple(np.array(c) for c in self.cols)


def with_planes(base, edit):
    """base with edit(cols) applied to a copy of its planes"""
    cols = [np.array(c) for c in base.leaf_fields()]
    edit(cols)
    return PlaneState(base, cols)


def set_token(cols, j, token):
    cols[0][j, 0:4] = np.frombuffer(int(token).to_bytes(4, "little"), dtype=np.uint8)


def set_eth(cols, j, eth):
    cols[3][j] = D.to_bytes([eth])[0]


@functools.lru_cache(maxsize=None)
def mixed_state(k, seed=5):
    """about a quarter of the accounts hold token 2, an eighth the "any" address, an eighth an address of their own; the rest share the
    base's eight addresses, so the lowest-index rule decides almost every lookup"""
    base = C.base_state(k)
    rng = np.random.default_rng(seed)

    def edit(cols):
        for j in range(base.N):
            r = int(rng.integers(0, 8))
            if int(rng.integers(0, 4)) == 0:
                set_token(cols, j, 2)
            if r == 0:
                set_eth(cols, j, ANY)
            elif r == 1:
                set_eth(cols, j, int.from_bytes(rng.bytes(20), "little") | 1 << 159)
    return with_planes(base, edit)


@functools.lru_cache(maxsize=None)
def special_state(k=4):
    """accounts 2 and 9 share an address under tokens 1 and 2; 7 holds an address of its own; three accounts hold the "any" address:
    any_a = 5, any_b with another key, any_c above both with any_a's key (the lowest holder of a key wins)"""
    base = C.base_state(k)
    key = [int(x) for x in base.key_idx]
    free = [j for j in range(10, base.N)]
    b = next(j for j in free if key[j] != key[5])
    c = next(j for j in free if j > b and key[j] == key[5])

    def edit(cols):
        cols[3][9] = cols[3][2]
        set_token(cols, 9, 2)
        for j in (5, b, c):
            set_eth(cols, j, ANY)
        set_eth(cols, 7, 0xABCDEF << 130 | 77)
    st = with_planes(base, edit)
    st.any_a, st.any_b, st.any_c = base.first_idx + 5, base.first_idx + b, base.first_idx + c
    return st


# ---- batches ----------------------------------------------------------------------------------------------------------------------------
def to_addr(t, leaf):
    """t with its receiver named by the leaf's address, or by its key when the leaf holds the "any" address"""
    t = dict(t, toIdx=0, toEthAddr=leaf["ethAddr"])
    if leaf["ethAddr"] == ANY:
        t.update(toBjjAy=leaf["ay"], toBjjSign=leaf["sign"])
    return t


def draw_batch(state, m, seed, pool=None, n_tx=None, share=3):
    """ledger_common.draw_batch over a state of several tokens, with about one transfer in `share` naming its receiver by address or key
    (the account drawn is then only some holder of it: the lowest holder receives), zero amounts and a sender's own address among them"""
    rng = np.random.default_rng(seed)
    accounts = min(state.N, pool or state.N)
    off = int(rng.integers(0, state.N - accounts + 1))
    leaf = {i: state.state(i) for i in range(state.first_idx, state.first_idx + state.N)}
    by_token = {}
    for i in range(state.first_idx + off, state.first_idx + off + accounts):
        by_token.setdefault(leaf[i]["tokenID"], []).append(i)
    bal, nonce, txs = {}, {}, []
    for _ in range(m):
        f = state.first_idx + off + int(rng.integers(0, accounts))
        same = by_token[leaf[f]["tokenID"]]
        t = f if rng.integers(0, 16) == 0 else same[int(rng.integers(0, len(same)))]
        b = bal.get(f, leaf[f]["balance"])
        amount = 0 if rng.integers(0, 8) == 0 else B.float2fix(B.floor_fix2float(b // int(rng.integers(8, 40))))
        sel = C.SELECTORS[int(rng.integers(0, len(C.SELECTORS)))]
        x = C.tx(f, t, amount, sel, token=leaf[f]["tokenID"], nonce=nonce.get(f, 0))
        if rng.integers(0, share) == 0:
            x = to_addr(x, leaf[t])
            t = brute_force(state, x)
        txs.append(x)
        bal[f] = b - amount - B.compute_fee(amount, sel)
        nonce[f] = nonce.get(f, 0) + 1
        if amount:
            bal[t] = bal.get(t, leaf[t]["balance"]) + amount
    return txs + [{} for _ in range((n_tx or m) - m)]


def amount_of(t):
    return B.float2fix(t.get("amountF", 0))


def is_to_addr(t):
    return bool(t.get("fromIdx", 0)) and t.get("toIdx", 0) == 0


def aux_list(state, txs, aux=None):
    """auxToIdx as the ledger reports it: the receiver of a to-address transfer with an amount (supplied, or the lowest holder), else 0"""
    return [(aux[i] if aux is not None else brute_force(state, t)) if is_to_addr(t) and amount_of(t) else 0 for i, t in enumerate(txs)]


def builder_batch(state, txs, plan_tokens, fee_idxs, n_levels, db=None, max_l1=0, aux=None):
    """the checker: BatchBuilder with auxToIdx given explicitly in every to-address transaction (its own lookup walks only the leaves a
    batch has touched and never finds an account of the base) -> (db, built BatchBuilder)"""
    ax = aux_list(state, txs, aux)
    with_aux = [dict(t, auxToIdx=ax[i]) if is_to_addr(t) else t for i, t in enumerate(txs)]
    return C.builder_batch(state, with_aux, plan_tokens, fee_idxs, n_levels, db=db, max_l1=max_l1)


def zero_amount_rows(txs):
    """{row: {leaf-2 signal: value}} of the zero-amount to-address transfers: what the circuit compares with the signed destination"""
    out = {}
    for i, t in enumerate(txs):
        if is_to_addr(t) and not amount_of(t):
            out[i] = {"ethAddr2": t.get("toEthAddr", 0)}
            if t.get("toEthAddr", 0) == ANY:
                out[i].update(ay2=t.get("toBjjAy", 0), sign2=t.get("toBjjSign", 0))
    return out


def expected_arrays(bb, txs):
    """ledger_common.expected_arrays plus auxToIdx, with the zero-amount rows as specified (the builder leaves ethAddr2 = 0 there and
    the circuit rejects that: for these rows the oracle is the judge)"""
    exp = C.expected_arrays(bb)
    exp["auxToIdx"] = C.to_bytes(bb.get_input()["auxToIdx"])
    for i, row in zero_amount_rows(txs).items():
        for name, v in row.items():
            exp[name][i] = C.to_bytes([v])[0]
    return exp


def touched(state, txs, fee_idxs, aux=None):
    ax = aux_list(state, txs, aux)
    acc = {t["fromIdx"] for t in txs if t.get("fromIdx")} | {t["toIdx"] for t in txs if t.get("fromIdx") and t["toIdx"]} | {a for a in ax if a}
    return sorted(acc | {i for i in fee_idxs if i})


# ---- the scheme with reasons 9 - 11 ---------------------------------------------------------------------------------------------------
def scheme_model(state, txs, plan_tokens, fee_idxs, aux=None):
    """ledger_common.scheme_model on the effective receivers. Reason 9 comes first (the lowest unresolved transaction, whatever else is
    wrong); 10 and 11 rank with 1 - 6 by (index, reason). -> ("refused", unit, reason) or ("ok", fields, acc_fee_after, final, auxToIdx)"""
    if aux is None:
        found, _ = resolve_model(state, txs, skip_zero=True)
        for i, t in enumerate(txs):
            if wants_lookup(t, True) and not found[i]:
                return "refused", i, 9
    else:
        found = list(aux)
    eff, fails = [], []
    for i, t in enumerate(txs):
        if is_to_addr(t) and amount_of(t):
            leaf = state.state(found[i])
            if leaf["ethAddr"] != t.get("toEthAddr", 0):
                fails.append((i, 10))
            if t.get("toEthAddr", 0) == ANY and (leaf["ay"], leaf["sign"]) != (t.get("toBjjAy", 0), t.get("toBjjSign", 0)):
                fails.append((i, 11))
            t = dict(t, toIdx=found[i])
        eff.append(t)
    res = C.scheme_model(state.state, eff, plan_tokens, fee_idxs)
    if res[0] == "refused":
        fails.append((res[1], res[2]))
    if fails:
        return ("refused",) + min(fails)
    for i, row in zero_amount_rows(txs).items():
        for name, v in row.items():
            res[1][name][i] = v
    return res + ([found[i] if is_to_addr(t) and amount_of(t) else 0 for i, t in enumerate(txs)],)


# ---- tests/native/ledger_addr_check.cpp's input ---------------------------------------------------------------------------------------
def check_lines(tables, keys):
    """tables: [(slots, [key words to insert], [key words to probe])]; keys: [(token, eth, ay, sign)] whose key words the program must
    form itself. Expectations come from the model."""
    lines = []

    def fmt(w):
        return " ".join("%x" % x for x in w)
    for token, eth, ay, sign in keys:
        lines.append("k %x %x %x %x %s %x" % (token, eth, ay, sign, fmt(key_words(token, eth, ay, sign)), hash_words(key_words(token, eth, ay, sign))))
    for slots, ins, probes in tables:
        t = Table(slots)
        lines.append("t %x" % slots)
        for w in ins:
            lines.append("i %s %x" % (fmt(w), t.insert(w) & M32))
        for w in probes:
            lines.append("p %s %x" % (fmt(w), t.probe(w) & M32))
    return "\n".join(lines) + "\n"
