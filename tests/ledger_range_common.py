"""Shared by tests/test_ledger_ranges.py (GPU) and tests/test_ledger_ranges_cpu.py: states and batches at the edges of the ledger's value
ranges -- balances up to 2^192 - 1, float40 amounts with all 32 exponents and bits in limb 4, all 256 fee selectors, nonces that carry
into and fill the high byte beside the sign bit, token ids with bit 31 set, 64 fee slots -- and tests/native/u256_check.cpp's input.
Every batch carries explicit nonces: the builder's nonce pre-pass assumes 0 for an account it has not touched yet."""
import functools

import numpy as np

import fee_bound_common as FB
import ledger_addr_common as A
import ledger_common as C
import ledger_l1_common as L1
import ledger_sig_common as S
from circuits_amd import builder as B

MANT = (1 << 35) - 1
MANTISSAS = (1, MANT, (1 << 32) - 1, 1 << 32, 0x555555555)
TOP = MANT | (31 << 35)                      # the largest float40
V = B.float2fix(TOP)                         # (2^35 - 1) x 10^31, 138 bits: limb 4 is not zero
NONCE_MAX = (1 << 40) - 1
TOK_MAX, TOK_B31 = (1 << 32) - 1, 1 << 31
RICH = 1 << 191
assert V >> 128 and V < 1 << 138


def f40(mant, expo):
    return mant | (expo << 35)


def txf(frm, to, amount_f, fee=0, token=1, nonce=0):
    """ledger_common.tx with the float40 given as it is"""
    return {"fromIdx": frm, "toIdx": to, "amountF": amount_f, "tokenID": token, "userFee": fee, "onChain": 0, "nonce": nonce}


def set_e0(cols, j, token, nonce, sign):
    cols[0][j] = C.to_bytes([token + (nonce << 32) + (sign << 72)])[0]


def set_balance(cols, j, balance):
    cols[1][j] = C.to_bytes([balance])[0]


# ---- the wide state ----------------------------------------------------------------------------------------------------------------------
EXACT_F, EXACT_SEL = TOP, 30                                       # the transfer that empties its sender exactly: the highest selector that the
assert FB.float40_table()[30][2] is None and FB.float40_table()[31][2] is not None   # largest amount can carry (a fee of 2^128 or more is reason 16)
FEE_255, FEE_191 = FB.float40_table()[255][1], FB.float40_table()[191][1]   # the largest amounts those two selectors can carry
EXACT = V + B.compute_fee(V, EXACT_SEL)


@functools.lru_cache(maxsize=None)
def wide_state():
    """k = 6. Offsets from first_idx: 1-4 hold 2^191; 5 holds 2^192 - 8; 6 holds exactly amount + fee of the emptying transfer and 7 one
    unit less; 8 and 9 are plain accounts of a known balance; 31, 32 hold token 2^32 - 1 and 33, 34 token 2^31; 40 takes the fees of
    token 1; 41-47 are the L1 cases'; 48-63 receive. The accounts of the nonces 2^32 - 2, 2^40 - 3 and 2^40 - 1 (two of these) are picked
    from 10-30 by the sign of their key, so that both signs sit beside a full high byte"""
    base = C.base_state(6)
    sign = [base.state(base.first_idx + j)["sign"] for j in range(base.N)]
    free = list(range(10, 31))

    def pick(sg):
        j = next(j for j in free if sign[j] == sg)
        free.remove(j)
        return j
    role = {"n32": pick(1), "n40m3": pick(0), "last1": pick(1), "last0": pick(0)}
    nonce = {"n32": (1 << 32) - 2, "n40m3": NONCE_MAX - 2, "last1": NONCE_MAX, "last0": NONCE_MAX}

    def edit(cols):
        for j in (1, 2, 3, 4):
            set_balance(cols, j, RICH)
        set_balance(cols, 5, (1 << 192) - 8)
        set_balance(cols, 6, EXACT)
        set_balance(cols, 7, EXACT - 1)
        for j in (8, 9, 31, 32, 33, 34):
            set_balance(cols, j, 10 ** 30)
        for name, j in role.items():
            set_e0(cols, j, 1, nonce[name], sign[j])
            set_balance(cols, j, 10 ** 30)
        for j, tok in ((31, TOK_MAX), (32, TOK_MAX), (33, TOK_B31), (34, TOK_B31)):
            set_e0(cols, j, tok, 0, sign[j])
        set_balance(cols, 41, 5)
        set_balance(cols, 43, V - (1 << 128))
        set_balance(cols, 45, (1 << 192) - 1 - V)
        set_balance(cols, 46, (1 << 192) - V)
    st = A.with_planes(base, edit)
    st.role = {name: base.first_idx + j for name, j in role.items()}
    assert {st.state(a)["sign"] for a in st.role.values()} == {0, 1}
    return st


WIDE_FEE = 40   # offset of token 1's fee account


def all_selectors_rows():
    """[(selector, float40, overflowing float40 or None)]: row i has selector i, mantissa MANTISSAS[i % 5] and exponent i % 32 lowered until amount + fee is below
    1/256 of a 2^191 balance. The circuit
    rejects a fee of 2^128 or more (src/compute-fee.circom:89-91) and so does the ledger (reason 16): where that mantissa gives such a fee
    (32 rows, fees of 129 to 183 bits) the row takes the largest mantissa of its exponent whose fee stays below 2^128 -- 0, a zero amount,
    where a mantissa of 1 is already above it -- and the original goes to the refusal tests"""
    rows = []
    for i in range(256):
        mant, expo = MANTISSAS[i % 5], i % 32
        while B.float2fix(f40(mant, expo)) + B.compute_fee(B.float2fix(f40(mant, expo)), i) >= RICH >> 8:   # below 1/256 of a 2^191 balance
            expo -= 1
        f = f40(mant, expo)
        if B.compute_fee(B.float2fix(f), i) >> 128:
            rows.append((i, f40(FB._search(i, expo), expo), f))
        else:
            rows.append((i, f, None))
    return rows


def all_selectors(st):
    """256 transfers, transaction i with selector i, all_selectors_rows' amounts (every exponent, every fee below 2^128) ->
    (txs, plan, idxs)"""
    f0, txs, nonce = st.first_idx, [], {}
    for i, f, _ in all_selectors_rows():
        assert B.float2fix(f) + B.compute_fee(B.float2fix(f), i) < RICH >> 8
        frm = f0 + 1 + i % 4
        txs.append(txf(frm, f0 + 48 + i % 16, f, i, nonce=nonce.get(frm, 0)))
        nonce[frm] = nonce.get(frm, 0) + 1
    return txs, [1], [f0 + WIDE_FEE]


def overflowing_selectors(st):
    """the 32 rows all_selectors no longer holds, as single transfers from an account that could pay them: [(txs, plan, idxs)]"""
    f0 = st.first_idx
    return [([txf(f0 + 1 + i % 4, f0 + 48 + i % 16, over, i, nonce=0)], [1], [f0 + WIDE_FEE]) for i, _, over in all_selectors_rows() if over is not None]


def nonce_carry(st):
    """three sends across 2^32, two up to 2^40 - 1, one transfer of token 2^32 - 1 whose fee goes to a slot of that token"""
    f0, r = st.first_idx, st.role
    txs = [txf(r["n32"], f0 + 48 + i, f40(1000 + i, 3), 176, nonce=(1 << 32) - 2 + i) for i in range(3)]
    txs += [txf(r["n40m3"], f0 + 52 + i, f40(77 + i, 9), 100, nonce=NONCE_MAX - 2 + i) for i in range(2)]
    txs.append(txf(f0 + 31, f0 + 32, f40(MANT, 15), 191, token=TOK_MAX, nonce=0))
    return txs, [1, TOK_MAX], [f0 + WIDE_FEE, f0 + 32]


def to_the_brim(st):
    """-> (valid batch, [(refused batch, index, reason)]), each batch (txs, plan, idxs)"""
    f0 = st.first_idx
    plan, idxs = [1, TOK_B31], [f0 + WIDE_FEE, f0 + 33]
    into = lambda amount: txf(f0 + 8, f0 + 5, f40(amount, 0), 0, nonce=0)   # noqa: E731
    empty = lambda frm: txf(frm, f0 + 9, EXACT_F, EXACT_SEL, nonce=0)       # noqa: E731
    b31 = txf(f0 + 33, f0 + 34, f40(MANT, 12), 176, token=TOK_B31, nonce=0)   # the sender is its token's fee account
    valid = ([into(7), empty(f0 + 6), b31], plan, idxs)
    refused = [(([b31, into(8), empty(f0 + 6)], plan, idxs), 1, 5), (([into(7), b31, empty(f0 + 7)], plan, idxs), 2, 3)]
    return valid, refused


def nonce_refusals(st):
    """[((txs, plan, idxs), index, reason)]: reason 12 alone, on a key of either sign; reason 2 beside it reports 2; the third send of the
    2^40 - 3 account, which the scan reaches at 2^40 - 1; a transaction nonce of 2^40 + the resident one is reason 2"""
    f0, r = st.first_idx, st.role
    ok = txf(f0 + 8, f0 + 9, f40(5, 0), 176, nonce=0)
    one = ([1], [f0 + WIDE_FEE])
    carry = nonce_carry(st)[0][3:5]
    return [(([ok, txf(r["last1"], f0 + 9, f40(5, 0), 0, nonce=NONCE_MAX)],) + one, 1, 12),
            (([txf(r["last0"], f0 + 9, f40(5, 0), 0, nonce=NONCE_MAX), txf(f0 + 8, f0 + 9, f40(5, 0), 0, nonce=3)],) + one, 0, 12),
            (([ok, txf(r["last1"], f0 + 9, f40(5, 0), 0, nonce=NONCE_MAX - 1)],) + one, 1, 2),
            (([ok] + carry + [txf(r["n40m3"], f0 + 9, f40(5, 0), 0, nonce=NONCE_MAX)],) + one, 3, 12),
            (([ok, txf(r["n32"], f0 + 9, f40(5, 0), 0, nonce=(1 << 40) + (1 << 32) - 2)],) + one, 1, 2)]


# ---- 64 fee slots ------------------------------------------------------------------------------------------------------------------------
TOKENS_66 = tuple([0] + list(range(1, 60)) + [TOK_B31, TOK_B31 + 5, 0x80000001, 0xDEADBEEF, TOK_MAX - 1, TOK_MAX])
ABSENT = (0, 7)   # the two tokens no slot of the plan holds
assert len(set(TOKENS_66)) == 66


@functools.lru_cache(maxsize=None)
def slots_state():
    """k = 8: account j holds token TOKENS_66[j % 66], and 10^24 more than the base gives it (every fee is then above zero)"""
    base = C.base_state(8)

    def edit(cols):
        for j in range(base.N):
            A.set_token(cols, j, TOKENS_66[j % 66])
            set_balance(cols, j, C.to_int(cols[1][j]) + 10 ** 24)
    return A.with_planes(base, edit)


def slots_plan(st):
    """64 of the 66 tokens in a shuffled order; the fee account of a slot is the second holder of its token; about one slot in nine has none"""
    order = np.random.default_rng(64).permutation([t for t in TOKENS_66 if t not in ABSENT]).tolist()
    idxs = [0 if s % 9 == 4 else st.first_idx + TOKENS_66.index(t) + 66 for s, t in enumerate(order)]
    return order, idxs


def fee_slots_64(st, m, share=0):
    """m transfers whose tokens walk over all 66; the sender is the first holder of the token, every fifth time the token's fee account;
    the receiver the third holder. share: one receiver in `share` is named by address or key, and is then the lowest holder of it"""
    f0, (plan, idxs) = st.first_idx, slots_plan(st)
    rng = np.random.default_rng(6400 + m)
    leaf = {i: st.state(i) for i in range(f0, f0 + st.N)}
    bal, nonce, txs = {}, {}, []
    for i in range(m):
        ti = (7 * i + 3) % 66
        frm = f0 + ti + (66 if i % 5 == 2 else 0)
        to = f0 + ti + 132
        b = bal.get(frm, leaf[frm]["balance"])
        amount_f = B.floor_fix2float(b // int(rng.integers(8, 40)))
        sel = C.SELECTORS[1 + i % (len(C.SELECTORS) - 1)]   # not selector 0: every transfer pays
        x = txf(frm, to, amount_f, sel, token=TOKENS_66[ti], nonce=nonce.get(frm, 0))
        if share and i % share == 1:
            x = A.to_addr(x, leaf[to])
            to = A.brute_force(st, x)
        txs.append(x)
        amount = B.float2fix(amount_f)
        bal[frm] = b - amount - B.compute_fee(amount, sel)
        nonce[frm] = nonce.get(frm, 0) + 1
        if amount:
            bal[to] = bal.get(to, leaf[to]["balance"]) + amount
    return txs, plan, idxs


# ---- L1 amounts with bits in limb 4 --------------------------------------------------------------------------------------------------------
def top_l1(st, frm, to, amount=False, load=False):
    return dict(L1.own(st, frm, to), amountF=TOP if amount else 0, loadAmountF=TOP if load else 0)


def l1_high_limbs(st):
    """-> ((l1_txs, l2_txs, plan, idxs), [((l1_txs, l2_txs, plan, idxs), row, reason)]). Offsets: 41 holds 5 and is funded by its load alone;
    43 holds V - 2^128, which agrees with V in the four low limbs: its transfer of V underflows by limb 4 alone; 45 holds 2^192 - 1 - V
    and 46 holds 2^192 - V"""
    f0 = st.first_idx
    plan, idxs = [1], [f0 + WIDE_FEE]
    l1_txs = [top_l1(st, f0 + 41, f0 + 42, amount=True, load=True), top_l1(st, f0 + 43, f0 + 44, amount=True), top_l1(st, f0 + 1, f0 + 47, amount=True, load=True),
              top_l1(st, f0 + 45, 0, load=True), top_l1(st, f0 + 41, 0, load=True)]
    spend = B.floor_fix2float(st.state(f0 + 42)["balance"] + V // 2)   # more than 42 held before the run
    l2_txs = [txf(f0 + 42, f0 + 9, spend, EXACT_SEL, nonce=0), txf(f0 + 1, f0 + 48, TOP, EXACT_SEL, nonce=0)]
    counted = B.floor_fix2float(st.state(f0 + 44)["balance"] + V // 2)
    refused = [(([top_l1(st, f0 + 43, f0 + 44, amount=True)], [txf(f0 + 8, f0 + 9, f40(5, 0), 0, nonce=0), txf(f0 + 44, f0 + 9, counted, 0, nonce=0)], plan, idxs), 2, 3),
               (([top_l1(st, f0 + 41, 0, load=True), top_l1(st, f0 + 46, 0, load=True)], [], plan, idxs), 1, 5)]
    return (l1_txs, l2_txs, plan, idxs), refused


# ---- signed transfers whose fields are at their maxima together ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def signed_state():
    """k = 6: offsets 2-5 send (token 2^32 - 1, nonce 2^40 - 2, 2^191), 6-9 hold that token; st.any (one of 10-40, a key of sign 1) holds it
    under the "any" address"""
    base = C.base_state(6)
    sign = [base.state(base.first_idx + j)["sign"] for j in range(base.N)]
    any_j = next(j for j in range(10, 41) if sign[j] == 1)

    def edit(cols):
        for j in (2, 3, 4, 5):
            set_e0(cols, j, TOK_MAX, NONCE_MAX - 1, sign[j])
            set_balance(cols, j, RICH)
        for j in (6, 7, 8, 9, any_j):
            set_e0(cols, j, TOK_MAX, 0, sign[j])
        A.set_eth(cols, any_j, A.ANY)
    st = A.with_planes(base, edit)
    st.any = base.first_idx + any_j
    return st


def signed_extremes(st, by_addr=False):
    """four signed transfers: nonce 2^40 - 2, token 2^32 - 1, maxNumBatch 2^32 - 1 in all; userFee 255 on amount 0 (exponent 31, mantissa
    0), on the largest amount selector 255 can carry, the largest at selector 191, and one to the "any" address with a key of sign 1
    (by_addr: with toIdx = 0 and that amount of selector 255)"""
    f0, leaf = st.first_idx, st.state(st.any)
    assert leaf["sign"] == 1 and leaf["ethAddr"] == A.ANY
    rows = [(f0 + 6, f40(0, 31), 255), (f0 + 7, FEE_255, 255), (f0 + 8, FEE_191, 191), (st.any, f40(0, 31) if not by_addr else FEE_255, 255)]
    txs = []
    for i, (to, amount_f, sel) in enumerate(rows):
        t = dict(txf(f0 + 2 + i, to, amount_f, sel, token=TOK_MAX, nonce=NONCE_MAX - 1), maxNumBatch=(1 << 32) - 1)
        if i == 3:
            t.update(toEthAddr=A.ANY, toBjjAy=leaf["ay"], toBjjSign=1, toIdx=0 if by_addr else to)
        txs.append(S.sign(st, t))
    return txs, [TOK_MAX], [f0 + 9]


# ---- tests/native/u256_check.cpp's input -----------------------------------------------------------------------------------------------------
M256 = (1 << 256) - 1
SIG_SHIFTS = ((0, 32), (32, 16), (48, 48), (96, 48), (144, 32), (176, 40), (216, 8), (224, 1), (136, 32), (168, 40), (208, 8), (160, 40), (200, 32))


def check_lines():
    """one record per line, every field in hex, the expectation last (Python integers)"""
    lines = []
    amounts = [f40(m, e) for e in range(32) for m in MANTISSAS]
    for f in amounts:
        lines.append("f %x %x" % (f, B.float2fix(f)))
    for sel in range(256):
        for f in amounts:
            lines.append("g %x %x %x" % (f, sel, B.compute_fee(B.float2fix(f), sel)))
    for sel, below, above in FB.float40_table():   # the bound of 2^128 from both sides, for every selector
        lines += ["v %x %x %x" % (f, sel, FB.fee_of(f, sel) >> 128 != 0) for f in (below, above) if f is not None]
    for i in range(1, 8):   # a carry and a borrow across every limb boundary
        lo, one = (1 << 32 * i) - 1, 1
        lines.append("a %x %x %x" % (lo, one, lo + one))
        lines.append("a %x %x %x" % (M256 >> 32 * (8 - i), M256 >> 32 * (8 - i), (2 * (M256 >> 32 * (8 - i))) & M256))
        lines.append("n %x %x" % (1 << 32 * i, (-(1 << 32 * i)) & M256))
        lines.append("a %x %x %x" % (1 << 32 * i, M256, (1 << 32 * i) - 1))   # x + (-1): the borrow runs through i limbs
    lines += ["a %x %x %x" % (M256, 1, 0), "n 0 0", "n 1 %x" % M256, "n %x 1" % M256, "n %x %x" % (V, (-V) & M256)]
    pattern = sum((0x9ABCDEF1 + 0x11111111 * i & 0xFFFFFFFF) << 32 * i for i in range(8))
    for x in [pattern, M256, 1 << 255, (1 << 60) - 1, 1 << 60] + [0xF0000001 << 32 * i for i in range(8)]:
        x &= M256
        lines.append("s %x %x" % (x, x >> 60))
    for i in range(8):      # pairs that differ in one limb only
        a = pattern & ~(0xFFFFFFFF << 32 * i) | (0x1234 << 32 * i)
        b = a + (1 << 32 * i)
        lines += ["l %x %x 1" % (a, b), "l %x %x 0" % (b, a), "l %x %x 0" % (a, a)]
    for sh, bits in SIG_SHIFTS:   # every shift ledger_sig.h uses, the field all ones, on zero and beside set neighbours
        v = (1 << bits) - 1
        for r in (0, pattern & ~(v << sh) & M256):
            lines.append("o %x %x %x %x" % (r, v, sh, (r | v << sh) & M256))
    return "\n".join(lines) + "\n"
