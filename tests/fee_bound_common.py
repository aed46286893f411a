"""Shared by tests/test_fee_bound.py (GPU) and tests/test_fee_bound_cpu.py: ComputeFee's bound of 128 bits (reference
src/compute-fee.circom:86-93) as a plain-integer model, and the tables of amounts on either side of it that every kernel which
computes a fee is put to. Python integers only: nothing here goes through the field arithmetic of the product or of the oracle. The
fee table is the project's data file (circuits_amd/fee_table.json through builder.fee_table).

  verdict(amount, sel, apply_fee)   (ACCEPTED, feeOut), or (constraint, None) for the first violated constraint in the template's order
  float40_table()                   per selector the largest float40 amount whose fee stays below 2^128 and the smallest whose fee does
                                    not (selectors 31 .. 255), or the largest float40 of all, accepted (selectors 0 .. 30)
  exact_table()                     per selector the field elements ceil(bound / T) - 1 and ceil(bound / T), bound = 2^188 below selector
                                    192 and 2^128 from there on; pairs around a product of 2^253 for a few selectors of each branch"""
import functools

from circuits_amd import builder as B

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MANT = (1 << 35) - 1
ACCEPTED, BITS, OVF_SHIFTED, OVF_NOTSHIFTED = "accepted", "lcIn === feeOutNotShifted", "applyShift*lcOverflowShifted === 0", "(1-applyShift)*lcOverflowNotShifted === 0"
FIRST_REACHING = 31          # selectors 0 .. 30 never reach the bound with a float40 amount
REASON = 16                  # HZ_LEDGER_FEE_OVERFLOW


def shifted(sel):
    """applyShift = 1 - bit 6 * bit 7 of the selector: the table holds 2^60 x the factor below 192"""
    return not ((sel >> 6) & 1 and (sel >> 7) & 1)


def verdict(amount, sel, apply_fee=1):
    """ComputeFee on integers, for applyFee a bit (what RollupTx feeds it). The mux's selectors are the selector's bits times applyFee:
    with applyFee = 0 it gives table[0] = 0, so the factor is 0 whatever the amount. The product is a field element; its 253 stored
    bits must sum up to it (a product of 2^253 or more fails there first), then no bit at or above 60 + 128 (shifted) or 128 (not
    shifted) may be set. The shift is decided by the selector's own bits, with or without the fee"""
    assert apply_fee in (0, 1)
    product = (B.fee_table()[sel] if apply_fee else B.fee_table()[0]) * (amount % P) % P
    if product >> 253:
        return BITS, None
    if shifted(sel):
        return (OVF_SHIFTED, None) if product >> 188 else (ACCEPTED, product >> 60)
    return (OVF_NOTSHIFTED, None) if product >> 128 else (ACCEPTED, product)


def f40(mant, expo):
    return mant | (expo << 35)


def amount_of(f):
    return (f & MANT) * 10 ** (f >> 35)


def fee_of(f, sel):
    """the fee as an integer of any size: what the ledger computes before it judges"""
    t = B.fee_table()[sel] * amount_of(f)
    return t >> 60 if sel < 192 else t


def _search(sel, expo):
    """the largest mantissa of this exponent whose amount is accepted (0: none but the zero amount), by bisection on the model: the
    product grows with the mantissa"""
    lo, hi = 0, MANT
    if verdict(MANT * 10 ** expo, sel)[0] == ACCEPTED:
        return MANT
    while hi - lo > 1:   # lo accepted, hi rejected
        mid = (lo + hi) // 2
        if verdict(mid * 10 ** expo, sel)[0] == ACCEPTED:
            lo = mid
        else:
            hi = mid
    return lo


@functools.lru_cache(maxsize=None)
def float40_table():
    """[(sel, below, above)] for all 256 selectors, float40 words: `below` the accepted amount of the largest value, `above` the rejected
    amount of the smallest value (None where no float40 amount is rejected). Searched over every exponent and, by bisection, mantissa"""
    rows = []
    for sel in range(256):
        below = above = None
        for expo in range(32):
            m = _search(sel, expo)
            if m and (below is None or amount_of(f40(m, expo)) > amount_of(below)):
                below = f40(m, expo)
            if m < MANT and (above is None or amount_of(f40(m + 1, expo)) < amount_of(above)):
                above = f40(m + 1, expo)
        rows.append((sel, below, above))
    return rows


def reaching():
    """the rows of the selectors that reach the bound"""
    return [r for r in float40_table() if r[2] is not None]


def ceil_div(a, b):
    return -(-a // b)


PAIR_253 = (1, 31, 100, 191, 192, 193, 224, 255)   # selectors that also get the pair around a product of 2^253


@functools.lru_cache(maxsize=None)
def exact_table():
    """[(sel, amount, expected verdict name)]: any field element may be the amount of a standalone main"""
    rows = []
    for sel in range(1, 256):
        t = B.fee_table()[sel]
        edge = ceil_div(1 << (188 if sel < 192 else 128), t)
        rows += [(sel, edge - 1, ACCEPTED), (sel, edge, OVF_SHIFTED if sel < 192 else OVF_NOTSHIFTED)]
        if sel in PAIR_253:
            big = ceil_div(1 << 253, t)
            assert big * t < P
            rows += [(sel, big - 1, OVF_SHIFTED if sel < 192 else OVF_NOTSHIFTED), (sel, big, BITS)]
    return rows


def compute_fee_cases():
    """every instance of the ComputeFee launch: {"feeSel", "amount", "applyFee"} with the model's verdict beside it, ordered so that
    accepted and rejected lanes and the two branches alternate within every wavefront. Both tables, and the overflowing amounts with
    applyFee = 0 (accepted)"""
    acc, rej = [], []
    for sel, below, above in float40_table():
        acc.append((sel, amount_of(below), 1))
        if above is not None:
            rej.append((sel, amount_of(above), 1))
            acc.append((sel, amount_of(above), 0))
    for sel, amount, name in exact_table():
        (acc if name == ACCEPTED else rej).append((sel, amount, 1))
        if name == BITS:
            acc.append((sel, amount, 0))

    def spread(a, b):   # both lists run out together: element k of n sits at k / n of the way
        keyed = [((k + 0.5) / len(a), 0, r) for k, r in enumerate(a)] + [((k + 0.5) / len(b), 1, r) for k, r in enumerate(b)]
        return [r for _, _, r in sorted(keyed, key=lambda x: x[:2])]

    def weave(rows):   # the two branches
        return spread([r for r in rows if shifted(r[0])], [r for r in rows if not shifted(r[0])])
    out = spread(weave(acc), weave(rej))
    return [({"feeSel": s, "amount": a, "applyFee": f}, verdict(a, s, f)) for s, a, f in out]


def constraint_ids():
    """{constraint text: id} of the three ComputeFee constraints, from the oracle's names (include/hz_layout.h's list)"""
    import fuzz_common as FZ
    out, cid = {}, 0
    while len(out) < 3 and cid < 4096:
        name = FZ.constraint_name(cid)
        for text in (BITS, OVF_SHIFTED, OVF_NOTSHIFTED):
            if name.endswith("computeFee: " + text):
                out[text] = cid
        cid += 1
    assert len(out) == 3, out
    return out


# ---- ledger rows ---------------------------------------------------------------------------------------------------------------------------
SPAN = (31, 63, 100, 191, 192, 200, 224, 255)   # the selectors of the batches the circuit itself judges: both branches, all four corners


def pairs(selectors=SPAN):
    t = float40_table()
    return [t[s] for s in selectors]
