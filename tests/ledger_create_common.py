"""Shared by tests/test_ledger_create.py (GPU) and tests/test_ledger_create_cpu.py: L1 rows that create accounts on a growing ledger
(hz_ledger_apply_batch_creates). States of any number of consecutive accounts with the builder's database over them; a plain
Python model of the scheme -- the running index with its argument errors, the key decode, the static slots of the new accounts, then
ledger_exit_common's model over rows in which a create is a deposit on auxFromIdx, and the tree's plan for the inserts --; the lookup
over live plus created accounts; the checker's results lifted into the call's output layout; the named batches, a seeded drawer and
tests/native/ledger_create_check.cpp's input."""
import numpy as np

import ledger_addr_common as A
import ledger_common as C
import ledger_exit_common as X
import ledger_l1_common as L1
from circuits_amd import builder as B

P = B.P
EXIT = B.EXIT_IDX
ANY = (1 << 160) - 1
CREATE_ARRAYS = ("aux_from_idx", "is_old0_1", "old_key1", "old_value1", "out_idx_after", "new_last_idx")
MAX_L1 = 512


def account(n):
    """the n-th key pair new accounts are made of"""
    return B.Account(0x43524541 + n)


def compressed(acct):
    return acct.ay | acct.sign << 255


def create(key, token=1, eth=0, load=0, amount=0, to=0):
    """an L1 row that creates an account: key is fromBjjCompressed as an integer"""
    return {"onChain": 1, "fromIdx": 0, "toIdx": to, "amountF": B.fix2float(amount), "loadAmountF": B.fix2float(load), "tokenID": token, "fromEthAddr": eth,
            "fromBjjCompressed": key}


def create_for(acct, token=1, load=0, amount=0, to=0):
    return create(compressed(acct), token, acct.eth_addr, load, amount, to)


# ---- states ------------------------------------------------------------------------------------------------------------------------------
class Accounts:
    """n consecutive accounts from first_idx as leaf dictionaries: what a growing ledger is loaded with and the builder's database starts from"""

    def __init__(self, leaves, first_idx=256, dense=None):
        self.leaves, self.first_idx, self.dense = list(leaves), first_idx, dense
        self.n = len(self.leaves)

    @staticmethod
    def of(dense):
        return Accounts([dense.state(dense.first_idx + j) for j in range(dense.N)], dense.first_idx, dense)

    def state(self, idx):
        return self.leaves[idx - self.first_idx]

    def cols(self):
        rows = [B.leaf_fields(leaf) for leaf in self.leaves]
        return [C.to_bytes([r[f] for r in rows]) if rows else np.zeros((0, 32), dtype=np.uint8) for f in range(4)]

    def db(self):
        """the builder's database over these accounts, host hashing"""
        if self.dense is not None:
            return B.RollupDB(chain_id=1, base=self.dense)
        db = B.RollupDB(chain_id=1, first_idx=self.first_idx)
        for j, leaf in enumerate(self.leaves):
            db.state.insert(self.first_idx + j, B.hash_state(leaf))
            db.leaves[self.first_idx + j] = dict(leaf)
            db.last_idx = self.first_idx + j
        return db

    def to_ledger(self, lib, capacity, n_sib_max=17):
        lg = lib.ledger_growing(capacity, first_idx=self.first_idx, n_sib_max=n_sib_max)
        lg.load_accounts(*self.cols())
        return lg


def few_accounts(n, seed=7):
    """n accounts on the keys account(100 ..), token 1 (every third: token 2), a balance of a float40"""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(n):
        a = account(100 + j)
        out.append({"tokenID": 2 if j % 3 == 2 else 1, "nonce": 0, "sign": a.sign, "balance": int(rng.integers(1, 1 << 30)) * 10 ** 9, "ay": a.ay, "ethAddr": a.eth_addr})
    return Accounts(out)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def decode_key(key):
    """(ay, sign) of fromBjjCompressed: bits 0 .. 253 reduced once modulo r, bit 255; bit 254 is not read"""
    ay = key & ((1 << 254) - 1)
    return (ay - P if ay >= P else ay), (key >> 255) & 1


def new_leaf(t):
    ay, sign = decode_key(t.get("fromBjjCompressed", 0))
    return {"tokenID": t.get("tokenID", 0), "nonce": 0, "sign": sign, "balance": 0, "ay": ay, "ethAddr": t.get("fromEthAddr", 0)}


class Refused(Exception):
    """an argument error of the model: its text is a part of the library's message"""


def running_index(first_idx, size, capacity, l1_txs, growing=True, have_keys=True):
    """auxFromIdx (0: the row creates nothing) and the last idx after every L1 row; the argument errors in the library's order"""
    if len(l1_txs) > MAX_L1:
        raise Refused("at most 512")
    last, made, aux, after = first_idx + size - 1, 0, [], []
    for t in l1_txs:
        frm, to = t.get("fromIdx", 0), t.get("toIdx", 0)
        if not frm:
            if not growing:
                raise Refused("cannot grow")
            if not have_keys:
                raise Refused("from_bjj == NULL")
            if size + made + 1 > capacity:
                raise Refused("the ledger is full")
            made += 1
            last += 1
            aux.append(last)
            if to == EXIT:
                raise Refused("with to_idx = 1")
        else:
            if not first_idx <= frm <= last:
                raise Refused("from_idx = %d does not exist at its row" % frm)
            aux.append(0)
        after.append(last)
        if to > EXIT and not first_idx <= to <= last:
            raise Refused("to_idx = %d does not exist at its row" % to)
        if t.get("amountF", 0) >> 40:
            raise Refused("amount_f has more than 40 bits")
        if t.get("loadAmountF", 0) >> 40:
            raise Refused("load_amount_f has more than 40 bits")
        if t.get("fromEthAddr", 0) >> 160:
            raise Refused("more than 160 bits")
        if L1.has_amount(t) and to == 0:
            raise Refused("an amount with to_idx = 0")
    return aux, after


def lookup(leaf_of, first_idx, count, t):
    """the lowest index among `count` accounts that holds the signed destination of an L2 transfer to an address and its token, or 0"""
    for idx in range(first_idx, first_idx + count):
        leaf = leaf_of(idx)
        if leaf["tokenID"] != t.get("tokenID", 0):
            continue
        te = t.get("toEthAddr", 0)
        if (te != ANY and leaf["ethAddr"] == te) or (te == ANY and leaf["ay"] == t.get("toBjjAy", 0) and leaf["sign"] == t.get("toBjjSign", 0)):
            return idx
    return 0


def model(acc, l1_txs, l2_txs, plan_tokens, fee_idxs, capacity=1 << 12):
    """the scheme over a batch whose L1 rows may create accounts. -> ("refused", row, reason) or a dictionary: aux_from_idx, out_idx_after
    (rows), new_last_idx, slots {idx: the new account's static leaf}, aux_to_idx (rows), is_old0_1, old_key1 (rows), and res:
    ledger_exit_common.scheme_model's result over the rows the pipeline sees"""
    n_l1, f0 = len(l1_txs), acc.first_idx
    aux, after = running_index(f0, acc.n, capacity, l1_txs)
    slots = {a: new_leaf(t) for a, t in zip(aux, l1_txs) if a}
    count = acc.n + len(slots)
    last = f0 + count - 1
    leaf_of = lambda i: slots[i] if i in slots else acc.state(i)   # noqa: E731
    for t in l2_txs:
        if t.get("fromIdx", 0) and not f0 <= t["fromIdx"] <= last:
            raise Refused("outside the state")
        if t.get("fromIdx", 0) and t.get("toIdx", 0) > EXIT and not f0 <= t["toIdx"] <= last:
            raise Refused("outside the state")
    for a in fee_idxs:
        if a and not f0 <= a <= last:
            raise Refused("outside the state")
    eff_l1 = [dict(t, fromIdx=a) if a else t for a, t in zip(aux, l1_txs)]
    aux_to, eff_l2 = [0] * n_l1, []
    for i, t in enumerate(l2_txs):
        found = lookup(leaf_of, f0, count, t) if A.is_to_addr(t) and L1.has_amount(t) else 0
        if A.is_to_addr(t) and L1.has_amount(t) and not found:
            return ("refused", n_l1 + i, 9)
        aux_to.append(found)
        eff_l2.append(dict(t, toIdx=found) if found else t)
    res = X.scheme_model(leaf_of, eff_l1, eff_l2, plan_tokens, fee_idxs)
    if res[0] != "ok":
        return res
    # the tree: the live keys, then the state events in order; a create row's sender event is the insert of its key
    p = X.plan_model(eff_l1, eff_l2, plan_tokens, fee_idxs)
    held = list(range(f0, f0 + acc.n))
    tp = X.tree_plan_model(held + p["account"])[len(held):]
    is_old0, old_key = [0] * (n_l1 + len(l2_txs)), [0] * (n_l1 + len(l2_txs))
    for i, a in enumerate(aux):
        if a:
            insert, old0, key, _ = tp[p["ev_sender"][i]]
            assert insert == 1
            is_old0[i], old_key[i] = old0, 0 if old0 else key
    assert all(tp[e][0] == 0 for e in range(len(tp)) if e not in [p["ev_sender"][i] for i, a in enumerate(aux) if a])
    return {"aux_from_idx": aux + [0] * len(l2_txs), "out_idx_after": after + [last] * len(l2_txs), "new_last_idx": last, "slots": slots, "aux_to_idx": aux_to,
            "is_old0_1": is_old0, "old_key1": old_key, "res": res, "eff_l1": eff_l1, "eff_l2": eff_l2}


# ---- the checker -------------------------------------------------------------------------------------------------------------------------
def builder_batch(db, l1_txs, l2_txs, plan_tokens, fee_idxs, n_levels, aux_to=None, n_tx=None, max_l1=None):
    """BatchBuilder on db with host hashing; an L2 transfer to an address is given its auxToIdx (aux_to: per row, from the model)"""
    n_l1 = len(l1_txs)
    l2 = [dict(t, auxToIdx=aux_to[n_l1 + i]) if aux_to and A.is_to_addr(t) else t for i, t in enumerate(l2_txs)]
    n_tx = n_tx or n_l1 + len(l2)
    txs = [dict(t) for t in l1_txs] + l2 + [{} for _ in range(n_tx - n_l1 - len(l2))]
    return C.builder_batch(None, txs, plan_tokens, fee_idxs, n_levels, db=db, max_l1=n_l1 if max_l1 is None else max_l1)


def expected_arrays(bb, l2_txs, n_l1):
    """ledger_exit_common.expected_arrays plus the six create arrays from the builder's dictionary"""
    exp = X.expected_arrays(bb, l2_txs, n_l1)
    inp = bb.get_input()
    exp.update(aux_from_idx=C.to_bytes(inp["auxFromIdx"]), is_old0_1=C.to_bytes(inp["isOld0_1"]), old_key1=C.to_bytes(inp["oldKey1"]),
               old_value1=C.to_bytes(inp["oldValue1"]), out_idx_after=C.to_bytes(inp["imOutIdx"] + [bb.new_last_idx]), new_last_idx=C.to_bytes([bb.new_last_idx]))
    return exp


def touched(m, l2_txs, fee_idxs):
    """the accounts a modelled batch touches or creates"""
    acc = set(m["slots"])
    for t in m["eff_l1"] + m["eff_l2"]:
        if t.get("fromIdx"):
            acc |= {t["fromIdx"]} | ({t["toIdx"]} if t.get("toIdx", 0) > EXIT else set())
    return sorted(acc | {i for i in fee_idxs if i})


# ---- batches -----------------------------------------------------------------------------------------------------------------------------
KEY_ABOVE_R = (P + 12345) | 1 << 254 | 1 << 255   # low bits >= r, bits 254 and 255 set


def kinds_batch(acc, n0=0):
    """every kind of create row and every use of a created account, on a state of acc.n accounts: the first new index is f0 + acc.n.
    -> (l1_txs, l2_txs, fee_plan_tokens, fee_idxs); account(n0 + j) is the key of the j-th create"""
    f0 = acc.first_idx
    new = f0 + acc.n
    k = [account(n0 + j) for j in range(7)]
    old = f0 if acc.n else new          # an account that exists before the batch when there is one
    l1_txs = [
        create_for(k[0], load=10 ** 12),                                                 # new + 0: createAccountDeposit
        create_for(k[1], load=5 * 10 ** 11, amount=2 * 10 ** 11, to=old),                # new + 1: transfers to an older account
        create_for(k[2], load=7 * 10 ** 11, amount=3 * 10 ** 11, to=new + 2),            # new + 2: transfers to itself
        create_for(k[3], load=10 ** 9, amount=2 * 10 ** 9, to=new),                      # new + 3: nullified by underflow
        create_for(k[4], token=2, load=10 ** 10, amount=10 ** 9, to=new),                # new + 4: nullified by the receiver's token
        create(KEY_ABOVE_R, token=1, eth=k[5].eth_addr, load=4 * 10 ** 11),              # new + 5: a key whose low bits are not below r
        create_for(k[6]),                                                                # new + 6: createAccount, nothing else
        L1.l1(new, 0, 0, 3 * 10 ** 11, 1, k[0].eth_addr),                                # a deposit into a created account
        L1.l1(new + 2, new + 6, 10 ** 11, 0, 1, k[2].eth_addr),                          # a forceTransfer between created accounts
    ]
    l2_txs = [dict(C.tx(new, new + 1, 10 ** 11, 100, nonce=0), signer=k[0]),             # a signed transfer from a created account
              dict(C.tx(new + 2, EXIT, 5 * 10 ** 10, 176, nonce=0), signer=k[2]),        # an exit from one
              dict(C.tx(new, new + 6, 0, 1, nonce=1), signer=k[0])]
    return l1_txs, l2_txs, [1, 2], [new + 1, 0]


def sign_all(l2_txs, chain_id=1):
    """the L2 rows signed by their `signer` (s, r8x, r8y filled in; the key object is kept for the builder)"""
    out = []
    for t in l2_txs:
        t = dict(t)
        if t.get("fromIdx", 0) and "signer" in t:
            t.update(t["signer"].sign_msg(B.build_hash_sig(t, chain_id)))
        out.append(t)
    return out


def draw_batch(acc, seed, n_create=5, n0=0):
    """a seeded batch on acc: creates of every kind, deposits and transfers on what they made, L2 transfers and exits from them"""
    rng = np.random.default_rng(seed)
    f0 = acc.first_idx
    new = f0 + acc.n
    keys, l1_txs, bal, tok = [], [], {}, {}
    for j in range(n_create):
        a = account(n0 + j)
        keys.append(a)
        kind = int(rng.integers(0, 6))
        load = int(rng.integers(1, 1 << 20)) * 10 ** 8
        token = 2 if kind == 4 else 1
        exists = list(range(f0, new + j + 1))
        to = exists[int(rng.integers(0, len(exists)))] if kind in (1, 2, 3, 4) else 0
        amount = L1.float_floor(load // 3) if kind in (1, 2, 4) else L1.float_floor(load * 2) if kind == 3 else 0
        if kind == 5:
            load = 0
        l1_txs.append(create_for(a, token=token, load=load, amount=amount, to=to))
        tok[new + j] = token
        to_tok = tok.get(to, acc.state(to)["tokenID"] if f0 <= to < new else None)
        moved = amount if kind in (1, 2, 4) and to_tok == token else 0
        bal[new + j] = load - moved
        if moved and to >= new:
            bal[to] = bal.get(to, 0) + moved
    for j in range(n_create):
        if rng.integers(0, 2):
            l1_txs.append(L1.l1(new + j, 0, 0, 10 ** 9, tok[new + j], keys[j].eth_addr))
            bal[new + j] += 10 ** 9
    l2_txs, nonce = [], {}
    for _ in range(4):
        j = int(rng.integers(0, n_create))
        f = new + j
        same = [i for i in tok if tok[i] == tok[f]]
        to = EXIT if rng.integers(0, 3) == 0 else same[int(rng.integers(0, len(same)))]
        amount = L1.float_floor(bal[f] // 10)
        sel = C.SELECTORS[int(rng.integers(0, len(C.SELECTORS)))]
        if bal[f] < amount + B.compute_fee(amount, sel):
            continue
        l2_txs.append(dict(C.tx(f, to, amount, sel, token=tok[f], nonce=nonce.get(f, 0)), signer=keys[j]))
        nonce[f] = nonce.get(f, 0) + 1
        bal[f] -= amount + B.compute_fee(amount, sel)
        if amount and to != EXIT:
            bal[to] += amount
    return l1_txs, l2_txs


def arg_cases(acc):
    """[(l1_txs, l2_txs, a part of the message)]: the argument errors of a batch with create rows that need no device to be found"""
    f0, new = acc.first_idx, acc.first_idx + acc.n
    k = account(0)
    ok = create_for(k, load=10)
    return [([dict(ok, toIdx=1)], [], "with to_idx = 1"), ([dict(ok, amountF=5)], [], "an amount with to_idx = 0"),
            ([dict(ok, amountF=5, toIdx=new + 1)], [], "to_idx = %d does not exist at its row" % (new + 1)),
            ([L1.l1(new, 0, 0, 5), ok], [], "from_idx = %d does not exist at its row" % new),
            ([ok, L1.l1(new, new + 1, 5, 5)], [], "to_idx = %d does not exist at its row" % (new + 1)),
            ([dict(ok, loadAmountF=1 << 40)], [], "load_amount_f has more than 40 bits"), ([dict(ok, fromEthAddr=1 << 160)], [], "more than 160 bits"),
            ([ok], [C.tx(new + 1, new, 5)], "outside the state"), ([ok], [C.tx(new, new + 1, 5)], "outside the state"), ([ok] * 513, [], "at most 512")]


# ---- tests/native/ledger_create_check.cpp's input ----------------------------------------------------------------------------------------
def check_lines(keys, tokens=(0, 1, 0xFFFFFFFF)):
    """expectations in plain Python: ay, sign and e0 of every key with every token; the running index; which rows report an old leaf"""
    lines = []
    for key in keys:
        ay, sign = decode_key(key)
        for token in tokens:
            lines.append("k %x %x %x %x %x" % (key, token, ay, sign, token | sign << 72))
    for last in (255, 256, (1 << 48) - 2):
        for creates in (0, 1):
            lines.append("i %x %x %x" % (last, creates, last + creates))
    for flags in range(4):
        lines.append("r %x %x" % (flags, 1 if flags == 1 else 0))
    return "\n".join(lines) + "\n"
