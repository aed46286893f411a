"""Shared by tests/test_device_state.py (GPU) and tests/test_device_state_cpu.py: the update draws, the independent checker -- the Python
builder.SMT over a DenseState, one update at a time with host hashing -- and a from-scratch rebuild of the level arrays."""
import functools

import numpy as np

from circuits_amd import builder as B

P = B.P


@functools.lru_cache(maxsize=None)
def base_state(k, seed=0x48455A31):
    return B.DenseState.build(k, seed=seed)


def to_bytes(vals):
    """ints -> [n, 32] uint8 little-endian"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


def to_int(a):
    return int.from_bytes(np.ascontiguousarray(a).tobytes(), "little")


def base_fields(base, idx):
    """the leaf fields (e0, balance, ay, ethAddr) the base holds for account idx, as ints"""
    s = base.state(idx)
    return [s["tokenID"] + (s["nonce"] << 32) + (s["sign"] << 72), s["balance"], s["ay"], s["ethAddr"]]


def draw_updates(base, m, seed, pool=None):
    """m updates as synthetic_batch draws senders and receivers (uniform over the accounts, so repeats happen; `pool` narrows the draw to
    that many accounts to force them): the account keeps its key, nonce and balance change. -> (idx list, fields as ints [m][4])"""
    rng = np.random.default_rng(seed)
    accounts = base.N if pool is None else pool
    off = int(rng.integers(0, base.N - accounts + 1))
    idx = [base.first_idx + off + int(x) for x in rng.integers(0, accounts, size=m)]
    fields = []
    for i in idx:
        f = base_fields(base, i)
        nonce = int(rng.integers(1, 1 << 40))
        f[0] = 1 + (nonce << 32) + (f[0] >> 72 << 72)
        f[1] = int(rng.integers(0, 1 << 62)) * int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62))   # below 2^192
        fields.append(f)
    return idx, fields


def edge_cases(base):
    """the orders of one call the issue names -> {name: (idx list, fields)}; the counter makes every update's fields distinct"""
    k, f0 = base.k, base.first_idx
    n = [0]

    def upd(i):
        n[0] += 1
        f = base_fields(base, i)
        return [1 + (n[0] << 32), f[1] + n[0], f[2], f[3]]

    def case(seq):
        return list(seq), [upd(i) for i in seq]
    a = f0 + 37
    out = {"same_account_5": case([a] * 5)}
    # siblings at the deepest level: residues p and p + 2^(k - 1)
    p = (f0 + 5) % base.N % (1 << (k - 1))
    x, y = base.key_of(p), base.key_of(p + (1 << (k - 1)))
    out["deepest_siblings_alternating"] = case([x, y, x, y, x, y, y, x])
    e = f0 + 10 + ((f0 + 10) & 1)   # even: e and e + 1 differ in bit 0 only
    out["bit0_pair"] = case([e, e + 1, e + 1, e, e + 1])
    b = f0 + base.N - 1
    out["restore_original"] = ([b, a, b, a], [upd(b), upd(a), base_fields(base, b), base_fields(base, a)])
    return out


def fields_array(fields):
    return to_bytes([x for f in fields for x in f]).reshape(len(fields), 4, 32)


def smt_apply(base, idx, fields, smt=None):
    """the checker: builder.SMT over the base, the updates one at a time in order -> (smt, [update results], [state hashes])"""
    t = smt or B.SMT(base=base)
    res, vals = [], []
    for i, f in zip(idx, fields):
        v = B.host().poseidon(f)
        vals.append(v)
        res.append(t.update(i, v))
    return t, res, vals


def expect_arrays(res, n_sib):
    """the checker's results in hz_state_apply's output layout"""
    m = len(res)
    sib = np.zeros((m, n_sib, 32), dtype=np.uint8)
    for j, r in enumerate(res):
        if r["siblings"]:
            sib[j, :len(r["siblings"])] = to_bytes(r["siblings"])
    return {"siblings": sib, "old_value": to_bytes([r["oldValue"] for r in res]), "old_root": to_bytes([r["oldRoot"] for r in res]),
            "new_root": to_bytes([r["newRoot"] for r in res])}


def rebuild_levels(k, first_idx, cols):
    """DenseState.build's bottom-up construction from explicit leaf fields (cols: e0, balance, ay, ethAddr as [N, 32]) with the host
    library's Poseidon -> (levels, value)"""
    N = 1 << k
    hash_rows = B.host().poseidon_many
    rows = np.stack(cols, axis=1)
    value = np.frombuffer(hash_rows(5, N, rows.tobytes()), dtype=np.uint8).reshape(N, 32)
    p = np.arange(N, dtype=np.int64)
    j = (p - first_idx) % N
    keycol = to_bytes((first_idx + j).tolist())
    one = np.zeros((N, 32), dtype=np.uint8)
    one[:, 0] = 1
    levels = [None] * (k + 1)
    levels[k] = np.frombuffer(hash_rows(4, N, np.stack([keycol, value[j], one], axis=1).tobytes()), dtype=np.uint8).reshape(N, 32)
    for d in range(k - 1, -1, -1):
        n = 1 << d
        rows = np.stack([levels[d + 1][:n], levels[d + 1][n:2 * n]], axis=1)
        levels[d] = np.frombuffer(hash_rows(3, n, rows.tobytes()), dtype=np.uint8).reshape(n, 32)
    return levels, value


def final_cols(base, idx, fields):
    """the leaf fields of every account after the updates, as State.load's four arrays"""
    cols = [np.array(c) for c in base.leaf_fields()]
    for i, f in zip(idx, fields):
        for c in range(4):
            cols[c][i - base.first_idx] = to_bytes([f[c]])[0]
    return cols


def processor_inputs(idx, vals, res, n_levels):
    """the updates as instances of circomlib's SMTProcessor(n_levels): UPDATE of an existing key"""
    return [{"oldRoot": r["oldRoot"], "siblings": list(r["siblings"]) + [0] * (n_levels - len(r["siblings"])), "oldKey": i, "oldValue": r["oldValue"],
             "isOld0": 0, "newKey": i, "newValue": v, "fnc": [0, 1]} for i, v, r in zip(idx, vals, res)]
