"""Shared by tests/test_sparse_tree.py (GPU) and tests/test_sparse_tree_cpu.py: the op sequences, the independent checker -- the Python
builder.SMT (no base, host hashing) one op at a time -- and a plain restatement of the COUNT RULE the device tree's planner follows."""
import functools

import numpy as np

from circuits_amd import builder as B

P = B.P
N_SIB = 17   # SMTProcessor / SMTVerifier (nLevels + 1) of the circuits' nLevels = 16


def to_bytes(vals):
    """ints -> [n, 32] uint8 little-endian"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


def to_int(a):
    return int.from_bytes(np.ascontiguousarray(a).tobytes(), "little")


def fields_array(fields):
    return to_bytes([x for f in fields for x in f]).reshape(len(fields), 4, 32)


def make_fields(keys, seed):
    """distinct leaf fields (e0, balance, ay, ethAddr) for every op: the counter in e0's nonce makes a re-update of a key a new value"""
    rng = np.random.default_rng(seed)
    out = []
    for n, _ in enumerate(keys):
        big = [int(x) for x in rng.integers(1, 1 << 62, size=8)]
        out.append([1 + ((n + 1) << 32) + ((n & 1) << 72), big[0] * big[1] * big[2], big[3] * big[4] * big[5] * big[6] % P, big[7] << 90])
    return out


def small_cases():
    """the smallest shapes, by name -> key sequence"""
    a = 0x155                      # low 10 bits 0101010101
    cases = {
        "one_insert": [300],
        "bit0_pair": [300, 301],
        "share_10_bits": [a, a | 1 << 10 | 1 << 30],          # differ in bit 10 first: ten zero siblings, the old leaf pushed down
        "insert_then_3_updates": [777, 777, 777, 777],
        "push_down_then_update_old": [a, a | 1 << 12, a],      # insert A, insert B that pushes A down, update A
        "three_share_5_bits_fwd": [0x0B, 0x0B | 1 << 5, 0x0B | 1 << 6 | 1 << 40],
        "consecutive_64_from_256": list(range(256, 320)),      # the exit tree's pattern
    }
    cases["three_share_5_bits_rev"] = cases["three_share_5_bits_fwd"][::-1]
    return cases


def draw_mix(m, seed):
    """m ops over a pool small enough to force repeats (so the draw holds inserts and updates): keys with DISTINCT low 16 bits (every leaf
    stays above depth 17) and random bits above; a third of the pool shares its low 6 bits, which makes deep push-downs"""
    rng = np.random.default_rng(seed)
    pool_n = max(8, m * 3 // 8)
    res = rng.choice(1 << 16, size=pool_n, replace=False).astype(np.int64)
    res[: pool_n // 3] = (res[: pool_n // 3] & ~0x3F) | 0x2A
    res = np.unique(res)
    rng.shuffle(res)
    pool = [int(r) | int(h) << 16 for r, h in zip(res, rng.integers(0, 1 << 32, size=res.size))]
    return [pool[int(i)] for i in rng.integers(0, len(pool), size=m)]


def regrow_calls():
    """three calls on one tree of n_sib_max = 10 -> [(keys, n_sib)] of 3, 200 and 3 ops with n_sib = 7, 10, 7. The large call draws from 120
    keys that share their low 6 bits eight at a time (distinct low 9 bits: leaves at depth 7 .. 9, inserts and updates); the small calls
    touch keys that are alone below bit 6, so their leaves stay above depth 7"""
    crowd = [(r & 63) << 20 | 1 << 16 | r for r in range(512) if (r & 63) < 15]
    lone = [7 << 16 | 60, 8 << 16 | 61, 9 << 16 | 62, 10 << 16 | 63]
    rng = np.random.default_rng(10)
    large = [crowd[int(i)] for i in rng.integers(0, len(crowd), size=198)] + lone[1:3]
    return [([lone[0], crowd[0], lone[0]], 7), (large, 10), ([lone[3], lone[1], lone[3]], 7)]


def smt_replay(keys, fields, smt=None):
    """the checker: builder.SMT, one op at a time -> (smt, per-op results). A result holds SMTProcessor's inputs as the SMT states them
    plus fnc (1 insert, 0 update), the new value, the depth of the op's leaf and of the walk that preceded it"""
    t = smt or B.SMT()
    H = B.host().poseidon
    out = []
    for k, f in zip(keys, fields):
        v = H(f)
        before = t.find(k)
        if before["found"]:
            r = t.update(k, v)
            r["isOld0"] = False
            r["fnc"] = 0
        else:
            r = t.insert(k, v)
            r["fnc"] = 1
        r["value"] = v
        r["find_depth"] = len(before["siblings"])
        r["depth"] = len(t.find(k)["siblings"])
        out.append(r)
    return t, out


@functools.lru_cache(maxsize=None)
def replay_case(name):
    keys = small_cases()[name]
    fields = make_fields(keys, seed=len(name))
    t, res = smt_replay(keys, fields)
    return keys, fields, t, res


@functools.lru_cache(maxsize=None)
def replay_mix(m, seed):
    keys = draw_mix(m, seed)
    fields = make_fields(keys, seed=seed + 1)
    t, res = smt_replay(keys, fields)
    return keys, fields, t, res


def expect_arrays(res, n_sib):
    """the checker's results in hz_smt_apply's output layout"""
    m = len(res)
    sib = np.zeros((m, n_sib, 32), dtype=np.uint8)
    for j, r in enumerate(res):
        if r["siblings"]:
            sib[j, :len(r["siblings"])] = to_bytes(r["siblings"])
    return {"siblings": sib, "old_key": np.array([r["oldKey"] for r in res], dtype=np.uint64), "old_value": to_bytes([r["oldValue"] for r in res]),
            "is_old0": np.array([1 if r["isOld0"] else 0 for r in res], dtype=np.uint8), "fnc": np.array([r["fnc"] for r in res], dtype=np.uint8),
            "old_root": to_bytes([r["oldRoot"] for r in res]), "new_root": to_bytes([r["newRoot"] for r in res])}


def count_rule(keys, bits=48):
    """The rule in plain Python, integers only. Slot (d, p), p = key mod 2^d, holds the COUNT of keys with that prefix (and their sum: the
    only key of a slot of count 1). The walk of an op on K ends at the shallowest depth f where K's slot has count <= 1; afterwards K's
    leaf sits at the shallowest depth D where K's slot has count 1. -> per op (D, fnc, old_key, is_old0, f)"""
    cnt, tot, present, out = {}, {}, set(), []
    for K in keys:
        f = 0
        while cnt.get((f, K & ((1 << f) - 1)), 0) > 1:
            f += 1
        slot = (f, K & ((1 << f) - 1))
        if K in present:
            assert cnt[slot] == 1 and tot[slot] == K
            out.append((f, 0, K, 0, f))
            continue
        met = tot[slot] if cnt.get(slot, 0) == 1 else None
        present.add(K)
        for d in range(bits + 1):
            s = (d, K & ((1 << d) - 1))
            cnt[s] = cnt.get(s, 0) + 1
            tot[s] = tot.get(s, 0) + K
        D = f
        while cnt[(D, K & ((1 << D) - 1))] > 1:
            D += 1
        out.append((D, 1, K if met is None else met, 1 if met is None else 0, f))
    return out


def processor_inputs(keys, got, j, values):
    """op j of a device call as an instance of circomlib's SMTProcessor"""
    return {"oldRoot": to_int(got["old_root"][j]), "siblings": [to_int(s) for s in got["siblings"][j]], "oldKey": int(got["old_key"][j]),
            "oldValue": to_int(got["old_value"][j]), "isOld0": int(got["is_old0"][j]), "newKey": keys[j], "newValue": values[j],
            "fnc": [1, 0] if got["fnc"][j] else [0, 1]}
