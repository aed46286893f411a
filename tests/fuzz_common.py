"""Adversarial differential fuzz: inputs no batch builder would produce, HIP path against the CPU oracle (test infrastructure).

The reference's calculator defines a witness AND a first failing constraint for ARBITRARY field elements in every input
(reference test/rollup-tx.test.js:911-918, test/rollup-main.test.js:868-877, test/withdraw.test.js:159-171 mutate inputs and expect
the first violated `===`); the kernels replace parts of the templates' arithmetic by shortcuts that are exact "for any input"
(k_smt: SMTLevIns / the state machine as integer logic, structurally empty and dead levels skipped per wavefront; compute_fee_dev:
the product-free path when applyFee is a bit on every lane; k_main_front: L1TxFullData rows copied instead of multiplied). This module
makes the inputs that claim is tested on: valid cases from the builder, then seeded mutations --

  * scalars replaced by 0, 1, 2, r - 1, a random field element, a random small number, value +- 1, value + 2^k (k >= nLevels for
    keys: bits above the tree), for function bits / isOld0 / enabled / onChain / newAccount and every other input alike;
  * sibling vectors with random zero patterns: all zero, zero only at the top, non-zero above the leaf, each entry zeroed with
    probability 1/2, all random;
  * a fraction of instances left valid and a fraction with a third of all their inputs replaced.

and the machinery that evaluates a chunk of instances on the oracle with one thread per slice (ctypes releases the GIL inside
orc_run; every thread owns its context)."""
import random
import threading

import numpy as np

from oracle_binding import OracleCtx, fr_to_bytes, flatten

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def garbage(rng, old=0, key_bits=None):
    """a replacement for one scalar input"""
    k = rng.randrange(10)
    if k == 0:
        return 0
    if k == 1:
        return 1
    if k == 2:
        return 2
    if k == 3:
        return P - 1
    if k == 4:
        return rng.randrange(P)
    if k == 5:
        return rng.randrange(1 << rng.choice((8, 16, 32, 48, 64, 128, 192)))
    if k == 6:
        return (old + 1) % P
    if k == 7:
        return (old - 1) % P
    if k == 8:   # a bit above the range the template decomposes (keys: above the tree)
        lo = key_bits if key_bits is not None else 8
        return (old + (1 << rng.randrange(lo, 253))) % P
    return old ^ (1 << rng.randrange(0, 48)) if old < (1 << 200) else rng.randrange(P)


def sibling_pattern(rng, sib):
    """one of the zero patterns the SMTLevIns / state-machine shortcuts have to survive"""
    n = len(sib)
    k = rng.randrange(7)
    out = list(sib)
    if k == 0:
        return [0] * n
    if k == 1:    # zero only at the top
        return [0 if i == 0 else (v or rng.randrange(1, P)) for i, v in enumerate(out)]
    if k == 2:    # non-zero above (deeper than) the leaf: the entries a valid proof leaves at zero
        nz = max((i for i, v in enumerate(out) if v), default=-1)
        for i in rng.sample(range(nz + 1, n), min(n - nz - 1, rng.randrange(1, 4))) if nz + 1 < n else []:
            out[i] = rng.randrange(1, P)
        return out
    if k == 3:    # each entry zeroed with probability 1/2
        return [0 if rng.random() < 0.5 else v for v in out]
    if k == 4:    # all random
        return [rng.randrange(P) for _ in range(n)]
    if k == 5:    # random entries, random zeros
        return [0 if rng.random() < 0.5 else rng.randrange(P) for _ in range(n)]
    out[n - 1] = rng.randrange(1, P)   # the last sibling must be 0 when the processor is enabled (SMTLevIns)
    return out


def _leaves(d):
    """[(name, index path)] of every scalar in an input object"""
    out = []

    def walk(name, v, path):
        if isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk(name, x, path + (i,))
        else:
            out.append((name, path))
    for k, v in d.items():
        walk(k, v, ())
    return out


def _copy(v):
    return [_copy(x) for x in v] if isinstance(v, (list, tuple)) else v


def _get(d, name, path):
    v = d[name]
    for i in path:
        v = v[i]
    return v


def _set(d, name, path, val):
    if not path:
        d[name] = val
        return
    v = d[name]
    for i in path[:-1]:
        v = v[i]
    v[path[-1]] = val


def mutate(rng, base, sibling_fields=(), key_fields=(), key_bits=None, bit_fields=()):
    """a seeded mutation of a valid input object: 10 % untouched, 5 % a third of all inputs replaced, the rest one to four edits"""
    d = {k: _copy(v) for k, v in base.items()}
    r = rng.random()
    if r < 0.10:
        return d
    leaves = _leaves(d)
    if r < 0.15:
        for name, path in rng.sample(leaves, max(1, len(leaves) // 3)):
            _set(d, name, path, garbage(rng, _get(d, name, path)))
        return d
    for _ in range(rng.randrange(1, 5)):
        k = rng.random()
        if sibling_fields and k < 0.3:
            f = rng.choice(sibling_fields)   # (name, path to the vector)
            name, path = f if isinstance(f, tuple) else (f, ())
            _set(d, name, path, sibling_pattern(rng, _get(d, name, path)))
        elif key_fields and k < 0.45:
            f = rng.choice(key_fields)
            name, path = f if isinstance(f, tuple) else (f, ())
            _set(d, name, path, garbage(rng, _get(d, name, path), key_bits))
        elif bit_fields and k < 0.7:
            f = rng.choice(bit_fields)
            name, path = f if isinstance(f, tuple) else (f, ())
            _set(d, name, path, rng.choice((0, 1, 2, P - 1, rng.randrange(P), 1 - _get(d, name, path) if _get(d, name, path) in (0, 1) else 0)))
        else:
            name, path = rng.choice(leaves)
            _set(d, name, path, garbage(rng, _get(d, name, path)))
    return d


# ---- evaluation ----------------------------------------------------------------------------------------------------------------
def run_oracle_threads(template, shape, cases, n_threads=None, set_case=None):
    """the oracle over `cases`, one context per thread (contiguous slices). Returns [(ctx, first, count)], the contexts already run.
    set_case(ctx, i, k): another way than set_inputs to give instance k of a context the inputs of case i (set_packed_case)."""
    import os
    n = len(cases)
    if n_threads is None:
        try:
            n_threads = len(os.sched_getaffinity(0))
        except Exception:
            n_threads = os.cpu_count() or 1
        try:   # the GPU box shows 256 CPUs and allows 16 (cgroup cpu.max)
            q, per = open("/sys/fs/cgroup/cpu.max").read().split()
            if q != "max":
                n_threads = min(n_threads, max(1, int(q) // int(per)))
        except Exception:
            pass
    n_threads = max(1, min(n_threads, 32, n))
    bounds = [n * t // n_threads for t in range(n_threads + 1)]
    parts = [None] * n_threads
    errs = []

    def work(t):
        try:
            lo, hi = bounds[t], bounds[t + 1]
            o = OracleCtx(template, *shape, n_instances=hi - lo)
            for i in range(lo, hi):
                if set_case is None:
                    o.set_inputs(cases[i], instance=i - lo)
                else:
                    set_case(o, i, i - lo)
            o.run_result = o.run()
            parts[t] = (o, lo, hi - lo)
        except Exception as e:   # pragma: no cover
            errs.append(e)
    ths = [threading.Thread(target=work, args=(t,)) for t in range(n_threads)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    if errs:
        raise errs[0]
    return parts


def oracle_failures(parts):
    """{instance: (unit, constraint id, lhs, rhs)} over all slices"""
    out = {}
    for o, lo, cnt in parts:
        for k in range(cnt):
            f = o.failure_of(k)
            if f is not None:
                out[lo + k] = f
    return out


def constraint_name(cid):
    import ctypes
    from oracle_binding import Oracle
    f = Oracle().c.orc_constraint_name
    f.restype = ctypes.c_char_p
    return f(cid).decode()


def set_all_inputs(g, cases):
    """every input of every instance of a product context, one call per signal (instance = -1)"""
    for name, _ in g.input_names():
        g.set_input(name, [c[name] for c in cases], instance=-1)


_FR_0, _FR_1 = bytes(32), (1).to_bytes(32, "little")


def pack_case(case):
    """{input name: (its values as 32-byte little-endian records, their number)} of one input object. Inputs that are mostly bits
    (HashInputs: 10^4 per instance) cost a tenth of fr_to_bytes over flatten, and the records serve the product and the oracle alike."""
    out = {}
    for name, v in case.items():
        flat = v if isinstance(v, list) and not any(isinstance(x, (list, tuple)) for x in v) else flatten(v)
        out[name] = (b"".join([_FR_1 if x == 1 else _FR_0 if x == 0 else int(x % P).to_bytes(32, "little") for x in flat]), len(flat))
    return out


def set_packed_case(ctx, packed, instance):
    """pack_case's records into one instance of an oracle context (run_oracle_threads' set_case)"""
    for name, (raw, cnt) in packed.items():
        rc = ctx.o.c.orc_set_input(ctx.h, instance, name.encode(), raw, cnt)
        assert rc == 0, "oracle rejected input %s (rc %d)" % (name, rc)


def set_all_packed(g, packed):
    """set_all_inputs from pack_case's records: every input of every instance of a product context, one call per signal"""
    for name, _ in g.input_names():
        g.L._check(g.L.c.hz_set_input(g.h, -1, name.encode(), b"".join(pk[name][0] for pk in packed), sum(pk[name][1] for pk in packed)))


def compare_instanced(g, parts, n, rows_per_chunk=512):
    """whole physical buffer of an instanced template ([signal][instance]) against the oracle slices"""
    wl = g.witness_len()
    assert g.total() == wl * n
    for r0 in range(0, wl, rows_per_chunk):
        rows = min(rows_per_chunk, wl - r0)
        a = np.frombuffer(g.read_raw_bytes(r0 * n, rows * n), dtype=np.uint8).reshape(rows, n, 32)
        for o, lo, cnt in parts:
            assert o.witness_len() == wl
            b = np.frombuffer(o.read_raw_bytes(r0 * cnt, rows * cnt), dtype=np.uint8).reshape(rows, cnt, 32)
            if not np.array_equal(a[:, lo:lo + cnt, :], b):
                r, k = np.argwhere((a[:, lo:lo + cnt, :] != b).any(axis=2))[0]
                name = "?"
                try:
                    for i in range(g.symbol_count()):
                        nm, idx = g.symbol(i)
                        if idx == r0 + r:
                            name = nm
                            break
                except Exception:
                    pass
                raise AssertionError("witness differs at signal row %d (%s), instance %d: gpu=%d oracle=%d" % (
                    r0 + r, name, lo + k, int.from_bytes(a[r, lo + k].tobytes(), "little"), int.from_bytes(b[r, k].tobytes(), "little")))


def compare_replicated(g, o, n_gpu, n_dist, which, rows_per_chunk=256):
    """Instanced template (one section, physical layout [signal][instance]): instance k of the GPU context holds the inputs of the
    oracle's instance which[k] (o: one oracle context, or run_oracle_threads' slices); whole physical buffers, a few hundred signal
    rows at a time."""
    parts = o if isinstance(o, list) else [(o, 0, n_dist)]
    wl = g.witness_len()
    assert g.total() == wl * n_gpu and sum(cnt for _, _, cnt in parts) == n_dist
    assert all(p.witness_len() == wl and p.total() == wl * cnt for p, _, cnt in parts) and [lo for _, lo, _ in parts] == [sum(c for _, _, c in parts[:i]) for i in range(len(parts))]
    idx = np.asarray(which)
    assert idx.shape == (n_gpu,)
    for r0 in range(0, wl, rows_per_chunk):
        rows = min(rows_per_chunk, wl - r0)
        a = np.frombuffer(g.read_raw_bytes(r0 * n_gpu, rows * n_gpu), dtype=np.uint8).reshape(rows, n_gpu, 32)
        b = np.concatenate([np.frombuffer(p.read_raw_bytes(r0 * cnt, rows * cnt), dtype=np.uint8).reshape(rows, cnt, 32) for p, _, cnt in parts], axis=1)[:, idx, :]
        if not np.array_equal(a, b):
            r, k = np.argwhere((a != b).any(axis=2))[0]
            raise AssertionError("witness differs at signal row %d, instance %d (oracle instance %d): gpu=%d oracle=%d" % (
                r0 + r, k, which[k], int.from_bytes(a[r, k].tobytes(), "little"), int.from_bytes(b[r, k].tobytes(), "little")))


def check_failures(g, parts, run_error, which=None):
    """the product's per-instance first-failure records == the oracle's, and the launch-wide report == the lowest of them. Returns the
    number of rejected instances. which: instance k of the product holds the oracle's case which[k] (a replicated launch; every one of
    the len(which) instances is compared); None: instance k is case k."""
    exp = oracle_failures(parts)
    if which is not None:
        assert len(which) == g.n_instances
        exp = {k: exp[d] for k, d in enumerate(which) if d in exp}
    got = {f[0]: (f[1], f[2], f[4], f[5]) for f in g.failures()}
    if got != exp:
        for i in sorted(set(got) | set(exp)):
            if got.get(i) != exp.get(i):
                nm = lambda r: None if r is None else (r[0], constraint_name(r[1]), r[2], r[3])   # noqa: E731
                raise AssertionError("first failure of instance %d%s: gpu %r, oracle %r" % (
                    i, "" if which is None else " (case %d)" % which[i], nm(got.get(i)), nm(exp.get(i))))
    if exp:
        i0 = min(exp)
        assert run_error is not None, "the oracle rejects instance %d, the HIP path accepted the launch" % i0
        assert (run_error.instance, run_error.unit, run_error.constraint_id, run_error.lhs, run_error.rhs) == (i0,) + exp[i0]
    else:
        assert run_error is None
    return len(exp)


# ---- case generators -----------------------------------------------------------------------------------------------------------
def smt_processor_cases(n, n_levels, seed):
    """valid inserts / updates / deletes / nops on a growing tree, then mutated"""
    from circuits_amd import builder as B
    rng = random.Random(seed)
    t = B.SMT()
    keys, valid = [], []

    def pad(s):
        return list(s) + [0] * (n_levels - len(s))
    n_valid = max(8, min(400, n // 8))
    while len(valid) < n_valid:
        r = rng.random()
        if keys and r < 0.3:
            k = rng.choice(keys)
            v = rng.randrange(1, 1 << 200)
            u = t.update(k, v)
            valid.append({"oldRoot": u["oldRoot"], "siblings": pad(u["siblings"]), "oldKey": k, "oldValue": u["oldValue"], "isOld0": 0, "newKey": k, "newValue": v, "fnc": [0, 1]})
        elif keys and r < 0.4:   # NOP with the inputs of an inclusion proof
            k = rng.choice(keys)
            f = t.find(k)
            valid.append({"oldRoot": t.root, "siblings": pad(f["siblings"]), "oldKey": k, "oldValue": f["foundValue"], "isOld0": 0, "newKey": k, "newValue": f["foundValue"], "fnc": [0, 0]})
        else:
            k = rng.randrange(1 << (n_levels - 2))
            while k in keys:
                k = rng.randrange(1 << (n_levels - 2))
            keys.append(k)
            v = rng.randrange(1, 1 << 200)
            ins = t.insert(k, v)
            c = {"oldRoot": ins["oldRoot"], "siblings": pad(ins["siblings"]), "oldKey": 0 if ins["isOld0"] else ins["oldKey"], "oldValue": 0 if ins["isOld0"] else ins["oldValue"],
                 "isOld0": 1 if ins["isOld0"] else 0, "newKey": k, "newValue": v, "fnc": [1, 0]}
            valid.append(c)
            valid.append(dict(c, oldRoot=ins["newRoot"], fnc=[1, 1]))   # DELETE: the same proof walked backwards
    out = []
    for i in range(n):
        out.append(mutate(rng, valid[rng.randrange(len(valid))], sibling_fields=("siblings",), key_fields=("oldKey", "newKey"), key_bits=n_levels,
                          bit_fields=(("fnc", (0,)), ("fnc", (1,)), "isOld0")))
    return out


def smt_verifier_cases(n, n_levels, seed):
    from circuits_amd import builder as B
    rng = random.Random(seed)
    t = B.SMT()
    keys = []

    def pad(s):
        return list(s) + [0] * (n_levels - len(s))
    for _ in range(200):
        k = rng.randrange(1 << (n_levels - 2))
        if k in keys:
            continue
        keys.append(k)
        t.insert(k, rng.randrange(1, 1 << 200))
    valid = []
    for k in keys[:120]:
        f = t.find(k)
        valid.append({"enabled": 1, "root": t.root, "siblings": pad(f["siblings"]), "oldKey": 0, "oldValue": 0, "isOld0": 0, "key": k, "value": f["foundValue"], "fnc": 0})
    while len(valid) < 240:
        k = rng.randrange(1 << (n_levels - 2))
        f = t.find(k)
        if f["found"]:
            continue
        valid.append({"enabled": 1, "root": t.root, "siblings": pad(f["siblings"]), "oldKey": 0 if f["isOld0"] else f["notFoundKey"], "oldValue": 0 if f["isOld0"] else f["notFoundValue"],
                      "isOld0": 1 if f["isOld0"] else 0, "key": k, "value": 0, "fnc": 1})
    out = []
    for i in range(n):
        out.append(mutate(rng, valid[rng.randrange(len(valid))], sibling_fields=("siblings",), key_fields=("oldKey", "key"), key_bits=n_levels,
                          bit_fields=("fnc", "isOld0", "enabled")))
    return out


RTX_BITS = ("onChain", "newAccount", "isOld0_1", "isOld0_2", "newExit", "toBjjSign", "sign1", "sign2")
RTX_KEYS = ("fromIdx", "toIdx", "auxFromIdx", "auxToIdx", "oldKey1", "oldKey2")


def rollup_tx_cases(n, n_levels, max_fee, seed):
    """standalone RollupTx inputs of a synthetic batch (creates, transfers, exits), mutated"""
    from circuits_amd import builder as B
    rng = random.Random(seed)
    bb = B.synthetic_batch(40, n_levels, 6, max_fee, n_accounts=12, exits=3, seed=seed)
    valid = [bb.get_single_tx_input(i)[0] for i in range(bb.nTx)]
    return [mutate(rng, valid[rng.randrange(len(valid))], sibling_fields=("siblings1", "siblings2"), key_fields=RTX_KEYS, key_bits=n_levels, bit_fields=RTX_BITS) for _ in range(n)]


def withdraw_cases(n, n_levels, seed):
    from circuits_amd import builder as B
    rng = random.Random(seed)
    fx = B.ExitTreeFixture(96, seed=seed)
    idxs = sorted(fx.exit_leaves)
    valid = [B.withdraw_input(fx, i, n_levels)[0] for i in idxs]
    return [mutate(rng, valid[rng.randrange(len(valid))], sibling_fields=("siblingsState",), key_fields=("idx",), key_bits=n_levels, bit_fields=("sign",)) for _ in range(n)]


def rollup_main_cases(n, shape, seed):
    """whole RollupMain input objects (several synthetic batches), mutated anywhere: transactions, fee slots, intermediate signals"""
    from circuits_amd import builder as B
    rng = random.Random(seed)
    nTx, L, m1, F = shape
    valid = [B.synthetic_batch(nTx, L, m1, F, n_accounts=4 + b, exits=min(1, nTx - m1 - 1) if nTx - m1 > 1 else 0, seed=seed + b).get_input() for b in range(6)]
    sib = [("siblings1", (i,)) for i in range(nTx)] + [("siblings2", (i,)) for i in range(nTx)] + [("siblings3", (j,)) for j in range(F)]
    bits = [(f, (i,)) for f in ("onChain", "newAccount", "isOld0_1", "isOld0_2", "newExit") for i in range(nTx)] + [("fromBjjCompressed", (i, rng.randrange(256))) for i in range(nTx)]
    keys = [(f, (i,)) for f in ("auxFromIdx", "auxToIdx", "oldKey1", "oldKey2") for i in range(nTx)]
    return [mutate(rng, valid[rng.randrange(len(valid))], sibling_fields=sib, key_fields=keys, key_bits=L, bit_fields=bits) for _ in range(n)]


# ---- HashInputs as main component ------------------------------------------------------------------------------------------------
L1_FULL_BITS = 2 * 48 + 32 + 40 + 40 + 256 + 160   # bits of one L1TxsFullData slot (reference src/hash-inputs.circom)


def hash_inputs_valid(rng, shape, fill=None):
    """one valid input object of HashInputs(nLevels, nTx, maxL1Tx, maxFeeTx) as main component, shape = (nTx, nLevels, maxL1Tx,
    maxFeeTx): the two data-availability arrays as random bits (fill = 0 / 1: all zero / all one), every scalar random inside its range"""
    nTx, L, m1, F = shape

    def bits(n):
        if fill is not None:
            return [fill] * n
        return [int(c) for c in bin(rng.getrandbits(n) | (1 << n))[3:]] if n else []
    return {"oldLastIdx": rng.randrange(1 << L), "newLastIdx": rng.randrange(1 << L), "oldStateRoot": rng.randrange(P), "newStateRoot": rng.randrange(P),
            "newExitRoot": rng.randrange(P), "L1TxsFullData": bits(m1 * L1_FULL_BITS), "L1L2TxsData": bits(nTx * (2 * L + 48)),
            "feeTxsData": [rng.randrange(1 << L) for _ in range(F)], "globalChainID": rng.randrange(1 << 16), "currentNumBatch": rng.randrange(1 << 32)}


def hash_inputs_checked(d, shape):
    """the range-checked elements of a HashInputs input object in the template's evaluation order (reference src/hash-inputs.circom):
    [(name, path, value, bits of its Num2Bits, padded)] -- padded: the bits from nLevels up to 48 must be zero as well"""
    F = shape[3]
    return ([("oldLastIdx", (), d["oldLastIdx"], 48, True), ("newLastIdx", (), d["newLastIdx"], 48, True)] +
            [("feeTxsData", (j,), d["feeTxsData"][j], 48, True) for j in range(F)] +
            [("globalChainID", (), d["globalChainID"], 16, False), ("currentNumBatch", (), d["currentNumBatch"], 32, False)])


def hash_inputs_lowest_failures(d, shape):
    """how many elements of an input object fail the constraint that is the object's first failure -- "Num2Bits sum" (value >= 2^n)
    where any element fails it, "index padding" (a bit between nLevels and 48 in the value's low 48 bits) otherwise. 0: valid;
    2 or more: a double failure with equal keys, whose reported operands are those of the first such element."""
    L = shape[1]
    n2b = pad = 0
    for _, _, v, n, padded in hash_inputs_checked(d, shape):
        v %= P
        n2b += v >> n != 0
        pad += padded and ((v & ((1 << 48) - 1)) >> L) != 0
    return n2b or pad


def hash_inputs_cases(n, shape, seed, sample=16, p_scalar=0.12, p_double=0.4):
    """standalone HashInputs inputs for the differential fuzz: valid random inputs (hash_inputs_valid), then
      * `mutate` over `sample` random positions of each of the two bit arrays as bit_fields (non-bits -- 2, r - 1, random -- of which the
        hash takes the least significant bit; walking all 10^4 bits of every case for one to four edits would be the generator's whole cost),
      * every scalar and fee index replaced by `garbage(..., key_bits=nLevels)` with probability p_scalar,
      * with probability p_double a deliberate double failure: two or three of {oldLastIdx, newLastIdx, several feeTxsData[j],
        globalChainID, currentNumBatch} out of range at once -- all >= 2^n ("Num2Bits sum"), all below 2^48 with bits at or above nLevels
        ("index padding", a different number of bits each so that the operands tell the elements apart), the earlier ones padding and the
        later ones Num2Bits, or a random mix. The reference reports the first element in its evaluation order among equal keys."""
    rng = random.Random(seed)
    nTx, L, m1, F = shape
    out = []
    for _ in range(n):
        d = hash_inputs_valid(rng, shape, fill=(None, None, None, 0, 1)[rng.randrange(5)])
        for name in ("L1TxsFullData", "L1L2TxsData"):
            pos = rng.sample(range(len(d[name])), min(sample, len(d[name])))
            proxy = mutate(rng, {name: [d[name][q] for q in pos]}, bit_fields=[(name, (k,)) for k in range(len(pos))])
            for k, q in enumerate(pos):
                d[name][q] = proxy[name][k]
        checked = hash_inputs_checked(d, shape)
        for name, path, v, _, _ in checked:
            if rng.random() < p_scalar:
                _set(d, name, path, garbage(rng, v, key_bits=L))
        for name in ("oldStateRoot", "newStateRoot", "newExitRoot"):
            if rng.random() < p_scalar:
                d[name] = garbage(rng, d[name])
        if rng.random() < p_double:
            idx = [c for c in checked if c[4]]
            mode = rng.randrange(4) if L < 48 else 0
            pool = idx if mode == 1 else checked
            chosen = sorted(rng.sample(range(len(pool)), min(len(pool), rng.randrange(2, 4))))
            for k, c in enumerate(chosen):
                name, path, v, nb, padded = pool[c]
                v = _get(d, name, path) % (1 << nb)
                if mode == 0:
                    n2b = True
                elif mode == 1:
                    n2b = False
                elif mode == 2:   # the earlier elements fail the padding, the last one Num2Bits
                    n2b = k == len(chosen) - 1 or not padded
                else:
                    n2b = not padded or rng.random() < 0.5
                if n2b:
                    v = (v + (1 << rng.randrange(nb, 253))) % P if rng.random() < 0.7 else rng.randrange(1 << nb, P)
                else:
                    v &= (1 << L) - 1
                    for b in rng.sample(range(L, 48), min(48 - L, k + 1)):
                        v |= 1 << b
                _set(d, name, path, v)
        out.append(d)
    return out


# ---- signature edges -------------------------------------------------------------------------------------------------------------
# Baby Jubjub (circomlib babyjub.circom): a x^2 + y^2 = 1 + d x^2 y^2 over F_P, group order 8 l, B8 of order l.
BJJ_A, BJJ_D = 168700, 168696


def bjj_add(p, q):
    (x1, y1), (x2, y2) = p, q
    t = BJJ_D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + y1 * x2) * pow(1 + t, -1, P) % P, (y1 * y2 - BJJ_A * x1 * x2) * pow(1 - t, -1, P) % P)


def bjj_mul(p, k):
    r = (0, 1)
    while k:
        if k & 1:
            r = bjj_add(r, p)
        p = bjj_add(p, p)
        k >>= 1
    return r


def bjj_on_curve(p):
    x2, y2 = p[0] * p[0] % P, p[1] * p[1] % P
    return (BJJ_A * x2 + y2 - 1 - BJJ_D * x2 * y2) % P == 0


def fr_sqrt(n):
    """a square root of n mod P (Tonelli-Shanks: P - 1 = 2^28 * odd), None for a non-residue"""
    n %= P
    if n == 0:
        return 0
    if pow(n, (P - 1) // 2, P) != 1:
        return None
    q, s = P - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    z = 2
    while pow(z, (P - 1) // 2, P) == 1:
        z += 1
    m, c, t, r = s, pow(z, q, P), pow(n, q, P), pow(n, (q + 1) // 2, P)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % P, i + 1
        b = pow(c, 1 << (m - i - 1), P)
        m, c, t, r = i, b * b % P, t * b * b % P, r * b % P
    return r


def bjj_x_of(y):
    """an x with (x, y) on the curve, None where there is none (an `ay` AySign2Ax finds no point for)"""
    y2 = y * y % P
    den = (BJJ_A - BJJ_D * y2) % P
    return None if den == 0 else fr_sqrt((1 - y2) * pow(den, -1, P))


_ORDER8 = []


def bjj_order8_point():
    """a point of order exactly 8: l times a curve point outside the subgroup, the first small y that gives one"""
    from circuits_amd.builder import SUBORDER
    y = 2
    while not _ORDER8:
        x = bjj_x_of(y)
        if x is not None:
            q = bjj_mul((x, y), SUBORDER)
            if bjj_mul(q, 4) != (0, 1):
                _ORDER8.append(q)
        y += 1
    return _ORDER8[0]


def signature_edge_cases(valid_l2_input, other_l2_input=None, l1_create_input=None):
    """[(label, input object)]: one valid signed L2 RollupTx input with its signature inputs moved to the edges of
    EdDSAPoseidonVerifier (circomlib eddsaposeidon.circom) and AySign2Ax (reference src/lib/utils-bjj.circom) --

      s          0, 1, l - 1, l, l + 1, s + k l while < 2^253 (the same point S * B8: only CompConstant rejects it, the malleability
                 guard), 2^253 - 1, 2^253 and s + 2^253 (Num2Bits(253) fails), P - 1
      (r8x, r8y) the neutral point (0, 1), the order-2 point (0, P - 1), (0, 0), the order-4 points (+-1 / sqrt(a), 0), -R8, the R8 of
                 another transaction (other_l2_input; 2 * R8 without one), an off-curve point
      ay1, sign1 ay1 = 0, 1, P - 1, 2 (no x: (1 - ay^2) / (a - d ay^2) is a non-residue), 5 (a point outside the subgroup), sign1 flipped, sign1 = 2, a key of order 8

    -- each of them also with fromIdx = 0 and with onChain = 1 (verifier disabled: the witness is still written, the verifier reports
    nothing), and, with l1_create_input (an account-creating L1 transaction), the key edges in its fromBjjCompressed bits. The first
    entry is the unmodified input. Labels are unique."""
    from circuits_amd.builder import SUBORDER as l
    base = {k: _copy(v) for k, v in valid_l2_input.items()}
    assert not base["onChain"] and base["fromIdx"], "needs a signed L2 transaction"
    s, r8 = base["s"], (base["r8x"], base["r8y"])
    inv_sqrt_a = pow(fr_sqrt(BJJ_A), -1, P)
    o8 = bjj_order8_point()
    edges = [("s=0", {"s": 0}), ("s=1", {"s": 1}), ("s=l-1", {"s": l - 1}), ("s=l", {"s": l}), ("s=l+1", {"s": l + 1})]
    k = 1
    while s + k * l < (1 << 253):
        edges.append(("s=s+%dl" % k, {"s": s + k * l}))
        k += 1
    edges += [("s=2^253-1", {"s": (1 << 253) - 1}), ("s=2^253", {"s": 1 << 253}), ("s=s+2^253", {"s": s + (1 << 253)}), ("s=p-1", {"s": P - 1})]
    other = (other_l2_input["r8x"], other_l2_input["r8y"]) if other_l2_input is not None else bjj_add(r8, r8)
    assert other != r8
    off = (r8[0] + 1) % P, r8[1]
    assert not bjj_on_curve(off) and bjj_on_curve((inv_sqrt_a, 0)) and bjj_mul((inv_sqrt_a, 0), 2) == (0, P - 1)
    for label, (x, y) in (("r8=(0,1)", (0, 1)), ("r8=(0,p-1)", (0, P - 1)), ("r8=(0,0)", (0, 0)), ("r8=(1/sqrt(a),0)", (inv_sqrt_a, 0)),
                          ("r8=(-1/sqrt(a),0)", (P - inv_sqrt_a, 0)), ("r8=-R8", (P - r8[0], r8[1])), ("r8=other", other), ("r8=off-curve", off)):
        edges.append((label, {"r8x": x, "r8y": y}))
    assert bjj_x_of(2) is None and bjj_x_of(5) is not None
    keys = [("ay1=0", {"ay1": 0}), ("ay1=1", {"ay1": 1}), ("ay1=p-1", {"ay1": P - 1}), ("ay1=2", {"ay1": 2}), ("ay1=5", {"ay1": 5}), ("sign1^1", {"sign1": 1 - base["sign1"]}),
            ("sign1=2", {"sign1": 2}), ("key=order8", {"ay1": o8[1], "sign1": 1 if o8[0] > (P - 1) // 2 else 0})]
    edges += keys
    out = [("valid", base)]
    for label, edit in edges:
        for gate, extra in (("", {}), (" & fromIdx=0", {"fromIdx": 0}), (" & onChain=1", {"onChain": 1})):
            d = {k: _copy(v) for k, v in base.items()}
            d.update(edit)
            d.update(extra)
            out.append((label + gate, d))
    if l1_create_input is not None:
        c = l1_create_input
        assert c["onChain"] and c["newAccount"], "needs an account-creating L1 transaction"
        for label, edit in keys:
            ay = edit.get("ay1", sum(b << i for i, b in enumerate(c["fromBjjCompressed"][:255])))
            sign = edit.get("sign1", c["fromBjjCompressed"][255])
            d = {k: _copy(v) for k, v in c.items()}
            d["fromBjjCompressed"] = [(ay >> i) & 1 for i in range(255)] + [sign]
            out.append(("create," + label.replace("ay1", "ay").replace("sign1", "sign"), d))
    assert len({lb for lb, _ in out}) == len(out)
    return out


def rollup_main_signature_edges(main_input, labels=None):
    """[(label, input object)]: a valid RollupMain input in which the first signed L2 transaction carries one of signature_edge_cases'
    edges (those of s, r8x, r8y, ay1, sign1; `labels` selects some). RollupMain takes fromIdx from txCompressedData: the two gated
    variants of every edge belong to the standalone RollupTx and are left out here."""
    n_tx = len(main_input["onChain"])
    tx = next(i for i in range(n_tx) if not main_input["onChain"][i] and (main_input["txCompressedData"][i] >> 48) & ((1 << 48) - 1))
    fields = ("s", "r8x", "r8y", "ay1", "sign1")
    single = {f: main_input[f][tx] for f in fields}
    single.update(onChain=0, fromIdx=(main_input["txCompressedData"][tx] >> 48) & ((1 << 48) - 1))
    other = next(({f: main_input[f][i] for f in fields} for i in range(tx + 1, n_tx) if not main_input["onChain"][i] and main_input["r8x"][i] and
                  main_input["r8x"][i] != single["r8x"]), None)
    out = []
    for label, e in signature_edge_cases(single, other)[1:]:
        if " & " in label or (labels is not None and label not in labels):
            continue
        d = {k: _copy(v) for k, v in main_input.items()}
        for f in fields:
            d[f][tx] = e[f]
        out.append(("tx %d: %s" % (tx, label), d))
    assert labels is None or len(out) == len(labels)
    return out


def signature_form_tx_cases(n_levels, max_fee, seed, n_bases, n_garbage):
    """(labels, cases) of standalone RollupTx inputs for the launches that compare the forms of the signature kernels: the transactions
    of a synthetic batch as they are, signature_edge_cases of `n_bases` of its signed L2 transactions (another transaction's R8 and an
    account-creating L1 transaction beside each), `n_garbage` rollup_tx_cases"""
    from circuits_amd import builder as B
    bb = B.synthetic_batch(40, n_levels, 6, max_fee, n_accounts=12, exits=3, seed=seed)
    ins = [bb.get_single_tx_input(i)[0] for i in range(bb.nTx)]
    l2 = [i for i, d in enumerate(ins) if not d["onChain"] and d["fromIdx"]]
    l1c = [i for i, d in enumerate(ins) if d["onChain"] and d["newAccount"]]
    assert len(l2) >= n_bases and l1c
    out = [("valid tx %d" % i, d) for i, d in enumerate(ins)]
    for j, i in enumerate(l2[:n_bases]):
        edges = signature_edge_cases(ins[i], ins[l2[(j + 1) % len(l2)]], ins[l1c[j]] if j < len(l1c) else None)
        out += [("tx %d: %s" % (i, lb), d) for lb, d in edges[1:]]
    out += [("garbage %d" % k, d) for k, d in enumerate(rollup_tx_cases(n_garbage, n_levels, max_fee, seed + 1))]
    return [lb for lb, _ in out], [d for _, d in out]


def place_replicas(g, cases, which):
    """Inputs of a replicated launch: instance k of the product context gets cases[which[k]]. Every distinct case is uploaded once, to
    the first instance that holds it, and copied on the device to the others (copy_instance_inputs)."""
    home = {}
    for k, d in enumerate(which):
        if d not in home:
            home[d] = k
            g.set_inputs(cases[d], instance=k)
    for k, d in enumerate(which):
        if home[d] != k:
            g.copy_instance_inputs(home[d], k)


def lane_units(n, per_lane):
    """The signatures of every lane of the throughput kernels (eddsa_kernels.hip k_eddsa_seg<G> / k_eddsa_fix<G> `mk_io`): lane li of
    nl = ceil(n / G) lanes holds units li, li + nl, li + 2 nl, ... -- slot g of every lane is the g-th nl-long stretch of the launch,
    the units of a lane are NOT consecutive -- and a slot past the end (ragged launch) repeats the lane's first unit. Returns
    [[unit of slot 0, ...] per lane], padding slots left out."""
    nl = (n + per_lane - 1) // per_lane
    return [[li + g * nl for g in range(per_lane) if li + g * nl < n] for li in range(nl)]


# ---- the twelve other mains: the gadget templates, AySign2Ax, HashState, DecodeTx, FeeTx as `component main` ----------------------
# Inputs outside the ranges the enclosing RollupTx feeds them (tests/test_standalone_fuzz*.py). Every list is built by _assemble: the
# named edges first, one per instance, then seeded draws; compute-fee and balance-updater lay whole wavefronts out as well (WAVE = the
# workgroup of k_gadget<..>, one wavefront).
WAVE = 64
HALF = (P - 1) // 2
SEL_PALETTE = (0, 1, 2, P - 1)   # what a selector or "bit" is set to, beside a random field element
FEE_SEL_EDGES = (0, 191, 192, 207, 208, 255, 256, 256 + 7, 256 + 192, P - 1)
AMOUNT_EDGES = (0, (1 << 128) - 1, 1 << 128, (1 << 192) - 1, 1 << 192, P - 1)
BALANCE_EDGES = (0, (1 << 192) - 1, 1 << 192, P - 1)


def is_bit(v):
    return v % P in (0, 1)


def _sel(rng):
    """a selector input: one of SEL_PALETTE or a random field element"""
    k = rng.randrange(len(SEL_PALETTE) + 1)
    return SEL_PALETTE[k] if k < len(SEL_PALETTE) else rng.randrange(2, P)


def _assemble(n, edges, draw):
    """n cases: the named edges in order (all of them where n >= len(edges)), then draw() until the list is full"""
    out = [{k: _copy(v) for k, v in e.items()} for e in edges[:n]]
    while len(out) < n:
        out.append(draw())
    return out


def _gadget_bases(template):
    """the valid inputs tests/test_gadget_mains.py holds for one gadget main (the reference's literal vectors)"""
    import test_gadget_mains as G
    return [it[0] for c in G.all_cases() if c.template == template for it in c.items if not isinstance(it[1], str)]


def decode_float_cases(n, seed):
    """`in` = mantissa | exponent << 35 at exponent 0 / 31 and mantissa 0 / 2^35 - 1, 2^40 - 1, 2^40, 2^40 + 1, P - 1; then 40-bit
    values, half of them through `garbage` (mostly above 40 bits: Num2Bits(40) fails, the decoder reads the low bits)"""
    rng = random.Random(seed)
    m35 = (1 << 35) - 1
    edges = [{"in": m | (e << 35)} for e in (0, 31) for m in (0, m35, 1, 0x400000000)]
    edges += [{"in": v} for v in ((1 << 40) - 1, 1 << 40, (1 << 40) + 1, P - 1, P - 2, (1 << 41) - 1, (1 << 253) + 5, HALF, HALF + 1)]

    def draw():
        v = rng.getrandbits(40)
        return {"in": garbage(rng, v) if rng.random() < 0.5 else v}
    return _assemble(n, edges, draw)


def _fee_triplet(rng, i):
    """(feeSel, amount) walking the named edges in coprime strides, so that every value and many pairs of them occur in 64 lanes"""
    fs = FEE_SEL_EDGES + (rng.randrange(192), rng.randrange(256), rng.randrange(P))
    am = AMOUNT_EDGES + (rng.getrandbits(100), 10 ** 18, rng.randrange(P), rng.getrandbits(60))
    return fs[i % len(fs)], am[i % len(am)]


def apply_fee_of(template, d):
    """the selector ComputeFee sees: its input, or BalanceUpdater's (1 - onChain) * (1 - nop)"""
    return d["applyFee"] % P if template == "compute-fee" else (1 - d["onChain"]) * (1 - d["nop"]) % P


def compute_fee_cases(n, seed):
    """ComputeFee with garbage selectors. Wavefront by wavefront (64 instances, the kernel's fast path is chosen per wavefront):
      0   the named edges: feeSel in FEE_SEL_EDGES, amount in AMOUNT_EDGES, applyFee in {0, 1, 2, P - 1, random}, mixed
      1   applyFee a bit on every lane, feeSel and amount garbage (the product-free path with out-of-range selectors)
      2-4 exactly one non-bit applyFee, at lane 0, 17, 63 (the general path running over bit lanes)
      5   no applyFee a bit
      6.. inputs in range (feeSel < 192, amount < 2^100: accepted), one in four of them through `garbage`, applyFee a bit on most lanes"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        w, lane = divmod(i, WAVE)
        sel, amount = _fee_triplet(rng, i + 3 * w)
        if w == 0:
            ap = (0, 1, 2, P - 1, rng.randrange(2, P))[lane % 5]
        elif w == 1:
            ap = rng.getrandbits(1)
        elif w in (2, 3, 4):
            ap = rng.getrandbits(1)
            if lane == (0, 17, 63)[w - 2]:
                ap = (2, P - 1, rng.randrange(2, P))[w - 2]
        elif w == 5:
            ap = (2, P - 1, rng.randrange(2, P), 7)[lane % 4]
        else:
            ap = rng.getrandbits(1) if rng.random() < 0.9 else _sel(rng)
        if w >= 6 or (w >= 1 and lane % 3 == 0):   # a share of every wavefront stays in range: accepted instances beside rejected ones
            sel, amount = rng.randrange(192), rng.getrandbits(100)
            if w >= 6 and rng.random() < 0.25:
                sel, amount = garbage(rng, sel), garbage(rng, amount)
        out.append({"feeSel": sel, "amount": amount, "applyFee": ap})
    return out


def balance_updater_cases(n, seed):
    """BalanceUpdater with garbage everywhere; the wavefronts of compute_fee_cases by the EFFECTIVE selector (1 - onChain) * (1 - nop)
    (onChain = nop = 2 gives 1: a bit made of two non-bits), balances and loads at BALANCE_EDGES so that the 193-bit sum
    2^192 + balance + load - amount - fee wraps mod P, the two nullifiers in {0, 1, 2, P - 1, random}"""
    rng = random.Random(seed)
    nonbit_pairs = ((2, 0), (0, 2), (P - 1, 0), (0, P - 1), (2, P - 1))
    out = []
    for i in range(n):
        w, lane = divmod(i, WAVE)
        sel, amount = _fee_triplet(rng, i + 3 * w)
        on, nop = rng.getrandbits(1), rng.getrandbits(1)
        be = BALANCE_EDGES + (rng.getrandbits(120), (1 << 100) + rng.getrandbits(100), rng.randrange(P))
        d = {"oldStBalanceSender": be[i % len(be)], "oldStBalanceReceiver": be[(i // 2) % len(be)], "amount": amount,
             "loadAmount": be[(i // 3) % len(be)], "feeSelector": sel, "onChain": on, "nop": nop,
             "nullifyLoadAmount": (0, 1, 2, P - 1, rng.randrange(P))[i % 5], "nullifyAmount": (0, 1, 2, P - 1, rng.randrange(P))[(i // 5) % 5]}
        if w == 0:
            d["onChain"], d["nop"] = (0, 1, 2, P - 1, rng.randrange(2, P))[lane % 5], (0, 1, 2, P - 1, rng.randrange(2, P))[(lane // 5) % 5]
        elif w == 1 and lane % 16 == 5:
            d["onChain"] = d["nop"] = 2
        elif w in (2, 3, 4) and lane == (0, 17, 63)[w - 2]:
            d["onChain"], d["nop"] = nonbit_pairs[w - 2]
        elif w == 5:
            d["onChain"], d["nop"] = nonbit_pairs[lane % len(nonbit_pairs)] if lane % 3 else (rng.randrange(3, P - 1), 0)
        elif w >= 6 and rng.random() < 0.1:
            d["onChain"], d["nop"] = _sel(rng), _sel(rng)
        if w >= 6 or (w >= 1 and lane % 3 == 0):   # in range: what RollupTx feeds (accepted), a quarter of the late ones through `garbage`
            d.update(oldStBalanceSender=(1 << 100) + rng.getrandbits(100), oldStBalanceReceiver=rng.getrandbits(120), amount=rng.getrandbits(90),
                     loadAmount=rng.getrandbits(90) if is_bit(d["onChain"]) and d["onChain"] else 0, feeSelector=rng.randrange(192),
                     nullifyLoadAmount=rng.getrandbits(1), nullifyAmount=rng.getrandbits(1))
            if w >= 6 and rng.random() < 0.25:
                f = rng.choice(("oldStBalanceSender", "oldStBalanceReceiver", "amount", "loadAmount", "feeSelector", "nullifyLoadAmount", "nullifyAmount"))
                d[f] = garbage(rng, d[f])
        out.append(d)
    return out


def fee_accumulator_cases(n, max_fee, seed):
    """FeeAccumulator(max_fee): the token in no slot, in slot 0, in the last slot, in every slot; tokenID and plan entries that differ
    by P - 1 (unequal: IsEqual works in the field, x and x + P - 1 = x - 1 are different elements); fee2Charge and accumulators at
    P - 1 (the sum wraps); then random plans with field-sized values. No constraint of this main can fail."""
    rng = random.Random(seed)
    F = max_fee
    acc = [1000 + j for j in range(F)]
    plan = [100 + j for j in range(F)]
    edges = [{"tokenID": 999, "fee2Charge": 7, "feePlanTokenID": plan, "accFeeIn": acc},
             {"tokenID": 100, "fee2Charge": 7, "feePlanTokenID": plan, "accFeeIn": acc},
             {"tokenID": 100 + F - 1, "fee2Charge": 7, "feePlanTokenID": plan, "accFeeIn": acc},
             {"tokenID": 5, "fee2Charge": 7, "feePlanTokenID": [5] * F, "accFeeIn": acc},
             {"tokenID": 5, "fee2Charge": 7, "feePlanTokenID": [(5 + P - 1) % P] * F, "accFeeIn": acc},
             {"tokenID": 0, "fee2Charge": 7, "feePlanTokenID": [P - 1] * (F - 1) + [0], "accFeeIn": acc},
             {"tokenID": P - 1, "fee2Charge": 1, "feePlanTokenID": [0] * (F - 1) + [P - 1], "accFeeIn": acc},
             {"tokenID": 100, "fee2Charge": P - 1, "feePlanTokenID": plan, "accFeeIn": [P - 1] * F},
             {"tokenID": 100 + F - 1, "fee2Charge": P - 1, "feePlanTokenID": plan, "accFeeIn": [P - 1] * F},
             {"tokenID": 101 % P, "fee2Charge": 1, "feePlanTokenID": plan, "accFeeIn": [P - 1] * F},
             {"tokenID": 0, "fee2Charge": 0, "feePlanTokenID": [0] * F, "accFeeIn": [0] * F}]

    def draw():
        toks = [rng.choice((rng.randrange(24), rng.randrange(P), P - 1 - rng.randrange(4))) for _ in range(F)]
        r = rng.random()
        token = rng.choice(toks) if r < 0.6 else (rng.choice(toks) + P - 1) % P if r < 0.75 else rng.randrange(P)
        big = rng.random() < 0.6
        return {"tokenID": token, "fee2Charge": rng.choice((P - 1, rng.randrange(P), 1 << 192)) if big else rng.getrandbits(100), "feePlanTokenID": toks,
                "accFeeIn": [rng.choice((P - 1, rng.randrange(P), (1 << 192) - 1, 1 << 192)) if big and rng.random() < 0.5 else rng.getrandbits(120) for _ in range(F)]}
    return _assemble(n, edges, draw)


STATES_BITS = ("newExit", "newAccount", "onChain")
STATES_FIELDS = ("fromIdx", "toIdx", "toEthAddr", "auxFromIdx", "auxToIdx", "amount", "newExit", "loadAmount", "newAccount", "onChain", "fromEthAddr",
                 "ethAddr1", "tokenID", "tokenID1", "tokenID2")


def rollup_tx_states_cases(n, seed):
    """RollupTxStates: every bit input non-boolean in turn; toIdx in {0, 1, 2, 255, 256}; toEthAddr = 2^160 - 1 and +- 1; the three
    token ids and the two addresses equal or unequal in every combination; fromIdx = auxFromIdx = 0; L2 rows with a load amount AND
    newAccount (both L2 checks violated at once: the first in the template's order is the one reported); then the reference's
    vectors mutated"""
    rng = random.Random(seed)
    bases = _gadget_bases("rollup-tx-states")
    l1 = next(b for b in bases if b["onChain"] == 1 and not b["newAccount"] and b["fromIdx"])
    l2 = next(b for b in bases if b["onChain"] == 0 and b["fromIdx"])
    edges = []
    for f in STATES_BITS:
        for v in (2, P - 1, rng.randrange(2, P)):
            for b in (l1, l2):
                edges.append(dict(b, **{f: v}))
    for v in (0, 1, 2, 255, 256):
        edges += [dict(l1, toIdx=v), dict(l2, toIdx=v)]
    for v in ((1 << 160) - 2, (1 << 160) - 1, 1 << 160):
        edges += [dict(l2, toIdx=0, toEthAddr=v), dict(l1, toEthAddr=v)]
    for t1 in (0, 1):
        for t2 in (0, 1):
            for e in (0, 1):
                for amt in (0, 7):
                    edges.append(dict(l1, tokenID=3, tokenID1=3 + t1, tokenID2=3 + t2, fromEthAddr=0x1234, ethAddr1=0x1234 + e, amount=amt, loadAmount=5))
    edges += [dict(l1, fromIdx=0, auxFromIdx=0), dict(l2, fromIdx=0, auxFromIdx=0), dict(l1, fromIdx=0, auxFromIdx=0, newAccount=1)]
    # both L2 checks at once, and each alone
    edges += [dict(l2, loadAmount=v, newAccount=a) for v, a in ((5, 1), (P - 1, 1), (5, 2), (1 << 200, P - 1), (5, 0), (0, 1))]
    edges += [dict(l2, loadAmount=5, newAccount=1, onChain=v) for v in (2, P - 1)]

    def draw():
        b = rng.choice(bases)
        r = rng.random()
        if r < 0.12:   # an L2 row that violates both of its checks
            return dict(b, onChain=rng.choice((0, 0, 2, P - 1)), loadAmount=rng.choice((1, rng.randrange(1, P))), newAccount=rng.choice((1, 1, 2, rng.randrange(1, P))))
        return mutate(rng, b, key_fields=("fromIdx", "toIdx", "auxFromIdx", "auxToIdx"), key_bits=20, bit_fields=STATES_BITS)
    return _assemble(n, edges, draw)


RQ_KINDS = ("TxCompressedDataV2", "ToEthAddr", "ToBjjAy")


def _rq_selected(d, kind, off3):
    return ([0] + list(d["future" + kind]) + list(d["past" + kind])[::-1])[off3]


def rq_tx_verifier_cases(n, seed):
    """RqTxVerifier: rqTxOffset 0..7, 8, 9, 8 + k, P - 1 (Num2Bits(3) fails, the multiplexers take the low three bits); for each, the
    requested values right in the selected slot, wrong there and right in another slot, and one, two or all three of the comparisons
    wrong at once"""
    rng = random.Random(seed)

    def fresh(off):
        d = {"rqTxOffset": off}
        for k in RQ_KINDS:
            d["future" + k] = [rng.randrange(1, P) for _ in range(3)]
            d["past" + k] = [rng.randrange(1, P) for _ in range(4)]
        for k in RQ_KINDS:
            d["rq" + k] = _rq_selected(d, k, off % P & 7)
        return d

    def spoil(d, kinds, how):
        for k in kinds:
            off3 = d["rqTxOffset"] % P & 7
            if how == 0:
                d["rq" + k] = _rq_selected(d, k, (off3 + 1 + rng.randrange(7)) & 7)   # the value of a slot that is not selected
            elif how == 1:
                d["rq" + k] = (d["rq" + k] + rng.choice((1, P - 1))) % P
            else:
                d["rq" + k] = rng.randrange(P)
        return d
    offsets = list(range(8)) + [8, 9, 8 + 5, 8 + 7, 16 + 3, (1 << 3) + (1 << 100), P - 1, P - 8]
    edges = [fresh(off) for off in offsets]
    for j, off in enumerate(offsets):
        edges.append(spoil(fresh(off), [RQ_KINDS[j % 3]], j % 3))
    for off in (1, 3, 4, 7, 9, P - 1):
        for kinds in ((0, 1), (0, 2), (1, 2), (0, 1, 2)):
            edges.append(spoil(fresh(off), [RQ_KINDS[k] for k in kinds], rng.randrange(3)))
    edges.append({k: (0 if not isinstance(v, list) else [0] * len(v)) for k, v in fresh(0).items()})

    def draw():
        r = rng.random()
        off = rng.randrange(8) if r < 0.7 else rng.choice((8, 9, 8 + rng.randrange(8), P - 1, rng.randrange(P), 1 << rng.randrange(3, 253)))
        d = fresh(off)
        r = rng.random()
        if r < 0.45:
            return d
        return spoil(d, rng.sample(RQ_KINDS, rng.choice((1, 1, 2, 2, 3))), rng.randrange(3))
    return _assemble(n, edges, draw)


def mux256_cases(n, seed):
    """Mux256: each of the eight selectors in {0, 1, 2, P - 1, random} in turn over a base selection, all eight of them garbage,
    field-sized inputs. No constraint of this main can fail."""
    rng = random.Random(seed)
    big = [rng.randrange(P) for _ in range(256)]
    small = list(range(256))
    edges = []
    for pos in range(8):
        for v in (0, 1, 2, P - 1, rng.randrange(2, P)):
            base = rng.randrange(256)
            s = [(base >> b) & 1 for b in range(8)]
            s[pos] = v
            edges.append({"s": s, "in": big if (pos + v) % 2 else small})
    edges += [{"s": [v] * 8, "in": big} for v in (0, 1, 2, P - 1)]
    edges.append({"s": [1] * 8, "in": [P - 1] * 256})

    def draw():
        r = rng.random()
        s = [rng.getrandbits(1) for _ in range(8)]
        if r < 0.7:
            for pos in rng.sample(range(8), rng.randrange(1, 9)):
                s[pos] = _sel(rng)
        ins = [rng.randrange(P) for _ in range(256)] if rng.random() < 0.5 else rng.choice((big, small))
        return {"s": s, "in": ins}
    return _assemble(n, edges, draw)


def bits_compressed_cases(n, seed):
    """BitsCompressed2AySign: "bits" that are 2, P - 1 or random at single positions (0, 1, 127, 253, 254, 255) and everywhere; all
    ones (ay = 2^254 - 1 >= P before the reduction); bit 255 (the sign) non-boolean. No constraint of this main can fail."""
    rng = random.Random(seed)
    from circuits_amd import builder as B
    comp = B.BASE8[1] | (1 << 255)
    base = [(comp >> i) & 1 for i in range(256)]
    edges = [{"bjjCompressed": list(base)}, {"bjjCompressed": [1] * 256}, {"bjjCompressed": [1] * 254 + [0, 0]}, {"bjjCompressed": [0] * 256}]
    for pos in (0, 1, 127, 253, 254, 255):
        for v in (2, P - 1, rng.randrange(2, P)):
            b = list(base)
            b[pos] = v
            edges.append({"bjjCompressed": b})
    edges += [{"bjjCompressed": [v] * 256} for v in (2, P - 1)]
    edges.append({"bjjCompressed": [rng.randrange(P) for _ in range(256)]})

    def draw():
        v = rng.getrandbits(256)
        b = [(v >> i) & 1 for i in range(256)]
        if rng.random() < 0.75:
            for pos in rng.sample(range(256), rng.choice((1, 2, 8, 256))):
                b[pos] = _sel(rng)
        return {"bjjCompressed": b}
    return _assemble(n, edges, draw)


def ay_sign_2_ax_ays(seed):
    """(with, without): the `ay` of the named edges that have a point on the curve, and those that have none (bjj_x_of)"""
    from circuits_amd import builder as B
    rng = random.Random(seed)
    named = [0, 1, P - 1, 2, P - 2, B.BASE8[1], bjj_order8_point()[1], 1 << 253, (1 << 253) - 1, (1 << 253) + 1, HALF, HALF + 1]
    named += [B.Account(200 + i).ay for i in range(4)]
    have = [y for y in named if bjj_x_of(y) is not None]
    none = [y for y in named if bjj_x_of(y) is None]
    while len(have) < 10 or len(none) < 10:
        y = rng.randrange(P)
        (have if bjj_x_of(y) is not None else none).append(y)
    return have, none


def ay_sign_2_ax_cases(n, seed):
    """AySign2Ax: ay in {0, 1, P - 1, 2, P - 2} (for +-1 the root is x = 0), Base8's ay, an order-8 point's, 2^253 and 2^253 +- 1,
    (P +- 1) / 2, at least eight ay with a point and eight without -- each with sign in {0, 1, 2, P - 1}; then random ay (half of
    them have a point) with the sign of one of the two roots, the other root's, or garbage"""
    rng = random.Random(seed)
    have, none = ay_sign_2_ax_ays(seed)
    edges = [{"ay": y, "sign": s} for y in have + none for s in (0, 1, 2, P - 1)]

    def draw():
        y = rng.randrange(P) if rng.random() < 0.8 else garbage(rng, rng.choice(have))
        x = bjj_x_of(y)
        r = rng.random()
        if x is not None and r < 0.7:   # the sign of the smaller root (0) or of the larger one (1): both are accepted
            return {"ay": y, "sign": rng.getrandbits(1)}
        return {"ay": y, "sign": _sel(rng) if r < 0.85 else rng.getrandbits(1)}
    return _assemble(n, edges, draw)


HASH_STATE_WIDTH = {"tokenID": 32, "nonce": 40, "sign": 1, "balance": 192, "ay": 253, "ethAddr": 160}


def hash_state_cases(n, seed):
    """HashState: every input at 0, 1, P - 1 and at 2^k - 1, 2^k, 2^k + 1 around its own width (sign and nonce out of range among
    them), all of them at once, then `garbage`. No constraint of this main can fail: the template packs and hashes."""
    rng = random.Random(seed)
    base = {"tokenID": 1, "nonce": 49, "sign": 1, "balance": 12343256, "ay": 0x144e7e10fd47e0c67a733643b760e80ed399f70e78ae97620dbb719579cd645d,
            "ethAddr": 0x7e5f4552091a69125d5dfcb7b8c2659029395bdf}
    edges = [dict(base)]
    for f, w in HASH_STATE_WIDTH.items():
        for v in (0, 1, 2, P - 1, (1 << w) - 1, 1 << w, (1 << w) + 1, 1 << 192, 1 << 253):
            edges.append(dict(base, **{f: v % P}))
    edges += [{f: v for f in base} for v in (0, 1, P - 1, 1 << 192)]

    def draw():
        d = dict(base)
        for f in rng.sample(list(base), rng.randrange(1, 7)):
            d[f] = garbage(rng, d[f]) if rng.random() < 0.7 else rng.randrange(1 << 192, P)
        return d
    return _assemble(n, edges, draw)


DECODE_TX_BITS = ("onChain", "newAccount", "previousOnChain")
DECODE_TX_WIDTH = {"maxNumBatch": 32, "amountF": 40, "loadAmountF": 40, "toEthAddr": 160, "fromEthAddr": 160, "txCompressedData": 225}


def decode_tx_bases(n_levels):
    """valid DecodeTx inputs: every transaction of two synthetic batches, cut out the way src/rollup-main.circom wires them"""
    from circuits_amd import builder as B
    out = []
    for seed, n_acc in ((31, 6), (32, 9)):
        bb = B.synthetic_batch(10, n_levels, 4, 2, n_accounts=n_acc, exits=1, seed=seed)
        inp = bb.get_input()
        for i in range(bb.nTx):
            d = {k: _copy(inp[k][i]) for k in ("txCompressedData", "maxNumBatch", "amountF", "toEthAddr", "toBjjAy", "rqTxCompressedDataV2", "rqToEthAddr", "rqToBjjAy",
                                               "fromEthAddr", "fromBjjCompressed", "loadAmountF", "onChain", "newAccount", "auxFromIdx", "auxToIdx")}
            d.update(previousOnChain=inp["onChain"][i - 1] if i else 1, globalChainID=inp["globalChainID"], currentNumBatch=inp["currentNumBatch"],
                     inIdx=inp["imOutIdx"][i - 1] if i else inp["oldLastIdx"])
            out.append(d)
    return out


def decode_tx_cases(n, n_levels, seed):
    """DecodeTx(n_levels): the bit inputs non-boolean; each decomposed input one bit above its width (32, 40, 48, 160, 225 bits) and at
    its last value inside; fromBjjCompressed with non-bits; inIdx at 2^nLevels - 1 and 2^48 - 1; several of these at once; then every
    scalar through `mutate` / `garbage`"""
    rng = random.Random(seed)
    bases = decode_tx_bases(n_levels)
    l1 = [b for b in bases if b["onChain"]]
    l2 = [b for b in bases if not b["onChain"]]
    create = [b for b in l1 if b["newAccount"]]
    assert l1 and l2 and create
    edges = []
    for f in DECODE_TX_BITS:
        for v in (2, P - 1, rng.randrange(2, P)):
            edges.append(dict(rng.choice(l1 if f != "previousOnChain" else bases), **{f: v}))
    for f, w in DECODE_TX_WIDTH.items():
        for b in (l1[0], l2[0]):
            edges.append(dict(b, **{f: b[f] | (1 << w)}))
            edges.append(dict(b, **{f: (1 << w) - 1}))
    for f in ("auxFromIdx", "auxToIdx", "inIdx"):   # indexes: 48 bits in the data, nLevels in the tree
        for v in ((1 << n_levels) - 1, 1 << n_levels, (1 << 48) - 1, 1 << 48):
            edges.append(dict(rng.choice(create if f != "auxToIdx" else l2), **{f: v}))
    for pos, v in ((0, 2), (100, P - 1), (253, 2), (254, rng.randrange(2, P)), (255, 2), (255, P - 1)):
        b = rng.choice(create)
        bits = list(b["fromBjjCompressed"])
        bits[pos] = v
        edges.append(dict(b, fromBjjCompressed=bits))
    edges.append(dict(create[0], fromBjjCompressed=[1] * 256))
    edges.append(dict(l2[0], fromBjjCompressed=[2] * 256))
    scalars = [k for k in bases[0] if k != "fromBjjCompressed"]

    def draw():
        b = rng.choice(bases)
        r = rng.random()
        if r < 0.2:    # two or three range failures at once
            d = dict(b)
            for f in rng.sample(list(DECODE_TX_WIDTH), rng.randrange(2, 4)):
                d[f] = (d[f] + (1 << rng.randrange(DECODE_TX_WIDTH[f], 253))) % P
            return d
        if r < 0.3:    # every scalar garbage
            return dict(b, **{f: garbage(rng, b[f]) for f in scalars})
        if r < 0.4:
            return dict(b, **{f: garbage(rng, b[f], key_bits=n_levels) for f in rng.sample(scalars, 2)})
        return mutate(rng, b, key_fields=("auxFromIdx", "auxToIdx", "inIdx"), key_bits=n_levels,
                      bit_fields=DECODE_TX_BITS + tuple(("fromBjjCompressed", (rng.randrange(256),)) for _ in range(2)))
    return _assemble(n, edges, draw)


def fee_tx_cases(n, n_levels, seed):
    """FeeTx(n_levels): the fee slots of a built batch and the reference's two literal cases (scenarios.fee_tx_cases); feeIdx 0, the
    same index in several instances, 2^nLevels and above; a plan token that is not the leaf's; balance and accFee at 2^192 - 1 and
    P - 1; then `mutate` with the sibling and key patterns rollup_tx_cases uses"""
    import scenarios
    rng = random.Random(seed)
    bases = [c for c, _ in scenarios.fee_tx_cases(n_levels)]
    slots = [b for b in bases if b["feeIdx"] and b["feeIdx"] < (1 << n_levels)]
    assert slots
    s0 = slots[0]
    edges = [dict(s0), dict(s0), dict(s0, feeIdx=0), dict(slots[-1], feeIdx=0, accFee=P - 1)]
    # two checks violated at once (the plan token and the proof): which one is reported is the template's order
    edges += [dict(s0, feePlanToken=(s0["feePlanToken"] + 1) % P, oldStateRoot=(s0["oldStateRoot"] + 1) % P),
              dict(s0, feePlanToken=(s0["feePlanToken"] + 1) % P, siblings=[0] * (n_levels + 1)),
              dict(s0, feePlanToken=(s0["feePlanToken"] + 1) % P, siblings=list(s0["siblings"][:-1]) + [5])]
    edges += [dict(s0, feeIdx=v) for v in (1 << n_levels, s0["feeIdx"] + (1 << n_levels), (1 << 48) - 1, P - 1, s0["feeIdx"] ^ 1)]
    edges += [dict(s0, feePlanToken=v) for v in ((s0["feePlanToken"] + 1) % P, (s0["feePlanToken"] + P - 1) % P, rng.randrange(P))]
    edges += [dict(s0, tokenID=(s0["tokenID"] + 1) % P), dict(s0, tokenID=(s0["tokenID"] + 1) % P, feePlanToken=(s0["feePlanToken"] + 1) % P)]
    for v in ((1 << 192) - 1, 1 << 192, P - 1):
        edges += [dict(s0, balance=v), dict(s0, accFee=v), dict(s0, balance=v, accFee=v)]
    edges += [dict(s0, sign=2, nonce=P - 1), dict(s0, siblings=list(s0["siblings"][:-1]) + [5])]

    def draw():
        b = rng.choice(slots if rng.random() < 0.8 else bases)
        if rng.random() < 0.15:   # the plan token AND the proof wrong
            return dict(b, feePlanToken=garbage(rng, b["feePlanToken"]), **{rng.choice(("balance", "oldStateRoot", "ay", "nonce")): rng.randrange(P)})
        return mutate(rng, b, sibling_fields=("siblings",), key_fields=("feeIdx",), key_bits=n_levels, bit_fields=("sign",))
    return _assemble(n, edges, draw)

