"""What the two halves of the standalone-main fuzz share (tests/test_standalone_fuzz_cpu.py, tests/test_standalone_fuzz.py): the
twelve mains the adversarial fuzz of tests/test_adversarial_fuzz.py does not reach -- DecodeTx, FeeTx, HashState, the eight gadget
templates and AySign2Ax as `component main` -- at the shapes their constraint systems are recorded at (tests/golden/declared_forms/),
the generators of tests/fuzz_common.py behind one call, the oracle's results computed once per list, and the recorded system as the
judge of a witness (test infrastructure)."""
import declared_forms as DF
import fuzz_common as FZ
from test_declared_signals import KEYS

P = FZ.P
# mains whose constraints an input can violate: the least number of distinct first-failure constraints a launch must show
MIN_IDS = {"decode-float": 1, "compute-fee": 4, "balance-updater": 6, "rollup-tx-states": 2, "rq-tx-verifier": 4, "ay-sign-2-ax": 2, "decode-tx": 10, "fee-tx": 3}
# mains without a constraint an input can violate (they pack, select, add and hash): neither side may report anything
NEVER_FAIL = ("hash-state", "fee-accumulator", "mux256", "bits-compressed-2-ay-sign")
MAINS = list(MIN_IDS) + list(NEVER_FAIL)
SEED = {k: 5100 + i for i, k in enumerate(MAINS)}
N_GPU = {k: 449 for k in MAINS}          # seven wavefronts and one lane
N_GPU.update({"decode-tx": 193, "fee-tx": 129})
N_CPU = {k: 128 for k in MAINS}          # what the recorded system is solved for on the CPU (Python: 0.1 s to 1.3 s a case)
N_CPU.update({"decode-tx": 64, "fee-tx": 16})
ROTATE = 37
_CACHE = {}


def kw_of(key):
    """the template parameters of the recorded shape, by name (hz.ctx) ..."""
    return dict(zip(KEYS.get(key, ()), DF.load(key)["args"]))


def shape_of(key):
    """... and as the oracle's (nTx, nLevels, maxL1Tx, maxFeeTx)"""
    kw = kw_of(key)
    return tuple(kw.get(k, 0) for k in ("nTx", "nLevels", "maxL1Tx", "maxFeeTx"))


def cases_of(key, n=None, seed=None):
    """the list of one main: N_GPU[key] cases unless told otherwise (a shorter list is a prefix of a longer one of the same seed only
    for the generators that draw nothing while they lay out their edges; the tests ask for the prefix of the full list instead)"""
    n = N_GPU[key] if n is None else n
    seed = SEED[key] if seed is None else seed
    kw = kw_of(key)
    if key == "fee-accumulator":
        return FZ.fee_accumulator_cases(n, kw["maxFeeTx"], seed)
    if key in ("decode-tx", "fee-tx"):
        return getattr(FZ, key.replace("-", "_") + "_cases")(n, kw["nLevels"], seed)
    name = {"bits-compressed-2-ay-sign": "bits_compressed"}.get(key, key.replace("-", "_"))
    return getattr(FZ, name + "_cases")(n, seed)


def full_list(key):
    """(cases, oracle slices, {instance: first failure}) of the full list, computed once per process and never changed"""
    if key not in _CACHE:
        cases = cases_of(key)
        parts = FZ.run_oracle_threads(key, shape_of(key), cases)
        _CACHE[key] = (cases, parts, FZ.oracle_failures(parts))
    return _CACHE[key]


def check_mix(key, n, failures):
    """the conditions on one launch of n instances with the oracle's {instance: first failure}"""
    if key in NEVER_FAIL:
        assert not failures, (key, sorted(failures)[:4])
        return
    assert 8 * len(failures) >= n and 8 * (n - len(failures)) >= n, (key, len(failures), n)
    ids = {f[1] for f in failures.values()}
    assert len(ids) >= MIN_IDS[key], (key, sorted(FZ.constraint_name(c) for c in ids))


def out_of_range(key, d):
    """does a case of a NEVER_FAIL main carry an input outside the range RollupTx would feed it: a selector or bit that is no bit, a
    value at or above 2^192 (hash-state: above the width RollupTx range-checks the field to; its ay is a field element by right)"""
    if key == "mux256":
        return any(not FZ.is_bit(v) for v in d["s"])
    if key == "bits-compressed-2-ay-sign":
        return any(not FZ.is_bit(v) for v in d["bjjCompressed"])
    if key == "hash-state":
        return any(d[f] % P >= (1 << w) for f, w in FZ.HASH_STATE_WIDTH.items() if f != "ay")
    return any(v % P >= (1 << 192) for v in FZ.flatten(list(d.values())))


class Judge:
    """the recorded system of one main over the oracle's witness: judge(o, k) -> the constraints instance k's witness violates"""

    def __init__(self, key):
        from oracle_binding import OracleCtx
        self.key, self.m = key, DF.load(key)
        probe = OracleCtx(key, *shape_of(key))
        self.idx = {}
        for n in DF.all_names(self.m):
            try:
                self.idx[n] = probe.lookup(n)
            except KeyError:
                pass

    def __call__(self, o, k):
        from circuits_amd import builder as B
        vals = o.read(0, o.witness_len(), k)
        val, unknown = DF.solve_with_hashes(self.m, {n: vals[i] for n, i in self.idx.items()}, lambda xs: B.host().poseidon([x % P for x in xs]))
        assert not unknown, (self.key, k, len(unknown), unknown[:6])
        return DF.violated(self.m, val)
