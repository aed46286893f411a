"""Shared by tests/test_export_derived.py (GPU) and tests/test_export_derived_cpu.py: the inputs of the launches, the LITERAL reference
of every variable of an unreduced compile, the synthetic .sym files and the comparison.

Expected values come from neither evaluator of the library. A stored variable is the ORACLE's witness of the same input; a derived
one is what tests/test_derived_signals.py states literally -- circomlib's Poseidon template signal by signal on the inputs the oracle
logged for each component, the reference's `<==` right-hand sides over the oracle's witness (LITERAL_RULES, _sm_literal) -- and the
inputs of IsZero / Num2Bits components are held to the template's own constraints (_constraint_checked_names). Those functions are
imported, not copied. They are defined whether or not a `===` of the circuit holds, so a rejected instance has a reference too."""
import functools
import os
import random
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_derived_signals as TDS   # noqa: E402
from oracle_binding import OracleCtx, P   # noqa: E402

# poseidon_params.generate runs the Grain LFSR anew on every call (0.3 s for t = 5) and literal_poseidon calls it per component:
# 776 components per RollupMain(8,16,4,4) input. Same parameters, computed once per width.
if not hasattr(TDS.generate, "cache_info"):
    TDS.generate = functools.lru_cache(maxsize=None)(TDS.generate)
    # the garbage cases are mutations of a few valid transactions: most of their components hash what another case's did. (The callers
    # only read the returned dict.)
    _literal = functools.lru_cache(maxsize=4096)(TDS.literal_poseidon)
    TDS.literal_poseidon = lambda t, inputs: _literal(t, tuple(int(v) % P for v in inputs))

STORED, POSEIDON, FORM, ISZERO, PRODUCT, QUOTIENT = 0, 1, 2, 3, 4, 5
KIND_NAMES = ("stored", "Poseidon", "form", "IsZero", "product", "quotient")
N_SOLVED = (64, 24, 24)          # linear / product / quotient variables an .r1cs adds to every full map (Names.add_solved)
DERIVED_BIT = 1 << 63

MAIN_SHAPE = (8, 16, 4, 4)       # sections with lines (8 transactions, 4 fee slots per instance), multi-unit sections, HashInputs singles
MAIN_KW = dict(nTx=8, nLevels=16, maxL1Tx=4, maxFeeTx=4)
N_MAIN_BATCHES = 3
RTX_KW = dict(nLevels=16, maxFeeTx=2)
RTX_N, RTX_SEED = 48, 93         # FZ.rollup_tx_cases(48, 16, 2, 93): the accepted / rejected shares are asserted in the CPU file
WD_N = 37

_POS_NAME = re.compile(r"^(.*)\.(?:(?:ark|mix)\[\d+\]\.(?:in|out)\[\d+\]|sigmaF\[\d+\]\[\d+\]\.in|sigmaP\[\d+\]\.in|inputs\[\d+\]|out)$")


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def main_batches():
    """the three distinct batches the RollupMain launches cycle through (instance k holds batch k % 3)"""
    from test_export_dev import _main_batches
    return [bb.get_input() for bb in _main_batches(MAIN_SHAPE, N_MAIN_BATCHES)]


def withdraw_inputs():
    """Withdraw(16): one input per exit leaf of a batch with three of them (instance k holds leaf k % 3)"""
    from circuits_amd import builder as B
    bb = B.synthetic_batch(8, 16, 3, 4, n_accounts=8, exits=4, seed=9)
    out = []
    for idx in list(bb.exit_leaves):
        w = B.withdraw_input(bb, idx, 16)
        out.append(w[0] if isinstance(w, tuple) else w)
    return out


def rollup_tx_cases():
    import fuzz_common as FZ
    return FZ.rollup_tx_cases(RTX_N, 16, 2, RTX_SEED)


# ---- the oracle's side -----------------------------------------------------------------------------------------------------------------
class OracleView:
    """ONE instance of a run oracle context with the interface _declared_linear_names uses (read, poseidon_inputs); the witness is
    fetched once"""

    def __init__(self, o, instance=0):
        self.o, self.instance = o, instance
        self.raw = o.read_bytes(0, o.witness_len(), instance)
        self.rows = np.frombuffer(self.raw, dtype=np.uint8).reshape(-1, 32)

    def value(self, idx):
        return int.from_bytes(self.raw[32 * idx:32 * idx + 32], "little")

    def read(self, first, count):
        return [self.value(first + i) for i in range(count)]

    def poseidon_inputs(self, virt_first):
        return self.o.poseidon_inputs(virt_first, self.instance)


def run_oracle(template, kw, inputs):
    """one oracle context over `inputs` (one instance each), Poseidon inputs logged -> (context, [OracleView])"""
    o = OracleCtx(template, kw.get("nTx", 0), kw.get("nLevels", 0), kw.get("maxL1Tx", 0), kw.get("maxFeeTx", 0), n_instances=len(inputs))
    o.log_poseidon()
    for k, inp in enumerate(inputs):
        o.set_inputs(inp, instance=k)
    o.run()
    return o, [OracleView(o, k) for k in range(len(inputs))]


def stored_of(o):
    """[(name, index)] of every stored signal of one instance, from the ORACLE's tables (its name list keeps a Poseidon block as one
    '<component>.sigma*' line: expanded here into the S-box signals poseidon.circom declares, each looked up by name)"""
    out = []
    for nm in o.symbol_names():
        if not nm.endswith(".sigma*"):
            out.append((nm, o.lookup(nm)))
            continue
        pre = nm[:-len(".sigma*")]
        t = 2
        while t < 7:
            try:
                o.lookup("%s.sigmaF[0][%d].in2" % (pre, t))
            except KeyError:
                break
            t += 1
        boxes = ["sigmaF[%d][%d]" % (k, j) for k in range(4) for j in range(t)] + ["sigmaP[%d]" % k for k in range(TDS.N_ROUNDS_P[t - 2])]
        boxes += ["sigmaF[%d][%d]" % (k, j) for k in range(4, 8) for j in range(t)]
        for b in boxes:
            for s in ("in2", "in4", "out"):
                full = "%s.%s.%s" % (pre, b, s)
                out.append((full, o.lookup(full)))
    idx = [i for _, i in out]   # (a layout may leave a few slots unnamed: no variable can name those)
    assert len(set(idx)) == len(idx) and max(idx) < o.witness_len() and len(idx) == o.o.c.orc_symbol_count(o.h)
    return out


class Names:
    """The variables of an unreduced compile of one main: every stored signal but the constant, every signal the literal rules cover,
    every constraint-pinned component input, and the variables an .r1cs defines over those (add_solved); with their kind. The same for
    every input of the main (asserted by Reference)."""

    def __init__(self, o, view):
        self.stored = stored_of(o)
        # (no rule reads a signal inside Sha256, and its 2.8 x 10^5 names would cost the rule scan 10 s per input)
        self.light = [(nm, i) for nm, i in self.stored if ".sha256compression[" not in nm]
        self.index = dict(self.stored)
        linear = TDS._declared_linear_names(view, self.light)
        self.checks = {nm: f for nm, f in TDS._constraint_checked_names(self.light).items() if nm not in linear}
        blocks = {nm[:-len(".sigmaF[0][0].in2")] for nm, _ in self.light if nm.endswith(".sigmaF[0][0].in2")}
        self.blocks = blocks
        self.names, self.kind = [], []
        for nm, _ in self.stored:
            if nm != "main.one":
                self.names.append(nm)
                self.kind.append(STORED)
        for nm in sorted(linear):
            m = _POS_NAME.match(nm)
            self.names.append(nm)
            self.kind.append(POSEIDON if m and m.group(1) in blocks else FORM)
        for nm in sorted(self.checks):
            self.names.append(nm)
            self.kind.append(ISZERO if nm[:-len(".in")] + ".inv" in self.index else FORM)
        self.kind = np.array(self.kind, dtype=np.uint8)
        self.n_base = len(self.names)
        self.solved = []
        self.add_solved(0xD0)
        self.entry = {nm: e for e, nm in enumerate(self.names)}
        self.first_linear = linear

    def add_solved(self, seed):
        """Variables no rule knows by name, defined by the constraints of an .r1cs OVER DERIVED VARIABLES -- what a compile's own
        linear and product lines do to the signals of a component. A .sym alone never makes the library evaluate a derived variable
        from another one (its rules read stored signals); these do: `lin[i]` = a linear form over a Poseidon-internal, a rule's and a
        stored variable and, three times out of four, over lin[i - 1] (chains: several dependency levels); `prod[i]` * 1 = A * B - c S;
        `quot[i]` * B = C with B a rule's variable (0 / 1 valued ones among them: a zero divisor reads as 0, the `<--` of circom with
        inverse(0) = 0) or a Poseidon-internal one. solved[i] = (three forms (constant, [(coefficient, entry)]): the value is
        f0 for a linear one, f0 * f1 + f2 for a product, f2 / f1 for a quotient)."""
        rng = random.Random(seed)
        lit_form = [e for e in np.nonzero(self.kind == FORM)[0] if self.names[e] not in self.checks]
        pos, st = np.nonzero(self.kind == POSEIDON)[0], np.nonzero(self.kind == STORED)[0]
        co = lambda: rng.choice((2, 3, P - 1, P - 2, rng.randrange(2, P)))   # noqa: E731  (never 1: a lone term times 1 is a wire, not a form)
        pick = lambda a: int(a[rng.randrange(len(a))])   # noqa: E731
        first = len(self.names)
        kinds = []
        for i in range(N_SOLVED[0]):
            terms = [(co(), pick(pos)), (co(), pick(lit_form)), (co(), pick(st))]
            if i % 4:
                terms.append((co(), first + i - 1))
            self.solved.append(((rng.randrange(P), terms), None, None))
            self.names.append("main.solvedOverDerived.lin[%d]" % i)
            kinds.append(FORM)
        lins = list(range(first, first + N_SOLVED[0]))
        for i in range(N_SOLVED[1]):
            fa = (rng.randrange(P), [(co(), pick(pos))])
            fb = (0, [(co(), pick(lins)), (co(), pick(lit_form))])
            self.solved.append((fa, fb, (0, [(co(), pick(st))])))
            self.names.append("main.solvedOverDerived.prod[%d]" % i)
            kinds.append(PRODUCT)
        for i in range(N_SOLVED[2]):
            fb = (0, [(co(), pick(lit_form) if i % 2 else pick(pos))])
            fc = (rng.randrange(P), [(co(), pick(lins)), (co(), pick(pos))])
            self.solved.append((None, fb, fc))
            self.names.append("main.solvedOverDerived.quot[%d]" % i)
            kinds.append(QUOTIENT)
        self.kind = np.concatenate([self.kind, np.array(kinds, dtype=np.uint8)])

    def recorded(self, keep):
        """the constraints that define the solved variables among `keep`, in the form tests/declared_forms.py writes as an .r1cs"""
        keep = set(int(e) for e in keep)
        nm = lambda f: [f[0], [[c, self.names[e]] for c, e in f[1]]]   # noqa: E731
        forms, quads = {}, []
        for i, (fa, fb, fc) in enumerate(self.solved):
            e = self.n_base + i
            if e not in keep:
                continue
            assert all(t in keep for f in (fa, fb, fc) if f for _, t in f[1]), self.names[e]
            if self.kind[e] == FORM:
                forms[self.names[e]] = nm(fa)
            elif self.kind[e] == PRODUCT:    # A * B = prod - f2
                quads.append([nm(fa), nm(fb), [-fc[0] % P, [[1, self.names[e]]] + [[-c % P, self.names[t]] for c, t in fc[1]]]])
            else:                            # quot * B = C
                quads.append([[0, [[1, self.names[e]]]], nm(fb), nm(fc)])
        return {"forms": forms, "quads": quads}

    def component_of(self, e):
        """the Poseidon component an entry of kind POSEIDON lies in"""
        return _POS_NAME.match(self.names[e]).group(1)

    def widths(self):
        """{t} over the Poseidon components whose internals these variables name"""
        return {max(j for j in range(8) if "%s.sigmaF[0][%d].in2" % (pre, j) in self.index) + 1 for pre in self.blocks}


class Reference:
    """the expected value of every entry of `names` for ONE input: rows[e] (32 bytes, little endian) where literal[e], otherwise a
    predicate over the value (checks); the solved variables from their defining forms over the literal values"""

    def __init__(self, names, view, linear=None):
        self.names, self.view = names, view
        if linear is None:
            linear = TDS._declared_linear_names(view, names.light)
        n = len(names.names)
        n_stored = int((names.kind == STORED).sum())
        assert [nm for nm in names.names[n_stored:names.n_base] if nm not in names.checks] == sorted(linear)   # the same variables for every input
        self.rows = np.zeros((n, 32), dtype=np.uint8)
        self.rows[:n_stored] = view.rows[[names.index[nm] for nm in names.names[:n_stored]]]
        lit = b"".join(int(linear[nm]).to_bytes(32, "little") for nm in names.names[n_stored:names.n_base] if nm not in names.checks)
        n_lit = len(lit) // 32
        self.rows[n_stored:n_stored + n_lit] = np.frombuffer(lit, dtype=np.uint8).reshape(-1, 32)
        self.literal = np.ones(n, dtype=bool)
        self.literal[n_stored + n_lit:names.n_base] = False
        assert n_stored + n_lit + len(names.checks) == names.n_base
        ev = self.form_value
        for i, (fa, fb, fc) in enumerate(names.solved):   # in order: a solved variable reads earlier ones only
            e = names.n_base + i
            v = ev(fa) if names.kind[e] == FORM else (ev(fa) * ev(fb) + ev(fc)) % P if names.kind[e] == PRODUCT else ev(fc) * pow(ev(fb), P - 2, P) % P
            self.rows[e] = np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)

    def form_value(self, f):
        """(constant, [(coefficient, entry)]) over this input's values"""
        return (f[0] + sum(c * self.value(e) for c, e in f[1])) % P

    def get(self, name):
        return self.view.value(self.names.index[name])

    def value(self, e):
        return int.from_bytes(self.rows[e].tobytes(), "little")


def reference_set(template, kw, inputs):
    """(Names, [Reference per input], oracle context) -- one oracle run per distinct input"""
    o, views = run_oracle(template, kw, inputs)
    names = Names(o, views[0])
    refs = [Reference(names, views[0], names.first_linear)] + [Reference(names, v) for v in views[1:]]
    return names, refs, o


# ---- the compiler's files ----------------------------------------------------------------------------------------------------------------
class Sym:
    """A synthetic .sym in the style of an unreduced compile over the entries `keep` (all of them by default), each a variable of its
    own in a seeded random order (or numbered by name), the lines shuffled, and the .r1cs that defines the solved variables among
    them. var[i] = the variable of entry keep[i]."""

    def __init__(self, names, seed, keep=None, order="shuffled"):
        rng = random.Random(seed)
        self.names = names
        self.keep = np.arange(len(names.names)) if keep is None else np.asarray(sorted(keep))
        n = len(self.keep)
        var = list(range(1, n + 1))
        if order == "shuffled":
            rng.shuffle(var)
        else:   # by name: a component's signals in consecutive variables, as a compiler numbers them
            by_name = sorted(range(n), key=lambda i: names.names[self.keep[i]])
            for v, i in enumerate(by_name, 1):
                var[i] = v
        self.var = np.array(var, dtype=np.int64)
        lines = ["0,0,0,one"] + ["%d,%d,1,%s" % (label, v, names.names[e]) for label, (e, v) in enumerate(zip(self.keep, var), 1)]
        rng.shuffle(lines)
        self.text = "\n".join(lines) + "\n"
        self.nvars = n + 1
        # the .r1cs of the same compile: the constraints that define the solved variables (none when `keep` holds none of them)
        rec = names.recorded(self.keep)
        self.r1cs = None
        if rec["forms"] or rec["quads"]:
            import declared_forms as DF
            order = [None] * n
            for e, v in zip(self.keep, var):
                order[v - 1] = names.names[e]
            self.r1cs = DF.sym_and_r1cs(rec, order)[1]

    def expected(self, ref):
        """(rows in variable order, literal mask in variable order)"""
        rows = np.zeros((self.nvars, 32), dtype=np.uint8)
        rows[0, 0] = 1
        rows[self.var] = ref.rows[self.keep]
        lit = np.ones(self.nvars, dtype=bool)
        lit[self.var] = ref.literal[self.keep]
        return rows, lit

    def by_entry(self, rows):
        """rows in variable order -> rows of the kept entries, in entry order"""
        return rows[self.var]


def partial_keeps(names, seed):
    """Two seeded subsets of the entries for maps that name only SOME variables. `fifth`: every entry with probability 1/5 -- but of two
    Poseidon components (seeded) exactly ONE internal signal, a middle one and the last one of the name list (1/5 of the ~600 to ~1 500
    names of a component never leaves one alone). `half`: every derived entry with probability 1/2, and exactly the stored entries
    `fifth` dropped: every stored variable is in one of the two maps and not in the other."""
    rng = random.Random(seed)
    n = names.n_base   # (the variables an .r1cs defines need their operands in the map: the partial maps are .sym files alone)
    fifth = np.array([rng.random() < 0.2 for _ in range(n)])
    pos = np.nonzero(names.kind == POSEIDON)[0]
    comps = sorted({names.component_of(e) for e in pos})
    lone = rng.sample(comps, 2)
    for c, which in zip(lone, ("middle", "last")):
        mine = [e for e in pos if names.component_of(e) == c]
        fifth[mine] = False
        fifth[mine[len(mine) // 2] if which == "middle" else mine[-1]] = True
    half = np.array([rng.random() < 0.5 for _ in range(n)])
    st = names.kind[:n] == STORED
    half[st] = ~fifth[st]
    return np.nonzero(fifth)[0], np.nonzero(half)[0]


def named_per_component(names, keep):
    """{Poseidon component: (entries of `keep` inside it, all its entries)}"""
    total, named = {}, {}
    keep = set(int(e) for e in keep)
    for e in np.nonzero(names.kind == POSEIDON)[0]:
        c = names.component_of(e)
        total[c] = total.get(c, 0) + 1
        if int(e) in keep:
            named[c] = named.get(c, 0) + 1
    return {c: (named.get(c, 0), total[c]) for c in total}


# ---- comparison --------------------------------------------------------------------------------------------------------------------------
def _int(row):
    return int.from_bytes(np.asarray(row, dtype=np.uint8).tobytes(), "little")


def compare(sym, ref, got, instance, what):
    """`got`: one exported instance, rows in variable order. Every variable: bit-exact where the reference is literal, the template's
    constraint where it is a pinned component input. A failure names the instance, the variable, its name and its kind."""
    names = sym.names
    assert got.shape == (sym.nvars, 32), (what, instance, got.shape)
    want, lit = sym.expected(ref)
    bad = np.nonzero((got != want).any(axis=1) & lit)[0]
    if bad.size:
        ent = {int(v): int(e) for e, v in zip(sym.keep, sym.var)}
        first = ["variable %d %s (%s): got %d, want %d" % (v, names.names[ent[v]] if v else "one", KIND_NAMES[names.kind[ent[v]]] if v else "stored", _int(got[v]), _int(want[v]))
                 for v in map(int, bad[:4])]
        by_kind = {KIND_NAMES[k]: int((names.kind[[ent[int(v)] for v in bad if v]] == k).sum()) for k in range(6)}
        raise AssertionError("%s, instance %d: %d of %d variables differ %r; %s" % (what, instance, bad.size, sym.nvars, by_kind, "; ".join(first)))
    for e, v in zip(sym.keep, sym.var):
        if not ref.literal[e]:
            nm = names.names[e]
            assert names.checks[nm](_int(got[v]), ref.get), "%s, instance %d: variable %d %s (%s): %d does not satisfy the component's constraints" % (
                what, instance, v, nm, KIND_NAMES[names.kind[e]], _int(got[v]))


def compare_rows(a, b, sym, instance, what):
    """two routes to the same vector (rows in variable order), element by element"""
    assert a.shape == b.shape == (sym.nvars, 32), (what, instance, a.shape, b.shape)
    bad = np.nonzero((a != b).any(axis=1))[0]
    if bad.size:
        ent = {int(v): int(e) for e, v in zip(sym.keep, sym.var)}
        v = int(bad[0])
        raise AssertionError("%s, instance %d: %d variables differ, first: variable %d %s (%s): %d != %d" % (
            what, instance, bad.size, v, sym.names.names[ent[v]] if v else "one", KIND_NAMES[sym.names.kind[ent[v]]] if v else "stored", _int(a[v]), _int(b[v])))


def neighbours_differ(names, ref_a, ref_b):
    """{kind name: number of derived entries whose expected value differs between two inputs}, for the kinds present. A constraint-pinned
    entry has no literal row: its value is a function of the stored signals the predicate reads, compared instead (IsZero: inv)."""
    out = {}
    for k in (POSEIDON, FORM, ISZERO, PRODUCT, QUOTIENT):
        sel = np.nonzero(names.kind == k)[0]
        if not sel.size:
            continue
        d = 0
        lit = sel[ref_a.literal[sel]]
        d += int((ref_a.rows[lit] != ref_b.rows[lit]).any(axis=1).sum())
        for e in sel[~ref_a.literal[sel]]:
            c = names.names[e][:-len(".in")]
            if k == ISZERO:
                d += ref_a.get(c + ".inv") != ref_b.get(c + ".inv")
            else:
                j = 0
                while "%s.out[%d]" % (c, j) in names.index:
                    if ref_a.get("%s.out[%d]" % (c, j)) != ref_b.get("%s.out[%d]" % (c, j)):
                        d += 1
                        break
                    j += 1
        out[KIND_NAMES[k]] = d
    return out
