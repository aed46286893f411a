"""The ledger's Python binding (capi.Ledger's apply and verify forms, the *_dev getters, Lib.ledger_plan_*) without a device: what each
public method hands the C function of its form. Part 1 puts a recording stand-in where the loaded library stands and checks, per form, the
function called, every argument by the name include/hermez_witness.h gives it, the bytes behind the input pointers, which pointers are
null, and the arrays that come back -- order, shapes, and that each is the one the header's struct member of its name points at. Part 2
calls the real library with a null ledger, which runs the argtypes of the ten functions. Nothing here depends on how capi.py is laid out
inside: the same file passes on the binding as it was before it had one call description (but for the one test marked below)."""
import ctypes

import numpy as np
import pytest

import capi_ledger_calls_common as S
from capi_ledger_calls_common import CHAIN_ID, IDXS, L1_TXS, M, N_L1, N_SIB, NUM_BATCH, PLAN, TXS
from circuits_amd import capi

# method -> (the C function, the prebuilt arrays it can be given beside txs as keyword arguments)
FORMS = {
    "apply_l2": ("hz_ledger_apply_l2", ()),
    "apply_l2_signed": ("hz_ledger_apply_l2_signed", None),            # builds its hz_l2sig array from the dictionaries: no prebuilt form
    "apply_l2_addr": ("hz_ledger_apply_l2_addr", ("sigs",)),
    "apply_batch": ("hz_ledger_apply_batch", ("sigs",)),
    "apply_batch_exits": ("hz_ledger_apply_batch_exits", ("sigs",)),
    "apply_batch_creates": ("hz_ledger_apply_batch_creates", ("sigs", "from_bjj")),
    "apply_batch_atomic": ("hz_ledger_apply_batch_atomic", ("sigs", "from_bjj", "rq")),
}
BATCH = ("apply_batch", "apply_batch_exits", "apply_batch_creates", "apply_batch_atomic", "apply_resident")
HAS_FLAGS = tuple(FORMS)[2:]    # the forms with verify= and aux_to_idx=
POINTERS = ("l1", "from_bjj", "txs", "sigs", "rq", "aux_to_idx", "fee_plan_tokens", "fee_idxs", "out", "sig_out", "aux_to_idx_out", "l1_flags_out", "exit_out",
            "create_out", "verdict_out")
OUTPUTS = POINTERS[8:]


def call(led, method, prebuilt=False, n_l1=N_L1, m=M, n_sib=N_SIB, **kw):
    """led.method over the first n_l1 and m rows of the batch, as dictionaries or as prebuilt arrays -> (what it returned, the recorded call)"""
    l1, txs = L1_TXS[:n_l1], TXS[:m]
    if prebuilt:
        built = {"sigs": capi.l2sig_array(txs), "from_bjj": capi.from_bjj_array(l1), "rq": capi.l2rq_array(txs)}
        for name in FORMS.get(method, (None, ("sigs", "from_bjj", "rq")))[1]:
            kw.setdefault(name, built[name])
        # the length of a prebuilt array is the number of rows: none is an array of no element, not the one-element array of an empty list
        l1, txs = capi.l1tx_array(l1) if n_l1 else (capi.hz_l1tx * 0)(), capi.l2tx_array(txs) if m else (capi.hz_l2tx * 0)()
    args = ([l1] if method in BATCH else []) + [txs, PLAN, IDXS] + ([CHAIN_ID, NUM_BATCH] if method != "apply_l2" else [])
    got = getattr(led, method)(*args, n_sib=n_sib, **kw)
    return got, led.L.c.calls[-1]


def nulls(c):
    return {name for name in POINTERS if name in c.args and not c.args[name]}


def check_inputs(c, n_l1=N_L1, m=M, skip=()):
    want = S.inputs(n_l1, m)
    for name, got in c.bytes.items():
        if name not in skip:
            assert got == want[name], name


def check_returned(got, form, **kw):
    want, tags = S.shapes(form, **kw), S.tags()
    assert list(got) == list(want)
    for name, a in got.items():
        assert a.shape == want[name] and a.dtype == np.uint8 and a.flags.c_contiguous, name
        if a.size:
            assert a.flat[0] == tags[name], name
            assert not a.reshape(-1)[1:].any(), name


@pytest.fixture
def leds():
    return S.ledgers(S.Recorder(), k=S.K)


# ---- part 1: the recording stand-in ----

@pytest.mark.parametrize("prebuilt", [False, True])
@pytest.mark.parametrize("method", list(FORMS))
def test_apply_form(leds, method, prebuilt):
    """everything given, verified, outputs on: no pointer is null but the L1 ones of a form without L1 rows"""
    fn, takes = FORMS[method]
    if prebuilt and takes is None:
        return
    kw = {"verify": True, "aux_to_idx": S.AUX} if method in HAS_FLAGS else {}
    got, c = call(leds[1 if "creates" in method or "atomic" in method else 0], method, prebuilt, **kw)
    names = S.prototype(fn)
    assert c.fn == fn and c.n_args == len(names) and c.args["l"] == 0xBEEF
    want = {"n_l1": N_L1, "m": M, "flags": capi.LEDGER_VERIFY_SIGS, "chain_id": CHAIN_ID, "current_num_batch": NUM_BATCH, "F": S.F, "n_sib": N_SIB}
    for name in ("n_l1", "m", "flags", "chain_id", "current_num_batch", "F", "n_sib"):
        if name in names:
            assert c.args[name] == want[name], name
    assert nulls(c) == set()
    assert set(c.bytes) == {n for n in names if n in S.inputs()}
    check_inputs(c)
    check_returned(got, fn)


@pytest.mark.parametrize("method", list(FORMS))
def test_outputs_false_and_the_verify_flag(leds, method):
    fn, _ = FORMS[method]
    led = leds[1]
    got, c = call(led, method, outputs=False, **({"verify": True} if method in HAS_FLAGS else {}))
    assert got == {} and nulls(c) == {n for n in OUTPUTS + ("aux_to_idx",) if n in c.args}
    if method not in HAS_FLAGS:
        return
    assert c.args["flags"] == capi.LEDGER_VERIFY_SIGS
    got, c = call(led, method, verify=False)       # sig_out goes only with the verify flag: C refuses it without
    assert c.args["flags"] == 0 and nulls(c) == {"sig_out", "aux_to_idx"}
    check_inputs(c)
    check_returned(got, fn, verify=False)
    got, c = call(led, method, verify=True)
    assert c.args["flags"] == capi.LEDGER_VERIFY_SIGS and nulls(c) == {"aux_to_idx"}
    check_returned(got, fn, verify=True)


def test_apply_l2_signed_hands_sig_out_whenever_it_has_outputs(leds):
    got, c = call(leds[0], "apply_l2_signed")
    assert nulls(c) == set() and list(got)[-3:] == S.SIG_SLOTS
    got, c = call(leds[0], "apply_l2_signed", outputs=False)
    assert nulls(c) == {"out", "sig_out"} and got == {}


@pytest.mark.parametrize("method", BATCH[:4])
def test_sigs_false_is_a_null_pointer(leds, method):
    got, c = call(leds[1], method, sigs=False)
    assert "sigs" in nulls(c) and "sigs" not in c.bytes
    got, c = call(leds[1], method, prebuilt=True, sigs=False)
    assert "sigs" in nulls(c)
    check_inputs(c)


def test_rq_of_apply_batch_atomic(leds):
    led = leds[1]
    for prebuilt, kw, null in ((False, {}, False), (False, {"rq": False}, True), (False, {"rq": capi.l2rq_array(TXS)}, False), (True, {"rq": None}, True),
                               (True, {"rq": False}, True), (True, {}, False)):
        got, c = call(led, "apply_batch_atomic", prebuilt, **kw)
        assert ("rq" in nulls(c)) == null, (prebuilt, kw)
        check_inputs(c)
    got, c = call(led, "apply_batch_atomic", m=2)    # dictionaries without one rq field: l2rq_array makes none
    assert "rq" in nulls(c)


def test_from_bjj(leds):
    led = leds[1]
    for method in ("apply_batch_creates", "apply_batch_atomic"):
        got, c = call(led, method)                                  # dictionaries: built from them
        assert c.bytes["from_bjj"] == S.inputs()["from_bjj"]
        mine = np.full((N_L1, 32), 0x5A, dtype=np.uint8)
        got, c = call(led, method, from_bjj=mine)                   # given: used
        assert c.args["from_bjj"] == mine.ctypes.data
        got, c = call(led, method, prebuilt=True, from_bjj=None)    # a prebuilt hz_l1tx array and none given: null
        assert "from_bjj" in nulls(c)
        got, c = call(led, method, n_l1=1, prebuilt=True, from_bjj=mine[:1])
        assert c.args["from_bjj"] == mine.ctypes.data and c.args["n_l1"] == 1
        rows = [dict(L1_TXS[1])]
        led.apply_batch_creates(rows, TXS, PLAN, IDXS, CHAIN_ID, NUM_BATCH)    # no row creates an account: from_bjj_array makes none
        assert "from_bjj" in nulls(led.L.c.calls[-1])


@pytest.mark.parametrize("method", HAS_FLAGS)
def test_no_rows(leds, method):
    """auxToIdx goes only with a row to write, l1_flags only with an L1 row; the dictionary has them all the same"""
    fn, _ = FORMS[method]
    batch = method in BATCH
    for n_l1, m in ((0, 0), (N_L1, 0), (0, M)) if batch else ((0, 0),):
        got, c = call(leds[1], method, n_l1=n_l1, m=m, verify=True, **({"rq": False} if "atomic" in method else {}))
        want = {"aux_to_idx", "rq"} | ({"aux_to_idx_out"} if (n_l1 if batch else 0) + m == 0 else set()) | ({"l1_flags_out", "from_bjj"} if n_l1 == 0 else set())
        assert nulls(c) == want & set(c.args), (n_l1, m)
        assert c.args["m"] == m and c.args.get("n_l1", n_l1) == n_l1
        check_inputs(c, n_l1, m)
        check_returned(got, fn, n_l1=n_l1, m=m)


@pytest.mark.parametrize("method", list(FORMS))
def test_n_sib(leds, method):
    """None is the ledger's k; C is handed the number as given, the arrays have min(max(n_sib, 0), 64) sibling rows"""
    fn, _ = FORMS[method]
    for n_sib, dim in ((None, S.K), (70, 64), (0, 0)):
        got, c = call(leds[1], method, n_sib=n_sib)
        assert c.args["n_sib"] == (S.K if n_sib is None else n_sib)
        assert all(got["siblings%d" % i].shape[1] == dim for i in (1, 2, 3))
        check_returned(got, fn, n_sib=dim, verify=False)


@pytest.mark.parametrize("method", list(FORMS))
def test_into(leds, method):
    fn, _ = FORMS[method]
    kw = {"verify": True} if method in HAS_FLAGS else {}
    want = S.shapes(fn)
    into = {name: np.zeros(shape, dtype=np.uint8) for name, shape in want.items()}
    got, c = call(leds[1], method, into=into, **kw)
    assert list(got) == list(want) and all(got[name] is into[name] for name in want)
    check_returned(got, fn)
    # the base arrays and the signature arrays, when they are asked for, must be there
    for name in ["tokenID1", "new_root"] + (["sig_l2_hash"] if "sig_l2_hash" in want else []):
        with pytest.raises(KeyError):
            call(leds[1], method, into={k: v for k, v in into.items() if k != name}, **kw)
    # every other name is optional: a fresh array is made for it
    for name in [n for n in ("auxToIdx", "l1_flags", "new_exit", "new_exit_root", "aux_from_idx", "new_last_idx") if n in want]:
        for a in into.values():
            a[...] = 0
        got, c = call(leds[1], method, into={k: v for k, v in into.items() if k != name}, **kw)
        assert got[name] is not into[name] and all(got[k] is into[k] for k in want if k != name)
        check_returned(got, fn)
    if method in HAS_FLAGS:    # unverified: the signature arrays of `into` are not looked at
        got, c = call(leds[1], method, into={k: v for k, v in into.items() if k not in S.SIG_SLOTS}, verify=False)
        assert list(got) == list(S.shapes(fn, verify=False))


def test_into_of_a_wrong_shape_is_refused(leds):
    into = {name: np.zeros(shape, dtype=np.uint8) for name, shape in S.shapes("hz_ledger_apply_batch_atomic").items()}
    for name in ("siblings1", "sig_l2_hash", "auxToIdx", "l1_flags", "exit_root_after", "new_last_idx"):
        bad = dict(into)
        bad[name] = np.zeros((into[name].shape[0] + 1,) + into[name].shape[1:], dtype=np.uint8)
        with pytest.raises(AssertionError):
            call(leds[1], "apply_batch_atomic", into=bad, verify=True)


@pytest.mark.parametrize("prebuilt", [False, True])
@pytest.mark.parametrize("atomic", [False, True])
def test_apply_resident(leds, atomic, prebuilt):
    fn = "hz_ledger_apply_batch_atomic" if atomic else "hz_ledger_apply_batch_exits"
    got, c = call(leds[1], "apply_resident", prebuilt, verify=True, atomic=atomic)
    assert c.fn == fn and c.n_args == len(S.prototype(fn))
    assert nulls(c) == {"out", "sig_out", "aux_to_idx", "aux_to_idx_out", "create_out"} & set(c.args)
    assert (c.args["n_l1"], c.args["m"], c.args["flags"], c.args["chain_id"], c.args["current_num_batch"], c.args["F"], c.args["n_sib"]) == (
        N_L1, M, capi.LEDGER_VERIFY_SIGS, CHAIN_ID, NUM_BATCH, S.F, N_SIB)
    check_inputs(c)
    assert list(got) == ["l1_flags", "new_exit_root"]
    assert got["l1_flags"].shape == (N_L1,) and got["l1_flags"][0] == 0xF1
    assert got["new_exit_root"].shape == (1, 32) and got["new_exit_root"][0, 0] == len(S.EXIT_SLOTS)    # the last slot alone was set
    got, c = call(leds[1], "apply_resident", prebuilt, n_l1=0, atomic=atomic, sigs=False, rq=False)
    assert nulls(c) == {"out", "sig_out", "aux_to_idx", "aux_to_idx_out", "create_out", "l1_flags_out", "sigs", "rq", "from_bjj"} & set(c.args)
    assert c.args["flags"] == 0 and got["l1_flags"].shape == (0,)
    if prebuilt:    # prebuilt rows and nothing beside them: no sigs, no rq, no keys
        l1, txs = capi.l1tx_array(L1_TXS), capi.l2tx_array(TXS)
        leds[1].apply_resident(l1, txs, PLAN, IDXS, CHAIN_ID, NUM_BATCH, atomic=atomic)
        assert {"sigs", "rq", "from_bjj"} & set(c.args) <= nulls(leds[1].L.c.calls[-1])
    else:           # dictionaries: rq is built for the atomic form alone, and that has no place for it otherwise
        assert ("rq" in call(leds[1], "apply_resident", atomic=atomic)[1].bytes) == atomic


@pytest.mark.parametrize("atomic", [False, True])
def test_verify_forms(leds, atomic):
    fn = "hz_ledger_verify_l2_atomic" if atomic else "hz_ledger_verify_l2"
    led = leds[0]
    method = led.verify_l2_atomic if atomic else led.verify_l2
    for kw in ({}, {"rq": capi.l2rq_array(TXS)}) if atomic else ({},):
        verdict = method(TXS, CHAIN_ID, NUM_BATCH, **kw)
        c = led.L.c.calls[-1]
        assert c.fn == fn and c.n_args == len(S.prototype(fn)) and nulls(c) == {"sig_out"}
        assert (c.args["l"], c.args["m"], c.args["chain_id"], c.args["current_num_batch"]) == (0xBEEF, M, CHAIN_ID, NUM_BATCH)
        check_inputs(c)
        assert set(c.bytes) == {"txs", "sigs"} | ({"rq"} if atomic else set())
        assert verdict.shape == (M,) and verdict.dtype == np.uint8 and verdict.tolist() == [7, 0, 0]
    verdict, sig = method(TXS, CHAIN_ID, NUM_BATCH, outputs=True)
    assert nulls(led.L.c.calls[-1]) == set() and verdict.tolist() == [7, 0, 0]
    assert list(sig) == S.SIG_SLOTS and all(sig[name].shape == (M, 32) and sig[name].flat[0] == i + 1 for i, name in enumerate(S.SIG_SLOTS))
    verdict = method([], CHAIN_ID, NUM_BATCH)
    c = led.L.c.calls[-1]
    assert verdict.shape == (0,) and c.args["m"] == 0 and c.args["verdict_out"] and c.args["txs"] and c.args["sigs"]
    if atomic:
        assert "rq" in nulls(c)
        method(TXS[:2], CHAIN_ID, NUM_BATCH)    # no rq field in any dictionary
        assert "rq" in nulls(led.L.c.calls[-1])


def test_value_errors(leds):
    led = leds[1]
    for method in list(FORMS) + ["apply_resident"]:
        args = ([L1_TXS] if method in BATCH else []) + [TXS, PLAN, IDXS[:1]] + ([CHAIN_ID, NUM_BATCH] if method != "apply_l2" else [])
        with pytest.raises(ValueError, match="^fee_plan_tokens and fee_idxs differ in length$"):
            getattr(led, method)(*args)
    with pytest.raises(ValueError, match="^aux_to_idx: one entry per transaction$"):
        call(led, "apply_l2_addr", aux_to_idx=S.AUX[:2])
    for method in BATCH[:4]:
        with pytest.raises(ValueError, match="^aux_to_idx: one entry per L2 transaction$"):
            call(led, method, aux_to_idx=S.AUX + [0, 0])    # n_l1 + m entries are as wrong as any other number
    assert led.L.c.calls == []
    for plan in (led.L.ledger_plan_l2, lambda *a: led.L.ledger_plan_batch(L1_TXS, *a), lambda *a: led.L.ledger_plan_exits(L1_TXS, *a)):
        with pytest.raises(ValueError, match="^fee_plan_tokens and fee_idxs differ in length$"):
            plan(TXS, PLAN, IDXS[:1], S.K)


def test_plan_creates_checks_the_fee_lengths(leds):
    # EXPECTED TO FAIL on the binding before the one call description: ledger_plan_creates alone did not compare the two lengths there and
    # let C read past fee_idxs. (The stand-in has no hz_ledger_plan_creates, so the old binding fails here without reading anything.)
    with pytest.raises(ValueError, match="^fee_plan_tokens and fee_idxs differ in length$"):
        leds[0].L.ledger_plan_creates(L1_TXS, TXS, PLAN, IDXS[:1], 32, 16)


def test_dev_getters(leds):
    led = leds[1]
    getters = (led.outputs_dev, led.sig_outputs_dev, led.exit_outputs_dev, led.create_outputs_dev, led.withdraw_rows_dev)
    for get, fn in zip(getters, S.DEV_CALLS):
        got = get()
        assert list(got) == S.DEV_SLOTS[fn]
        assert [got[name] for name in got] == [S.Recorder.DEV_BASE + 16 * i for i in range(len(got))]


def test_the_constants_name_the_headers_members():
    assert [name for name, _, _ in capi.LEDGER_ARRAYS] == S.OUT_SLOTS and list(capi.LEDGER_SIG_ARRAYS) == S.SIG_SLOTS
    assert list(capi.LEDGER_EXIT_ARRAYS) == S.EXIT_SLOTS and list(capi.LEDGER_CREATE_ARRAYS) == S.CREATE_SLOTS and list(capi.WITHDRAW_ARRAYS) == S.WITHDRAW_SLOTS
    assert capi.Ledger.shapes(3, 2, 5)[6] == ("siblings1", (3, 5, 32)) and capi.Ledger.shapes(3, 2, 5)[15] == ("acc_fee_after", (3, 2, 32))


# ---- part 2: the real library, no device ----

@pytest.fixture(scope="module")
def real():
    return S.ledgers(capi.lib(), h=None, k=S.K)


def _null_ledger(fn, f, *args, **kw):
    with pytest.raises(capi.HzError) as e:    # not ctypes.ArgumentError, not TypeError: the argtypes take what the binding hands them
        f(*args, **kw)
    text = str(e.value).split(": ", 1)[1]
    assert text.startswith(fn + ":") and "null ledger" in text, text


@pytest.mark.parametrize("prebuilt", [False, True])
@pytest.mark.parametrize("method", list(FORMS) + ["apply_resident", "apply_resident atomic"])
def test_null_ledger_through_the_real_argtypes(real, method, prebuilt):
    atomic = method.endswith(" atomic")
    method = method.split()[0]
    fn, takes = FORMS.get(method, ("hz_ledger_apply_batch_atomic" if atomic else "hz_ledger_apply_batch_exits", ()))
    if prebuilt and takes is None:
        return
    l1, txs = (capi.l1tx_array(L1_TXS), capi.l2tx_array(TXS)) if prebuilt else (L1_TXS, TXS)
    kw = {name: {"sigs": capi.l2sig_array(TXS), "from_bjj": capi.from_bjj_array(L1_TXS), "rq": capi.l2rq_array(TXS)}[name] for name in takes} if prebuilt else {}
    if method == "apply_resident":
        kw.update(atomic=atomic, verify=True, **({"sigs": capi.l2sig_array(TXS), "from_bjj": capi.from_bjj_array(L1_TXS)} if prebuilt else {}))
    elif method in HAS_FLAGS:
        kw.update(verify=True, aux_to_idx=S.AUX)
    args = ([l1] if method in BATCH else []) + [txs, PLAN, IDXS] + ([CHAIN_ID, NUM_BATCH] if method != "apply_l2" else [])
    _null_ledger(fn, getattr(real[1], method), *args, n_sib=N_SIB, **kw)


def test_null_ledger_verify_forms(real):
    _null_ledger("hz_ledger_verify_l2", real[0].verify_l2, TXS, CHAIN_ID, NUM_BATCH)
    _null_ledger("hz_ledger_verify_l2", real[0].verify_l2, TXS, CHAIN_ID, NUM_BATCH, outputs=True)
    _null_ledger("hz_ledger_verify_l2_atomic", real[0].verify_l2_atomic, TXS, CHAIN_ID, NUM_BATCH, outputs=True)
    _null_ledger("hz_ledger_verify_l2_atomic", real[0].verify_l2_atomic, TXS, CHAIN_ID, NUM_BATCH, rq=capi.l2rq_array(TXS))


@pytest.mark.parametrize("fn", S.APPLY_CALLS + S.VERIFY_CALLS)
def test_argtypes_have_the_prototypes_length(real, fn):
    names = S.prototype(fn)
    argtypes = getattr(real[0].L.c, fn).argtypes
    assert len(argtypes) == len(names)
    # and its kinds: a size_t where the header counts, a uint32_t where it has a flag or a number, a pointer everywhere else
    want = {"n_l1": ctypes.c_size_t, "m": ctypes.c_size_t, "F": ctypes.c_size_t, "n_sib": ctypes.c_size_t, "flags": ctypes.c_uint32, "chain_id": ctypes.c_uint32,
            "current_num_batch": ctypes.c_uint32}
    assert [want.get(name, ctypes.c_void_p) for name in names] == list(argtypes)
