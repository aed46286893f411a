"""Atomic transactions on the ledger (hz_ledger_apply_batch_atomic) without a device: the host planner
(hz_ledger_plan_atomic: where every link points, whether it holds, the argument errors) against the Python model over all offsets and
positions; the model itself against the oracle's rollup-main on BatchBuilder's inputs; the HZ_HD routines of csrc/ledger_rq.h and the
message of csrc/ledger_sig.h with its rq fields built for the host under the address and undefined-behaviour sanitizers; the build's
resource remarks, the header's paragraph and the exported symbols. What the device computes is guarded by tests/test_ledger_atomic.py."""
import ctypes
import os
import subprocess
import sys

import pytest

import ledger_atomic_common as Q
import ledger_common as C
from circuits_amd import HzError
from circuits_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hz_ledger_apply_batch_atomic", "hz_ledger_verify_l2_atomic", "hz_ledger_plan_atomic", "hz_ledger_rq_ms"]


def _lib():
    from circuits_amd import lib
    if not os.path.exists(capi.lib_path()):
        pytest.skip("the library was not built in this tree")
    return lib()


def test_new_symbols_are_declared_and_exported():
    assert all(s in capi.EXPORTS for s in NEW_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    assert all(s + "(" in header for s in NEW_SYMBOLS) and "} hz_l2rq;" in header
    assert ctypes.sizeof(capi.hz_l2rq) == 97 and capi.hz_l2rq.rq_offset.offset == 96 and capi.LEDGER_RQ_REASON == Q.REASON
    if not os.path.exists(capi.lib_path()):
        pytest.skip("the library was not built in this tree")
    c = ctypes.CDLL(capi.lib_path())
    assert [s for s in NEW_SYMBOLS if not hasattr(c, s)] == []
    hz = _lib()
    vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    creates = hz.c.hz_ledger_apply_batch_creates.argtypes
    assert hz.c.hz_ledger_apply_batch_atomic.argtypes == creates[:7] + [vp] + creates[7:]   # rq behind sigs
    assert hz.c.hz_ledger_verify_l2_atomic.argtypes == [vp, sz, vp, vp, vp, u32, u32, vp, vp]
    assert hz.c.hz_ledger_plan_atomic.argtypes == [sz, sz, vp, vp, vp, vp, vp]
    assert hz.c.hz_ledger_rq_ms.restype == ctypes.c_double and hz.c.hz_ledger_rq_ms(None) == 0.0


def test_the_header_describes_the_calls_and_no_longer_lists_them_as_out_of_scope():
    header = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    at, scope = header.index(" * ATOMIC (DESIGN.md 8i)."), header.index(" * OUT OF SCOPE: L1 transactions that create accounts or exit through a call other than")
    assert at < scope and "atomic (rqOffset)" not in header[scope:scope + 800] and "exit trees of earlier batches kept resident, a resident address index" in header
    para = header[at:scope]
    for word in NEW_SYMBOLS + ["13 the rq fields", "rq_offset > 7", "HZ_ERR_INPUT: an rq field >= r", "without HZ_LEDGER_VERIFY_SIGS"]:
        assert word in para, word


def _batch(base, n_l1, m, i, k, nop=None):
    """m transfers behind n_l1 rows, transaction i linked at offset k with the fields its target has; nop: a transaction made a NOP"""
    txs = Q.transfers(base, m, offsets={i: k})
    if nop is not None:
        txs[nop] = {}
    return Q.derive(n_l1, txs)


def test_the_planner_equals_the_model_over_all_offsets_and_positions():
    hz = _lib()
    base = C.base_state(4)
    for n_l1 in (0, 3):
        for m in (1, 5, 9):
            for i in range(m):
                for k in range(8):
                    txs = _batch(base, n_l1, m, i, k)
                    row = Q.target_row(n_l1 + i, k, n_l1, n_l1 + m)
                    got = hz.ledger_plan_atomic(n_l1, txs)
                    assert got["target_row"] == [row if j == i else -1 for j in range(m)], (n_l1, m, i, k)
                    assert got["verdict"] == Q.verdicts(n_l1, txs) == [0] * m, (n_l1, m, i, k)
                    for f in Q.RQ_FIELDS:   # each field off by one, alone
                        bad = list(txs)
                        bad[i] = Q.off_by_one(txs[i], f)
                        exp = [Q.REASON if j == i else 0 for j in range(m)]
                        assert hz.ledger_plan_atomic(n_l1, bad)["verdict"] == Q.verdicts(n_l1, bad) == exp, (n_l1, m, i, k, f)
    # a NOP target and a NOP's own entry compare against zeros; a changed target breaks the link
    txs = _batch(base, 3, 5, 1, 2, nop=3)
    assert hz.ledger_plan_atomic(3, txs) == {"target_row": [-1] * 5, "verdict": [0] * 5} and not any(txs[1].get(f, 0) for f in Q.RQ_FIELDS)
    txs = _batch(base, 3, 5, 1, 2)
    txs[3] = dict(txs[3], amountF=txs[3]["amountF"] + 1)
    assert hz.ledger_plan_atomic(3, txs)["verdict"] == Q.verdicts(3, txs) == [0, Q.REASON, 0, 0, 0]
    txs[1] = {"rqOffset": 9, "rqToEthAddr": 1 << 255}   # a NOP's entry is not looked at, not even for the argument errors
    assert hz.ledger_plan_atomic(3, txs) == {"target_row": [-1] * 5, "verdict": [0] * 5}
    assert hz.ledger_plan_atomic(3, Q.transfers(base, 4)) == {"target_row": [-1] * 4, "verdict": [0] * 4}   # rq == NULL
    assert hz.ledger_plan_atomic(0, []) == {"target_row": [], "verdict": []}
    # an rq_to_eth_addr of 2^160 or more never matches: a signed to_eth_addr has 160 bits
    txs = _batch(base, 0, 2, 0, 1)
    txs[0]["rqToEthAddr"] = txs[1].get("toEthAddr", 0) | 1 << 160
    assert hz.ledger_plan_atomic(0, txs)["verdict"] == [Q.REASON, 0]


def test_argument_errors():
    hz = _lib()
    base = C.base_state(4)
    txs = _batch(base, 0, 3, 0, 1)
    with pytest.raises(HzError) as e:
        hz.ledger_plan_atomic(0, [txs[0], dict(txs[1], rqOffset=8), txs[2]])
    assert e.value.status == 1 and "tx 1: rq_offset = 8 (0 .. 7)" in str(e.value), str(e.value)
    for f, member in zip(Q.RQ_FIELDS, ("rq_tx_compressed_data_v2", "rq_to_eth_addr", "rq_to_bjj_ay")):
        with pytest.raises(HzError) as e:
            hz.ledger_plan_atomic(0, [txs[0], txs[1], dict(txs[2], **{f: Q.P})])
        assert e.value.status == 4 and "tx 2: %s is not below the field's modulus" % member in str(e.value), str(e.value)
        assert hz.ledger_plan_atomic(0, [txs[0], txs[1], dict(txs[2], **{f: Q.P - 1})])["verdict"] == [0, 0, Q.REASON]
    # what does not fit hz_l2rq's members never reaches the library: nothing is reduced modulo 2^256 or clamped
    for bad, text in (({Q.RQ_FIELDS[0]: 1 << 256}, "does not fit 32 bytes"), ({Q.RQ_FIELDS[2]: -1}, "does not fit 32 bytes"), ({"rqOffset": 256}, "does not fit a byte"),
                      ({"rqOffset": -1}, "does not fit a byte")):
        with pytest.raises(ValueError) as v:
            capi.l2rq_array([txs[0], dict(txs[1], **bad)])
        assert "tx 1: " in str(v.value) and text in str(v.value), str(v.value)
    assert capi.l2rq_array([dict(txs[1], rqOffset=255, rqToEthAddr=(1 << 256) - 1)])[0].rq_offset == 255
    arr = capi.l2tx_array(txs)
    with pytest.raises(HzError) as e:
        hz._check(hz.c.hz_ledger_plan_atomic(0, 3, ctypes.addressof(arr), None, None, None, None))
    assert e.value.status == 1 and "null argument" in str(e.value)
    with pytest.raises(HzError) as e:
        hz._check(hz.c.hz_ledger_plan_atomic(513, 0, None, None, None, None, None))
    assert e.value.status == 1 and "at most 512" in str(e.value)


def test_the_model_is_the_circuits():
    """the oracle's rollup-main on BatchBuilder's inputs accepts exactly the batches the model accepts: one link in each direction, the
    same with a field off by one, offset 0 with a nonzero field, a link at an L1 row"""
    base = C.base_state(4)
    shape = (8, 16, 2, 2)
    l1 = Q.deposits(base, 2)
    cases = []
    for i, k in ((1, 2), (2, 6)):
        good = _batch(base, 2, 4, i, k)
        cases += [good, good[:i] + [Q.off_by_one(good[i], Q.RQ_FIELDS[0])] + good[i + 1:]]
    plain = Q.transfers(base, 4)
    cases.append(plain[:1] + [dict(plain[1], rqToBjjAy=5)] + plain[2:])   # offset 0, a nonzero field
    at_l1 = _batch(base, 2, 4, 0, 7)   # row 2 links back to row 1, an L1 row: zeros
    assert not any(at_l1[0].get(f, 0) for f in Q.RQ_FIELDS)
    cases += [at_l1, [Q.off_by_one(at_l1[0], Q.RQ_FIELDS[1])] + at_l1[1:]]
    want = [True, False, True, False, False, True, False]
    for txs, ok in zip(cases, want):
        assert (Q.first_refusal(2, txs) is None) == ok
        assert Q.oracle_accepts(Q.builder_inputs(base, l1, txs, shape), shape) == ok


def test_host_build_of_the_link_routines_agrees_with_the_model(tmp_path):
    """csrc/ledger_rq.h and the six-input message of csrc/ledger_sig.h as a stand-alone host program under -fsanitize=address,undefined:
    rq_target_row at r = 0, 3 and n_rows - 1 with all eight offsets, rq_fields_match on elements that differ in the top limb only, and
    sig_message with and without rq fields against build_hash_sig, and with zero rq fields against the digest of the three-argument path"""
    base = C.base_state(4)
    linked = _batch(base, 0, 4, 0, 1) + _batch(base, 0, 4, 3, 5)
    linked[0] = dict(linked[0], toEthAddr=(1 << 160) - 1, toBjjAy=Q.P - 1, toBjjSign=1, maxNumBatch=77)
    text = Q.check_lines() + Q.message_lines(linked)
    assert sum(ln.startswith("s ") and ln.split()[11:14] != ["0", "0", "0"] for ln in text.splitlines()) == 2   # with and without rq fields
    n = len(text.splitlines())
    src = os.path.join(os.path.dirname(__file__), "native", "ledger_atomic_check.cpp")
    exe = str(tmp_path / "ledger_atomic_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and "cases=%d mismatches=0" % n in r.stdout, r.stdout + r.stderr
    lines = text.splitlines()   # the program does judge: one expectation changed is one mismatch
    at = next(i for i, ln in enumerate(lines) if ln.startswith("t 3 7 3 "))
    lines[at] = lines[at].rsplit(" ", 1)[0] + " 2"   # row 2 is an L1 row
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 1 and "mismatches=1" in r.stdout, r.stdout + r.stderr


def test_the_link_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as RU
    path, sig = os.path.join(RU.BUILD, "ledger.ru.txt"), os.path.join(RU.BUILD, "ledger_sig.ru.txt")
    if not os.path.exists(path) or not os.path.exists(sig):
        pytest.skip("the library was not built in this tree (no build/ledger.ru.txt)")
    rows = {r["name"]: r for r in RU.table([path])}
    assert "hz::k_ledger_rq" in rows, sorted(rows)
    assert rows["hz::k_ledger_rq"]["scratch"] == 0 and not rows["hz::k_ledger_rq"].get("lds", 0), rows["hz::k_ledger_rq"]
    rows = {r["name"]: r for r in RU.table([sig])}
    for name in ("hz::k_ledger_sig_msg", "hz::k_ledger_sig_v2"):
        assert name in rows, sorted(rows)
        assert rows[name]["scratch"] == 0, (name, rows[name])
