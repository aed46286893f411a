"""RollupMain's packed inputs of an applied batch (hz_ledger_main_inputs) without a device: the descriptor table
hz_ledger_plan_main_inputs makes of layouts built from the reference's signal list, in two orders and at two shapes, for every combination
of the kind flags; its argument errors; the HZ_HD packing routines of csrc/ledger_inputs.h as a stand-alone host program under the address
and undefined-behaviour sanitizers; the build's resource remarks, the header's paragraph and the exported symbols. What the device writes
is guarded by tests/test_ledger_main_inputs.py."""
import ctypes
import itertools
import os
import subprocess
import sys

import pytest

import ledger_main_inputs_common as M
from circuits_amd import HzError
from circuits_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 16, 4, 4), (3, 16, 2, 1)]


def _lib():
    from circuits_amd import lib
    if not os.path.exists(capi.lib_path()):
        pytest.skip("the library was not built in this tree")
    return lib()


def _orders():
    declared = [n for n, _ in M.signal_list()]
    return {"declared": declared, "reversed": declared[::-1]}


def test_new_symbols_are_declared_and_exported():
    assert all(s in capi.EXPORTS for s in M.NEW_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    assert all(s + "(" in header for s in M.NEW_SYMBOLS)
    for name, value in (("HZ_MI_SIGS", capi.MI_SIGS), ("HZ_MI_RQ", capi.MI_RQ), ("HZ_MI_EXITS", capi.MI_EXITS), ("HZ_MI_CREATES", capi.MI_CREATES),
                        ("HZ_MI_AUX", capi.MI_AUX), ("HZ_MI_GROWING", capi.MI_GROWING)):
        assert "#define %s %du" % (name, value) in header, name
    assert "HZ_MI_KINDS = %d" % len(capi.MI_KINDS) in header
    for name, value in (("NONE", capi.MI_SRC_NONE), ("OUT", capi.MI_SRC_OUT), ("EXIT", capi.MI_SRC_EXIT), ("CREATE", capi.MI_SRC_CREATE),
                        ("AUX_TO_IDX", capi.MI_SRC_AUX_TO_IDX), ("GLOBALS", capi.MI_SRC_GLOBALS), ("FEE_IDXS", capi.MI_SRC_FEE_IDXS),
                        ("FEE_PLAN_TOKENS", capi.MI_SRC_FEE_PLAN_TOKENS), ("ROWS", capi.MI_SRC_ROWS), ("KEYS", capi.MI_SRC_KEYS)):
        assert "HZ_MI_SRC_%s = %d" % (name, value) in header, name
    if not os.path.exists(capi.lib_path()):
        pytest.skip("the library was not built in this tree")
    c = ctypes.CDLL(capi.lib_path())
    assert [s for s in M.NEW_SYMBOLS if not hasattr(c, s)] == []
    hz = _lib()
    assert hz.c.hz_ledger_main_inputs_ms.restype == ctypes.c_double and hz.c.hz_ledger_main_inputs_ms(None) == 0.0


def test_the_header_states_the_contract():
    header = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    at, scope = header.index(" * MAIN INPUTS (DESIGN.md 8l)."), header.index(" * OUT OF SCOPE: L1 transactions that create accounts or exit through a call other than")
    assert header.index(" * SELECT (DESIGN.md 8j).") < at < scope
    para = header[at:scope]
    for word in M.NEW_SYMBOLS + ["every one but hz_ledger_apply_l2", "hz_inputs_packed_bytes", "hz_input_packed_offset", "the first nTx - 1 rows", "row nTx - 1 of state_root_after",
                                 "the first maxFeeTx - 1 rows", "zeros for from_bjj == NULL", "zeros for sigs == NULL", "zeros for rq == NULL", "changes nothing resident",
                                 "invalidates no *_dev output", "refuses nothing but arguments", "one synchronise", "hz_witness_check", "The target buffer is untouched"]:
        assert word in para, word
    tail = header[scope:].split("*/")[0]
    assert "the packed inputs of" in tail and "hz_inputs_stage_range" in tail and "One thread at a time." in tail


def test_the_golden_signal_list_is_the_layouts():
    """the list the tables are planned over: 64 signals, every one with a rule; its dimensions give the flat lengths the library's own
    layout has (checked on the device, where a context exists, by the byte-equality tests)"""
    sigs = M.signal_list()
    assert len(sigs) == 64 and len({n for n, _ in sigs}) == 64
    total, lay = M.layout(SHAPES[0])
    by = {n: (off, w, flat) for n, off, w, flat in lay}
    assert by["fromBjjCompressed"][1:] == (1, 8 * 256) and by["siblings1"][2] == 8 * 17 and by["imAccFeeOut"][2] == 7 * 4 and by["imStateRootFee"][2] == 3
    assert total % 32 == 0 and all(off % 32 == 0 for off, _, _ in by.values())
    assert M.layout(SHAPES[1])[1][[n for n, _ in sigs].index("imStateRootFee")][3] == 0   # maxFeeTx = 1: a signal without rows


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("order", ["declared", "reversed"])
def test_the_descriptor_table(shape, order):
    """every signal gets exactly one descriptor, the destination ranges tile [0, bytes), and each kind, source, first row and row count is
    what the list of sources says -- for all 64 combinations of the kind flags"""
    hz = _lib()
    lay = M.layout(shape, _orders()[order])
    total, sigs = lay
    for bits in itertools.product((0, 1), repeat=6):
        flags = sum(f for f, b in zip(M.FLAGS.values(), bits) if b)
        plan = hz.ledger_plan_main_inputs(lay, *shape, flags=flags)
        exp = M.expected_plan(shape, flags)
        assert set(plan) == set(exp) == {n for n, _, _, _ in sigs} and len(plan) == len(sigs) == 64
        for name in exp:
            assert plan[name] == exp[name], (name, flags, plan[name], exp[name])
    # the ranges the descriptors write: rows x inner x width of each, without overlap, and nothing of [0, bytes) left but alignment gaps
    inner = {n: (flat // plan[n][3] if plan[n][3] else 0) for n, _, _, flat in sigs}
    spans = sorted((off, off + plan[n][3] * inner[n] * w) for n, off, w, _ in sigs)
    assert all(a1 <= b0 for (_, a1), (b0, _) in zip(spans, spans[1:])) and spans[-1][1] <= total
    covered = sum(b - a for a, b in spans)
    assert total - covered < 32 * len(sigs) and covered == sum(w * flat for _, _, w, flat in sigs)


def test_every_argument_error_is_reported():
    hz = _lib()
    shape = SHAPES[0]
    total, sigs = M.layout(shape)

    def refused(lay, word, shape=shape, flags=0):
        with pytest.raises(HzError) as e:
            hz.ledger_plan_main_inputs(lay, *shape, flags=flags)
        assert e.value.status == 1 and word in str(e.value), str(e.value)
    i = [n for n, _, _, _ in sigs].index("siblings2")
    name, off, width, flat = sigs[i]
    refused((total, sigs[:i] + [("siblings9", off, width, flat)] + sigs[i + 1:]), "unknown signal siblings9")
    refused((total, sigs[:i] + [sigs[0]] + sigs[i + 1:]), "twice")
    refused((total, sigs[:-1]), "63 signals")
    refused((total, sigs[:i] + [(name, off, width, flat + 1)] + sigs[i + 1:]), "siblings2: flat length")
    refused((total, sigs[:i] + [(name, off, 1, flat)] + sigs[i + 1:]), "siblings2: element width")
    refused((total, sigs[:i] + [(name, off + 16, width, flat)] + sigs[i + 1:]), "not 32-byte aligned")
    refused((total, sigs[:i] + [(name, off - 32, width, flat)] + sigs[i + 1:]), "overlaps")
    refused((total - 32, sigs), "ends beyond the buffer")
    refused((total, sigs), "flat length", shape=(8, 15, 4, 4))   # a layout of another shape
    refused((total, sigs), "flat length", shape=(9, 16, 4, 4))
    refused((total, sigs), "flat length", shape=(8, 16, 4, 3))
    refused((total, sigs), "shape", shape=(0, 16, 0, 4))
    refused((total, sigs), "shape", shape=(8, 16, 9, 4))
    refused((total, sigs), "unknown flags", flags=64)
    bits = sigs[[n for n, _, _, _ in sigs].index("fromBjjCompressed")]
    at = sigs.index(bits)
    refused((total, sigs[:at] + [(bits[0], bits[1], 32, bits[3])] + sigs[at + 1:]), "fromBjjCompressed: element width")
    assert hz.c.hz_ledger_plan_main_inputs(64, None, None, None, None, total, *shape, 0, None, None, None, None) == 1


# ---- the routines on the host ------------------------------------------------------------------------------------------------------------
def test_host_build_of_the_packing_routines_agrees_with_the_builders_formulas(tmp_path):
    """csrc/ledger_inputs.h as a stand-alone host program under -fsanitize=address,undefined: every computed signal of an L1 row and of an
    L2 row at the field edges (chain id 0xFFFF, token id with bit 31, amountF and loadAmountF 2^40 - 1, maxNumBatch 2^32 - 1, toBjjSign 1,
    userFee 255, both addresses 2^160 - 1, s = r - 1, nonce 2^40 - 2, indices just below 2^48), at small values, for a create row, for a NOP,
    with and without links; the bit expansion at 0, 2^256 - 1, the single bits 0, 31, 32, 254, 255 and a key with bits 254 and 255 over r - 1"""
    text = M.check_lines()
    n = len(text.splitlines())
    assert n > 300
    src = os.path.join(os.path.dirname(__file__), "native", "ledger_main_inputs_check.cpp")
    exe = str(tmp_path / "ledger_main_inputs_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and "cases=%d mismatches=0" % n in r.stdout, r.stdout + r.stderr
    lines = text.splitlines()   # the program does judge: one expectation changed is one mismatch
    at = next(i for i, ln in enumerate(lines) if ln.startswith("b "))
    lines[at] = lines[at][:-1] + ("0" if lines[at][-1] != "0" else "1")
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 1 and "mismatches=1" in r.stdout, r.stdout + r.stderr


def test_the_kernel_uses_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as RU
    path = os.path.join(RU.BUILD, "ledger.ru.txt")
    if not os.path.exists(path):
        pytest.skip("the library was not built in this tree (no build/ledger.ru.txt)")
    rows = {r["name"]: r for r in RU.table([path])}
    assert "hz::k_ledger_main_inputs" in rows, sorted(rows)
    assert rows["hz::k_ledger_main_inputs"]["scratch"] == 0 and rows["hz::k_ledger_main_inputs"]["lds"] == 0, rows["hz::k_ledger_main_inputs"]


def test_no_launch_cap_was_added():
    """the kernel's grid is exact -- ceil(elements / 256) blocks per signal --: the audit of tests/launch_limits_common.py finds no line in
    the new header, and none in ledger.hip beyond those its table already holds"""
    import launch_limits_common as LL
    import re
    text = open(os.path.join(ROOT, "circuits_amd", "csrc", "ledger_inputs.h")).read()
    for pat in LL.AUDIT_PATTERNS:
        assert not re.search(pat, text), pat
