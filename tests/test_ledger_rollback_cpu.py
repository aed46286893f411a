"""hz_ledger's marks, undo journal and rollback without a device: the six symbols declared and exported, every argument error
that needs no ledger through the real argtypes, the journal's host half (csrc/ledger_journal.h) and the shape's undo (csrc/smt_plan.h) as
tests/native/ledger_journal_check.cpp -- a stand-alone program under the address and undefined-behaviour sanitizers, run directly --, and the
resource remarks of the six new kernels."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from circuits_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hz_ledger_journal", "hz_ledger_applied", "hz_ledger_rollback", "hz_ledger_journal_stats", "hz_ledger_journal_ms", "hz_ledger_rollback_ms"]
NEW_KERNELS = {"ledger.ru.txt": ("hz::k_ledger_journal_save", "hz::k_ledger_journal_restore"),
               "state.ru.txt": ("hz::k_state_journal_save", "hz::k_state_journal_restore"),
               "smt_tree.ru.txt": ("hz::k_smt_journal_save", "hz::k_smt_journal_restore")}


def test_the_six_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.EXPORTS and hasattr(L.c, name), name
    assert re.search(r"#define HZ_LEDGER_JOURNAL_MAX 64\b", header)
    for method in ("journal", "applied", "rollback", "journal_stats", "journal_ms", "rollback_ms"):
        assert callable(getattr(capi.Ledger, method)) and getattr(capi.GrowingLedger, method) is getattr(capi.Ledger, method)


def test_argument_errors_need_no_ledger():
    """a null ledger, and a null output, through the argtypes the bindings use: HZ_ERR_ARG and a message that names the call"""
    L = capi.lib()
    c = L.c
    mark = ctypes.c_uint64(77)
    cases = [("hz_ledger_journal", (None, 4)), ("hz_ledger_journal", (None, 65)), ("hz_ledger_applied", (None, ctypes.byref(mark))),
             ("hz_ledger_rollback", (None, 0)), ("hz_ledger_rollback", (None, (1 << 64) - 1)), ("hz_ledger_journal_stats", (None, None, None, None, None, None))]
    for name, args in cases:
        st = getattr(c, name)(*args)
        msg = c.hz_last_error().decode()
        assert st == 1 and msg.startswith(name + ": null"), (name, st, msg)
    assert mark.value == 77                       # a refused call writes nothing
    assert c.hz_ledger_journal_ms(None) == 0.0 and c.hz_ledger_rollback_ms(None) == 0.0
    with pytest.raises(ctypes.ArgumentError):     # the argtypes are set: a depth that is no integer does not reach C
        c.hz_ledger_journal(None, "4")


def test_host_build_of_the_journal_under_sanitizers(tmp_path):
    src = os.path.join(os.path.dirname(__file__), "native", "ledger_journal_check.cpp")
    exe = str(tmp_path / "ledger_journal_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and re.search(r"ok checks=\d{4,}", r.stderr), r.stdout + r.stderr[-2000:]
    # the checks do judge: one expectation altered fails the program, at that expectation alone
    r = subprocess.run([exe, "spoil"], capture_output=True, text=True)
    assert r.returncode == 1 and "FAILED" in r.stderr and "older than" not in r.stderr and "CHECK(std::string(g_err) == want)" in r.stderr, r.stderr[-2000:]


def test_the_new_kernels_use_no_scratch_and_no_lds():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as RU
    paths = {f: os.path.join(RU.BUILD, f) for f in NEW_KERNELS}
    if not all(os.path.exists(p) for p in paths.values()):
        pytest.skip("the library was not built in this tree (no build/*.ru.txt)")
    for f, names in NEW_KERNELS.items():
        rows = {r["name"]: r for r in RU.table([paths[f]])}
        for name in names:
            assert name in rows, (f, sorted(rows))
            assert rows[name]["scratch"] == 0 and not rows[name].get("lds", 0), (name, rows[name])
