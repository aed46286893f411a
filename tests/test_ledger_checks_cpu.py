"""The ledger's argument checks (csrc/ledger_checks.h) without a device, on the cpu part of tests/golden/ledger_arg_errors.json.gz -- every
hz_ledger_plan_* export with each of its checks failing alone, the edges that must pass, and the pairs of errors that pin which one wins,
recorded on the commit before the checks moved into their header. The library must answer every case with the recorded status and message;
tests/native/ledger_checks_check.cpp, the header alone built for the host under the address and undefined-behaviour sanitizers with every
input array in a heap block of exactly its size, must too, without reading past any of them."""
import os
import subprocess

import ledger_arg_errors_common as E
from circuits_amd import capi

EXPORTS = ("hz_ledger_plan_l2", "hz_ledger_plan_batch", "hz_ledger_plan_exits", "hz_ledger_plan_creates", "hz_ledger_plan_atomic", "hz_ledger_plan_select",
           "hz_ledger_plan_main_inputs")


def test_the_plan_exports_answer_as_recorded():
    cases = E.load("cpu")
    assert {c["call"] for c in cases} == set(EXPORTS) and len(cases) >= 200
    assert sum(not c["status"] for c in cases) >= 50 and len({c["message"] for c in cases}) >= 100    # edges that pass, and many ways to fail
    L = capi.lib()
    wrong = [(c["call"], c["args"], got, (c["status"], c["message"])) for c in cases for got in [E.call(L, c)] if got != (c["status"], c["message"])]
    assert not wrong, wrong[:5]


def test_host_build_of_the_checks_answers_as_recorded(tmp_path):
    cases = [c for c in E.load("cpu") if c["call"] != "hz_ledger_plan_main_inputs"]    # (its one check of ledger.hip's own is no part of the header)
    text = "\n".join(ln for c in cases for ln in E.lines(c)) + "\n"
    want = [E.expected_line(c) for c in cases]
    src = os.path.join(os.path.dirname(__file__), "native", "ledger_checks_check.cpp")
    exe = str(tmp_path / "ledger_checks_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    got = r.stdout.splitlines()
    assert r.returncode == 0 and "cases=%d" % len(cases) in r.stderr, r.stderr[-2000:]
    assert [(c["call"], c["args"], g, w) for c, g, w in zip(cases, got, want) if g != w][:5] == [] and len(got) == len(want)
    # the comparison does judge: one expectation altered is one mismatch
    at = next(i for i, c in enumerate(cases) if "F = 65" in c["message"])
    altered = list(want)
    altered[at] = altered[at].replace("F = 65", "F = 66")
    assert sum(g != w for g, w in zip(got, altered)) == 1
