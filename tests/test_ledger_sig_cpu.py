"""The ledger's signature check without a device: the Python model of ledger_sig_common against Account.sign_msg, fuzz_common's signature
edges and the BatchBuilder's message hashes; the HZ_HD routines of csrc/ledger_sig.h built for the host under the address and
undefined-behaviour sanitizers against that model; the build's resource remarks of the signature kernels; the exported symbols."""
import ctypes
import os
import subprocess
import sys

import pytest

import ledger_common as C
import ledger_sig_common as S
from circuits_amd import builder as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 6
# what each class of fuzz_common.signature_edge_cases must come to: only these leave the signature valid
ACCEPTED = {"valid"}


def _edge_expectation(label):
    return 0 if label in ACCEPTED else 7


def test_model_accepts_signed_transfers_and_rejects_forgeries():
    base = C.base_state(K)
    cols = base.leaf_fields()
    txs = S.signed_batch(base, 6, seed=21, pool=8, n_tx=8)
    assert S.verdicts(txs, cols, base.first_idx) == [0] * 8
    for how in ("s", "r8", "malleable", "stale"):
        bad = [S.forge(txs[2], how)]
        assert S.verdicts(bad, cols, base.first_idx) == [7], how
    late = S.sign(base, dict(C.tx(base.first_idx, base.first_idx + 1, 5, nonce=0), maxNumBatch=4))
    assert [S.verdict(late, *S.key_of(cols, base.first_idx, late["fromIdx"]), cur) for cur in (3, 4, 5)] == [0, 0, 8]
    assert S.verdict(S.forge(late, "s"), *S.key_of(cols, base.first_idx, late["fromIdx"]), 5) == 7   # 7 beside 8 is 7


def test_model_rejects_every_edge_class():
    base = S.edge_state()
    edges = S.edge_batches(base)
    labels = [lb for lb, _, _ in edges]
    assert labels[0] == "valid" and len(labels) == len(set(labels)) >= 26
    for label, txs, cols in edges:
        assert S.verdicts(txs, cols, base.first_idx) == [0, _edge_expectation(label), 0], label


def test_model_message_is_the_builders():
    base = C.base_state(K)
    txs = S.signed_batch(base, 5, seed=33, pool=6, n_tx=7)
    _, bb = C.builder_batch(base, txs, [1, 0], [base.first_idx + 9, 0], 8)
    inp = bb.get_input()
    for i, t in enumerate(txs):
        tcd, v2, msg = S.message(t)
        assert msg == bb.tx_meta[i]["sigL2Hash"], i
        assert tcd == inp["txCompressedData"][i] and v2 == inp["txCompressedDataV2"][i], i


def test_host_build_of_the_device_routines_agrees_with_the_model(tmp_path):
    """csrc/ledger_sig.h (packing, message, Ax recovery, both scalar multiplications, the comparison) as a stand-alone host program
    under -fsanitize=address,undefined: every signed transfer, forgery, expiry and edge class, verdict and the three packed values"""
    base = C.base_state(K)
    cols = base.leaf_fields()
    f0 = base.first_idx
    cases = []
    txs = S.signed_batch(base, 6, seed=44, pool=8)
    for t in txs:
        cases.append((t, *S.key_of(cols, f0, t["fromIdx"]), 1))
        cases.append((t, *S.key_of(cols, f0, t["fromIdx"]), 1500))   # maxNumBatch 1000 has expired by now
    for how in ("s", "r8", "malleable", "stale"):
        cases.append((S.forge(txs[1], how), *S.key_of(cols, f0, txs[1]["fromIdx"]), 1500))
    for label, batch, ecols in S.edge_batches(S.edge_state()):
        cases.append((batch[1], *S.key_of(ecols, S.edge_state().first_idx, batch[1]["fromIdx"]), 1))
    src = os.path.join(os.path.dirname(__file__), "native", "ledger_sig_check.cpp")
    exe = str(tmp_path / "ledger_sig_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", src, "-o", exe])
    r = subprocess.run([exe], input=S.check_lines(cases), capture_output=True, text=True)
    assert r.returncode == 0 and "cases=%d mismatches=0" % len(cases) in r.stdout, r.stdout + r.stderr


def test_signature_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as RU
    path = os.path.join(RU.BUILD, "ledger_sig.ru.txt")
    if not os.path.exists(path):
        pytest.skip("the library was not built in this tree (no build/ledger_sig.ru.txt)")
    rows = {r["name"]: r for r in RU.table([path])}
    names = [n for n in rows if n.startswith("hz::k_ledger_sig_")]
    assert len(names) >= 2, sorted(rows)
    assert {n: rows[n]["scratch"] for n in names if rows[n]["scratch"]} == {}


def test_new_symbols_are_declared_and_exported():
    from circuits_amd.capi import EXPORTS, lib_path
    new = ["hz_ledger_apply_l2_signed", "hz_ledger_verify_l2", "hz_ledger_sig_outputs_dev", "hz_ledger_sig_ms"]
    assert all(s in EXPORTS for s in new)
    if not os.path.exists(lib_path()):
        pytest.skip("the library was not built in this tree")
    c = ctypes.CDLL(lib_path())
    assert [s for s in new if not hasattr(c, s)] == []
    header = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    assert all(s + "(" in header for s in new)
