"""L1 rows that create accounts (hz_ledger_apply_batch_creates) without a device: the scheme model -- running index, key decode,
static slots, events, the create arrays' integers -- against BatchBuilder on the named batch (from genesis, on 5 and on 64 accounts) and on
seeded batches; the host planner (hz_ledger_plan_creates) against the model, argument errors included; the HZ_HD routines of
csrc/ledger_create.h built for the host under the address and undefined-behaviour sanitizers; the build's resource remarks and the exported
symbols. The model tests validate the reference the GPU tests use; what the device computes is guarded by tests/test_ledger_create.py."""
import ctypes
import os
import subprocess
import sys

import pytest

import ledger_common as C
import ledger_create_common as K
import ledger_l1_common as L1
from circuits_amd import HzError
from circuits_amd import builder as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hz_ledger_create_growing", "hz_ledger_load_accounts", "hz_ledger_size", "hz_ledger_last_idx", "hz_ledger_state_smt", "hz_ledger_apply_batch_creates",
               "hz_ledger_create_outputs_dev", "hz_ledger_create_ms", "hz_ledger_plan_creates"]


def _states():
    return {"genesis": K.Accounts([]), "five": K.few_accounts(5), "dense64": K.Accounts.of(C.base_state(6))}


def _model_vs_builder(acc, l1_txs, l2_txs, plan, idxs):
    m = K.model(acc, l1_txs, l2_txs, plan, idxs)
    assert isinstance(m, dict), m
    db, bb = K.builder_batch(acc.db(), l1_txs, l2_txs, plan, idxs, 16, aux_to=m["aux_to_idx"])
    inp, n_l1 = bb.get_input(), len(l1_txs)
    assert m["aux_from_idx"] == inp["auxFromIdx"] and m["out_idx_after"][:-1] == inp["imOutIdx"] and m["new_last_idx"] == bb.new_last_idx
    assert m["is_old0_1"] == inp["isOld0_1"] and m["old_key1"] == inp["oldKey1"]
    assert [1 if a else 0 for a in m["aux_from_idx"]] == inp["newAccount"]
    res = m["res"]
    for name, vals in res[1].items():
        assert vals == inp[name], name
    assert res[2][:-1] == inp["imAccFeeOut"] and res[3] == inp["imFinalAccFee"]
    assert res[4] == L1.builder_flags(bb, n_l1)
    for a, leaf in res[5].items():
        assert leaf == db.leaves[a], a
    for a, slot in m["slots"].items():   # the static fields never change
        assert all(db.leaves[a][f] == slot[f] for f in ("tokenID", "sign", "ay", "ethAddr")), a
    assert res[6] == inp["newExit"] and res[7] == bb.exit_leaves
    return m, bb


@pytest.mark.parametrize("name", ["genesis", "five", "dense64"])
def test_the_named_batch_matches_the_builder(name):
    acc = _states()[name]
    l1_txs, l2_txs, plan, idxs = K.kinds_batch(acc)
    m, bb = _model_vs_builder(acc, l1_txs, l2_txs, plan, idxs)
    inp = bb.get_input()
    new = acc.first_idx + acc.n
    assert m["aux_from_idx"][:7] == list(range(new, new + 7)) and m["new_last_idx"] == new + 6
    assert inp["isOld0_1"][0] == (1 if name == "genesis" else 0) and not any(inp["isOld0_1"][1:])   # consecutive keys meet a leaf ever after
    if name == "dense64":   # new key K meets K - 64 at depth 6
        assert inp["oldKey1"][:7] == [new + j - 64 for j in range(7)]
    assert [t["isAmountNullified"] for t in bb.tx_meta[:7]] == [0, 0, 0, 1, 1, 0, 0]
    ay, sign = K.decode_key(K.KEY_ABOVE_R)
    assert (inp["ay1"][5], inp["sign1"][5]) == (ay, sign) == (12345, 1) and inp["balance1"][:7] == [0] * 7


def test_seeded_batches_match_the_builder():
    for seed in range(6):
        acc = (K.Accounts([]), K.few_accounts(5), K.Accounts.of(C.base_state(4)))[seed % 3]
        l1_txs, l2_txs = K.draw_batch(acc, seed)
        _model_vs_builder(acc, l1_txs, l2_txs, [1, 2], [0, 0])


def test_key_decode_at_the_edges():
    P = K.P
    for key, ay in ((5, 5), (P - 1, P - 1), (P, 0), ((1 << 254) - 1, (1 << 254) - 1 - P), (P + 7 | 1 << 254, 7), (3 | 1 << 255, 3)):
        assert K.decode_key(key) == (ay, key >> 255), hex(key)
        assert K.new_leaf(K.create(key))["ay"] == (key & ((1 << 254) - 1)) % P   # the builder's formula


def test_the_planner_equals_the_model():
    from circuits_amd import lib
    from circuits_amd.capi import lib_path
    if not os.path.exists(lib_path()):
        pytest.skip("the library was not built in this tree")
    hz = lib()
    for name, acc in _states().items():
        l1_txs, l2_txs, plan, idxs = K.kinds_batch(acc)
        m = K.model(acc, l1_txs, l2_txs, plan, idxs)
        got = hz.ledger_plan_creates(l1_txs, l2_txs, plan, idxs, 1 << 10, acc.n, first_idx=acc.first_idx)
        assert got["aux_from_idx"] == m["aux_from_idx"] and got["out_idx_after"] == m["out_idx_after"] and got["n_creates"] == 7, name
        for l1, l2, text in K.arg_cases(acc):
            with pytest.raises(K.Refused) as r:
                K.model(acc, l1, l2, [1], [0])
            assert text in str(r.value)
            with pytest.raises(HzError) as e:
                hz.ledger_plan_creates(l1, l2, [1], [0], 1 << 10, acc.n, first_idx=acc.first_idx)
            assert e.value.status == 1 and text in str(e.value), str(e.value)
        # no room, a dense ledger, no keys
        with pytest.raises(K.Refused) as r:
            K.running_index(acc.first_idx, acc.n, acc.n + 6, l1_txs)
        with pytest.raises(HzError) as e:
            hz.ledger_plan_creates(l1_txs, l2_txs, plan, idxs, acc.n + 6, acc.n, first_idx=acc.first_idx)
        assert e.value.status == 1 and str(r.value) in str(e.value) and "L1 tx 6" in str(e.value), str(e.value)
        with pytest.raises(HzError) as e:
            hz.ledger_plan_creates(l1_txs, l2_txs, plan, idxs, 1 << 10, acc.n, first_idx=acc.first_idx, growing=False)
        assert e.value.status == 1 and "creates an account" in str(e.value) and "cannot grow" in str(e.value), str(e.value)
    # without a create row: zeros and a constant
    st = K.Accounts.of(C.base_state(4))
    got = hz.ledger_plan_creates([L1.own(st, 256, 257, 5)], [C.tx(257, 258, 1)], [1], [0], 16, 16)
    assert got == {"aux_from_idx": [0, 0], "out_idx_after": [271, 271], "n_creates": 0}


def test_host_build_of_the_create_routines_agrees_with_the_model(tmp_path):
    """csrc/ledger_create.h (key decode and reduction, e0 packing, the running index, which rows report an old leaf) as a stand-alone host
    program under -fsanitize=address,undefined: keys below r, at r - 1, r, 2^254 - 1, and with bits 254 and 255 set"""
    P = K.P
    keys = [0, 1, 12345, K.compressed(K.account(0)), P - 1, P, P + 1, (1 << 254) - 1, 1 << 254, 1 << 255, 3 << 254, (1 << 256) - 1, K.KEY_ABOVE_R, (P - 1) | 1 << 254,
            P | 1 << 255]
    text = K.check_lines(keys)
    n = len(text.splitlines())
    src = os.path.join(os.path.dirname(__file__), "native", "ledger_create_check.cpp")
    exe = str(tmp_path / "ledger_create_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and "cases=%d mismatches=0" % n in r.stdout, r.stdout + r.stderr
    lines = text.splitlines()   # the program does judge: one expectation changed is one mismatch
    at = next(i for i, ln in enumerate(lines) if ln.startswith("k ") and " %x " % (P - 1) in ln)
    f = lines[at].split()
    f[3] = "%x" % (int(f[3], 16) ^ 1)
    lines[at] = " ".join(f)
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 1 and "mismatches=1" in r.stdout, r.stdout + r.stderr


def test_create_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as RU
    path = os.path.join(RU.BUILD, "ledger.ru.txt")
    if not os.path.exists(path):
        pytest.skip("the library was not built in this tree (no build/ledger.ru.txt)")
    rows = {r["name"]: r for r in RU.table([path])}
    for name in ("hz::k_ledger_create", "hz::k_ledger_create_pack", "hz::k_ledger_load_records", "hz::k_ledger_resolve", "hz::k_ledger_scan", "hz::k_ledger_l1"):
        assert name in rows, sorted(rows)
        assert rows[name]["scratch"] == 0, (name, rows[name])


def test_new_symbols_are_declared_and_exported():
    from circuits_amd.capi import EXPORTS, LEDGER_CREATE_ARRAYS, lib_path
    assert all(s in EXPORTS for s in NEW_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    assert all(s + "(" in header for s in NEW_SYMBOLS) and "#define HZ_LEDGER_CREATE_ARRAYS 6" in header and "} hz_ledger_create_out;" in header
    assert LEDGER_CREATE_ARRAYS == K.CREATE_ARRAYS and "OUT OF SCOPE: L1 transactions that create accounts or exit through a call other than" in header
    if not os.path.exists(lib_path()):
        pytest.skip("the library was not built in this tree")
    c = ctypes.CDLL(lib_path())
    assert [s for s in NEW_SYMBOLS if not hasattr(c, s)] == []
