"""Receivers named by address or key (hz_ledger_apply_l2_addr) without a device: the table model against a brute-force
search, the HZ_HD routines of csrc/ledger_resolve.h built for the host under the address and undefined-behaviour sanitizers against that
model, the extended scheme model against BatchBuilder field by field, the build's resource remarks and the exported symbols."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import ledger_addr_common as A
import ledger_common as C
from circuits_amd import builder as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hz_ledger_apply_l2_addr", "hz_ledger_resolve_l2", "hz_ledger_aux_to_idx_dev", "hz_ledger_resolve_ms"]


def _special_state():
    return A.special_state(4)


def test_model_receivers_equal_a_brute_force_search():
    st = _special_state()
    f0 = st.first_idx
    leaf = st.state
    shared = leaf(f0 + 2)["ethAddr"]
    lowest_shared = min(i for i in range(f0, f0 + 16) if leaf(i)["ethAddr"] == shared and leaf(i)["tokenID"] == 1)
    txs = [A.to_addr(C.tx(f0 + 1, 0, 5), leaf(f0 + 2)),                       # a shared address: the lowest holder
           dict(A.to_addr(C.tx(f0 + 9, 0, 5, token=2), leaf(f0 + 9))),        # the same address under token 2
           A.to_addr(C.tx(f0 + 1, 0, 5), leaf(f0 + 5)),                       # an "any" account, by key
           A.to_addr(C.tx(f0 + 1, 0, 5), leaf(st.any_b)),
           A.to_addr(C.tx(f0 + 1, 0, 5), leaf(f0 + 7)),                       # an address of its own
           dict(C.tx(f0 + 1, 0, 5), toEthAddr=12345),                         # nobody's
           dict(C.tx(f0 + 1, 0, 5, token=3), toEthAddr=shared),               # a token nobody holds
           dict(C.tx(f0 + 1, 0, 5), toEthAddr=A.ANY, toBjjAy=leaf(f0 + 5)["ay"], toBjjSign=1 - leaf(f0 + 5)["sign"]),   # the other sign
           dict(C.tx(f0 + 1, 0, 0), toEthAddr=shared),                        # a zero amount
           C.tx(f0 + 1, f0 + 3, 5), {}]
    got, table = A.resolve_model(st, txs)
    assert got == [A.brute_force(st, t) if A.is_to_addr(t) else 0 for t in txs]
    assert got[0] == lowest_shared and got[1] == f0 + 9 and got[4] == f0 + 7 and got[5:7] == [0, 0] and got[8] == lowest_shared and got[9:] == [0, 0]
    assert got[2] == st.any_a and got[3] == st.any_b and got[7] == 0
    assert A.resolve_model(st, [A.to_addr(C.tx(f0 + 1, 0, 5), leaf(st.any_c))])[0] == [st.any_a]   # the lowest holder of that key
    assert A.resolve_model(st, txs, skip_zero=True)[0][8] == 0
    for k, seed in ((4, 1), (6, 2), (9, 3)):
        ms = A.mixed_state(k)
        batch = A.draw_batch(ms, 40, seed)
        assert sum(A.is_to_addr(t) for t in batch) >= 8
        got, table = A.resolve_model(ms, batch)
        assert got == [A.brute_force(ms, t) if A.is_to_addr(t) else 0 for t in batch], k
        assert all(got[i] for i, t in enumerate(batch) if A.is_to_addr(t))


def test_host_build_of_the_table_routines_agrees_with_the_model(tmp_path):
    """csrc/ledger_resolve.h (key, hash, insert, probe) as a stand-alone host program under -fsanitize=address,undefined"""
    rng = np.random.default_rng(9)
    big = lambda bits: int.from_bytes(rng.bytes(32), "little") >> (256 - bits)   # noqa: E731
    ay = big(253)
    keys = [(1, big(160), ay, 0), (1, A.ANY, ay, 0), (1, A.ANY, ay, 1), (2, A.ANY, ay, 1), (0, 0, 0, 0), (0xFFFFFFFF, A.ANY - 1, ay, 1),
            (1, A.ANY | 1 << 160, ay, 1), (1, A.ANY, ay ^ 1 << 252, 0)]
    words = [A.key_words(*k) for k in keys]
    assert len({tuple(w) for w in words}) == len(words)
    tables = [(2, [words[0]], [words[0], words[1]])]                 # one query in the minimum table
    tables.append((8, words, words + [A.key_words(7, 1, 0, 0)]))     # a full table (slots == queries): probes wrap past the last slot, and end
    near = [A.key_words(1, A.ANY, ay, 0), A.key_words(2, A.ANY, ay, 0), A.key_words(1, A.ANY, ay, 1), A.key_words(1, A.ANY, ay ^ 1 << 230, 0),
            A.key_words(1, 5, 0, 0), A.key_words(2, 5, 0, 0), A.key_words(1, 5 | 1 << 159, 0, 0)]   # differ in the token, the sign or the top limb only
    tables.append((16, near, near + [A.key_words(3, 5, 0, 0)]))
    many = [A.key_words(1 + i % 3, big(160), 0, 0) for i in range(200)]
    tables.append((A.slots_for(200), many + many[:5], many[::7] + [A.key_words(9, big(160), 0, 0) for _ in range(20)]))
    full = A.Table(8)
    assert [full.insert(w) for w in words].count(-1) == 0 and full.longest >= 2 and full.insert(A.key_words(7, 1, 0, 0)) == -1
    src = os.path.join(os.path.dirname(__file__), "native", "ledger_addr_check.cpp")
    exe = str(tmp_path / "ledger_addr_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    text = A.check_lines(tables, keys)
    n = sum(1 for ln in text.splitlines() if ln[0] in "kip")
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and "cases=%d mismatches=0" % n in r.stdout, r.stdout + r.stderr


def _model_vs_builder(st, txs, plan, idxs, aux=None):
    _, bb = A.builder_batch(st, txs, plan, idxs, 8, aux=aux)
    inp = bb.get_input()
    res = A.scheme_model(st, txs, plan, idxs, aux=aux)
    assert res[0] == "ok", res
    skip = A.zero_amount_rows(txs)
    for name, vals in res[1].items():
        for i, (g, e) in enumerate(zip(vals, inp[name])):
            if name.endswith("2") and i in skip:
                assert g == skip[i].get(name, e), (name, i)
            else:
                assert g == e, (name, i)
    assert res[2][:-1] == inp["imAccFeeOut"] and res[3] == inp["imFinalAccFee"] and res[4] == inp["auxToIdx"]


def test_scheme_model_matches_the_builder_field_by_field():
    st = A.mixed_state(4)
    f0 = st.first_idx
    tok = lambda i: st.state(i)["tokenID"]   # noqa: E731
    _model_vs_builder(st, A.draw_batch(st, 40, seed=11, pool=9, n_tx=44), [1, 2], [f0 + [tok(f0 + j) for j in range(16)].index(1), 0])
    _model_vs_builder(st, A.draw_batch(st, 30, seed=12), [2, 1, 0], [0, 0, 0])
    sp = _special_state()
    f0, leaf = sp.first_idx, sp.state
    # to one's own address; a receiver by address that sends before and after; the same address under two tokens; "any" by key
    own = A.brute_force(sp, A.to_addr(C.tx(f0 + 7, 0, 9), leaf(f0 + 7)))
    assert own == f0 + 7
    txs = [A.to_addr(C.tx(f0 + 7, 0, 900, 176, nonce=0), leaf(f0 + 7)), C.tx(f0 + 7, f0 + 1, 50, 100, nonce=1),
           A.to_addr(C.tx(f0 + 1, 0, 70, 0, nonce=0), leaf(f0 + 7)), C.tx(f0 + 7, f0 + 1, 5, 192, nonce=2),
           A.to_addr(C.tx(f0 + 1, 0, 33, 1, nonce=1), leaf(f0 + 2)), A.to_addr(C.tx(f0 + 9, 0, 33, 1, token=2, nonce=0), leaf(f0 + 9)),
           A.to_addr(C.tx(f0 + 1, 0, 44, 1, nonce=2), leaf(sp.any_b)), A.to_addr(C.tx(f0 + 1, 0, 45, 1, nonce=3), leaf(sp.any_c))]
    _model_vs_builder(sp, txs, [1, 2], [0, 0])
    # a supplied, valid, non-lowest holder
    shared = [i for i in range(f0, f0 + 16) if leaf(i)["ethAddr"] == leaf(f0 + 2)["ethAddr"] and leaf(i)["tokenID"] == 1]
    assert len(shared) >= 2
    one = [A.to_addr(C.tx(f0 + 1, 0, 70, 0, nonce=0), leaf(shared[0]))]
    _model_vs_builder(sp, one, [1], [0], aux=[shared[-1]])


def test_scheme_model_refusals():
    sp = _special_state()
    f0, leaf = sp.first_idx, sp.state
    nobody = dict(C.tx(f0 + 1, 0, 5, nonce=0), toEthAddr=12345)
    ok = C.tx(f0 + 3, f0 + 4, 10, nonce=0)
    assert A.scheme_model(sp, [ok, nobody], [1], [0]) == ("refused", 1, 9)
    # 9 is reported first, whatever else is wrong: a bad nonce at a lower transaction does not win
    assert A.scheme_model(sp, [C.tx(f0 + 3, f0 + 4, 10, nonce=5), ok, nobody], [1], [0]) == ("refused", 2, 9)
    # a zero amount to nobody needs no receiver
    assert A.scheme_model(sp, [dict(nobody, amountF=0)], [1], [0])[0] == "ok"
    to7 = A.to_addr(C.tx(f0 + 1, 0, 5, nonce=0), leaf(f0 + 7))
    assert A.scheme_model(sp, [to7], [1], [0], aux=[f0 + 3]) == ("refused", 0, 10)
    to5 = A.to_addr(C.tx(f0 + 1, 0, 5, nonce=0), leaf(f0 + 5))
    assert A.scheme_model(sp, [to5], [1], [0], aux=[sp.any_b]) == ("refused", 0, 11)
    assert A.scheme_model(sp, [to5], [1], [0], aux=[sp.any_c])[0] == "ok"
    with pytest.raises(ValueError):
        A.builder_batch(sp, [to5], [1], [0], 8, aux=[sp.any_b])
    # 10 beside 4 at one index is 4; a lower index with 3 wins over both
    assert A.scheme_model(sp, [ok, to7], [1], [0], aux=[0, f0 + 9]) == ("refused", 1, 4)
    poor = C.tx(f0 + 3, f0 + 4, B.float2fix(B.floor_fix2float(leaf(f0 + 3)["balance"] * 2)), nonce=0)
    assert A.scheme_model(sp, [poor, to7], [1], [0], aux=[0, f0 + 9]) == ("refused", 0, 3)
    # the builder raises for 10 and 11
    with pytest.raises(ValueError):
        A.builder_batch(sp, [to7], [1], [0], 8, aux=[f0 + 3])


def test_resolve_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage as RU
    path = os.path.join(RU.BUILD, "ledger.ru.txt")
    if not os.path.exists(path):
        pytest.skip("the library was not built in this tree (no build/ledger.ru.txt)")
    rows = {r["name"]: r for r in RU.table([path])}
    for name in ("hz::k_ledger_resolve", "hz::k_ledger_resolve_pick", "hz::k_ledger_scan", "hz::k_ledger_pack"):
        assert name in rows, sorted(rows)
        assert rows[name]["scratch"] == 0, (name, rows[name])


def test_new_symbols_are_declared_and_exported():
    from circuits_amd.capi import EXPORTS, lib_path
    assert all(s in EXPORTS for s in NEW_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "hermez_witness.h")).read()
    assert all(s + "(" in header for s in NEW_SYMBOLS) and "#define HZ_LEDGER_VERIFY_SIGS 1u" in header
    if not os.path.exists(lib_path()):
        pytest.skip("the library was not built in this tree")
    c = ctypes.CDLL(lib_path())
    assert [s for s in NEW_SYMBOLS if not hasattr(c, s)] == []
