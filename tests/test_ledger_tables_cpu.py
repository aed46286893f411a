"""The ledger's integer tables (csrc/ledger_tables.h) without a device: tests/native/ledger_tables_check.cpp built for the host under the
address and undefined-behaviour sanitizers lays out and fills the blocks of the apply, selection, lookup and withdraw calls into heap
blocks of exactly their size and compares them with a plain recomputation, on the seeded batches of the exit and create drawers, the
named exit edges and the small shapes at which a length can go wrong. What the device computes of these tables is guarded by the GPU
tests of every call family."""
import os
import subprocess

import ledger_addr_common as A
import ledger_common as C
import ledger_create_common as K
import ledger_exit_common as X
import ledger_l1_common as L1

ACTIVE, EXIT, UNRESOLVED, RECEIVER = 1, 2, 4, 8


def select_flags(t, eff_to):
    """SelectTxDev.flags as hz_ledger_select_batch states them"""
    if not t.get("fromIdx", 0):
        return 0
    to, amount = t.get("toIdx", 0), L1.has_amount(t)
    exits, unresolved = to == X.EXIT, to == 0 and amount and eff_to == 0
    return ACTIVE | (EXIT if exits else 0) | (UNRESOLVED if unresolved else 0) | (RECEIVER if amount and not exits and not unresolved else 0)


def batch_lines(first_idx, l1_txs, l2_txs, plan, idxs, eff_to=None, exits=True, creates=False, running=None, partner=None):
    """one batch in the program's line format. l1_txs carry auxFromIdx in fromIdx's place already; running: (aux_from, idx_after)"""
    eff_to = eff_to or [0] * len(l2_txs)
    aux, after = running or ([0] * len(l1_txs), [0] * len(l1_txs))
    lines = ["b %x %x %x %x" % (first_idx, exits, creates, partner is not None)]
    lines += ["f %x %x" % (tok, idx) for tok, idx in zip(plan, idxs)]
    for i, t in enumerate(l1_txs):
        lines.append("l %x %x %x %x %x %x %x %x" % (t["fromIdx"], t.get("toIdx", 0), t.get("amountF", 0), t.get("loadAmountF", 0), t.get("tokenID", 0),
                                                     t.get("fromEthAddr", 0), aux[i], after[i]))
    flags = []
    for i, t in enumerate(l2_txs):
        flags.append(select_flags(t, eff_to[i]))
        lines.append("t %x %x %x %x %x %x %x %x %x" % (t.get("fromIdx", 0), t.get("toIdx", 0), t.get("amountF", 0), t.get("nonce", 0), t.get("tokenID", 0),
                                                        t.get("userFee", 0), eff_to[i], (partner[i] + 1) if partner else 0, flags[-1]))
    return lines + ["e"], flags


def all_batches():
    """-> [(name, lines, flags)]"""
    out = []

    def add(name, *a, **kw):
        lines, flags = batch_lines(*a, **kw)
        out.append((name, lines, flags))
    sp = X.exit_state(6)
    f0 = sp.first_idx
    for n, (st, l1_txs, l2_txs) in enumerate([(st, a, b) for _, st, a, b in X.seeded_batches()] + [(sp, a, b) for a, b in X.edge_batches(sp).values()]):
        eff = [A.brute_force(st, t) if A.is_to_addr(t) and L1.has_amount(t) else 0 for t in l2_txs]
        partner = [(i + 1) % len(l2_txs) if i % 3 == 0 else -1 for i in range(len(l2_txs))] if n % 2 and len(l2_txs) > 1 else None
        add("exit %d" % n, st.first_idx, l1_txs, l2_txs + [{}], [1, 2, 0], L1.fee_accounts(st)[:3], eff + [0], partner=partner + [-1] if partner else None)
        if any(eff):   # the same pool with its destinations unresolved: the selection alone
            add("unresolved %d" % n, st.first_idx, l1_txs, l2_txs, [], [], [0] * len(l2_txs))
    for seed in range(6):   # create rows: the rows with auxFromIdx in fromIdx's place, the running index beside them
        acc = (K.Accounts([]), K.few_accounts(5), K.Accounts.of(C.base_state(4)))[seed % 3]
        l1_txs, l2_txs = K.draw_batch(acc, seed)
        aux, after = K.running_index(acc.first_idx, acc.n, 1 << 12, l1_txs)
        rows = [dict(t, fromIdx=aux[i] or t["fromIdx"]) for i, t in enumerate(l1_txs)]
        add("create %d" % seed, acc.first_idx, rows, l2_txs, [1, 2], [after[-1], 0], creates=True, running=(aux, after))
    # ---- the small shapes
    t1, t2 = C.tx(f0 + 3, f0 + 4, 5, 176, nonce=0), C.tx(f0 + 4, f0 + 3, 7, 0, nonce=0)
    add("R = 0 with F = 1", f0, [], [], [1], [f0 + 9])
    add("R = 0, no fee account", f0, [], [], [1], [0])
    add("R = 1", f0, [], [t1], [1], [f0 + 9])
    add("n_l1 = 0", f0, [], [t1, t2], [], [])
    add("m = 0", f0, [X.fx(sp, f0 + 1, 5), L1.own(sp, f0 + 2, f0 + 1, 3, 9)], [], [1], [f0 + 9])
    add("X = 0 with exits allowed", f0, [L1.own(sp, f0 + 2, 0, 0, 9)], [t1, X.x2(f0 + 5, 0, nonce=0)], [1], [0])
    add("M = 0: all NOP", f0, [], [{}, {}, {}], [1, 2], [0, 0])
    add("R = 65: two fee chunks", f0, [], [C.tx(f0 + i % 7, f0 + 8 + i % 5, 1 + i, 176, nonce=i // 7) for i in range(65)], [1, 2, 3], [f0 + 20, 0, f0 + 21])
    add("a hot receiver", f0, [], [C.tx(f0 + 1 + i, f0, 2, 0, nonce=0) for i in range(39)], [1], [f0])
    add("a forceExit without amount", f0, [X.fx(sp, f0 + 1, 0), X.fx(sp, f0 + 1, 6)], [X.x2(f0 + 1, 3, nonce=0)], [1], [0])
    add("creates with n_creates = 0", f0, [L1.own(sp, f0 + 2, f0 + 1, 3, 9)], [t1], [1], [f0 + 9], creates=True, running=([0], [f0 + 63]))
    add("exits not allowed", f0, [L1.own(sp, f0 + 2, f0 + 1, 3, 9)], [t1, t2], [1], [f0 + 9], exits=False)
    return out


def test_host_build_of_the_tables_agrees_with_a_plain_recomputation(tmp_path):
    batches = all_batches()
    flags = {f for _, _, fl in batches for f in fl}
    # the five flag combinations the selection can state, and the shapes
    assert flags == {0, ACTIVE, ACTIVE | EXIT, ACTIVE | UNRESOLVED, ACTIVE | RECEIVER}, sorted(flags)
    hot = next(lines for name, lines, _ in batches if name == "a hot receiver")
    assert sum(ln.startswith("t ") for ln in hot) == 39   # 39 receiver events and the fee event on one account: a group of 40
    text = "\n".join(ln for _, lines, _ in batches for ln in lines) + "\n"
    src = os.path.join(os.path.dirname(__file__), "native", "ledger_tables_check.cpp")
    exe = str(tmp_path / "ledger_tables_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    unresolved = sum(name.startswith("unresolved") for name, _, _ in batches)
    n = 14 * (len(batches) - unresolved) + 5 * unresolved   # nine checks of the apply call's blocks, three of the selection's, two of the lookups'
    assert r.returncode == 0 and "cases=%d mismatches=0" % n in r.stdout, r.stdout + r.stderr
    # the program does judge: one expectation changed is one mismatch
    lines = text.splitlines()
    at = next(i for i, ln in enumerate(lines) if ln.startswith("t ") and ln.endswith(" %x" % (ACTIVE | RECEIVER)))
    lines[at] = lines[at][:-1] + "1"
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 1 and "mismatches=1" in r.stdout and "SelectTxDev flags" in r.stderr, r.stdout + r.stderr
