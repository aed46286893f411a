// hz_ledger's exits: an L2 exit or an L1 forceExit (to_idx == 1) takes its amount out of the sender as a transfer does
// and puts it into the leaf at key from_idx of the batch's EXIT TREE, an hz_smt that is empty when the batch starts
// (src/rollup-tx-states.circom:137-221, src/rollup-tx.circom:382-443, 551-590). The state side is the ledger's as it stands: the row's
// sender event, no receiver event. The exit side is three kernels around smt_internal.h's tree update:
//   k_ledger_exit_scan    a lane per exit key: its operations lie behind each other (grouped order, ledger_plan.h) and the lane carries
//                         the exit leaf's balance through them. The first is the INSERT of {tokenID, sign, ay, ethAddr} of the sender's
//                         resident leaf (no batch changes them), nonce 0, balance eff3; every later one an UPDATE, balance += eff3. It
//                         writes the leaf before each operation, the new leaf as the [4][32] record the tree update reads, the leaf the
//                         key ends with, and lowers the failure word with reason 5 where a new exit balance reaches 2^192
//   -- the ledger's one synchronise: the failure word. A refused batch has written per-call buffers only --
//   the tree update       smt_apply_launch on the exit tree's own stream, behind an event: it does not depend on the state tree's
//   k_ledger_exit_pack    a lane per row: the leaf-2 rows of an exit row (zero for an insert, the exit leaf before for an update),
//                         newExit, isOld0_2, oldKey2 and oldValue2 as 32-byte elements
//   k_ledger_exit_gather  thread (row, d): siblings2 of an exit row from the tree's siblings, the exit root after every row
// eff3 is the amount of an L2 exit (k_ledger_tx leaves it) and effectiveAmount3 of a forceExit (k_ledger_l1 leaves it: 0 where the
// amount is nullified, and the operation still happens), both in the exit-amount buffer at the operation's grouped position.
// The per-operation routines are HZ_HD: the kernels and tests/native/ledger_exit_check.cpp share them.
#pragma once
#include <stdint.h>
#include "u256.h"

namespace hz {

enum : uint32_t { EXIT_OP_INSERT = 1u, EXIT_OP_IS_OLD0 = 2u };

// one exit operation in grouped order
struct LedgerExitPos {
    uint32_t op, row, acct;   // its number in row order, its row, the sender: account - first_idx
};

// one exit operation in row order, as the pack kernel reads it: the planners' integers (ledger_plan.h, smt_plan.h)
struct LedgerExitOp {
    uint64_t old_key;
    uint32_t acct, flags;   // EXIT_OP_INSERT | EXIT_OP_IS_OLD0
};

// e0 of the exit leaf of a sender whose leaf holds e0_s: tokenID | nonce 0 | sign << 72
HZ_HD Fc exit_leaf_e0(const Fc& e0_s) {
    Fc r = fc_zero();
    r.v[0] = e0_s.v[0];
    r.v[2] = e0_s.v[2] & 0x100u;
    return r;
}

// one operation on the exit leaf's balance; -> the new balance is a leaf field (below 2^192). Amounts are below 2^138 and a batch
// has at most 65536 operations: the sum cannot wrap
HZ_HD bool exit_step(Fc& bal, const Fc& eff3) {
    bal = u256_add(bal, eff3);
    return (bal.v[6] | bal.v[7]) == 0u;
}

// tokenID, nonce, sign, balance of an exit leaf (e0, bal) as the circuit's leaf-2 rows
HZ_HD void exit_leaf_rows(const Fc& e0, const Fc& bal, Fc f[4]) {
    f[0] = fc_zero();
    f[1] = fc_zero();
    f[2] = fc_zero();
    f[0].v[0] = e0.v[0];
    f[1].v[0] = e0.v[1];
    f[1].v[1] = e0.v[2] & 0xFFu;
    f[2].v[0] = (e0.v[2] >> 8) & 1u;
    f[3] = bal;
}

// oldKey2 / oldValue2 of an operation: the tree's, on an insert that met a leaf; zero otherwise
HZ_HD bool exit_reports_old(uint32_t flags) { return (flags & EXIT_OP_INSERT) != 0u && (flags & EXIT_OP_IS_OLD0) == 0u; }

#if defined(__HIPCC__)
// the arrays the exit kernels write, as device pointers: the leaf-2 rows and siblings2 of hz_ledger_out, hz_ledger_exit_out's six
struct LedgerExitOutDev {
    uint8_t* tx2[6];
    uint8_t* sib2;
    uint8_t* x[6];
};
enum { XO_NEW_EXIT = 0, XO_IS_OLD0 = 1, XO_OLD_KEY = 2, XO_OLD_VALUE = 3, XO_ROOT_AFTER = 4, XO_NEW_ROOT = 5 };

// a lane per exit key. final: the leaf each key ends with, plane-major [4][G] as the resident planes are
__global__ __launch_bounds__(64) void k_ledger_exit_scan(const LedgerExitPos* __restrict__ pos, const uint32_t* __restrict__ seg_start, const uint8_t* __restrict__ amt,
                                                         const uint8_t* __restrict__ planes, uint8_t* __restrict__ before, uint8_t* __restrict__ records,
                                                         uint8_t* __restrict__ final_leaf, uint32_t* __restrict__ fail_word, uint32_t N, uint32_t G) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const uint32_t p0 = seg_start[g], p1 = seg_start[g + 1];
    const uint32_t acct = pos[p0].acct;
    const Fc e0 = exit_leaf_e0(load_fr(planes + (size_t)acct * 32));
    const Fc ay = load_fr(planes + ((size_t)2 * N + acct) * 32);
    const Fc eth = load_fr(planes + ((size_t)3 * N + acct) * 32);
    Fc bal = fc_zero();
    for (uint32_t p = p0; p < p1; p++) {
        const LedgerExitPos x = pos[p];
        store_fr(before + (size_t)x.op * 64, p == p0 ? fc_zero() : e0);   // the insert has no leaf before it
        store_fr(before + (size_t)x.op * 64 + 32, bal);
        if (!exit_step(bal, load_fr(amt + (size_t)p * 32))) atomicMin(fail_word, (x.row << 8) | 5u);
        uint8_t* rec = records + (size_t)x.op * 128;
        store_fr(rec, e0);
        store_fr(rec + 32, bal);
        store_fr(rec + 64, ay);
        store_fr(rec + 96, eth);
    }
    store_fr(final_leaf + (size_t)g * 32, e0);
    store_fr(final_leaf + ((size_t)G + g) * 32, bal);
    store_fr(final_leaf + ((size_t)2 * G + g) * 32, ay);
    store_fr(final_leaf + ((size_t)3 * G + g) * 32, eth);
}

// a lane per row with an exit operation (the other rows keep k_ledger_pack's leaf-2 rows and the zeros of the exit arrays)
__global__ __launch_bounds__(64) void k_ledger_exit_pack(const LedgerExitOutDev o, const int32_t* __restrict__ ev_x, const LedgerExitOp* __restrict__ ops,
                                                         const uint8_t* __restrict__ before, const uint8_t* __restrict__ old_value, const uint8_t* __restrict__ planes,
                                                         uint32_t N, uint32_t R) {
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= R) return;
    const int32_t x = ev_x[u];
    if (x < 0) return;
    const LedgerExitOp op = ops[x];
    const bool insert = (op.flags & EXIT_OP_INSERT) != 0u;
    Fc f[6];
#pragma unroll
    for (int q = 0; q < 6; q++) f[q] = fc_zero();
    if (!insert) {
        exit_leaf_rows(load_fr(before + (size_t)x * 64), load_fr(before + (size_t)x * 64 + 32), f);
        f[4] = load_fr(planes + ((size_t)2 * N + op.acct) * 32);
        f[5] = load_fr(planes + ((size_t)3 * N + op.acct) * 32);
    }
#pragma unroll
    for (int q = 0; q < 6; q++) store_fr(o.tx2[q] + (size_t)u * 32, f[q]);
    const bool old = exit_reports_old(op.flags);
    store_fr(o.x[XO_NEW_EXIT] + (size_t)u * 32, u256_u64(insert ? 1ull : 0ull));
    store_fr(o.x[XO_IS_OLD0] + (size_t)u * 32, u256_u64((op.flags & EXIT_OP_IS_OLD0) ? 1ull : 0ull));
    store_fr(o.x[XO_OLD_KEY] + (size_t)u * 32, u256_u64(old ? op.old_key : 0ull));
    store_fr(o.x[XO_OLD_VALUE] + (size_t)u * 32, old ? load_fr(old_value + (size_t)x * 32) : fc_zero());
}

// thread (row u, d): sibling d of the row's exit operation (d < n_sib; the tree's buffer is zero-padded), or the exit root after the
// row (d == n_sib): the root version after the last exit operation of rows 0 .. u, roots[0] (the empty tree's 0) when there is none
__global__ __launch_bounds__(256) void k_ledger_exit_gather(const LedgerExitOutDev o, const int32_t* __restrict__ ev_x, const int32_t* __restrict__ last_x,
                                                            const uint8_t* __restrict__ sib, const uint8_t* __restrict__ roots, uint32_t n_sib, uint32_t R) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)R * (n_sib + 1)) return;
    const uint32_t u = (uint32_t)(t / (n_sib + 1)), d = (uint32_t)(t - (size_t)u * (n_sib + 1));
    if (d == n_sib) {
        store_fr(o.x[XO_ROOT_AFTER] + (size_t)u * 32, load_fr(roots + (size_t)(last_x[u] + 1) * 32));
        return;
    }
    const int32_t x = ev_x[u];
    if (x >= 0) store_fr(o.sib2 + ((size_t)u * n_sib + d) * 32, load_fr(sib + ((size_t)x * n_sib + d) * 32));
}
#endif

}  // namespace hz
