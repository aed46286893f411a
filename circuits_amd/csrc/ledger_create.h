// hz_ledger's create rows: an L1 row with from_idx == 0 -- createAccount, createAccountDeposit,
// createAccountDepositTransfer -- makes account auxFromIdx = last_idx + 1, last_idx running over the rows
// (src/rollup-tx-states.circom:41-54, 187, 250-313, src/rollup-tx.circom:278-380, src/lib/utils-bjj.circom:12-28). The new leaf takes every
// field from the row: tokenID, nonce 0, ethAddr = from_eth_addr, sign = bit 255 of fromBjjCompressed, ay = its bits 0 .. 253 as an
// integer reduced once modulo r (below 2^254 < 2r; bit 254 is not read), balance 0. Only a growing ledger (hz_ledger_create_growing) can
// take one: its planes have room behind the live accounts and its state tree is an hz_smt.
//   k_ledger_create       a lane per create row, queued before everything else of the call: the key decoded, the static fields of the
//                         new account into its plane slot (e0 = token | sign << 72, balance 0, ay, ethAddr). The slots lie beyond the
//                         ledger's size: nothing observes them unless the call succeeds and raises it
//   -- from here the pipeline sees a deposit on auxFromIdx: k_ledger_l1's nullifiers read a matching token and address, the scan
//      carries the balance from 0, the tree's planner finds the key absent and makes the update an INSERT --
//   k_ledger_create_pack  a lane per row: auxFromIdx, isOld0_1, oldKey1, oldValue1 (the tree's, on an insert that met a leaf; zero
//                         otherwise) and the last idx after the row as 32-byte elements; lane 0 the new last idx
//   k_ledger_load_records a lane per account: the four plane fields as the [4][32] record the tree update reads (hz_ledger_load_accounts)
// The per-row routines are HZ_HD: the kernels and tests/native/ledger_create_check.cpp share them.
#pragma once
#include <stdint.h>
#include "u256.h"

namespace hz {

enum : uint32_t { CREATE_ROW = 1u, CREATE_IS_OLD0 = 2u };

// one create row as k_ledger_create reads it
struct LedgerCreateDev {
    uint32_t acct, token_id;   // auxFromIdx - first_idx: the plane slot
    uint32_t bjj[8];           // fromBjjCompressed, little-endian limbs
    uint32_t from_eth[5];      // 160 bits
};

// one row of the batch as k_ledger_create_pack reads it: the planners' integers (ledger_plan.h, smt_plan.h)
struct LedgerCreateRow {
    uint64_t aux_from, idx_after, old_key;
    int32_t ev;        // the row's sender event: the insert, for a create row
    uint32_t flags;    // CREATE_ROW | CREATE_IS_OLD0
};

// bits 0 .. 253 of the compressed key as an integer, reduced once modulo r; -> ay, *sign = bit 255
HZ_HD Fc create_decode_key(const Fc& bjj, uint32_t* sign) {
    Fc ay = bjj;
    ay.v[7] &= 0x3FFFFFFFu;
    fc_cond_sub_p(ay.v);
    *sign = bjj.v[7] >> 31;
    return ay;
}

// e0 of the new leaf: tokenID | nonce 0 | sign << 72
HZ_HD Fc create_leaf_e0(uint32_t token_id, uint32_t sign) {
    Fc r = fc_zero();
    r.v[0] = token_id;
    r.v[2] = (sign & 1u) << 8;
    return r;
}

// the running index: the last idx after a row that starts at `last`
HZ_HD uint64_t create_next_idx(uint64_t last, bool creates) { return last + (creates ? 1ull : 0ull); }

// oldKey1 / oldValue1 of a row: the tree's, on a create whose insert met a leaf; zero otherwise
HZ_HD bool create_reports_old(uint32_t flags) { return (flags & CREATE_ROW) != 0u && (flags & CREATE_IS_OLD0) == 0u; }

#if defined(__HIPCC__)
enum { CO_AUX_FROM = 0, CO_IS_OLD0 = 1, CO_OLD_KEY = 2, CO_OLD_VALUE = 3, CO_IDX_AFTER = 4, CO_NEW_LAST = 5 };
struct LedgerCreateOutDev {
    uint8_t* a[6];
};

// a lane per create row; N is the plane stride (the ledger's capacity), every acct is below it (the host has checked)
__global__ __launch_bounds__(64) void k_ledger_create(const LedgerCreateDev* __restrict__ rows, uint8_t* __restrict__ planes, uint32_t N, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const LedgerCreateDev c = rows[i];
    if (c.acct >= N) return;
    Fc bjj, eth = fc_zero();
#pragma unroll
    for (int q = 0; q < 8; q++) bjj.v[q] = c.bjj[q];
#pragma unroll
    for (int q = 0; q < 5; q++) eth.v[q] = c.from_eth[q];
    uint32_t sign;
    const Fc ay = create_decode_key(bjj, &sign);
    store_fr(planes + (size_t)c.acct * 32, create_leaf_e0(c.token_id, sign));
    store_fr(planes + ((size_t)N + c.acct) * 32, fc_zero());
    store_fr(planes + ((size_t)2 * N + c.acct) * 32, ay);
    store_fr(planes + ((size_t)3 * N + c.acct) * 32, eth);
}

// a lane per row (at least one lane: lane 0 writes the new last idx)
__global__ __launch_bounds__(64) void k_ledger_create_pack(const LedgerCreateOutDev o, const LedgerCreateRow* __restrict__ rows, const uint8_t* __restrict__ old_value,
                                                           uint64_t new_last, uint32_t R) {
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u == 0) store_fr(o.a[CO_NEW_LAST], u256_u64(new_last));
    if (u >= R) return;
    const LedgerCreateRow r = rows[u];
    const bool old = create_reports_old(r.flags);
    store_fr(o.a[CO_AUX_FROM] + (size_t)u * 32, u256_u64(r.aux_from));
    store_fr(o.a[CO_IS_OLD0] + (size_t)u * 32, u256_u64((r.flags & CREATE_IS_OLD0) ? 1ull : 0ull));
    store_fr(o.a[CO_OLD_KEY] + (size_t)u * 32, u256_u64(old ? r.old_key : 0ull));
    store_fr(o.a[CO_OLD_VALUE] + (size_t)u * 32, old ? load_fr(old_value + (size_t)r.ev * 32) : fc_zero());
    store_fr(o.a[CO_IDX_AFTER] + (size_t)u * 32, u256_u64(r.idx_after));
}

// a lane per account base + j, j < n: records[j] = {e0, balance, ay, ethAddr} of the planes (stride N)
__global__ __launch_bounds__(256) void k_ledger_load_records(const uint8_t* __restrict__ planes, uint8_t* __restrict__ records, uint32_t N, uint32_t base, uint32_t n) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
#pragma unroll
    for (int f = 0; f < 4; f++) store_fr(records + ((size_t)j * 4 + f) * 32, load_fr(planes + ((size_t)f * N + base + j) * 32));
}
#endif

}  // namespace hz
