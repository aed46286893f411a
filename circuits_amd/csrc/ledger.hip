// hz_ledger: an hz_state -- or, on a growing ledger, an hz_smt -- plus the resident leaf fields, and batches computed and applied on the
// device (DESIGN.md 8c .. 8k).
//
// The split is the library's: the host does integer work on indices only (ledger_plan.h: events, their grouping by account, fee slots;
// ledger_tables.h: the typed tables of one call; ledger_checks.h: every argument check, the ledger as five integers), the device everything
// that touches a 256-bit value. Every exported apply call states
// itself as a LedgerCall -- the request, the host destinations, and what it accepts: by_addr (to_idx == 0, a receiver named by address or
// key, 8e), is_batch (an L1 run in front: the batch has n_l1 + m rows and "transaction" below reads "row", 8f), exits (to_idx == 1 into
// the batch's exit tree, an hz_smt the ledger owns, 8g), creates (from_idx == 0 in L1 rows of a growing ledger, 8h), rq != NULL (atomic
// links, 8i) -- and ledger_apply runs it in stages over one LedgerApply on the stack:
//   1 plan      the argument checks (ledger_checks.h) in the order their errors win, run once for either kind of call (ledger_prepare). A
//               by_addr call makes the rows the plan is made of: the L1 rows with auxFromIdx in from_idx's place; k_ledger_create, a lane per create row, the new account's
//               static fields into its plane slot beyond `live`; the receivers -- k_ledger_resolve, a lane per account probing the table of
//               the batch's distinct queries, k_ledger_resolve_pick, a lane per transaction, and the lookup's synchronise: the planner needs
//               them, and a destination nobody holds is reason 9 here. Then the plan, and the exit tree's own (smt_apply_prepare)
//   2 buffers   the layouts (LedgerTables, LedgerWork) and the room: no allocation after this stage but the signatures' and the links'
//   3 tables    LedgerTables::fill into the pinned block, the state tree's plan (state_apply_prepare / smt_apply_prepare on the same record
//               buffer), then the create rows, which read it
//   4 launch    one upload, then on the tree's stream
//                 k_ledger_tx        a lane per row: float40 -> amount, fee = amount x table[selector], the signed deltas of its events; a
//                                    fee of 2^128 or more is reason 16
//                 k_ledger_l1        (ledger_l1.h) one workgroup: the nullifiers and the ordered recurrence of the L1 run over balances in
//                                    LDS; the L1 events' deltas beside k_ledger_tx's, and the flag bytes
//                 k_ledger_fee_sum / _fee_scan   the accumulated fees after every row, per slot; the last row is the fee events' delta
//                 k_ledger_scan      a lane per account: balance and e0 carried through its events in order, token, nonce, underflow and
//                                    overflow checked (not on L1 events: an invalid L1 transaction is nullified, not refused), the receiver
//                                    against the signed destination (10, 11), every event's leaf before and after
//                 k_ledger_exit_scan a lane per exit key: the exit leaf before and after each of its operations
//                 the signature kernels of ledger_sig.hip (7, 8) where the call verifies; k_ledger_rq, a lane per L2 row: its rq fields
//                                    against the link fields of the row rqOffset names (13), on V2 rows k_ledger_sig_v2 writes otherwise
//               all lowering one failure word with atomicMin -- and the one synchronise
//   5 verdict   a refused batch ends here; nothing resident has been written
//   6 commit    k_ledger_pack (the before-fields, auxToIdx, the leaf-2 rows of a zero-amount transfer to an address), the tree update
//               (state_apply_launch / smt_apply_launch), k_ledger_create_pack, k_ledger_gather (siblings, the root after each row and fee
//               slot), k_ledger_writeback (the last leaf of every touched account into the planes); the exit tree's update on its own
//               stream behind an event, then k_ledger_exit_pack / _gather
//   7 copy out  to the host arrays the caller gave    8 finish   the trees' updates finished, the times, what the getters hand out
// hz_ledger_verify_l2 runs the signature kernels alone (ledger_sig_links_launch: the one launch of them and of the link check, for every
// call). The hz_ledger_plan_* exports, the host half alone, stand in one section at the end. hz_ledger_select_batch (8j) shares ledger_prepare's pieces and runs
// k_ledger_select over a pool. hz_ledger_exit_keep (8k) freezes the exit tree a batch left into the ledger's archive -- copies, no kernel --
// and hz_ledger_withdraw_rows answers (batch, idx) queries over the kept trees (ledger_archive.h: k_withdraw_walk, k_withdraw_fill).
// Values are plain 256-bit integers in eight 32-bit limbs (the Fc container of fr.h, nothing is reduced modulo r); deltas are two's
// complement: every true prefix is below 2^220 in magnitude, so a set top bit means "negative"; the arithmetic is u256.h's, shared with
// ledger_sig.h. Buffers are hostutil.h's, events and time spans resident.h's; the stream is the tree's (state_stream / smt_stream).
#define HZ_FR_INLINE 1
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <utility>
#include <vector>
#include "../../include/hermez_witness.h"
#include "devcommon.h"
#include "ledger_plan.h"
#include "ledger_resolve.h"
#include "resident.h"
#include "state_internal.h"
#include "u256.h"
#include "ledger_fee.h"
#include "ledger_l1.h"
#include "ledger_exit.h"
#include "ledger_create.h"
#include "ledger_rq.h"
#include "ledger_select.h"
#include "ledger_archive.h"
#include "ledger_inputs.h"
#include "ledger_tables.h"
#include "ledger_checks.h"
#include "ledger_journal.h"
#include "ctx_internal.h"
#include "smt_internal.h"
#include "smt_plan.h"

#define HZ_ARCHIVE_SLAB_BYTES ((size_t)1 << 20)   // a slab of the exit archive; a snapshot larger than this gets a slab of its own size

namespace hz {

// the 27 output arrays in hz_ledger_out's order, as device pointers
struct LedgerOutDev {
    uint8_t* a[HZ_LEDGER_ARRAYS];
};
enum { LO_TX1 = 0, LO_SIB1 = 6, LO_TX2 = 7, LO_SIB2 = 13, LO_ROOT_AFTER = 14, LO_ACC_FEE = 15, LO_TX3 = 16, LO_SIB3 = 22, LO_ROOT_FEE = 23,
       LO_FINAL_FEE = 24, LO_OLD_ROOT = 25, LO_NEW_ROOT = 26 };

// ---- kernels ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ledger_fail(uint32_t* word, uint32_t unit, uint32_t reason) { atomicMin(word, (unit << 8) | reason); }

// amount = mantissa x 10^exponent (src/lib/decode-float.circom), fee (src/compute-fee.circom); deltas at the events' grouped positions.
// A fee of 2^128 or more lowers the failure word with reason 16 at the row: only where the circuit applies the fee, an L2 row that is no NOP
__global__ __launch_bounds__(64) void k_ledger_tx(const hz_l2tx* __restrict__ txs, const int32_t* __restrict__ pos_s, const int32_t* __restrict__ pos_r,
                                                  uint8_t* __restrict__ fee_out, uint8_t* __restrict__ delta, const int32_t* __restrict__ pos_x,
                                                  uint8_t* __restrict__ exit_amt, uint32_t* __restrict__ fail_word, uint32_t m, uint32_t n_l1) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    Fc fee = fc_zero();
    if (i >= n_l1 && txs[i].from_idx != 0) {   // an L1 row pays no fee; its deltas are k_ledger_l1's
        const Fc amount = l1_float40(txs[i].amount_f);
        const uint32_t sel = txs[i].user_fee;
        fee = ledger_fee(amount, sel);
        if (ledger_fee_overflows(fee)) ledger_fail(fail_word, i, HZ_LEDGER_FEE_OVERFLOW);
        store_fr(delta + (size_t)pos_s[i] * 32, u256_neg(u256_add(amount, fee)));
        if (pos_r[i] >= 0) store_fr(delta + (size_t)pos_r[i] * 32, amount);
        if (pos_x && pos_x[i] >= 0) store_fr(exit_amt + (size_t)pos_x[i] * 32, amount);   // an exit: no receiver delta (pos_x == NULL: the call takes none)
    }
    store_fr(fee_out + (size_t)i * 32, fee);
}

// fee of slot j summed over the transactions of chunk c
__global__ __launch_bounds__(64) void k_ledger_fee_sum(const uint8_t* __restrict__ fee, const int32_t* __restrict__ slot, uint8_t* __restrict__ chunk_sum,
                                                       uint32_t m, uint32_t F) {
    const uint32_t c = blockIdx.x, j = threadIdx.x;
    if (j >= F) return;
    Fc acc = fc_zero();
    const uint32_t end = min(m, (c + 1) * HZ_LEDGER_CHUNK);
    for (uint32_t i = c * HZ_LEDGER_CHUNK; i < end; i++)
        if (slot[i] == (int32_t)j) acc = u256_add(acc, load_fr(fee + (size_t)i * 32));
    store_fr(chunk_sum + ((size_t)c * F + j) * 32, acc);
}

// accumulated fee j after every transaction of chunk c; the last chunk leaves the final fees and the fee events' deltas
__global__ __launch_bounds__(64) void k_ledger_fee_scan(const uint8_t* __restrict__ fee, const int32_t* __restrict__ slot, const uint8_t* __restrict__ chunk_sum,
                                                        const int32_t* __restrict__ pos_fee, uint8_t* __restrict__ acc_after, uint8_t* __restrict__ final_fee,
                                                        uint8_t* __restrict__ delta, uint32_t m, uint32_t F, uint32_t n_chunks) {
    const uint32_t c = blockIdx.x, j = threadIdx.x;
    if (j >= F) return;
    Fc acc = fc_zero();
    for (uint32_t b = 0; b < c; b++) acc = u256_add(acc, load_fr(chunk_sum + ((size_t)b * F + j) * 32));
    const uint32_t end = min(m, (c + 1) * HZ_LEDGER_CHUNK);
    for (uint32_t i = c * HZ_LEDGER_CHUNK; i < end; i++) {
        if (slot[i] == (int32_t)j) acc = u256_add(acc, load_fr(fee + (size_t)i * 32));
        store_fr(acc_after + ((size_t)i * F + j) * 32, acc);
    }
    if (c + 1 == n_chunks) {
        store_fr(final_fee + (size_t)j * 32, acc);
        if (pos_fee[j] >= 0) store_fr(delta + (size_t)pos_fee[j] * 32, acc);
    }
}

// a lane per account group: the leaf before and after every event of the account, in order
__global__ __launch_bounds__(64) void k_ledger_scan(const LedgerPos* __restrict__ pos, const uint32_t* __restrict__ seg_start, const hz_l2tx* __restrict__ txs,
                                                    const hz_l2sig* __restrict__ sigs, const uint32_t* __restrict__ plan_tok, const uint8_t* __restrict__ delta, const uint8_t* __restrict__ planes,
                                                    uint8_t* __restrict__ before, uint8_t* __restrict__ records, uint32_t* __restrict__ fail_word, uint32_t N,
                                                    uint32_t G, uint32_t m, uint32_t n_l1) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const uint32_t p0 = seg_start[g], p1 = seg_start[g + 1];
    const uint32_t acct = pos[p0].acct;
    Fc e0 = load_fr(planes + (size_t)acct * 32);
    Fc bal = load_fr(planes + ((size_t)N + acct) * 32);
    const Fc ay = load_fr(planes + ((size_t)2 * N + acct) * 32);
    const Fc eth = load_fr(planes + ((size_t)3 * N + acct) * 32);
    for (uint32_t p = p0; p < p1; p++) {
        const LedgerPos ev = pos[p];
        store_fr(before + (size_t)ev.ev * 64, e0);
        store_fr(before + (size_t)ev.ev * 64 + 32, bal);
        const bool sender = ev.kind == LEDGER_EV_SENDER, fee = ev.kind == LEDGER_EV_FEE;
        const bool l1 = ev.kind >= LEDGER_EV_L1_SENDER;   // nullified by k_ledger_l1 where L2 is refused: no token check, no nonce
        const uint32_t tok = fee ? plan_tok[ev.unit - m] : txs[ev.unit].token_id;
        if (!l1 && e0.v[0] != tok) ledger_fail(fail_word, ev.unit, sender ? 1u : fee ? 6u : 4u);
        if (sigs && ev.kind == LEDGER_EV_RECEIVER && txs[ev.unit].to_idx == 0) {   // the signed destination against the receiver's leaf
            const hz_l2sig* sig = sigs + (ev.unit - n_l1);   // sigs belong to the L2 rows
            const Fc to_eth = resolve_load32(sig->to_eth_addr);
            if (!resolve_fc_same(to_eth, eth)) ledger_fail(fail_word, ev.unit, 10u);
            if (resolve_is_any(to_eth) && (!resolve_fc_same(resolve_load32(sig->to_bjj_ay), ay) || (uint32_t)sig->to_bjj_sign != ((e0.v[2] >> 8) & 1u)))
                ledger_fail(fail_word, ev.unit, 11u);
        }
        if (sender) {
            const uint64_t nonce = (uint64_t)e0.v[1] | ((uint64_t)(e0.v[2] & 0xFFu) << 32);
            if (nonce != txs[ev.unit].nonce) ledger_fail(fail_word, ev.unit, 2u);
            const uint64_t next = nonce + 1;   // not wrapped: the circuit feeds nonce + 1 into the state hash (rollup-tx.circom:519)
            if (next >> 40) ledger_fail(fail_word, ev.unit, 12u);
            e0.v[1] = (uint32_t)next;
            e0.v[2] = (e0.v[2] & ~0xFFu) | ((uint32_t)(next >> 32) & 0xFFu);
        }
        bal = u256_add(bal, load_fr(delta + (size_t)p * 32));
        if (bal.v[7] >> 31)
            ledger_fail(fail_word, ev.unit, 3u);
        else if ((bal.v[6] | bal.v[7]) != 0u)
            ledger_fail(fail_word, ev.unit, 5u);
        uint8_t* rec = records + (size_t)ev.ev * 128;
        store_fr(rec, e0);
        store_fr(rec + 32, bal);
        store_fr(rec + 64, ay);
        store_fr(rec + 96, eth);
    }
}

// tokenID, nonce, sign, balance, ay, ethAddr of the leaf event `ev` found, into six arrays at row `row`; ev < 0: zeros, tokenID = tok
__device__ __forceinline__ void ledger_put_leaf(const LedgerOutDev& o, int base, uint32_t row, int32_t ev, uint32_t tok, const uint32_t* __restrict__ ev_acct,
                                                const uint8_t* __restrict__ before, const uint8_t* __restrict__ planes, uint32_t N) {
    Fc f[6];
#pragma unroll
    for (int q = 0; q < 6; q++) f[q] = fc_zero();
    f[0].v[0] = tok;
    if (ev >= 0) {
        const Fc e0 = load_fr(before + (size_t)ev * 64);
        const uint32_t acct = ev_acct[ev];
        f[0].v[0] = e0.v[0];
        f[1].v[0] = e0.v[1];
        f[1].v[1] = e0.v[2] & 0xFFu;
        f[2].v[0] = (e0.v[2] >> 8) & 1u;
        f[3] = load_fr(before + (size_t)ev * 64 + 32);
        f[4] = load_fr(planes + ((size_t)2 * N + acct) * 32);
        f[5] = load_fr(planes + ((size_t)3 * N + acct) * 32);
    }
#pragma unroll
    for (int q = 0; q < 6; q++) store_fr(o.a[base + q] + (size_t)row * 32, f[q]);
}

// a lane per transaction, then a lane per fee slot. With sigs (hz_ledger_apply_l2_addr): the auxToIdx rows, and for a zero-amount
// transfer to an address the leaf-2 rows the circuit compares with the signed destination (processor 2 is a NOP)
__global__ __launch_bounds__(64) void k_ledger_pack(const LedgerOutDev o, const hz_l2tx* __restrict__ txs, const hz_l2sig* __restrict__ sigs,
                                                    uint8_t* __restrict__ aux_rows, uint64_t first_idx, const int32_t* __restrict__ ev_s,
                                                    const int32_t* __restrict__ ev_r, const int32_t* __restrict__ ev_fee, const uint32_t* __restrict__ ev_acct,
                                                    const uint8_t* __restrict__ before, const uint8_t* __restrict__ planes, uint32_t N, uint32_t m, uint32_t F,
                                                    uint32_t n_l1) {
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= m + F) return;
    if (u < m) {
        const bool active = u >= n_l1 && txs[u].from_idx != 0;   // an L2 row; the tokenID2 = token_id row of a NOP processor 2 is L2's only
        ledger_put_leaf(o, LO_TX1, u, ev_s[u], 0u, ev_acct, before, planes, N);
        ledger_put_leaf(o, LO_TX2, u, ev_r[u], active ? txs[u].token_id : 0u, ev_acct, before, planes, N);
        if (sigs) {
            const bool to_addr = active && txs[u].to_idx == 0;
            store_fr(aux_rows + (size_t)u * 32, u256_u64(to_addr && ev_r[u] >= 0 ? first_idx + ev_acct[ev_r[u]] : 0ull));
            if (to_addr && ev_r[u] < 0) {
                const hz_l2sig* sig = sigs + (u - n_l1);
                const Fc to_eth = resolve_load32(sig->to_eth_addr);
                store_fr(o.a[LO_TX2 + 5] + (size_t)u * 32, to_eth);
                if (resolve_is_any(to_eth)) {
                    store_fr(o.a[LO_TX2 + 4] + (size_t)u * 32, resolve_load32(sig->to_bjj_ay));
                    store_fr(o.a[LO_TX2 + 2] + (size_t)u * 32, u256_u64(sig->to_bjj_sign));
                }
            }
        }
    } else {
        ledger_put_leaf(o, LO_TX3, u - m, ev_fee[u - m], 0u, ev_acct, before, planes, N);
    }
}

// thread (unit u, d): sibling d of the unit's events (d < n_sib), or the root after the unit (d == n_sib)
__global__ __launch_bounds__(256) void k_ledger_gather(const LedgerOutDev o, const int32_t* __restrict__ ev_s, const int32_t* __restrict__ ev_r,
                                                       const int32_t* __restrict__ ev_fee, const int32_t* __restrict__ last_ev, const uint8_t* __restrict__ sib,
                                                       const uint8_t* __restrict__ new_root, const uint8_t* __restrict__ root0, uint32_t k, uint32_t n_sib,
                                                       uint32_t m, uint32_t F) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)(m + F) * (n_sib + 1)) return;
    const uint32_t u = (uint32_t)(t / (n_sib + 1)), d = (uint32_t)(t - (size_t)u * (n_sib + 1));
    if (d == n_sib) {
        const int32_t le = last_ev[u];   // [m] of the transactions, then [F] of the fee slots
        uint8_t* dst = u < m ? o.a[LO_ROOT_AFTER] + (size_t)u * 32 : o.a[LO_ROOT_FEE] + (size_t)(u - m) * 32;
        store_fr(dst, le >= 0 ? load_fr(new_root + (size_t)le * 32) : load_fr(root0));
        return;
    }
    if (u < m) {
        const int32_t a = ev_s[u], b = ev_r[u];
        store_fr(o.a[LO_SIB1] + ((size_t)u * n_sib + d) * 32, a >= 0 && d < k ? load_fr(sib + ((size_t)a * n_sib + d) * 32) : fc_zero());
        store_fr(o.a[LO_SIB2] + ((size_t)u * n_sib + d) * 32, b >= 0 && d < k ? load_fr(sib + ((size_t)b * n_sib + d) * 32) : fc_zero());
    } else {
        const int32_t a = ev_fee[u - m];
        store_fr(o.a[LO_SIB3] + ((size_t)(u - m) * n_sib + d) * 32, a >= 0 && d < k ? load_fr(sib + ((size_t)a * n_sib + d) * 32) : fc_zero());
    }
}

// the leaf the last event of every group left, into the resident planes (ay and ethAddr never change)
__global__ __launch_bounds__(64) void k_ledger_writeback(const LedgerPos* __restrict__ pos, const uint32_t* __restrict__ seg_start, const uint8_t* __restrict__ records,
                                                         uint8_t* __restrict__ planes, uint32_t N, uint32_t G) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const LedgerPos ev = pos[seg_start[g + 1] - 1];
    store_fr(planes + (size_t)ev.acct * 32, load_fr(records + (size_t)ev.ev * 128));
    store_fr(planes + ((size_t)N + ev.acct) * 32, load_fr(records + (size_t)ev.ev * 128 + 32));
}

// the undo journal's plane part (ledger_journal.h): thread f * G + g saves plane f of group g's account, consecutive lanes on
// consecutive journal addresses, and the first G threads note the accounts. A create row's account lies at or beyond `live`, the accounts
// the batch found: its slot holds nothing to save. Before k_ledger_writeback, on the same stream
__global__ __launch_bounds__(256) void k_ledger_journal_save(const LedgerPos* __restrict__ pos, const uint32_t* __restrict__ seg_start, const uint8_t* __restrict__ planes,
                                                             uint8_t* __restrict__ out, uint32_t* __restrict__ index, uint32_t N, uint32_t G, uint32_t live) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 4 * G) return;
    const uint32_t f = t / G, g = t - f * G;
    const uint32_t acct = pos[seg_start[g]].acct;
    if (f == 0) index[g] = acct;
    if (acct >= live) return;
    store_fr(out + (size_t)t * 32, load_fr(planes + ((size_t)f * N + acct) * 32));
}

// the same list run the other way: every account appears once in a record
__global__ __launch_bounds__(256) void k_ledger_journal_restore(const uint32_t* __restrict__ index, const uint8_t* __restrict__ saved, uint8_t* __restrict__ planes, uint32_t N,
                                                                uint32_t G, uint32_t live) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 4 * G) return;
    const uint32_t f = t / G, g = t - f * G;
    const uint32_t acct = index[g];
    if (acct >= live) return;
    store_fr(planes + ((size_t)f * N + acct) * 32, load_fr(saved + (size_t)t * 32));
}

// thread (i, f): field f of account i
__global__ __launch_bounds__(256) void k_ledger_accounts(const uint32_t* __restrict__ acct, const uint8_t* __restrict__ planes, uint8_t* __restrict__ out, uint32_t N,
                                                         uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 4 * n) return;
    store_fr(out + (size_t)t * 32, load_fr(planes + ((size_t)(t & 3u) * N + acct[t >> 2]) * 32));
}

// a lane per account: its key probed in the table of the batch's queries; a hit lowers the slot's result to the lowest account
__global__ __launch_bounds__(256) void k_ledger_resolve(const uint8_t* __restrict__ planes, const ResolveKey* __restrict__ table, uint32_t* __restrict__ result,
                                                        uint32_t slots, uint32_t N, uint32_t n) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;   // n accounts to scan, N the plane stride (equal on a dense ledger)
    const Fc e0 = load_fr(planes + (size_t)a * 32);
    const Fc eth = load_fr(planes + ((size_t)3 * N + a) * 32);
    Fc ay = fc_zero();
    if (resolve_is_any(eth)) ay = load_fr(planes + ((size_t)2 * N + a) * 32);
    const int32_t s = resolve_probe(table, slots, resolve_key(e0.v[0], eth, ay, (e0.v[2] >> 8) & 1u));
    // the result only falls: a lane that sees a lower account there already has nothing to add, and the holders of one address (all of
    // them, in a state of few addresses) do not queue on one word
    if (s >= 0 && a < __atomic_load_n(result + s, __ATOMIC_RELAXED)) atomicMin(result + s, a);
}

// a lane per transaction: the receiver its slot found as an index, or 0 (no query, or no account matches)
__global__ __launch_bounds__(64) void k_ledger_resolve_pick(const int32_t* __restrict__ tx_slot, const uint32_t* __restrict__ result, uint64_t* __restrict__ out,
                                                            uint64_t first_idx, uint32_t m) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int32_t s = tx_slot[i];
    const uint32_t a = s >= 0 ? result[s] : HZ_RESOLVE_NONE;
    out[i] = a != HZ_RESOLVE_NONE ? first_idx + a : 0ull;
}

// a lane per L2 transaction, row n_l1 + i of n_l1 + m: its rq fields against its target's link fields (ledger_rq.h). v2: the message
// kernel's (or k_ledger_sig_v2's) rows of this call, written by an earlier kernel of the same stream; a NOP target's row is zero there
// already, its toEthAddr / toBjjAy are masked here
__global__ __launch_bounds__(64) void k_ledger_rq(const hz_l2tx* __restrict__ txs, const hz_l2sig* __restrict__ sigs, const uint8_t* __restrict__ rq,
                                                  const uint8_t* __restrict__ v2, uint32_t* __restrict__ fail_word, uint8_t* __restrict__ verdict, uint32_t m,
                                                  uint32_t n_l1, uint32_t unit_base) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    if (txs[i].from_idx == 0) return;   // a NOP's entry is not looked at
    const uint8_t* off = rq + (size_t)3 * m * 32;
    const int64_t row = rq_target_row((uint64_t)n_l1 + i, off[i], n_l1, (uint64_t)n_l1 + m);
    Fc t_v2 = fc_zero(), t_eth = fc_zero(), t_ay = fc_zero();
    if (row >= 0) {
        const uint32_t j = (uint32_t)(row - (int64_t)n_l1);   // n_l1 <= row < n_l1 + m
        if (txs[j].from_idx != 0) {
            t_v2 = load_fr(v2 + (size_t)j * 32);
            t_eth = resolve_load32(sigs[j].to_eth_addr);
            t_ay = resolve_load32(sigs[j].to_bjj_ay);
        }
    }
    const bool ok = rq_fields_match(load_fr(rq + (size_t)i * 32), load_fr(rq + ((size_t)m + i) * 32), load_fr(rq + ((size_t)2 * m + i) * 32), t_v2, t_eth, t_ay);
    if (!ok) {
        if (verdict && verdict[i] == 0u) verdict[i] = (uint8_t)HZ_RQ_REASON;   // 7 and 8 stay
        if (fail_word) atomicMin(fail_word, ((unit_base + i) << 8) | HZ_RQ_REASON);
    }
}

// RollupMain's packed inputs (ledger_inputs.h): one launch over the descriptor table, a block range per signal found by
// bisection as k_unpack_inputs does. A lane writes one 32-byte element as two 16-byte stores -- a row of a source array, one element of it,
// zeros, or a signal packed from the uploaded rows (txs: the R rows as the per-row kernels read them, l1 / crow: the L1 run's and the create
// rows' tables, sigs / rq: the m L2 rows') -- or, for the bit signal, sixteen one-byte elements as one 16-byte store: consecutive lanes,
// consecutive addresses. Every destination lies inside the signal's range of the layout, which the host has checked against the buffer
__global__ __launch_bounds__(256) void k_ledger_main_inputs(const MainInputsDesc* __restrict__ desc, uint32_t n_desc, uint8_t* __restrict__ dst,
                                                            const hz_l2tx* __restrict__ txs, const LedgerL1Dev* __restrict__ l1,
                                                            const LedgerCreateRow* __restrict__ crow, const hz_l2sig* __restrict__ sigs,
                                                            const uint8_t* __restrict__ rq, const uint8_t* __restrict__ keys, uint32_t n_l1, uint32_t m,
                                                            uint32_t chain_id) {
    uint32_t lo = 0, hi = n_desc - 1;   // the last signal whose first block is not beyond this one: an empty signal never wins
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (desc[mid].first_block <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const MainInputsDesc d = desc[lo];
    const uint64_t t = (uint64_t)(blockIdx.x - d.first_block) * 256 + threadIdx.x;
    const uint64_t elems = (uint64_t)d.outer * d.inner;
    if (d.ebytes == 1) {   // inner == 256 bits a row, 16 lanes a row
        if (t * 16 >= elems) return;
        const uint32_t row = (uint32_t)(t >> 4), g = (uint32_t)t & 15u;
        uint32_t w = 0;
        if (keys && row < n_l1) w = ((const __attribute__((address_space(1))) uint32_t*)keys)[(size_t)row * 8 + (g >> 1)];
        const uint32_t half = mi_half(w, g);
        const hz_u32x4 v = {mi_bits4(half, 0), mi_bits4(half, 1), mi_bits4(half, 2), mi_bits4(half, 3)};
        *(hz_g_u32x4*)(dst + d.dst_off + t * 16) = v;
        return;
    }
    if (t >= elems) return;
    Fc v = fc_zero();
    if (d.kind == HZ_MI_KIND_COPY) {
        v = load_fr(d.src + t * 32);
    } else if (d.kind == HZ_MI_KIND_BROADCAST) {
        v = load_fr(d.src);
    } else if (d.kind != HZ_MI_KIND_ZERO) {   // inner == 1: t is the row
        const uint32_t i = (uint32_t)t;
        if (i < n_l1)
            v = mi_l1_value(d.kind, chain_id, txs[i], l1[i], crow != nullptr && crow[i].aux_from != 0);
        else
            v = mi_l2_value(d.kind, chain_id, txs[i], sigs[i - n_l1], rq, i - n_l1, m);
    }
    store_fr(dst + d.dst_off + t * 32, v);
}

// ledger_sig.hip
hipError_t launch_ledger_sig(const hz_l2tx* d_txs, const hz_l2sig* d_sigs, uint32_t chain_id, uint32_t current_num_batch, uint8_t* d_tcd, uint8_t* d_v2, uint8_t* d_hash,
                             const uint8_t* planes, const void* b8_table, uint32_t N, uint64_t first_idx, uint32_t* d_fail_word, uint8_t* d_verdict, uint32_t m,
                             hipStream_t s, uint32_t unit_base = 0, const uint8_t* d_rq = nullptr);
hipError_t launch_ledger_sig_v2(const hz_l2tx* d_txs, const hz_l2sig* d_sigs, uint8_t* d_v2, uint32_t m, hipStream_t s);
void ledger_sig_link_fields_host(const hz_l2tx& tx, const hz_l2sig& sig, Fc* v2, Fc* eth, Fc* ay);
void ledger_sig_b8_table_host(void* out);
size_t ledger_sig_b8_table_bytes();

// the link check over the m L2 rows behind n_l1 L1 rows; d_v2 as an earlier kernel of stream s left it
static hipError_t launch_ledger_rq(const hz_l2tx* d_txs, const hz_l2sig* d_sigs, const uint8_t* d_rq, const uint8_t* d_v2, uint32_t* d_fail_word, uint8_t* d_verdict, uint32_t m,
                            uint32_t n_l1, hipStream_t s, uint32_t unit_base) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ledger_rq, dim3((m + 63) / 64), dim3(64), 0, s, d_txs, d_sigs, d_rq, d_v2, d_fail_word, d_verdict, m, n_l1, unit_base);
    return hipGetLastError();
}

}  // namespace hz

using namespace hz;

// the archive of exit trees (ledger_archive.h): snapshots in ascending batch order, each inside one slab; a slab is
// allocated when the last one has no room for the next snapshot and freed when every snapshot in it is forgotten. Made by the first
// hz_ledger_exit_keep / hz_ledger_withdraw_rows: a ledger that keeps nothing owns none of this
struct ArchiveSlab {
    DevBuf buf;
    size_t used = 0;
    uint32_t live = 0;   // snapshots in it
};
struct ArchiveSnap {
    uint32_t batch_num = 0;
    ArchiveSlab* slab = nullptr;   // nullptr: the empty tree, no bytes
    size_t bytes = 0;
    ArchiveDesc desc{};
};
struct LedgerArchive {
    std::vector<ArchiveSnap> snaps;
    std::vector<std::unique_ptr<ArchiveSlab>> slabs;   // in allocation order: the last one is the current one
    DevBuf table;                                      // ArchiveDesc[snaps.size()], room for table.bytes / 64
    DevSpan t_keep, t_withdraw;                        // around a keep's copies, around the two kernels of hz_ledger_withdraw_rows
    double keep_ms = 0.0, withdraw_ms = 0.0;
    uint8_t* rows_dev[HZ_WITHDRAW_ARRAYS] = {};
    bool have_rows = false;
};

// what hz_ledger_main_inputs needs of the last successful apply call with a chain id beside what lies in device memory: the shape, the
// kind of call, where the row tables lie in the integer block, and the part of the request no kernel of the apply reads
struct LedgerMainCall {
    bool valid = false;
    size_t n_l1 = 0, m = 0, F = 0, n_sib = 0;
    uint32_t chain_id = 0, current_num_batch = 0, flags = 0;   // HZ_MI_*
    uint64_t last_before = 0;                                  // the ledger's last idx before the batch
    Span<hz_l2tx> tx;
    Span<LedgerL1Dev> l1;
    Span<LedgerCreateRow> crow;
    std::vector<uint8_t> keys;   // from_bjj, [n_l1][32], empty: none given
    std::vector<uint64_t> fee_idxs;
    std::vector<uint32_t> plan_tokens;
};

// the undo journal (ledger_journal.h): the ring's bookkeeping, its slabs -- one per slot, all of one capacity --, and per
// slot what an hz_smt state tree handed out of its shape. Made by hz_ledger_journal(depth > 0): a ledger without a journal owns none of this
struct LedgerJournal {
    JournalRing ring;
    std::unique_ptr<DevBuf[]> slab;        // [ring.slots()]: depth + 1, one always free for the apply in progress
    size_t cap = 0;
    std::vector<SmtShape::UndoLog> undo;   // [ring.slots()]
    std::vector<uint8_t> has_undo;         // [ring.slots()]: the record's apply updated the growing ledger's tree
    DevSpan t_tree, t_planes, t_rollback;  // around the tree's save kernel, the planes', a rollback's restores
};

struct hz_ledger {
    int32_t device = 0;
    uint32_t k = 0, N = 0;
    uint64_t first_idx = 0;
    hz_state* tree = nullptr;
    DevBuf planes;             // resident: e0 | balance | ay | ethAddr, [N][32] each
    DevBuf ints, work, outs;   // per call, grown on demand
    PinnedBuf h_ints, h_fail;   // the call's integer tables; the failure word as the device left it
    LedgerPlan plan;
    LedgerOutDev out_dev{};
    bool have_outputs = false;
    DevSpan t_semantic;        // on the tree's stream (state_stream): around the semantic kernels;
    DevEvent e_done;           // after the write-back
    double device_ms = 0.0, semantic_ms = 0.0;
    // signatures: the uploaded hz_l2sig, the three per-transaction arrays and the verdict bytes, the fixed-base table (once per ledger)
    DevBuf sig_in, sig_outs, b8_table;
    uint8_t* sig_dev[3] = {nullptr, nullptr, nullptr};
    uint8_t* verdict_dev = nullptr;
    bool have_sig_outputs = false;
    DevSpan t_sig;
    double sig_ms = 0.0;
    // receivers by address (hz_ledger_apply_l2_addr / _resolve_l2): the query table and the per-transaction results, the auxToIdx rows
    DevBuf res, aux_rows;
    PinnedBuf h_res;
    bool have_aux = false;
    DevSpan t_resolve;
    double resolve_ms = 0.0;
    // the L1 run (hz_ledger_apply_batch): the flag bytes
    DevBuf l1_flags;
    bool have_l1 = false;
    DevSpan t_l1;
    double l1_ms = 0.0;
    // exits (hz_ledger_apply_batch_exits): the batch's exit tree, the six exit arrays, the leaf every exit key ends with (plane-major,
    // [4][exit_keys.size()]) and which key lies where
    hz_smt* exit = nullptr;
    DevBuf exit_outs, exit_final;
    uint8_t* exit_dev[HZ_LEDGER_EXIT_ARRAYS] = {};
    std::vector<std::pair<uint64_t, uint32_t>> exit_keys;   // (key, its place in exit_final), ascending
    bool have_exit_outputs = false;
    DevSpan t_exit_scan, t_exit_rows;   // around the scan, around pack and gather (the tree's stream)
    DevEvent e_exit_tree;               // after the exit tree's update (its own stream)
    double exit_ms = 0.0;
    // a growing ledger (hz_ledger_create_growing): the state tree is an hz_smt, tree == nullptr, N is the capacity -- the
    // plane stride -- and live the number of accounts; a dense ledger has live == N for good
    hz_smt* smt = nullptr;
    uint64_t live = 0;
    uint32_t n_sib_max = 0;
    bool loaded = false;
    DevBuf create_in, create_outs, root_buf;
    PinnedBuf h_create;
    uint8_t* create_dev[HZ_LEDGER_CREATE_ARRAYS] = {};
    bool have_create_outputs = false;
    DevSpan t_create, t_create_pack;   // around k_ledger_create, around k_ledger_create_pack
    double create_ms = 0.0;
    // atomic links (hz_ledger_apply_batch_atomic / _verify_l2_atomic): the rq fields plane-major, [3][m][32], then the m offsets
    DevBuf rq_in;
    PinnedBuf h_rq;
    DevSpan t_rq;   // around k_ledger_rq
    double rq_ms = 0.0;
    // a batch selected from a pool (hz_ledger_select_batch): what k_ledger_select left, back on the host
    PinnedBuf h_sel;
    DevSpan t_select;   // around k_ledger_select
    double select_ms = 0.0;
    // exit trees of earlier batches (hz_ledger_exit_keep)
    std::unique_ptr<LedgerArchive> archive;
    // RollupMain's packed inputs of the last apply (hz_ledger_main_inputs): what of the request the device does not hold,
    // the descriptor table's upload
    LedgerMainCall main_call;
    DevBuf mi_in;
    PinnedBuf h_mi;
    DevSpan t_mi;   // around k_ledger_main_inputs
    double mi_ms = 0.0;
    // marks and the undo journal (hz_ledger_journal / _rollback)
    uint64_t applied = 0;
    std::unique_ptr<LedgerJournal> journal;
    double journal_ms = 0.0, rollback_ms = 0.0;
    bool rollback_failed = false;   // a rollback failed behind its first queued restore: tree, planes and shape may disagree until a load
    ~hz_ledger() {
        journal.reset();
        archive.reset();
        if (exit) hz_smt_destroy(exit);
        if (smt) hz_smt_destroy(smt);
        if (tree) hz_state_destroy(tree);
    }
};

static hipStream_t ledger_stream(const hz_ledger* l) { return l->smt ? smt_stream(l->smt) : state_stream(l->tree); }

// the exit tree and the exit leaves are those of the last successful call: every call that applies a batch starts from the empty tree
static void ledger_exit_reset(hz_ledger* l) {
    smt_clear(l->exit);   // (no synchronise: every update of this tree ends in smt_apply_finish or smt_apply_abort)
    l->exit_keys.clear();
    l->exit_ms = 0.0;
}

// the rq entries are copied to the device from a pinned buffer the ledger reuses: a call that returns before its synchronise waits for
// the stream here, so the next call does not fill the buffer under a copy still in flight
struct LedgerDrain {
    hipStream_t s = nullptr;
    bool armed = false;
    ~LedgerDrain() {
        if (armed) (void)hipStreamSynchronize(s);
    }
};

// a prepared update of the exit tree -- or of a growing ledger's state tree -- that does not reach smt_apply_finish did not happen
struct LedgerExitGuard {
    hz_smt* t = nullptr;
    ~LedgerExitGuard() {
        if (t) smt_apply_abort(t);
    }
};

// the device pointers and the L1 time of the last successful call are no longer what the getters may hand out
static void ledger_forget(hz_ledger* l) {
    l->have_outputs = l->have_sig_outputs = l->have_aux = l->have_l1 = l->have_exit_outputs = l->have_create_outputs = false;
    l->l1_ms = 0.0;
    l->create_ms = 0.0;
    if (l->archive) l->archive->have_rows = false;
    l->main_call.valid = false;
}

// a reload starts a new history: no exit tree of the old one is kept
static void ledger_archive_clear(hz_ledger* l) {
    if (!l->archive) return;
    l->archive->snaps.clear();
    l->archive->slabs.clear();
}

// a load starts a new history of marks too: no record of the old one is kept
static void ledger_history_reset(hz_ledger* l) {
    l->applied = 0;
    l->rollback_failed = false;
    l->journal_ms = 0.0;
    if (l->journal) l->journal->ring.clear();
}

static hz_status ledger_ready(const hz_ledger* l, const char* who) {
    if (!l) return set_err(HZ_ERR_ARG, "%s: null ledger", who);
    if (l->rollback_failed)
        return set_err(HZ_ERR_HIP, "%s: an earlier hz_ledger_rollback failed on the device after its first restore was queued; loading the ledger makes it usable again", who);
    if (l->smt) {
        if (!l->loaded) return set_err(HZ_ERR_ARG, "%s: the ledger has not been loaded yet (hz_ledger_load_accounts)", who);
        if (smt_poisoned(l->smt))
            return set_err(HZ_ERR_HIP, "%s: an earlier call failed on the device after the state tree's write-back was queued; hz_ledger_load_accounts makes the ledger usable again", who);
        return HZ_OK;
    }
    if (!state_loaded(l->tree)) return set_err(HZ_ERR_ARG, "%s: the ledger holds no accounts yet (hz_ledger_load)", who);
    return HZ_OK;
}

// the ledger as the checks see it (ledger_checks.h)
static LedgerShape ledger_shape(const hz_ledger* l) { return LedgerShape{l->smt != nullptr, l->N, l->first_idx, l->live, l->smt ? l->n_sib_max : l->k}; }

// one apply call, as its exported function states it
struct LedgerCall {
    const char* who = "";
    // the request: the L1 run with the compressed keys of its create rows, the m L2 rows with their signatures and links (rq == null: no
    // transaction links, nothing to check), the fee plan; aux_to_idx: the receivers by address as the caller found them, or null
    size_t n_l1 = 0, m = 0, F = 0, n_sib = 0;
    const hz_l1tx* l1 = nullptr;
    const uint8_t* from_bjj = nullptr;
    const hz_l2tx* txs = nullptr;
    const hz_l2sig* sigs = nullptr;
    const hz_l2rq* rq = nullptr;
    uint32_t flags = 0, chain_id = 0, current_num_batch = 0;
    bool verify = false;   // flags & HZ_LEDGER_VERIFY_SIGS, or hz_ledger_apply_l2_signed
    const uint32_t* plan_tokens = nullptr;
    const uint64_t *fee_idxs = nullptr, *aux_to_idx = nullptr;
    // where the outputs go on the host; each may be null
    const hz_ledger_out* out = nullptr;
    const hz_ledger_sig_out* sig_out = nullptr;
    uint8_t *aux_to_idx_out = nullptr, *flags_out = nullptr;
    const hz_ledger_exit_out* exit_out = nullptr;
    const hz_ledger_create_out* create_out = nullptr;
    // what the call accepts: to_idx == 0 in L2 rows (and sigs uploaded for their destination fields whether or not they are verified), an
    // L1 run, to_idx == 1 in L1 and L2 rows, from_idx == 0 in L1 rows
    bool by_addr = false, is_batch = false, exits = false, creates = false;
};

// what both kinds of ledger own once device, N and the trees are set: the planes, the failure word's pinned home, the events
static hz_status ledger_open(hz_ledger* l) {
    HZ_HIP(hipSetDevice(l->device));
    HZ_HIP(l->planes.alloc((size_t)4 * l->N * 32));
    HZ_HIP(l->h_fail.grow(64));
    for (DevSpan* t : {&l->t_semantic, &l->t_sig, &l->t_resolve, &l->t_l1, &l->t_exit_scan, &l->t_exit_rows, &l->t_create, &l->t_create_pack, &l->t_rq, &l->t_select, &l->t_mi})
        HZ_HIP(t->create());
    HZ_HIP(l->e_done.create());
    HZ_HIP(l->e_exit_tree.create());
    return HZ_OK;
}

extern "C" hz_status hz_ledger_create(int32_t device, int32_t k, uint64_t first_idx, hz_ledger** out) {
    if (!out) return set_err(HZ_ERR_ARG, "hz_ledger_create: null argument");
    *out = nullptr;
    std::unique_ptr<hz_ledger> l(new hz_ledger);
    if (hz_status e = hz_state_create(device, k, first_idx, &l->tree)) return e;
    if (hz_status e = hz_smt_create(device, HZ_SMT_MAX_DEPTH, &l->exit)) return e;
    l->device = device;
    l->k = (uint32_t)k;
    l->N = 1u << k;
    l->live = l->N;
    l->first_idx = first_idx;
    if (hz_status e = ledger_open(l.get())) return e;
    *out = l.release();
    return HZ_OK;
}

extern "C" hz_status hz_ledger_create_growing(int32_t device, uint64_t capacity, uint64_t first_idx, int32_t n_sib_max, hz_ledger** out) {
    const char* who = "hz_ledger_create_growing";
    if (!out) return set_err(HZ_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    if (capacity < 1 || capacity > HZ_LEDGER_MAX_CAPACITY) return set_err(HZ_ERR_ARG, "%s: capacity = %llu accounts (1 .. 2^24)", who, (unsigned long long)capacity);
    if (first_idx < 2 || (first_idx + capacity) >> HZ_SMT_KEY_BITS)
        return set_err(HZ_ERR_ARG, "%s: first_idx = %llu (0 and 1 are not accounts; the circuits' idx has 48 bits)", who, (unsigned long long)first_idx);
    std::unique_ptr<hz_ledger> l(new hz_ledger);
    if (hz_status e = hz_smt_create(device, n_sib_max, &l->smt)) return e;
    if (hz_status e = hz_smt_create(device, HZ_SMT_MAX_DEPTH, &l->exit)) return e;
    l->device = device;
    l->N = (uint32_t)capacity;
    l->n_sib_max = (uint32_t)n_sib_max;
    l->first_idx = first_idx;
    if (hz_status e = ledger_open(l.get())) return e;
    HZ_HIP(l->root_buf.alloc(32));
    *out = l.release();
    return HZ_OK;
}

extern "C" void hz_ledger_destroy(hz_ledger* l) {
    if (!l) return;
    (void)hipSetDevice(l->device);
    (void)hipStreamSynchronize(ledger_stream(l));
    (void)hipStreamSynchronize(smt_stream(l->exit));
    delete l;
}

extern "C" hz_status hz_ledger_load(hz_ledger* l, const uint8_t* e0, const uint8_t* balance, const uint8_t* ay, const uint8_t* eth_addr) {
    if (!l || !e0 || !balance || !ay || !eth_addr) return set_err(HZ_ERR_ARG, "hz_ledger_load: null argument");
    if (l->smt) return set_err(HZ_ERR_ARG, "hz_ledger_load: a growing ledger is loaded with hz_ledger_load_accounts");
    // a leaf's ranges, which every kernel assumes: before the tree or the planes are touched, so a refused load leaves a loaded ledger as it was
    if (hz_status e = ledger_check_leaves("hz_ledger_load", l->first_idx, l->N, e0, balance, eth_addr)) return e;
    ledger_forget(l);
    ledger_archive_clear(l);
    ledger_history_reset(l);
    if (hz_status e = hz_state_load(l->tree, e0, balance, ay, eth_addr)) return e;   // checks every field < r
    const uint8_t* src[4] = {e0, balance, ay, eth_addr};
    hipStream_t s = ledger_stream(l);
    HZ_HIP(hipSetDevice(l->device));
    for (int f = 0; f < 4; f++) HZ_HIP(hipMemcpyAsync((uint8_t*)l->planes.p + (size_t)f * l->N * 32, src[f], (size_t)l->N * 32, hipMemcpyHostToDevice, s));
    HZ_HIP(hipStreamSynchronize(s));
    return HZ_OK;
}

// n consecutive accounts from first_idx into a growing ledger (n == 0: the genesis state, root 0): the planes by copy, the tree by ordered
// inserts through smt_internal.h, at most 65536 a call, on records a kernel makes of the planes
extern "C" hz_status hz_ledger_load_accounts(hz_ledger* l, uint64_t n, const uint8_t* e0, const uint8_t* balance, const uint8_t* ay, const uint8_t* eth_addr) {
    const char* who = "hz_ledger_load_accounts";
    if (!l) return set_err(HZ_ERR_ARG, "%s: null ledger", who);
    if (!l->smt) return set_err(HZ_ERR_ARG, "%s: a dense ledger is loaded with hz_ledger_load", who);
    if (n > l->N) return set_err(HZ_ERR_ARG, "%s: n = %llu accounts (the capacity is %u)", who, (unsigned long long)n, l->N);
    if (n && (!e0 || !balance || !ay || !eth_addr)) return set_err(HZ_ERR_ARG, "%s: null argument", who);
    if (hz_status e = ledger_check_leaves(who, l->first_idx, n, e0, balance, eth_addr)) return e;
    const uint8_t* src[4] = {e0, balance, ay, eth_addr};
    static const char* const name[4] = {"e0", "balance", "ay", "ethAddr"};
    for (int f = 0; f < 4; f++)
        for (size_t i = 0; i < n; i++)
            if (!canon_lt_p(src[f] + i * 32))
                return set_err(HZ_ERR_INPUT, "%s: %s of account %llu (row %zu) is not below the field's modulus", who, name[f], (unsigned long long)(l->first_idx + i), i);
    // a depth the tree cannot express is found before anything is touched: the shape of n consecutive keys, planned alone
    {
        SmtShape sh;
        sh.begin();
        for (uint64_t i = 0; i < n; i++)
            if (sh.add(l->first_idx + i, l->n_sib_max) != SMT_PLAN_OK)
                return set_err(HZ_ERR_ARG, "%s: account %llu would have its leaf at depth >= n_sib_max = %u", who, (unsigned long long)(l->first_idx + i), l->n_sib_max);
    }
    ledger_forget(l);
    ledger_exit_reset(l);
    ledger_archive_clear(l);
    ledger_history_reset(l);
    HZ_HIP(hipSetDevice(l->device));
    if (hz_status e = hz_smt_reset(l->smt)) return e;   // synchronises the stream
    l->live = 0;
    l->loaded = false;
    hipStream_t s = ledger_stream(l);
    for (int f = 0; f < 4 && n; f++) HZ_HIP(hipMemcpyAsync((uint8_t*)l->planes.p + (size_t)f * l->N * 32, src[f], (size_t)n * 32, hipMemcpyHostToDevice, s));
    std::vector<uint64_t> keys;
    for (uint64_t base = 0; base < n; base += HZ_LEDGER_MAX_EVENTS) {
        const uint32_t M = (uint32_t)std::min<uint64_t>(HZ_LEDGER_MAX_EVENTS, n - base);
        keys.resize(M);
        for (uint32_t j = 0; j < M; j++) keys[j] = l->first_idx + base + j;
        SmtCallBufs sb{};
        if (hz_status e = smt_apply_prepare(l->smt, who, HZ_ERR_ARG, M, keys.data(), l->n_sib_max, false, &sb)) return e;
        LedgerExitGuard guard;
        guard.t = l->smt;
        hipLaunchKernelGGL(k_ledger_load_records, dim3((M + 255) / 256), dim3(256), 0, s, (const uint8_t*)l->planes.p, sb.fields, l->N, (uint32_t)base, M);
        HZ_HIP(hipGetLastError());
        if (hz_status e = smt_apply_launch(l->smt, M, l->n_sib_max, false)) return e;
        if (hz_status e = smt_apply_finish(l->smt)) return e;
        guard.t = nullptr;
    }
    HZ_HIP(hipStreamSynchronize(s));
    l->live = n;
    l->loaded = true;
    return HZ_OK;
}

extern "C" uint64_t hz_ledger_size(const hz_ledger* l) { return l ? l->live : 0; }
extern "C" uint64_t hz_ledger_last_idx(const hz_ledger* l) { return l ? l->first_idx + l->live - 1 : 0; }
extern "C" hz_smt* hz_ledger_state_smt(hz_ledger* l) { return l ? l->smt : nullptr; }

extern "C" hz_status hz_ledger_root(hz_ledger* l, uint8_t* out32) {
    if (hz_status e = ledger_ready(l, "hz_ledger_root")) return e;
    if (l->smt) return hz_smt_root(l->smt, out32);
    return hz_state_root(l->tree, out32);
}

extern "C" hz_state* hz_ledger_tree(hz_ledger* l) { return l ? l->tree : nullptr; }
extern "C" double hz_ledger_device_ms(const hz_ledger* l) { return l ? l->device_ms : 0.0; }
extern "C" double hz_ledger_semantic_ms(const hz_ledger* l) { return l ? l->semantic_ms : 0.0; }

extern "C" hz_status hz_ledger_accounts(hz_ledger* l, size_t n, const uint64_t* idx, uint8_t* fields_out) {
    if (hz_status e = ledger_ready(l, "hz_ledger_accounts")) return e;
    if (n == 0) return HZ_OK;
    if (!idx || !fields_out) return set_err(HZ_ERR_ARG, "hz_ledger_accounts: null argument");
    if (n > l->live) return set_err(HZ_ERR_ARG, "hz_ledger_accounts: %zu accounts in one call (the state holds %u)", n, (unsigned)l->live);
    std::vector<uint32_t> acct(n);
    for (size_t i = 0; i < n; i++) {
        if (!ledger_has(l->first_idx, l->live, idx[i]))
            return set_err(HZ_ERR_ARG, "hz_ledger_accounts: idx[%zu] = %llu is outside the state", i, (unsigned long long)idx[i]);
        acct[i] = (uint32_t)(idx[i] - l->first_idx);
    }
    HZ_HIP(hipSetDevice(l->device));
    ledger_forget(l);   // the call's buffers are reused
    hipStream_t s = ledger_stream(l);
    HZ_HIP(l->ints.grow(n * 4));
    HZ_HIP(l->work.grow(n * 128));
    HZ_HIP(hipMemcpyAsync(l->ints.p, acct.data(), n * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ledger_accounts, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, s, (const uint32_t*)l->ints.p, (const uint8_t*)l->planes.p,
                       (uint8_t*)l->work.p, l->N, (uint32_t)n);
    HZ_HIP(hipGetLastError());
    HZ_HIP(hipMemcpyAsync(fields_out, l->work.p, n * 128, hipMemcpyDeviceToHost, s));
    HZ_HIP(hipStreamSynchronize(s));
    return HZ_OK;
}

// the *_dev getters: the n device pointers of the last successful `call` into dev, a struct of n pointers; have == nullptr: the ledger
// holds none of them
static hz_status ledger_hand_out(const char* who, const hz_ledger* l, void* dev, const bool* have, const char* call, uint8_t* const* src, int n) {
    if (!l || !dev) return set_err(HZ_ERR_ARG, "%s: null argument", who);
    if (!have || !*have) return set_err(HZ_ERR_ARG, "%s: no successful %s since the ledger's last other call", who, call);
    for (int a = 0; a < n; a++) ((uint8_t**)dev)[a] = src[a];
    return HZ_OK;
}

extern "C" hz_status hz_ledger_outputs_dev(hz_ledger* l, hz_ledger_out* dev) {
    return ledger_hand_out("hz_ledger_outputs_dev", l, dev, l ? &l->have_outputs : nullptr, "hz_ledger_apply_l2", l ? l->out_dev.a : nullptr, HZ_LEDGER_ARRAYS);
}

// the signatures and the fixed-base table on the device, room for the three arrays and the verdict bytes; verify == false: the upload
// alone, for the destination fields
static hz_status ledger_sig_prepare(hz_ledger* l, size_t m, const hz_l2sig* sigs, hipStream_t s, bool verify = true) {
    if (verify && !l->b8_table.p) {
        std::vector<uint8_t> table(ledger_sig_b8_table_bytes());
        ledger_sig_b8_table_host(table.data());
        HZ_HIP(l->b8_table.alloc(table.size()));
        HZ_HIP(hipMemcpy(l->b8_table.p, table.data(), table.size(), hipMemcpyHostToDevice));
    }
    const size_t rows = m ? m : 1;
    HZ_HIP(l->sig_in.grow(rows * sizeof(hz_l2sig)));
    HZ_HIP(l->sig_outs.grow(rows * 96 + rows));
    uint8_t* at = (uint8_t*)l->sig_outs.p;
    for (int a = 0; a < 3; a++) l->sig_dev[a] = at + (size_t)a * rows * 32;
    l->verdict_dev = at + rows * 96;
    if (m) HZ_HIP(hipMemcpyAsync(l->sig_in.p, sigs, m * sizeof(hz_l2sig), hipMemcpyHostToDevice, s));
    return HZ_OK;
}

// the signature kernels over the m L2 rows at d_txs and, where the call has links, the link check behind them: a failure lowers the failure
// word d_fail at unit_base + i (the rows stand behind unit_base L1 rows), or goes to the verdict bytes. verify: both signature kernels, under
// t_sig; otherwise, for the links, the V2 rows of the message kernel's packing alone. own_link_kernel: the caller launches its own behind this
static hz_status ledger_sig_links_launch(hz_ledger* l, const hz_l2tx* d_txs, uint32_t m, uint32_t chain_id, uint32_t current_num_batch, uint32_t* d_fail, uint8_t* d_verdict,
                                         uint32_t unit_base, bool verify, bool links, hipStream_t s, bool own_link_kernel = false) {
    const hz_l2sig* d_sigs = (const hz_l2sig*)l->sig_in.p;
    const uint8_t* d_rq = links ? (const uint8_t*)l->rq_in.p : nullptr;
    if (verify) {
        HZ_HIP(l->t_sig.begin(s));
        HZ_HIP(launch_ledger_sig(d_txs, d_sigs, chain_id, current_num_batch, l->sig_dev[0], l->sig_dev[1], l->sig_dev[2], (const uint8_t*)l->planes.p, l->b8_table.p, l->N,
                                 l->first_idx, d_fail, d_verdict, m, s, unit_base, d_rq));
        HZ_HIP(l->t_sig.end(s));
    } else if (links) {
        HZ_HIP(launch_ledger_sig_v2(d_txs, d_sigs, l->sig_dev[1], m, s));
    }
    if (links && !own_link_kernel) {
        HZ_HIP(l->t_rq.begin(s));
        HZ_HIP(launch_ledger_rq(d_txs, d_sigs, d_rq, (const uint8_t*)l->sig_dev[1], d_fail, d_verdict, m, unit_base, s, unit_base));
        HZ_HIP(l->t_rq.end(s));
    }
    return HZ_OK;
}

// the links on the device as the kernels read them: the three fields plane-major, [3][m][32], then the m offsets
static hz_status ledger_rq_upload(hz_ledger* l, size_t m, const hz_l2rq* rq, hipStream_t s) {
    const size_t bytes = m * 97;
    HZ_HIP(l->h_rq.grow(bytes));
    HZ_HIP(l->rq_in.grow(bytes));
    uint8_t* h = (uint8_t*)l->h_rq.p;
    for (size_t i = 0; i < m; i++) {
        memcpy(h + i * 32, rq[i].rq_tx_compressed_data_v2, 32);
        memcpy(h + (m + i) * 32, rq[i].rq_to_eth_addr, 32);
        memcpy(h + (2 * m + i) * 32, rq[i].rq_to_bjj_ay, 32);
        h[3 * m * 32 + i] = rq[i].rq_offset;
    }
    HZ_HIP(hipMemcpyAsync(l->rq_in.p, h, bytes, hipMemcpyHostToDevice, s));
    return HZ_OK;
}

static hz_status ledger_sig_copy_out(hz_ledger* l, size_t m, const hz_ledger_sig_out* sig_out, hipStream_t s) {
    if (!sig_out || !m) return HZ_OK;
    uint8_t* const h[3] = {sig_out->tx_compressed_data, sig_out->tx_compressed_data_v2, sig_out->sig_l2_hash};
    for (int a = 0; a < 3; a++)
        if (h[a]) HZ_HIP(hipMemcpyAsync(h[a], l->sig_dev[a], m * 32, hipMemcpyDeviceToHost, s));
    return HZ_OK;
}

// hz_ledger_verify_l2, and hz_ledger_verify_l2_atomic with the links of the m transactions (rows 0 .. m - 1 of a batch without L1 rows)
static hz_status ledger_verify(hz_ledger* l, const char* who, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, const hz_l2rq* rq, uint32_t chain_id,
                               uint32_t current_num_batch, uint8_t* verdict_out, const hz_ledger_sig_out* sig_out) {
    if (hz_status e = ledger_ready(l, who)) return e;
    if (m && (!txs || !verdict_out)) return set_err(HZ_ERR_ARG, "%s: null argument", who);
    if (m > HZ_LEDGER_MAX_TX) return set_err(HZ_ERR_ARG, "%s: %zu transactions in one call (at most %u)", who, m, HZ_LEDGER_MAX_TX);
    if (hz_status e = ledger_check_txs(who, m, txs, l->first_idx, l->live)) return e;
    if (hz_status e = ledger_check_sigs(who, m, txs, sigs, chain_id)) return e;
    if (hz_status e = ledger_check_rq(who, m, txs, rq)) return e;
    const bool links = rq != nullptr && m != 0;
    ledger_forget(l);
    HZ_HIP(hipSetDevice(l->device));
    hipStream_t s = ledger_stream(l);
    LedgerDrain drain;
    if (links) {
        drain.s = s;
        drain.armed = true;
        if (hz_status e = ledger_rq_upload(l, m, rq, s)) return e;
    }
    HZ_HIP(l->ints.grow((m ? m : 1) * sizeof(hz_l2tx)));
    if (m) HZ_HIP(hipMemcpyAsync(l->ints.p, txs, m * sizeof(hz_l2tx), hipMemcpyHostToDevice, s));
    if (hz_status e = ledger_sig_prepare(l, m, sigs, s)) return e;
    // the link check behind both signature kernels: 13 goes where the verdict is still 0
    if (hz_status e = ledger_sig_links_launch(l, (const hz_l2tx*)l->ints.p, (uint32_t)m, chain_id, current_num_batch, nullptr, l->verdict_dev, 0, true, links, s)) return e;
    if (m) HZ_HIP(hipMemcpyAsync(verdict_out, l->verdict_dev, m, hipMemcpyDeviceToHost, s));
    if (hz_status e = ledger_sig_copy_out(l, m, sig_out, s)) return e;
    HZ_HIP(hipStreamSynchronize(s));
    drain.armed = false;
    HZ_HIP(l->t_sig.read(l->sig_ms));
    if (links) HZ_HIP(l->t_rq.read(l->rq_ms));
    l->have_sig_outputs = true;
    return HZ_OK;
}

extern "C" hz_status hz_ledger_verify_l2(hz_ledger* l, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, uint32_t chain_id, uint32_t current_num_batch,
                                         uint8_t* verdict_out, const hz_ledger_sig_out* sig_out) {
    return ledger_verify(l, "hz_ledger_verify_l2", m, txs, sigs, nullptr, chain_id, current_num_batch, verdict_out, sig_out);
}

extern "C" hz_status hz_ledger_sig_outputs_dev(hz_ledger* l, hz_ledger_sig_out* dev) {
    static_assert(sizeof(hz_ledger_sig_out) == 3 * sizeof(uint8_t*), "hz_ledger_sig_out is an array of pointers");
    return ledger_hand_out("hz_ledger_sig_outputs_dev", l, dev, l ? &l->have_sig_outputs : nullptr, "hz_ledger_apply_l2_signed / hz_ledger_verify_l2",
                           l ? l->sig_dev : nullptr, 3);
}

extern "C" double hz_ledger_sig_ms(const hz_ledger* l) { return l ? l->sig_ms : 0.0; }

// ---- receivers named by address or key ----------------------------------------------------------------------------------
// The lookup: out[i] is the lowest account that holds transaction i's signed destination and its token, 0 for a NOP, for to_idx != 0, for
// a zero amount when skip_zero (processor 2 is a NOP then: no receiver is needed), or when no account matches. Host: the distinct
// queries into the table; device: one pass over the planes, then a lane per transaction; one copy back and a synchronise.
static hz_status ledger_resolve(hz_ledger* l, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, bool skip_zero, uint64_t* out, uint64_t count) {
    l->resolve_ms = 0.0;
    size_t queries = 0;
    for (size_t i = 0; i < m; i++) {
        out[i] = 0;
        queries += ResolveTables::asks(txs[i], skip_zero);
    }
    if (!queries) return HZ_OK;
    const uint32_t slots = resolve_slots(queries), m32 = (uint32_t)m;
    ResolveTables T;
    T.layout(slots, m);
    HZ_HIP(hipSetDevice(l->device));
    HZ_HIP(l->h_res.grow(T.end));
    HZ_HIP(l->res.grow(T.end));
    void *hb = l->h_res.p, *db = l->res.p;
    T.fill(hb, txs, sigs, skip_zero);
    hipStream_t s = ledger_stream(l);
    HZ_HIP(hipMemcpyAsync(db, hb, T.up, hipMemcpyHostToDevice, s));
    HZ_HIP(l->t_resolve.begin(s));
    hipLaunchKernelGGL(k_ledger_resolve, dim3(((uint32_t)count + 255) / 256), dim3(256), 0, s, (const uint8_t*)l->planes.p, T.table.dev(db), T.result.dev(db), slots, l->N,
                       (uint32_t)count);
    HZ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ledger_resolve_pick, dim3((m32 + 63) / 64), dim3(64), 0, s, T.slot.dev(db), T.result.dev(db), T.out.dev(db), l->first_idx, m32);
    HZ_HIP(hipGetLastError());
    HZ_HIP(l->t_resolve.end(s));
    HZ_HIP(hipMemcpyAsync(T.out.host(hb), T.out.dev(db), T.out.bytes(), hipMemcpyDeviceToHost, s));
    HZ_HIP(hipStreamSynchronize(s));   // the round trip of the lookup: the planner needs the receivers
    memcpy(out, T.out.host(hb), T.out.bytes());
    HZ_HIP(l->t_resolve.read(l->resolve_ms));
    return HZ_OK;
}

extern "C" hz_status hz_ledger_resolve_l2(hz_ledger* l, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, uint64_t* aux_to_idx_out) {
    const char* who = "hz_ledger_resolve_l2";
    if (hz_status e = ledger_ready(l, who)) return e;
    if (m && (!txs || !sigs || !aux_to_idx_out)) return set_err(HZ_ERR_ARG, "%s: null argument", who);
    if (m > HZ_LEDGER_MAX_TX) return set_err(HZ_ERR_ARG, "%s: %zu transactions in one call (at most %u)", who, m, HZ_LEDGER_MAX_TX);
    l->main_call.valid = false;   // hz_ledger_main_inputs packs the batch of the ledger's LAST call (the *_dev getters are not touched here)
    return ledger_resolve(l, m, txs, sigs, false, aux_to_idx_out, l->live);
}

// ---- what the by_addr apply calls and hz_ledger_select_batch share: the checks and preparations before a plan can be made -----------------
// k_ledger_create on the ledger's stream, before everything else of the call, the lookup included: the new accounts' static fields into
// their plane slots. Every slot lies at or beyond the ledger's size and below its capacity (ledger_effective_l1)
static hz_status ledger_create_launch(hz_ledger* l, size_t n_l1, const hz_l1tx* l1, const uint8_t* from_bjj, const LedgerRows& r) {
    const uint32_t n = (uint32_t)r.n_creates;
    HZ_HIP(hipSetDevice(l->device));
    HZ_HIP(l->h_create.grow((size_t)n * sizeof(LedgerCreateDev)));
    HZ_HIP(l->create_in.grow((size_t)n * sizeof(LedgerCreateDev)));
    LedgerCreateDev* h = (LedgerCreateDev*)l->h_create.p;
    uint32_t q = 0;
    for (size_t i = 0; i < n_l1; i++) {
        if (!r.aux_from[i]) continue;
        LedgerCreateDev c{};
        c.acct = (uint32_t)(r.aux_from[i] - l->first_idx);
        c.token_id = l1[i].token_id;
        memcpy(c.bjj, from_bjj + i * 32, 32);
        memcpy(c.from_eth, l1[i].from_eth_addr, 20);
        h[q++] = c;
    }
    hipStream_t s = ledger_stream(l);
    HZ_HIP(hipMemcpyAsync(l->create_in.p, h, (size_t)n * sizeof(LedgerCreateDev), hipMemcpyHostToDevice, s));
    HZ_HIP(l->t_create.begin(s));
    hipLaunchKernelGGL(k_ledger_create, dim3((n + 63) / 64), dim3(64), 0, s, (const LedgerCreateDev*)l->create_in.p, (uint8_t*)l->planes.p, l->N, n);
    HZ_HIP(hipGetLastError());
    HZ_HIP(l->t_create.end(s));
    return HZ_OK;
}

// r.eff: the L2 rows with the receivers of those that want one -- the caller's, checked, or the lookup's. A destination nobody holds
// keeps to_idx == 0; where refuse, it is reason 9 at once, before the plan can exist: reported whatever else is wrong with the batch
static hz_status ledger_effective_receivers(hz_ledger* l, const char* who, size_t n_l1, size_t m, const hz_l2tx* txs, const uint64_t* aux_to_idx, bool refuse, LedgerRows& r) {
    r.eff.assign(txs, txs + m);
    const bool given = aux_to_idx != nullptr;
    std::vector<uint64_t> found(given ? 0 : m ? m : 1);
    if (!given) {
        ledger_forget(l);
        if (hz_status e = ledger_resolve(l, m, txs, r.sigs, true, found.data(), r.count)) return e;
    }
    const uint64_t* to = given ? aux_to_idx : found.data();
    for (size_t i = 0; i < m; i++) {
        if (!ledger_wants_receiver(txs[i])) continue;
        if (given && !ledger_has(l->first_idx, r.count, to[i]))
            return set_err(HZ_ERR_ARG, "%s: tx %zu: aux_to_idx = %llu is outside the state (%llu .. %llu)", who, i, (unsigned long long)to[i],
                           (unsigned long long)l->first_idx, (unsigned long long)(l->first_idx + r.count - 1));
        if (!given && to[i] == 0 && refuse) return ledger_refused(who, n_l1 + i, 9, n_l1 + m, n_l1);
        r.eff[i].to_idx = to[i];
    }
    if (given) l->resolve_ms = 0.0;
    return HZ_OK;
}

// the checks of an apply call, in the order their errors win -- a plain L2 form's, then a by_addr form's; -> the rows, and the plan made of them
static hz_status ledger_prepare(hz_ledger* l, const LedgerCall& c, LedgerRows& r) {
    if (hz_status e = ledger_ready(l, c.who)) return e;
    ledger_exit_reset(l);
    const LedgerShape g = ledger_shape(l);
    r.sigs = c.sigs;
    if (!c.by_addr) {
        if (hz_status e = ledger_n_sib(g, c.who, c.n_sib)) return e;
        if (hz_status e = ledger_check_plan(c.who, c.m, c.txs, c.F, c.plan_tokens, c.fee_idxs, l->live, l->first_idx, l->plan)) return e;
        return c.verify ? ledger_check_sigs(c.who, c.m, c.txs, c.sigs, c.chain_id) : HZ_OK;
    }
    if (c.is_batch) l->l1_ms = 0.0;   // the time of THIS call, whatever becomes of it
    if (hz_status e = ledger_check_flags(c.who, c.flags)) return e;
    if (!c.verify && c.sig_out) return set_err(HZ_ERR_ARG, "%s: sig_out without HZ_LEDGER_VERIFY_SIGS", c.who);
    if (hz_status e = ledger_n_sib(g, c.who, c.n_sib)) return e;
    if (hz_status e = ledger_effective_l1(g, c.who, c.n_l1, c.l1, c.from_bjj, c.creates, c.exits, r)) return e;
    if (hz_status e = ledger_check_plan(c.who, c.m, c.txs, c.F, c.plan_tokens, c.fee_idxs, r.count, l->first_idx, l->plan, true, r.l1_events, c.exits)) return e;
    if (c.is_batch)   // (without an L1 run the call is hz_ledger_apply_l2_addr's: null sigs is its error)
        if (hz_status e = ledger_stand_in_sigs(c.who, c.m, c.txs, c.sigs, c.verify, r)) return e;
    if (hz_status e = ledger_check_sigs(c.who, c.m, c.txs, r.sigs, c.chain_id, c.verify)) return e;
    if (hz_status e = ledger_check_rq(c.who, c.m, c.txs, c.rq)) return e;
    if (r.n_creates)
        if (hz_status e = ledger_create_launch(l, c.n_l1, c.l1, c.from_bjj, r)) return e;
    if (hz_status e = ledger_effective_receivers(l, c.who, c.n_l1, c.m, c.txs, c.aux_to_idx, true, r)) return e;
    ledger_plan_rows(c.n_l1, r.l1, c.m, r.eff.data(), c.F, c.plan_tokens, c.fee_idxs, c.exits, l->plan);
    return HZ_OK;
}

// ---- one apply call, in stages (the header comment names them) ----------------------------------------------------------------------------
// What the stages share. The batch has R = n_l1 + m rows: every per-transaction table, kernel and output is per row, while sigs, sig_out
// and the signature kernels keep to the m L2 rows. The plan is made of the effective rows (rows.l1, rows.eff), while c.txs -- the signed
// ones, to_idx == 0 where the receiver is named by address -- are what the kernels see. Every early return drains the stream under a
// copy from the ledger's pinned rq buffer and aborts a prepared tree update (the members are destroyed in that order)
struct LedgerApply {
    hz_ledger* const l;
    const LedgerCall& c;
    LedgerRows rows;
    hipStream_t s = nullptr;
    bool growing = false, links = false;
    size_t R = 0;
    uint32_t m32 = 0, R32 = 0, L32 = 0, F32 = 0, S = 0, N = 0, k = 0, M = 0, G = 0, n_slots = 0, n_chunks = 0, X = 0, GX = 0;
    LedgerTables T;
    LedgerWork W;
    void *db = nullptr, *wb = nullptr;   // the integer tables and the work buffer on the device
    SmtCallBufs xb{}, sb{};              // the exit tree's update; a growing ledger's state tree's
    StateCallBufs tb{};                  // the state tree's update, whichever tree it is
    LedgerExitGuard exit_guard, tree_guard;
    LedgerDrain drain;
    size_t elems[HZ_LEDGER_ARRAYS] = {}, exit_out_bytes = 0;
    LedgerOutDev od{};
    uint8_t* xd[HZ_LEDGER_EXIT_ARRAYS] = {};
    LedgerCreateOutDev cd{};
    uint64_t new_last = 0;
    const hz_l2sig* d_dest = nullptr;   // by_addr: the signed destinations, for reasons 10 and 11 and the zero-amount rows
    // the undo record of this call (journal on): its layout in the slab, the slot, the accounts the batch found
    bool journal = false;
    JournalLayout jl;
    size_t j_tree = 0;
    int32_t j_slot = -1;
    uint64_t live0 = 0;
    bool j_has_kept = false;
    uint32_t j_last_kept = 0;
    LedgerApply(hz_ledger* l_, const LedgerCall& c_) : l(l_), c(c_) {}
    const hz_l2tx* d_txs() const { return T.tx.dev(db); }
    const uint8_t* planes() const { return (const uint8_t*)l->planes.p; }
    uint32_t* d_fail() const { return (uint32_t*)W.fail.dev(wb); }
};

// stage 1: the argument checks, the plan, the exit tree's plan -- a leaf it cannot hold refuses the call before anything is launched,
// and the pack kernel's integers are the planner's
static hz_status ledger_apply_plan(LedgerApply& a) {
    static_assert(sizeof(hz_ledger_out) == HZ_LEDGER_ARRAYS * sizeof(uint8_t*), "hz_ledger_out is an array of pointers");
    hz_ledger* l = a.l;
    const LedgerCall& c = a.c;
    if (hz_status e = ledger_prepare(l, c, a.rows)) return e;
    a.growing = l->smt != nullptr;
    const LedgerPlan& p = l->plan;
    ledger_forget(l);
    a.R = c.n_l1 + c.m;
    a.m32 = (uint32_t)c.m, a.R32 = (uint32_t)a.R, a.L32 = (uint32_t)c.n_l1, a.F32 = (uint32_t)c.F, a.S = (uint32_t)c.n_sib;
    // N is the plane stride; a growing ledger's tree hands out siblings zero-padded to n_sib, so the gather reads all of them
    a.N = l->N, a.k = a.growing ? a.S : l->k;
    a.M = (uint32_t)p.account.size(), a.G = (uint32_t)p.seg_start.size() - 1, a.n_slots = (uint32_t)p.slot_account.size();
    a.n_chunks = a.R32 ? (a.R32 + HZ_LEDGER_CHUNK - 1) / HZ_LEDGER_CHUNK : 1u;
    a.X = (uint32_t)p.exit_row.size(), a.GX = (uint32_t)p.exit_seg_start.size() - 1;   // exit operations, exit keys
    a.links = c.rq != nullptr && c.m != 0;   // (an atomic call is by_addr: sigs are uploaded, the three arrays have room)
    HZ_HIP(hipSetDevice(l->device));
    a.s = ledger_stream(l);
    if (a.X) {
        if (hz_status e = smt_apply_prepare(l->exit, c.who, HZ_ERR_ARG, a.X, p.exit_key.data(), a.S, true, &a.xb)) return e;
        a.exit_guard.t = l->exit;
    }
    return HZ_OK;
}

// stage 2: the layouts and the room. ints = the integer tables; work = LedgerWork; outs = the 27 arrays; exit_outs = the six exit
// arrays (five per row, the new exit root), create_outs likewise (the new last idx)
static hz_status ledger_apply_buffers(LedgerApply& a) {
    hz_ledger* l = a.l;
    const size_t R = a.R, F = a.c.F;
    a.T.layout(R, F, a.M, a.G, a.X, a.GX, a.c.n_l1, a.n_slots, a.c.creates);
    a.W.layout(R, F, a.M, a.X);
    for (int q = 0; q < HZ_LEDGER_ARRAYS; q++) a.elems[q] = q < LO_TX3 ? R : F;
    a.elems[LO_SIB1] = a.elems[LO_SIB2] = R * a.c.n_sib;
    a.elems[LO_ACC_FEE] = R * F;
    a.elems[LO_SIB3] = F * a.c.n_sib;
    a.elems[LO_OLD_ROOT] = a.elems[LO_NEW_ROOT] = 1;
    size_t out_bytes = 0;
    for (int q = 0; q < HZ_LEDGER_ARRAYS; q++) out_bytes += a.elems[q] * 32;
    HZ_HIP(l->h_ints.grow(a.T.end));
    HZ_HIP(l->ints.grow(a.T.end));
    HZ_HIP(l->work.grow(a.W.end));
    HZ_HIP(l->outs.grow(out_bytes));
    if (a.c.creates) {
        HZ_HIP(l->create_outs.grow(((size_t)(HZ_LEDGER_CREATE_ARRAYS - 1) * R + 1) * 32));
        for (int q = 0; q < HZ_LEDGER_CREATE_ARRAYS; q++) a.cd.a[q] = (uint8_t*)l->create_outs.p + (size_t)q * R * 32;
    }
    if (a.c.exits) {
        a.exit_out_bytes = ((size_t)(HZ_LEDGER_EXIT_ARRAYS - 1) * R + 1) * 32;
        HZ_HIP(l->exit_outs.grow(a.exit_out_bytes));
        HZ_HIP(l->exit_final.grow((size_t)4 * (a.GX ? a.GX : 1) * 32));
        for (int q = 0; q < HZ_LEDGER_EXIT_ARRAYS; q++) a.xd[q] = (uint8_t*)l->exit_outs.p + (size_t)q * R * 32;
    }
    uint8_t* at = (uint8_t*)l->outs.p;
    for (int q = 0; q < HZ_LEDGER_ARRAYS; q++) {
        a.od.a[q] = at;
        at += a.elems[q] * 32;
    }
    a.db = l->ints.p;
    a.wb = l->work.p;
    return HZ_OK;
}

// the undo record of the call, journal on: the tree says how many resident entries its write-back will replace, the
// layout follows, and the slabs get room. The only allocation of the journal: a record larger than any before doubles every slab's
// capacity -- the records held are copied over --, so a steady run of applies allocates nothing here
static hz_status ledger_journal_room(LedgerApply& a) {
    hz_ledger* l = a.l;
    LedgerJournal& J = *l->journal;
    size_t n = 0;
    if (a.M)
        if (hz_status e = a.growing ? smt_journal_entries(l->smt, &n) : state_journal_entries(l->tree, a.M, &n)) return e;
    a.j_tree = n;
    a.jl = journal_layout(n, a.G);
    a.journal = true;
    if (a.jl.bytes <= J.cap) return HZ_OK;
    const size_t cap = journal_grown_cap(J.cap, a.jl.bytes);
    const uint32_t slots = J.ring.slots();
    std::unique_ptr<DevBuf[]> fresh(new DevBuf[slots]);
    for (uint32_t q = 0; q < slots; q++) HZ_HIP(fresh[q].alloc(cap));
    for (const JournalRecord& r : J.ring.rec)
        if (r.bytes) HZ_HIP(hipMemcpyAsync(fresh[r.slot].p, J.slab[r.slot].p, r.bytes, hipMemcpyDeviceToDevice, a.s));
    HZ_HIP(hipStreamSynchronize(a.s));
    J.slab.swap(fresh);
    J.cap = cap;
    return HZ_OK;
}

// stage 3: the tables, and the state tree's plan: hz_state's on a dense ledger; on a growing one hz_smt's, whose planner turns the first
// event of a key the tree does not hold -- a create row's sender event -- into an INSERT and refuses a leaf at depth >= n_sib before
// anything of the update is launched. The create rows read its integers, so they are written behind it
static hz_status ledger_apply_tables(LedgerApply& a) {
    hz_ledger* l = a.l;
    const LedgerPlan& p = l->plan;
    a.T.fill(l->h_ints.p, p, a.rows.l1, a.c.txs, a.c.plan_tokens, l->first_idx, a.xb.old_key, a.xb.fnc, a.xb.is_old0);
    if (a.M && a.growing) {
        if (hz_status e = smt_apply_prepare(l->smt, a.c.who, HZ_ERR_ARG, a.M, p.account.data(), a.S, true, &a.sb)) return e;
        a.tree_guard.t = l->smt;
        a.tb.fields = a.sb.fields;
        a.tb.siblings = a.sb.siblings;
        a.tb.old_value = a.sb.old_value;
        a.tb.old_root = a.sb.roots;
        a.tb.new_root = a.sb.roots + 32;
    } else if (a.M) {
        if (hz_status e = state_apply_prepare(l->tree, a.M, p.account.data(), a.S, &a.tb)) return e;
    }
    a.new_last = l->first_idx + l->live + a.rows.n_creates - 1;
    if (a.c.creates) a.T.fill_creates(l->h_ints.p, p, a.rows.aux_from.data(), a.rows.idx_after.data(), a.new_last, a.sb.old_key, a.sb.is_old0);
    a.live0 = l->live;
    if (l->journal)
        if (hz_status e = ledger_journal_room(a)) return e;
    return HZ_OK;
}

// stage 4: the uploads and the semantic kernels, up to the one synchronise: the failure word. Nothing resident has been written yet
static hz_status ledger_apply_launch(LedgerApply& a) {
    hz_ledger* l = a.l;
    const LedgerCall& c = a.c;
    const LedgerTables& T = a.T;
    const LedgerWork& W = a.W;
    void *db = a.db, *wb = a.wb;
    hipStream_t s = a.s;
    const uint32_t R32 = a.R32, L32 = a.L32, F32 = a.F32, G = a.G, X = a.X;
    HZ_HIP(hipMemcpyAsync(l->ints.p, l->h_ints.p, T.end, hipMemcpyHostToDevice, s));
    HZ_HIP(hipMemsetAsync(a.d_fail(), 0xFF, 4, s));
    if (c.verify || c.by_addr)
        if (hz_status e = ledger_sig_prepare(l, c.m, a.rows.sigs, s, c.verify)) return e;
    const hz_l2sig* d_sigs = (const hz_l2sig*)l->sig_in.p;
    a.d_dest = c.by_addr ? d_sigs : nullptr;
    if (c.by_addr) HZ_HIP(l->aux_rows.grow((a.R ? a.R : 1) * 32));
    if (a.links) {
        a.drain.s = s;
        a.drain.armed = true;
        if (hz_status e = ledger_rq_upload(l, c.m, c.rq, s)) return e;
    }
    if (c.is_batch) HZ_HIP(l->l1_flags.grow(c.n_l1 ? c.n_l1 : 1));
    HZ_HIP(l->t_semantic.begin(s));
    if (R32) {   // (pos_x == NULL: the batch has no exit operation)
        hipLaunchKernelGGL(k_ledger_tx, dim3((R32 + 63) / 64), dim3(64), 0, s, a.d_txs(), T.pos_s.dev(db), T.pos_r.dev(db), W.fee.dev(wb), W.delta.dev(wb),
                           X ? T.pos_x.dev(db) : nullptr, W.xamt.dev(wb), a.d_fail(), R32, L32);
        HZ_HIP(hipGetLastError());
    }
    if (L32) {   // the deltas of the L1 events, beside those k_ledger_tx wrote: one workgroup, no synchronise of its own
        HZ_HIP(l->t_l1.begin(s));
        hipLaunchKernelGGL(k_ledger_l1, dim3(1), dim3(256), 0, s, T.l1.dev(db), T.slot_acct.dev(db), a.planes(), W.delta.dev(wb), W.xamt.dev(wb), (uint8_t*)l->l1_flags.p,
                           a.N, L32, a.n_slots);
        HZ_HIP(hipGetLastError());
        HZ_HIP(l->t_l1.end(s));
    }
    if (F32) {
        hipLaunchKernelGGL(k_ledger_fee_sum, dim3(a.n_chunks), dim3(64), 0, s, W.fee.dev(wb), T.slot.dev(db), W.chunk.dev(wb), R32, F32);
        HZ_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_ledger_fee_scan, dim3(a.n_chunks), dim3(64), 0, s, W.fee.dev(wb), T.slot.dev(db), W.chunk.dev(wb), T.pos_fee.dev(db), a.od.a[LO_ACC_FEE],
                           a.od.a[LO_FINAL_FEE], W.delta.dev(wb), R32, F32, a.n_chunks);
        HZ_HIP(hipGetLastError());
    }
    if (G) {
        hipLaunchKernelGGL(k_ledger_scan, dim3((G + 63) / 64), dim3(64), 0, s, T.pos.dev(db), T.seg.dev(db), a.d_txs(), a.d_dest, T.plan_tok.dev(db), W.delta.dev(wb), a.planes(),
                           W.before.dev(wb), a.tb.fields, a.d_fail(), a.N, G, R32, L32);
        HZ_HIP(hipGetLastError());
    }
    if (X) {   // the exit leaves: it reads the amounts k_ledger_tx and k_ledger_l1 left and the planes, and writes per-call buffers only
        HZ_HIP(l->t_exit_scan.begin(s));
        hipLaunchKernelGGL(k_ledger_exit_scan, dim3((a.GX + 63) / 64), dim3(64), 0, s, T.xpos.dev(db), T.xseg.dev(db), W.xamt.dev(wb), a.planes(), W.xbefore.dev(wb),
                           a.xb.fields, (uint8_t*)l->exit_final.p, a.d_fail(), a.N, a.GX);
        HZ_HIP(hipGetLastError());
        HZ_HIP(l->t_exit_scan.end(s));
    }
    // the signature kernels read the planes and the uploads only: any place before the failure-word read would do. Reason 13, verified or not
    if (hz_status e = ledger_sig_links_launch(l, a.d_txs() + c.n_l1, a.m32, c.chain_id, c.current_num_batch, a.d_fail(), nullptr, L32, c.verify, a.links, s)) return e;
    HZ_HIP(l->t_semantic.end(s));
    HZ_HIP(hipMemcpyAsync(l->h_fail.p, a.d_fail(), 4, hipMemcpyDeviceToHost, s));
    HZ_HIP(hipStreamSynchronize(s));   // the one round trip
    a.drain.armed = false;
    if (a.links) HZ_HIP(l->t_rq.read(l->rq_ms));
    return HZ_OK;
}

// stage 5: the verdict. A refused batch ends here
static hz_status ledger_apply_verdict(LedgerApply& a) {
    const uint32_t word = *(const uint32_t*)a.l->h_fail.p;
    return word == 0xFFFFFFFFu ? HZ_OK : ledger_refused(a.c.who, word >> 8, word & 0xFFu, a.R, a.c.n_l1);
}

// stage 6: outputs, tree, resident planes
static hz_status ledger_apply_commit(LedgerApply& a) {
    hz_ledger* l = a.l;
    const LedgerTables& T = a.T;
    void *db = a.db, *wb = a.wb;
    hipStream_t s = a.s;
    const uint32_t R32 = a.R32, F32 = a.F32, S = a.S, M = a.M, G = a.G, X = a.X;
    if (X) {   // the exit tree's update depends on the scan alone: on its own stream, beside everything below
        HZ_HIP(hipStreamWaitEvent(smt_stream(l->exit), l->t_exit_scan.e1, 0));
        if (hz_status e = smt_apply_launch(l->exit, X, S, true)) return e;
        HZ_HIP(hipEventRecord(l->e_exit_tree, smt_stream(l->exit)));
    }
    if (a.c.exits) HZ_HIP(hipMemsetAsync(l->exit_outs.p, 0, a.exit_out_bytes, s));
    if (R32 + F32) {
        hipLaunchKernelGGL(k_ledger_pack, dim3((R32 + F32 + 63) / 64), dim3(64), 0, s, a.od, a.d_txs(), a.d_dest, (uint8_t*)l->aux_rows.p, l->first_idx, T.ev_s.dev(db),
                           T.ev_r.dev(db), T.ev_fee.dev(db), T.acct.dev(db), a.W.before.dev(wb), a.planes(), a.N, R32, F32, a.L32);
        HZ_HIP(hipGetLastError());
    }
    uint8_t* jbase = nullptr;   // the undo record's slab: the ring's free slot, beside every record held -- the ring changes in the last stage
    if (a.journal) {
        LedgerJournal& J = *l->journal;
        a.j_slot = J.ring.free_slot();
        jbase = (uint8_t*)J.slab[a.j_slot].p;
        a.j_has_kept = l->archive && !l->archive->snaps.empty();
        a.j_last_kept = a.j_has_kept ? l->archive->snaps.back().batch_num : 0u;
    }
    const uint8_t* root0 = nullptr;
    if (M) {
        const SmtJournalDst sj{jbase + a.jl.tree.values, (uint32_t*)(jbase + a.jl.tree.index), a.journal ? &l->journal->t_tree : nullptr};
        const StateJournalDst tj{sj.values, sj.index, sj.span};
        if (hz_status e = a.growing ? smt_apply_launch(l->smt, M, S, true, a.journal ? &sj : nullptr) : state_apply_launch(l->tree, M, S, false, a.journal ? &tj : nullptr))
            return e;
        root0 = a.tb.old_root;
    } else if (a.growing) {   // no update at all: the root as it stands, through the host
        uint8_t r32[32];
        if (hz_status e = hz_smt_root(l->smt, r32)) return e;
        HZ_HIP(hipMemcpy(l->root_buf.p, r32, 32, hipMemcpyHostToDevice));
        root0 = (const uint8_t*)l->root_buf.p;
    } else {
        root0 = state_root_dev(l->tree);
    }
    if (a.c.creates) {   // behind the tree's update: oldValue1 is its old-value buffer's
        HZ_HIP(l->t_create_pack.begin(s));
        hipLaunchKernelGGL(k_ledger_create_pack, dim3((R32 + 64) / 64), dim3(64), 0, s, a.cd, T.crow.dev(db), a.tb.old_value, a.new_last, R32);
        HZ_HIP(hipGetLastError());
        HZ_HIP(l->t_create_pack.end(s));
    }
    HZ_HIP(hipMemcpyAsync(a.od.a[LO_OLD_ROOT], root0, 32, hipMemcpyDeviceToDevice, s));
    HZ_HIP(hipMemcpyAsync(a.od.a[LO_NEW_ROOT], M ? a.tb.new_root + (size_t)(M - 1) * 32 : root0, 32, hipMemcpyDeviceToDevice, s));
    if (R32 + F32) {
        const size_t threads = (size_t)(R32 + F32) * (S + 1);
        hipLaunchKernelGGL(k_ledger_gather, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a.od, T.ev_s.dev(db), T.ev_r.dev(db), T.ev_fee.dev(db), T.last.dev(db),
                           a.tb.siblings, a.tb.new_root, root0, a.k, S, R32, F32);
        HZ_HIP(hipGetLastError());
    }
    if (G && a.journal) {   // the plane elements k_ledger_writeback is about to replace
        LedgerJournal& J = *l->journal;
        HZ_HIP(J.t_planes.begin(s));
        hipLaunchKernelGGL(k_ledger_journal_save, dim3((4 * G + 255) / 256), dim3(256), 0, s, T.pos.dev(db), T.seg.dev(db), a.planes(), jbase + a.jl.planes.values,
                           (uint32_t*)(jbase + a.jl.planes.index), a.N, G, (uint32_t)a.live0);
        HZ_HIP(hipGetLastError());
        HZ_HIP(J.t_planes.end(s));
    }
    if (G) {
        hipLaunchKernelGGL(k_ledger_writeback, dim3((G + 63) / 64), dim3(64), 0, s, T.pos.dev(db), T.seg.dev(db), a.tb.fields, (uint8_t*)l->planes.p, a.N, G);
        HZ_HIP(hipGetLastError());
    }
    if (X) {   // the exit rows, once the exit tree's update is through: leaf-2 rows and siblings2 over what k_ledger_pack / _gather left there
        LedgerExitOutDev xo;
        for (int q = 0; q < 6; q++) xo.tx2[q] = a.od.a[LO_TX2 + q];
        xo.sib2 = a.od.a[LO_SIB2];
        for (int q = 0; q < HZ_LEDGER_EXIT_ARRAYS; q++) xo.x[q] = a.xd[q];
        HZ_HIP(hipStreamWaitEvent(s, l->e_exit_tree, 0));
        HZ_HIP(l->t_exit_rows.begin(s));
        hipLaunchKernelGGL(k_ledger_exit_pack, dim3((R32 + 63) / 64), dim3(64), 0, s, xo, T.ev_x.dev(db), T.xop.dev(db), a.W.xbefore.dev(wb), a.xb.old_value, a.planes(), a.N,
                           R32);
        HZ_HIP(hipGetLastError());
        const size_t threads = (size_t)R32 * (S + 1);
        hipLaunchKernelGGL(k_ledger_exit_gather, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, xo, T.ev_x.dev(db), T.last_x.dev(db), a.xb.siblings, a.xb.roots,
                           S, R32);
        HZ_HIP(hipGetLastError());
        HZ_HIP(hipMemcpyAsync(a.xd[XO_NEW_ROOT], a.xb.roots + (size_t)X * 32, 32, hipMemcpyDeviceToDevice, s));
        HZ_HIP(l->t_exit_rows.end(s));
    }
    HZ_HIP(hipEventRecord(l->e_done, s));
    return HZ_OK;
}

// n arrays of `rows` elements each (the last one: a single element) to the host arrays of `out`, a struct of n nullable pointers
static hz_status ledger_copy_rows(const void* out, uint8_t* const* dev, int n, size_t rows, hipStream_t s) {
    uint8_t* const* h = (uint8_t* const*)out;
    for (int q = 0; out && q < n; q++) {
        const size_t count = q == n - 1 ? 1 : rows;
        if (h[q] && count) HZ_HIP(hipMemcpyAsync(h[q], dev[q], count * 32, hipMemcpyDeviceToHost, s));
    }
    return HZ_OK;
}

// stage 7: the copies to the host arrays the caller gave
static hz_status ledger_apply_copy_out(LedgerApply& a) {
    static_assert(XO_NEW_ROOT == HZ_LEDGER_EXIT_ARRAYS - 1 && CO_NEW_LAST == HZ_LEDGER_CREATE_ARRAYS - 1, "the single element is the last array");
    hz_ledger* l = a.l;
    const LedgerCall& c = a.c;
    if (hz_status e = ledger_copy_rows(c.create_out, a.cd.a, HZ_LEDGER_CREATE_ARRAYS, a.R, a.s)) return e;
    if (hz_status e = ledger_copy_rows(c.exit_out, a.xd, HZ_LEDGER_EXIT_ARRAYS, a.R, a.s)) return e;
    if (c.out) {
        uint8_t* const* h = (uint8_t* const*)c.out;
        for (int q = 0; q < HZ_LEDGER_ARRAYS; q++)
            if (h[q] && a.elems[q]) HZ_HIP(hipMemcpyAsync(h[q], a.od.a[q], a.elems[q] * 32, hipMemcpyDeviceToHost, a.s));
    }
    if (c.verify)
        if (hz_status e = ledger_sig_copy_out(l, c.m, c.sig_out, a.s)) return e;
    if (c.by_addr && c.aux_to_idx_out && a.R) HZ_HIP(hipMemcpyAsync(c.aux_to_idx_out, l->aux_rows.p, a.R * 32, hipMemcpyDeviceToHost, a.s));
    if (c.flags_out && c.n_l1) HZ_HIP(hipMemcpyAsync(c.flags_out, l->l1_flags.p, c.n_l1, hipMemcpyDeviceToHost, a.s));
    return HZ_OK;
}

// what hz_ledger_main_inputs will need of this call: host copies of a few kilobytes, no device work
static void ledger_main_call_keep(LedgerApply& a) {
    const LedgerCall& c = a.c;
    LedgerMainCall& k = a.l->main_call;
    k.n_l1 = c.n_l1, k.m = c.m, k.F = c.F, k.n_sib = c.n_sib;
    k.chain_id = c.chain_id, k.current_num_batch = c.current_num_batch;
    k.flags = (c.sigs ? HZ_MI_SIGS : 0u) | (a.links ? HZ_MI_RQ : 0u) | (c.exits ? HZ_MI_EXITS : 0u) | (c.creates ? HZ_MI_CREATES : 0u) | (c.by_addr ? HZ_MI_AUX : 0u) |
              (a.growing ? HZ_MI_GROWING : 0u);
    k.last_before = a.new_last - a.rows.n_creates;
    k.tx = a.T.tx, k.l1 = a.T.l1, k.crow = a.T.crow;
    if (c.from_bjj && c.n_l1)
        k.keys.assign(c.from_bjj, c.from_bjj + c.n_l1 * 32);
    else
        k.keys.clear();
    k.fee_idxs.assign(c.fee_idxs, c.fee_idxs + c.F);
    k.plan_tokens.assign(c.plan_tokens, c.plan_tokens + c.F);
    k.valid = true;
}

// stage 8: the trees' updates finished -- from there the created accounts exist --, the times, what the getters may hand out
static hz_status ledger_apply_finish(LedgerApply& a) {
    hz_ledger* l = a.l;
    const LedgerCall& c = a.c;
    const LedgerPlan& p = l->plan;
    if (a.M && a.growing) {
        a.tree_guard.t = nullptr;
        if (hz_status e = smt_apply_finish(l->smt, a.journal ? &l->journal->undo[a.j_slot] : nullptr)) {
            smt_apply_abort(l->smt);
            return e;
        }
        l->live += a.rows.n_creates;
    } else if (a.M) {
        if (hz_status e = state_apply_finish(l->tree)) return e;
    } else {
        HZ_HIP(hipStreamSynchronize(a.s));
    }
    double ms = 0.0;
    if (a.X) {
        a.exit_guard.t = nullptr;
        if (hz_status e = smt_apply_finish(l->exit)) {
            smt_apply_abort(l->exit);
            return e;
        }
        l->exit_ms = hz_smt_device_ms(l->exit);
        for (const DevSpan* t : {&l->t_exit_scan, &l->t_exit_rows}) {
            HZ_HIP(t->read(ms));
            l->exit_ms += ms;
        }
        for (uint32_t g = 0; g < a.GX; g++) l->exit_keys.push_back({p.exit_key[p.exit_perm[p.exit_seg_start[g]]], g});
        std::sort(l->exit_keys.begin(), l->exit_keys.end());
    }
    if (c.exits) {
        for (int q = 0; q < HZ_LEDGER_EXIT_ARRAYS; q++) l->exit_dev[q] = a.xd[q];
        l->have_exit_outputs = true;
    }
    HZ_HIP(l->t_semantic.read(l->semantic_ms));
    HZ_HIP(elapsed_ms(l->t_semantic.e0, l->e_done, l->device_ms));
    l->out_dev = a.od;
    l->have_outputs = true;
    l->have_aux = c.by_addr;
    l->have_l1 = c.is_batch;
    if (c.creates) {
        for (int q = 0; q < HZ_LEDGER_CREATE_ARRAYS; q++) l->create_dev[q] = a.cd.a[q];
        l->have_create_outputs = true;
        HZ_HIP(l->t_create_pack.read(l->create_ms));
        if (a.rows.n_creates) {
            HZ_HIP(l->t_create.read(ms));
            l->create_ms += ms;
        }
    }
    if (a.L32) HZ_HIP(l->t_l1.read(l->l1_ms));
    if (c.verify) {
        HZ_HIP(l->t_sig.read(l->sig_ms));
        l->have_sig_outputs = true;
    }
    if (c.verify || c.by_addr) ledger_main_call_keep(a);   // every call but hz_ledger_apply_l2: it has a chain id, and the sigs are uploaded
    double journal_ms = 0.0;   // the save kernels' time, read before the ring and the mark move: both move together or not at all
    if (a.journal && a.j_tree) {
        HZ_HIP(l->journal->t_tree.read(ms));
        journal_ms += ms;
    }
    if (a.journal && a.G) {
        HZ_HIP(l->journal->t_planes.read(ms));
        journal_ms += ms;
    }
    l->journal_ms = journal_ms;
    if (a.journal) {   // the call stands: so does its undo record
        LedgerJournal& J = *l->journal;
        JournalRecord r;
        r.mark = l->applied, r.live = a.live0, r.has_kept = a.j_has_kept, r.last_kept = a.j_last_kept;
        r.slot = (uint32_t)a.j_slot, r.tree_entries = a.j_tree, r.groups = a.G, r.bytes = a.jl.bytes;
        J.has_undo[r.slot] = a.M && a.growing;
        J.ring.push(r);
    }
    l->applied++;
    return HZ_OK;
}

static hz_status ledger_apply(hz_ledger* l, const LedgerCall& c) {
    LedgerApply a(l, c);
    for (hz_status (*stage)(LedgerApply&) : {ledger_apply_plan, ledger_apply_buffers, ledger_apply_tables, ledger_apply_launch, ledger_apply_verdict, ledger_apply_commit,
                                             ledger_apply_copy_out, ledger_apply_finish})
        if (hz_status e = stage(a)) return e;
    return HZ_OK;
}

// ---- the exported apply calls: each states its call, by family ---------------------------------------------------------------------------
static LedgerCall ledger_call_l2(const char* who, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, uint32_t chain_id, uint32_t current_num_batch, size_t F,
                                 const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs, size_t n_sib, const hz_ledger_out* out, const hz_ledger_sig_out* sig_out) {
    LedgerCall c;
    c.who = who, c.m = m, c.txs = txs, c.sigs = sigs, c.chain_id = chain_id, c.current_num_batch = current_num_batch;
    c.F = F, c.plan_tokens = fee_plan_tokens, c.fee_idxs = fee_idxs, c.n_sib = n_sib, c.out = out, c.sig_out = sig_out;
    return c;
}

// by_addr: flags and the receivers by address on top
static LedgerCall ledger_call_addr(LedgerCall c, uint32_t flags, const uint64_t* aux_to_idx, uint8_t* aux_to_idx_out) {
    c.by_addr = true, c.flags = flags, c.verify = (flags & HZ_LEDGER_VERIFY_SIGS) != 0, c.aux_to_idx = aux_to_idx, c.aux_to_idx_out = aux_to_idx_out;
    return c;
}

// is_batch: an L1 run in front
static LedgerCall ledger_call_batch(LedgerCall c, size_t n_l1, const hz_l1tx* l1, uint8_t* l1_flags_out) {
    c.is_batch = true, c.n_l1 = n_l1, c.l1 = l1, c.flags_out = l1_flags_out;
    return c;
}

extern "C" hz_status hz_ledger_apply_l2(hz_ledger* l, size_t m, const hz_l2tx* txs, size_t F, const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs,
                                        size_t n_sib, const hz_ledger_out* out) {
    return ledger_apply(l, ledger_call_l2("hz_ledger_apply_l2", m, txs, nullptr, 0, 0, F, fee_plan_tokens, fee_idxs, n_sib, out, nullptr));
}

extern "C" hz_status hz_ledger_apply_l2_signed(hz_ledger* l, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, uint32_t chain_id, uint32_t current_num_batch,
                                               size_t F, const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs, size_t n_sib, const hz_ledger_out* out,
                                               const hz_ledger_sig_out* sig_out) {
    LedgerCall c = ledger_call_l2("hz_ledger_apply_l2_signed", m, txs, sigs, chain_id, current_num_batch, F, fee_plan_tokens, fee_idxs, n_sib, out, sig_out);
    c.verify = true;
    return ledger_apply(l, c);
}

extern "C" hz_status hz_ledger_apply_l2_addr(hz_ledger* l, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, uint32_t flags, const uint64_t* aux_to_idx,
                                             uint32_t chain_id, uint32_t current_num_batch, size_t F, const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs,
                                             size_t n_sib, const hz_ledger_out* out, const hz_ledger_sig_out* sig_out, uint8_t* aux_to_idx_out) {
    return ledger_apply(l, ledger_call_addr(ledger_call_l2("hz_ledger_apply_l2_addr", m, txs, sigs, chain_id, current_num_batch, F, fee_plan_tokens, fee_idxs, n_sib, out, sig_out),
                                            flags, aux_to_idx, aux_to_idx_out));
}

// ---- an L1 run in front of the L2 transactions ---------------------------------------------------------------------------
extern "C" hz_status hz_ledger_apply_batch(hz_ledger* l, size_t n_l1, const hz_l1tx* l1, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, uint32_t flags,
                                           const uint64_t* aux_to_idx, uint32_t chain_id, uint32_t current_num_batch, size_t F, const uint32_t* fee_plan_tokens,
                                           const uint64_t* fee_idxs, size_t n_sib, const hz_ledger_out* out, const hz_ledger_sig_out* sig_out,
                                           uint8_t* aux_to_idx_out, uint8_t* l1_flags_out) {
    const LedgerCall l2 = ledger_call_l2("hz_ledger_apply_batch", m, txs, sigs, chain_id, current_num_batch, F, fee_plan_tokens, fee_idxs, n_sib, out, sig_out);
    return ledger_apply(l, ledger_call_batch(ledger_call_addr(l2, flags, aux_to_idx, aux_to_idx_out), n_l1, l1, l1_flags_out));
}

extern "C" hz_status hz_ledger_l1_flags_dev(hz_ledger* l, uint8_t** dev) {
    uint8_t* const p = l ? (uint8_t*)l->l1_flags.p : nullptr;
    return ledger_hand_out("hz_ledger_l1_flags_dev", l, dev, l ? &l->have_l1 : nullptr, "hz_ledger_apply_batch", &p, 1);
}

extern "C" double hz_ledger_l1_ms(const hz_ledger* l) { return l ? l->l1_ms : 0.0; }

extern "C" hz_status hz_ledger_aux_to_idx_dev(hz_ledger* l, uint8_t** dev) {
    uint8_t* const p = l ? (uint8_t*)l->aux_rows.p : nullptr;
    return ledger_hand_out("hz_ledger_aux_to_idx_dev", l, dev, l ? &l->have_aux : nullptr, "hz_ledger_apply_l2_addr", &p, 1);
}

extern "C" double hz_ledger_resolve_ms(const hz_ledger* l) { return l ? l->resolve_ms : 0.0; }

// ---- exits into the batch's exit tree ------------------------------------------------------------------------------------
extern "C" hz_status hz_ledger_apply_batch_exits(hz_ledger* l, size_t n_l1, const hz_l1tx* l1, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, uint32_t flags,
                                                 const uint64_t* aux_to_idx, uint32_t chain_id, uint32_t current_num_batch, size_t F, const uint32_t* fee_plan_tokens,
                                                 const uint64_t* fee_idxs, size_t n_sib, const hz_ledger_out* out, const hz_ledger_sig_out* sig_out,
                                                 uint8_t* aux_to_idx_out, uint8_t* l1_flags_out, const hz_ledger_exit_out* exit_out) {
    static_assert(sizeof(hz_ledger_exit_out) == HZ_LEDGER_EXIT_ARRAYS * sizeof(uint8_t*), "hz_ledger_exit_out is an array of pointers");
    const LedgerCall l2 = ledger_call_l2("hz_ledger_apply_batch_exits", m, txs, sigs, chain_id, current_num_batch, F, fee_plan_tokens, fee_idxs, n_sib, out, sig_out);
    LedgerCall c = ledger_call_batch(ledger_call_addr(l2, flags, aux_to_idx, aux_to_idx_out), n_l1, l1, l1_flags_out);
    c.exits = true, c.exit_out = exit_out;
    return ledger_apply(l, c);
}

extern "C" hz_status hz_ledger_exit_outputs_dev(hz_ledger* l, hz_ledger_exit_out* dev) {
    return ledger_hand_out("hz_ledger_exit_outputs_dev", l, dev, l ? &l->have_exit_outputs : nullptr, "hz_ledger_apply_batch_exits", l ? l->exit_dev : nullptr,
                           HZ_LEDGER_EXIT_ARRAYS);
}

extern "C" hz_smt* hz_ledger_exit_tree(hz_ledger* l) { return l ? l->exit : nullptr; }
extern "C" double hz_ledger_exit_ms(const hz_ledger* l) { return l ? l->exit_ms : 0.0; }

extern "C" hz_status hz_ledger_exit_accounts(hz_ledger* l, size_t n, const uint64_t* key, uint8_t* fields_out) {
    const char* who = "hz_ledger_exit_accounts";
    if (hz_status e = ledger_ready(l, who)) return e;
    if (n == 0) return HZ_OK;
    if (!key || !fields_out) return set_err(HZ_ERR_ARG, "%s: null argument", who);
    if (n > HZ_LEDGER_MAX_EVENTS) return set_err(HZ_ERR_ARG, "%s: %zu leaves in one call (at most %u)", who, n, HZ_LEDGER_MAX_EVENTS);
    const uint32_t GX = (uint32_t)l->exit_keys.size();
    std::vector<uint32_t> at(n);
    for (size_t i = 0; i < n; i++) {
        const auto it = std::lower_bound(l->exit_keys.begin(), l->exit_keys.end(), std::make_pair(key[i], 0u));
        if (it == l->exit_keys.end() || it->first != key[i])
            return set_err(HZ_ERR_ARG, "%s: key[%zu] = %llu is not in the exit tree of the last batch", who, i, (unsigned long long)key[i]);
        at[i] = it->second;
    }
    HZ_HIP(hipSetDevice(l->device));
    ledger_forget(l);   // the call's buffers are reused
    hipStream_t s = ledger_stream(l);
    HZ_HIP(l->ints.grow(n * 4));
    HZ_HIP(l->work.grow(n * 128));
    HZ_HIP(hipMemcpyAsync(l->ints.p, at.data(), n * 4, hipMemcpyHostToDevice, s));
    // the final leaves lie plane-major, [4][GX], as the resident planes do: the same gather
    hipLaunchKernelGGL(k_ledger_accounts, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, s, (const uint32_t*)l->ints.p, (const uint8_t*)l->exit_final.p,
                       (uint8_t*)l->work.p, GX, (uint32_t)n);
    HZ_HIP(hipGetLastError());
    HZ_HIP(hipMemcpyAsync(fields_out, l->work.p, n * 128, hipMemcpyDeviceToHost, s));
    HZ_HIP(hipStreamSynchronize(s));
    return HZ_OK;
}

// ---- exit trees of earlier batches kept, Withdraw's inputs in bulk (ledger_archive.h) ------------------------------------------
static hz_status ledger_archive(hz_ledger* l, LedgerArchive** out) {
    if (!l->archive) {
        std::unique_ptr<LedgerArchive> a(new LedgerArchive);
        HZ_HIP(hipSetDevice(l->device));
        for (DevSpan* t : {&a->t_keep, &a->t_withdraw}) HZ_HIP(t->create());
        l->archive = std::move(a);
    }
    *out = l->archive.get();
    return HZ_OK;
}

// the snapshot of batch_num, or -1
static int64_t archive_find(const LedgerArchive* a, uint32_t batch_num) {
    if (!a) return -1;
    const auto it = std::lower_bound(a->snaps.begin(), a->snaps.end(), batch_num, [](const ArchiveSnap& s, uint32_t b) { return s.batch_num < b; });
    return it != a->snaps.end() && it->batch_num == batch_num ? (int64_t)(it - a->snaps.begin()) : -1;
}

// the descriptors of `snaps` into a table with room for them; the caller synchronises
static hipError_t archive_upload_table(const std::vector<ArchiveSnap>& snaps, void* table, std::vector<ArchiveDesc>& host, hipStream_t s) {
    host.resize(snaps.size());
    for (size_t i = 0; i < snaps.size(); i++) host[i] = snaps[i].desc;
    return snaps.empty() ? hipSuccess : hipMemcpyAsync(table, host.data(), snaps.size() * sizeof(ArchiveDesc), hipMemcpyHostToDevice, s);
}

extern "C" hz_status hz_ledger_exit_keep(hz_ledger* l, uint32_t batch_num) {
    const char* who = "hz_ledger_exit_keep";
    if (hz_status e = ledger_ready(l, who)) return e;
    if (l->archive && !l->archive->snaps.empty() && batch_num <= l->archive->snaps.back().batch_num)
        return set_err(HZ_ERR_ARG, "%s: batch_num = %u is not above the last kept batch, %u", who, batch_num, l->archive->snaps.back().batch_num);
    if (smt_poisoned(l->exit)) return set_err(HZ_ERR_HIP, "%s: the exit tree's last update failed on the device", who);
    LedgerArchive* a = nullptr;
    if (hz_status e = ledger_archive(l, &a)) return e;
    const SmtView v = smt_view(l->exit);
    const size_t G = v.leaves;
    if (G != l->exit_keys.size()) return set_err(HZ_ERR_HIP, "%s: the exit tree holds %zu leaves, the ledger %zu exit leaves", who, G, l->exit_keys.size());
    const ArchiveLayout lay = archive_layout(v.nodes, G);
    // leaf number -> place among the final exit leaves
    std::vector<uint32_t> place(G);
    for (size_t i = 0; i < G; i++) {
        const auto it = std::lower_bound(l->exit_keys.begin(), l->exit_keys.end(), std::make_pair(v.leaf_key[i], 0u));
        if (it == l->exit_keys.end() || it->first != v.leaf_key[i]) return set_err(HZ_ERR_HIP, "%s: leaf %zu of the exit tree has no exit leaf", who, i);
        place[i] = it->second;
    }
    HZ_HIP(hipSetDevice(l->device));
    // every allocation comes first: where one fails nothing of the archive has changed
    std::unique_ptr<ArchiveSlab> fresh;
    ArchiveSlab* slab = nullptr;
    if (lay.bytes) {
        slab = a->slabs.empty() ? nullptr : a->slabs.back().get();
        if (!slab || slab->used + lay.bytes > slab->buf.bytes) {
            fresh.reset(new ArchiveSlab);
            HZ_HIP(fresh->buf.alloc(std::max(HZ_ARCHIVE_SLAB_BYTES, lay.bytes)));
            slab = fresh.get();
        }
    }
    DevBuf grown;
    const size_t want = (a->snaps.size() + 1) * sizeof(ArchiveDesc);
    if (want > a->table.bytes) HZ_HIP(grown.alloc(std::max((size_t)64 * sizeof(ArchiveDesc), 2 * a->table.bytes)));
    void* table = grown.p ? grown.p : a->table.p;
    ArchiveSnap snap;
    snap.batch_num = batch_num;
    snap.slab = slab;
    snap.bytes = lay.bytes;
    uint8_t* base = slab ? (uint8_t*)slab->buf.p + slab->used : nullptr;
    snap.desc.root = v.root;
    snap.desc.leaves = (uint32_t)G;
    snap.desc.nodes = (uint32_t)v.nodes;
    snap.desc.batch_num = batch_num;
    if (base) {   // (the empty tree: root 0, no address is ever read)
        snap.desc.child = (const int32_t*)(base + lay.child);
        snap.desc.leaf_key = (const uint64_t*)(base + lay.leaf_key);
        snap.desc.leaf_place = (const uint32_t*)(base + lay.leaf_place);
        snap.desc.node = base + lay.node;
        snap.desc.leaf = base + lay.leaf;
        snap.desc.fields = base + lay.fields;
    }
    std::vector<ArchiveSnap> next = a->snaps;
    next.push_back(snap);
    std::vector<ArchiveDesc> host_table;
    hipStream_t s = ledger_stream(l);
    // the tree's pools and the final exit leaves are at rest: every apply call ends behind its synchronise
    const hz_status st = [&]() -> hz_status {
        HZ_HIP(a->t_keep.begin(s));
        if (v.nodes) {
            HZ_HIP(hipMemcpyAsync(base + lay.child, v.child, v.nodes * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
            HZ_HIP(hipMemcpyAsync(base + lay.node, v.node_digest, v.nodes * 32, hipMemcpyDeviceToDevice, s));
        }
        if (G) {
            HZ_HIP(hipMemcpyAsync(base + lay.leaf_key, v.leaf_key, G * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            HZ_HIP(hipMemcpyAsync(base + lay.leaf_place, place.data(), G * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            HZ_HIP(hipMemcpyAsync(base + lay.leaf, v.leaf_hash, G * 32, hipMemcpyDeviceToDevice, s));
            HZ_HIP(hipMemcpyAsync(base + lay.fields, l->exit_final.p, G * 4 * 32, hipMemcpyDeviceToDevice, s));
        }
        HZ_HIP(archive_upload_table(next, table, host_table, s));
        HZ_HIP(a->t_keep.end(s));
        HZ_HIP(hipStreamSynchronize(s));
        HZ_HIP(a->t_keep.read(a->keep_ms));
        return HZ_OK;
    }();
    if (st) {
        (void)hipStreamSynchronize(s);   // nothing stays in flight over the host arrays; the old table's entries were rewritten with their own values
        return st;
    }
    if (grown.p) std::swap(a->table.p, grown.p), std::swap(a->table.bytes, grown.bytes);
    if (fresh) a->slabs.push_back(std::move(fresh));
    if (slab) {
        slab->used += lay.bytes;
        slab->live++;
    }
    a->snaps.swap(next);
    return HZ_OK;
}

// a slab no snapshot lies in any more is freed (no call is in flight: every one ends behind a synchronise)
static void archive_free_empty_slabs(LedgerArchive* a) {
    for (size_t i = a->slabs.size(); i-- > 0;)
        if (a->slabs[i]->live == 0) a->slabs.erase(a->slabs.begin() + (ptrdiff_t)i);
}

extern "C" hz_status hz_ledger_exit_forget(hz_ledger* l, uint32_t below_batch) {
    const char* who = "hz_ledger_exit_forget";
    if (!l) return set_err(HZ_ERR_ARG, "%s: null ledger", who);
    LedgerArchive* a = l->archive.get();
    if (!a) return HZ_OK;
    size_t drop = 0;
    while (drop < a->snaps.size() && a->snaps[drop].batch_num < below_batch) drop++;
    if (drop == 0) return HZ_OK;
    HZ_HIP(hipSetDevice(l->device));
    for (size_t i = 0; i < drop; i++)
        if (ArchiveSlab* slab = a->snaps[i].slab) slab->live--;
    a->snaps.erase(a->snaps.begin(), a->snaps.begin() + (ptrdiff_t)drop);
    archive_free_empty_slabs(a);
    std::vector<ArchiveDesc> host_table;
    hipStream_t s = ledger_stream(l);
    HZ_HIP(archive_upload_table(a->snaps, a->table.p, host_table, s));
    HZ_HIP(hipStreamSynchronize(s));
    return HZ_OK;
}

extern "C" hz_status hz_ledger_exit_kept(const hz_ledger* l, uint32_t* batch_out, size_t cap, size_t* n) {
    if (!l || !n || (cap && !batch_out)) return set_err(HZ_ERR_ARG, "hz_ledger_exit_kept: null argument");
    const size_t count = l->archive ? l->archive->snaps.size() : 0;
    for (size_t i = 0; i < count && i < cap; i++) batch_out[i] = l->archive->snaps[i].batch_num;
    *n = count;
    return HZ_OK;
}

extern "C" hz_status hz_ledger_exit_archive_stats(const hz_ledger* l, size_t* snapshots, size_t* slabs, size_t* bytes_used, size_t* bytes_reserved) {
    if (!l) return set_err(HZ_ERR_ARG, "hz_ledger_exit_archive_stats: null ledger");
    size_t used = 0, reserved = 0;
    const LedgerArchive* a = l->archive.get();
    if (a) {
        for (const ArchiveSnap& s : a->snaps) used += s.bytes;
        for (const auto& s : a->slabs) reserved += s->buf.bytes;
        reserved += a->table.bytes;
    }
    if (snapshots) *snapshots = a ? a->snaps.size() : 0;
    if (slabs) *slabs = a ? a->slabs.size() : 0;
    if (bytes_used) *bytes_used = used;
    if (bytes_reserved) *bytes_reserved = reserved;
    return HZ_OK;
}

extern "C" hz_status hz_ledger_exit_root_of(hz_ledger* l, uint32_t batch_num, uint8_t* out32) {
    const char* who = "hz_ledger_exit_root_of";
    if (!l || !out32) return set_err(HZ_ERR_ARG, "%s: null argument", who);
    const int64_t at = archive_find(l->archive.get(), batch_num);
    if (at < 0) return set_err(HZ_ERR_ARG, "%s: batch %u is not kept", who, batch_num);
    const ArchiveDesc& d = l->archive->snaps[(size_t)at].desc;
    memset(out32, 0, 32);
    if (d.root == 0) return HZ_OK;
    const uint32_t src = arc_src(d.root);
    HZ_HIP(hipSetDevice(l->device));
    hipStream_t s = ledger_stream(l);
    HZ_HIP(hipMemcpyAsync(out32, (src >> 30 == ARC_NODE ? d.node : d.leaf) + (size_t)(src & 0x3FFFFFFFu) * 32, 32, hipMemcpyDeviceToHost, s));
    HZ_HIP(hipStreamSynchronize(s));
    return HZ_OK;
}

extern "C" hz_status hz_ledger_withdraw_rows(hz_ledger* l, size_t n, const uint32_t* batch_num, const uint64_t* idx, int32_t n_levels, const hz_withdraw_rows_out* out) {
    static_assert(sizeof(hz_withdraw_rows_out) == HZ_WITHDRAW_ARRAYS * sizeof(uint8_t*), "hz_withdraw_rows_out is an array of pointers");
    const char* who = "hz_ledger_withdraw_rows";
    if (n_levels < 0 || n_levels + 1 > (int32_t)HZ_ARCHIVE_MAX_DEPTH) return set_err(HZ_ERR_ARG, "%s: n_levels + 1 = %d siblings (1 .. 64)", who, n_levels + 1);
    if (n > HZ_WITHDRAW_MAX_ROWS) return set_err(HZ_ERR_ARG, "%s: %zu queries in one call (at most 2^20)", who, n);
    if (n && (!batch_num || !idx)) return set_err(HZ_ERR_ARG, "%s: null argument", who);
    if (!l) return set_err(HZ_ERR_ARG, "%s: null ledger", who);
    if (hz_status e = ledger_ready(l, who)) return e;
    LedgerArchive* a = nullptr;
    if (hz_status e = ledger_archive(l, &a)) return e;
    ledger_forget(l);   // the call's buffers are reused
    a->withdraw_ms = 0.0;
    if (n == 0) return HZ_OK;
    const uint32_t S = (uint32_t)n_levels + 1, N = (uint32_t)n;
    HZ_HIP(hipSetDevice(l->device));
    hipStream_t s = ledger_stream(l);
    WithdrawTables T;
    T.layout(n, S);
    // the rows: the seven single arrays [7][n][32] | siblings [n][S][32] | status [n]
    const size_t o_sib = (size_t)WR_ROWS * n * 32, o_status = o_sib + n * S * 32, out_bytes = o_status + n;
    HZ_HIP(l->h_ints.grow(T.up));
    HZ_HIP(l->ints.grow(T.end));
    HZ_HIP(l->outs.grow(out_bytes));
    T.fill(l->h_ints.p, batch_num, idx, [&](uint32_t batch) { return archive_find(a, batch); });
    LedgerDrain drain;
    drain.s = s;
    drain.armed = true;   // the pinned block is the ledger's: no copy from it, or into the caller's arrays, outlives the call
    void* db = l->ints.p;
    uint8_t* ob = (uint8_t*)l->outs.p;
    HZ_HIP(hipMemcpyAsync(db, l->h_ints.p, T.up, hipMemcpyHostToDevice, s));
    HZ_HIP(a->t_withdraw.begin(s));
    hipLaunchKernelGGL(k_withdraw_walk, dim3((N + 63) / 64), dim3(64), 0, s, (const ArchiveDesc*)a->table.p, T.snap.dev(db), T.idx.dev(db), T.meta.dev(db), T.src.dev(db),
                       ob + o_status, S, N);
    HZ_HIP(hipGetLastError());
    const size_t lanes = n * (S + WR_ROWS) * 2;
    hipLaunchKernelGGL(k_withdraw_fill, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, (const ArchiveDesc*)a->table.p, T.snap.dev(db), T.idx.dev(db), T.meta.dev(db),
                       T.src.dev(db), ob, ob + o_sib, S, N);
    HZ_HIP(hipGetLastError());
    HZ_HIP(a->t_withdraw.end(s));
    uint8_t* dev[HZ_WITHDRAW_ARRAYS];
    for (uint32_t r = 0; r < WR_ROWS; r++) dev[r] = ob + (size_t)r * n * 32;
    dev[WR_ROWS] = ob + o_sib;
    dev[WR_ROWS + 1] = ob + o_status;
    if (out) {
        uint8_t* const* h = (uint8_t* const*)out;
        for (uint32_t r = 0; r < HZ_WITHDRAW_ARRAYS; r++)
            if (h[r]) HZ_HIP(hipMemcpyAsync(h[r], dev[r], r < WR_ROWS ? n * 32 : r == WR_ROWS ? n * S * 32 : n, hipMemcpyDeviceToHost, s));
    }
    HZ_HIP(hipStreamSynchronize(s));
    drain.armed = false;
    HZ_HIP(a->t_withdraw.read(a->withdraw_ms));
    for (uint32_t r = 0; r < HZ_WITHDRAW_ARRAYS; r++) a->rows_dev[r] = dev[r];
    a->have_rows = true;
    return HZ_OK;
}

extern "C" hz_status hz_ledger_withdraw_rows_dev(hz_ledger* l, hz_withdraw_rows_out* dev) {
    const LedgerArchive* a = l ? l->archive.get() : nullptr;
    return ledger_hand_out("hz_ledger_withdraw_rows_dev", l, dev, a ? &a->have_rows : nullptr, "hz_ledger_withdraw_rows (of at least one query)",
                           a ? a->rows_dev : nullptr, HZ_WITHDRAW_ARRAYS);
}

extern "C" double hz_ledger_withdraw_ms(const hz_ledger* l) { return l && l->archive ? l->archive->withdraw_ms : 0.0; }
extern "C" double hz_ledger_exit_keep_ms(const hz_ledger* l) { return l && l->archive ? l->archive->keep_ms : 0.0; }

// ---- L1 rows that create accounts, on a growing ledger -------------------------------------------------------------------
extern "C" hz_status hz_ledger_apply_batch_creates(hz_ledger* l, size_t n_l1, const hz_l1tx* l1, const uint8_t* from_bjj, size_t m, const hz_l2tx* txs,
                                                   const hz_l2sig* sigs, uint32_t flags, const uint64_t* aux_to_idx, uint32_t chain_id, uint32_t current_num_batch,
                                                   size_t F, const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs, size_t n_sib, const hz_ledger_out* out,
                                                   const hz_ledger_sig_out* sig_out, uint8_t* aux_to_idx_out, uint8_t* l1_flags_out, const hz_ledger_exit_out* exit_out,
                                                   const hz_ledger_create_out* create_out) {
    static_assert(sizeof(hz_ledger_create_out) == HZ_LEDGER_CREATE_ARRAYS * sizeof(uint8_t*), "hz_ledger_create_out is an array of pointers");
    const LedgerCall l2 = ledger_call_l2("hz_ledger_apply_batch_creates", m, txs, sigs, chain_id, current_num_batch, F, fee_plan_tokens, fee_idxs, n_sib, out, sig_out);
    LedgerCall c = ledger_call_batch(ledger_call_addr(l2, flags, aux_to_idx, aux_to_idx_out), n_l1, l1, l1_flags_out);
    c.exits = true, c.exit_out = exit_out;
    c.creates = true, c.from_bjj = from_bjj, c.create_out = create_out;
    return ledger_apply(l, c);
}

extern "C" hz_status hz_ledger_create_outputs_dev(hz_ledger* l, hz_ledger_create_out* dev) {
    return ledger_hand_out("hz_ledger_create_outputs_dev", l, dev, l ? &l->have_create_outputs : nullptr, "hz_ledger_apply_batch_creates",
                           l ? l->create_dev : nullptr, HZ_LEDGER_CREATE_ARRAYS);
}

extern "C" double hz_ledger_create_ms(const hz_ledger* l) { return l ? l->create_ms : 0.0; }

// ---- atomic transactions: the rqOffset links ----------------------------------------------------------------------------
extern "C" hz_status hz_ledger_apply_batch_atomic(hz_ledger* l, size_t n_l1, const hz_l1tx* l1, const uint8_t* from_bjj, size_t m, const hz_l2tx* txs,
                                                  const hz_l2sig* sigs, const hz_l2rq* rq, uint32_t flags, const uint64_t* aux_to_idx, uint32_t chain_id,
                                                  uint32_t current_num_batch, size_t F, const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs, size_t n_sib,
                                                  const hz_ledger_out* out, const hz_ledger_sig_out* sig_out, uint8_t* aux_to_idx_out, uint8_t* l1_flags_out,
                                                  const hz_ledger_exit_out* exit_out, const hz_ledger_create_out* create_out) {
    static_assert(sizeof(hz_l2rq) == 97, "hz_l2rq is three elements and a byte");
    const char* who = "hz_ledger_apply_batch_atomic";
    if (l) l->rq_ms = 0.0;   // the time of THIS call. (sigs == NULL is hz_ledger_apply_batch's: zero entries stand in, so the link fields
                             // of such rows are V2 and two zeros)
    const LedgerCall l2 = ledger_call_l2(who, m, txs, sigs, chain_id, current_num_batch, F, fee_plan_tokens, fee_idxs, n_sib, out, sig_out);
    LedgerCall c = ledger_call_batch(ledger_call_addr(l2, flags, aux_to_idx, aux_to_idx_out), n_l1, l1, l1_flags_out);
    c.exits = true, c.exit_out = exit_out;
    c.creates = true, c.from_bjj = from_bjj, c.create_out = create_out;
    c.rq = rq;
    return ledger_apply(l, c);
}

extern "C" hz_status hz_ledger_verify_l2_atomic(hz_ledger* l, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, const hz_l2rq* rq, uint32_t chain_id,
                                                uint32_t current_num_batch, uint8_t* verdict_out, const hz_ledger_sig_out* sig_out) {
    if (l) l->rq_ms = 0.0;
    return ledger_verify(l, "hz_ledger_verify_l2_atomic", m, txs, sigs, rq, chain_id, current_num_batch, verdict_out, sig_out);
}

extern "C" double hz_ledger_rq_ms(const hz_ledger* l) { return l ? l->rq_ms : 0.0; }

// ---- a batch selected from a pool ----------------------------------------------------------------------------------------
extern "C" double hz_ledger_select_ms(const hz_ledger* l) { return l ? l->select_ms : 0.0; }

// the argument checks of hz_ledger_select_batch, in the order their errors win; -> the rows (the L1 rows as hz_ledger_apply_batch_atomic
// takes them), and where the call has links (rq or partner) the rq entries without their offsets: positions do not survive a drop
static hz_status select_checks(hz_ledger* l, const char* who, size_t n_l1, const hz_l1tx* l1, const uint8_t* from_bjj, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs,
                               const hz_l2rq* rq, const int32_t* partner, uint32_t flags, uint32_t chain_id, const hz_ledger_select_out* out, LedgerRows& r,
                               std::vector<hz_l2rq>& rq_eff) {
    if (hz_status e = ledger_ready(l, who)) return e;
    l->select_ms = 0.0;
    if (!out || (m && !txs)) return set_err(HZ_ERR_ARG, "%s: null argument", who);
    const bool verify = (flags & HZ_LEDGER_VERIFY_SIGS) != 0;
    if (hz_status e = ledger_check_flags(who, flags)) return e;
    if (hz_status e = ledger_effective_l1(ledger_shape(l), who, n_l1, l1, from_bjj, true, true, r)) return e;
    if (hz_status e = select_check_pool(who, m)) return e;
    if (hz_status e = ledger_check_txs(who, m, txs, l->first_idx, r.count, true, true)) return e;
    if (hz_status e = select_check_partner(who, m, txs, partner)) return e;
    if (hz_status e = ledger_stand_in_sigs(who, m, txs, sigs, verify, r)) return e;
    if (hz_status e = ledger_check_sigs(who, m, txs, r.sigs, chain_id, verify)) return e;
    if ((rq != nullptr || partner != nullptr) && m != 0) {
        rq_eff.assign(m, hz_l2rq{});
        for (size_t i = 0; rq && i < m; i++) {
            rq_eff[i] = rq[i];
            rq_eff[i].rq_offset = 0;
        }
        if (hz_status e = ledger_check_rq(who, m, txs, rq_eff.data())) return e;
    }
    return HZ_OK;
}

extern "C" hz_status hz_ledger_select_batch(hz_ledger* l, size_t n_l1, const hz_l1tx* l1, const uint8_t* from_bjj, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs,
                                            const hz_l2rq* rq, const int32_t* partner, uint32_t flags, uint32_t chain_id, uint32_t current_num_batch, size_t max_keep,
                                            const hz_ledger_select_out* out) {
    const char* who = "hz_ledger_select_batch";
    LedgerRows r;
    std::vector<hz_l2rq> rq_eff;
    if (hz_status e = select_checks(l, who, n_l1, l1, from_bjj, m, txs, sigs, rq, partner, flags, chain_id, out, r, rq_eff)) return e;
    const bool verify = (flags & HZ_LEDGER_VERIFY_SIGS) != 0, links = !rq_eff.empty();
    ledger_forget(l);
    HZ_HIP(hipSetDevice(l->device));
    hipStream_t s = ledger_stream(l);
    if (r.n_creates)
        if (hz_status e = ledger_create_launch(l, n_l1, l1, from_bjj, r)) return e;
    if (hz_status e = ledger_effective_receivers(l, who, n_l1, m, txs, nullptr, false, r)) return e;   // to_idx == 0 stays: reason 9
    SelectPlan sp;
    if (hz_status e = select_plan(who, n_l1, r.l1, m, r.eff.data(), l->plan, sp)) return e;
    const uint32_t m32 = (uint32_t)m, L32 = (uint32_t)n_l1, n_slots = (uint32_t)sp.slot_account.size();
    SelectTables T;
    SelectWork W;
    T.layout(n_l1, m, n_slots, partner != nullptr);
    W.layout(n_l1 + m, m);
    const size_t back_bytes = W.end - W.hdr.at;
    HZ_HIP(l->h_ints.grow(T.end));
    T.fill(l->h_ints.p, r.l1, txs, r.eff.data(), sp.slot_s.data(), sp.slot_r.data(), sp.slot_account.data(), partner, l->first_idx);
    HZ_HIP(l->ints.grow(T.end));
    HZ_HIP(l->work.grow(W.end));
    HZ_HIP(l->h_sel.grow(back_bytes));
    void *db = l->ints.p, *wb = l->work.p;
    const hz_l2tx* d_txs = T.tx.dev(db);
    LedgerDrain drain;
    drain.s = s;
    drain.armed = true;
    HZ_HIP(hipMemcpyAsync(l->ints.p, l->h_ints.p, T.end, hipMemcpyHostToDevice, s));
    const uint8_t* d_sig_verdict = nullptr;
    if (verify || links) {
        if (hz_status e = ledger_sig_prepare(l, m, r.sigs, s, verify)) return e;
        const hz_l2sig* d_sigs = (const hz_l2sig*)l->sig_in.p;
        if (links)
            if (hz_status e = ledger_rq_upload(l, m, rq_eff.data(), s)) return e;
        if (!verify) HZ_HIP(hipMemsetAsync(l->verdict_dev, 0, m, s));   // the V2 rows alone, for the link compare (links: m != 0); no verdict yet
        if (hz_status e = ledger_sig_links_launch(l, d_txs, m32, chain_id, current_num_batch, nullptr, l->verdict_dev, 0, verify, links, s, true)) return e;
        if (links) {   // the selection's own link kernel
            hipLaunchKernelGGL(k_ledger_select_rq, dim3((m32 + 63) / 64), dim3(64), 0, s, d_txs, d_sigs, (const uint8_t*)l->rq_in.p, (const uint8_t*)l->sig_dev[1],
                               partner ? T.partner.dev(db) : nullptr, l->verdict_dev, m32);
            HZ_HIP(hipGetLastError());
        }
        if (m) d_sig_verdict = l->verdict_dev;
    }
    const uint32_t cap = (uint32_t)std::min<size_t>(max_keep, HZ_SELECT_MAX_POOL);
    HZ_HIP(l->t_select.begin(s));
    hipLaunchKernelGGL(k_ledger_select, dim3(1), dim3(256), 0, s, T.l1.dev(db), T.sel.dev(db), T.slot_acct.dev(db), partner ? T.partner.dev(db) : nullptr, d_sig_verdict,
                       (const uint8_t*)l->planes.p, W.ops.dev(wb), W.hdr.dev(wb), W.kept.dev(wb), W.verdict.dev(wb), W.off.dev(wb), l->N, L32, m32, n_slots, cap);
    HZ_HIP(hipGetLastError());   // (a workgroup with more LDS than the device grants is refused here, not faulted)
    HZ_HIP(l->t_select.end(s));
    HZ_HIP(hipMemcpyAsync(l->h_sel.p, W.hdr.dev(wb), back_bytes, hipMemcpyDeviceToHost, s));
    HZ_HIP(hipStreamSynchronize(s));
    drain.armed = false;
    HZ_HIP(l->t_select.read(l->select_ms));
    const uint8_t* back = (const uint8_t*)l->h_sel.p;   // the work buffer from the header on
    const uint32_t* hdr = (const uint32_t*)back;
    if (hdr[2] != 0xFFFFFFFFu) return ledger_refused(who, hdr[2], 5, n_l1 + m, n_l1);   // an L1 row
    const size_t n_kept = hdr[0];
    if (out->n_kept) *out->n_kept = n_kept;
    if (out->rounds) *out->rounds = hdr[1];
    if (out->kept && n_kept) memcpy(out->kept, back + (W.kept.at - W.hdr.at), n_kept * 4);
    if (out->verdict && m) memcpy(out->verdict, back + (W.verdict.at - W.hdr.at), m);
    if (out->rq_offset && m) memcpy(out->rq_offset, back + (W.off.at - W.hdr.at), m);
    for (size_t i = 0; out->aux_to_idx && i < m; i++) out->aux_to_idx[i] = ledger_wants_receiver(txs[i]) ? r.eff[i].to_idx : 0;
    return HZ_OK;
}

// ---- RollupMain's packed inputs of the applied batch -----------------------------------------------------------------------
extern "C" double hz_ledger_main_inputs_ms(const hz_ledger* l) { return l ? l->mi_ms : 0.0; }

// the first byte a COPY / BROADCAST descriptor reads: the array the apply left (or the call's own upload, at `up`) from row r0
static const uint8_t* ledger_mi_source(const hz_ledger* l, const MiSignal& d, const uint8_t* up_globals, const uint8_t* up_fee_idxs, const uint8_t* up_tokens) {
    const uint8_t* base = nullptr;
    if (d.source >= HZ_MI_SRC_OUT && d.source < HZ_MI_SRC_OUT + HZ_LEDGER_ARRAYS)
        base = l->out_dev.a[d.source - HZ_MI_SRC_OUT];
    else if (d.source >= HZ_MI_SRC_EXIT && d.source < HZ_MI_SRC_EXIT + HZ_LEDGER_EXIT_ARRAYS)
        base = l->exit_dev[d.source - HZ_MI_SRC_EXIT];
    else if (d.source >= HZ_MI_SRC_CREATE && d.source < HZ_MI_SRC_CREATE + HZ_LEDGER_CREATE_ARRAYS)
        base = l->create_dev[d.source - HZ_MI_SRC_CREATE];
    else if (d.source == HZ_MI_SRC_AUX_TO_IDX)
        base = (const uint8_t*)l->aux_rows.p;
    else if (d.source == HZ_MI_SRC_GLOBALS)
        base = up_globals;
    else if (d.source == HZ_MI_SRC_FEE_IDXS)
        base = up_fee_idxs;
    else if (d.source == HZ_MI_SRC_FEE_PLAN_TOKENS)
        base = up_tokens;
    return base ? base + d.r0 * d.inner * 32 : nullptr;
}

extern "C" hz_status hz_ledger_main_inputs(hz_ledger* l, const hz_ctx* ctx, uint64_t old_last_idx, void* d_packed, size_t bytes) {
    const char* who = "hz_ledger_main_inputs";
    if (!l || !ctx || !d_packed) return set_err(HZ_ERR_ARG, "%s: null argument", who);
    const LedgerMainCall& k = l->main_call;
    if (!k.valid || !l->have_outputs)
        return set_err(HZ_ERR_ARG, "%s: no successful apply call with a chain id (every one but hz_ledger_apply_l2) since the ledger's last other call", who);
    CtxShape cs;
    ctx_shape(ctx, cs);
    if (cs.tmpl != HZ_T_ROLLUP_MAIN) return set_err(HZ_ERR_ARG, "%s: the context is not a rollup-main context", who);
    if (cs.device != l->device) return set_err(HZ_ERR_ARG, "%s: the context lies on device %d, the ledger on device %d", who, cs.device, l->device);
    if (k.n_l1 + k.m != (size_t)cs.n_tx || k.n_l1 > (size_t)cs.max_l1 || k.F != (size_t)cs.max_fee || k.n_sib != (size_t)cs.n_levels + 1)
        return set_err(HZ_ERR_ARG, "%s: the applied batch (n_l1 = %zu, m = %zu, F = %zu, n_sib = %zu) does not fill RollupMain(%d, %d, %d, %d)", who, k.n_l1, k.m, k.F,
                       k.n_sib, cs.n_tx, cs.n_levels, cs.max_l1, cs.max_fee);
    const uint64_t packed = hz_inputs_packed_bytes(ctx);
    if (!packed) return HZ_ERR_HIP;   // (its own message stands)
    if (bytes != packed) return set_err(HZ_ERR_ARG, "%s: bytes = %zu, the packed inputs of the context take %llu", who, bytes, (unsigned long long)packed);
    if ((uintptr_t)d_packed & 31u) return set_err(HZ_ERR_ARG, "%s: d_packed is not 32-byte aligned", who);
    if ((k.flags & HZ_MI_GROWING) && old_last_idx != k.last_before)
        return set_err(HZ_ERR_ARG, "%s: old_last_idx = %llu, the ledger's last idx before the batch was %llu", who, (unsigned long long)old_last_idx,
                       (unsigned long long)k.last_before);
    // the layout through the context's own getters, then the table
    const int32_t n = hz_input_count(ctx);
    std::vector<const char*> names(n);
    std::vector<uint64_t> offsets(n), lens(n);
    std::vector<uint32_t> widths(n);
    for (int32_t i = 0; i < n; i++) {
        names[i] = hz_input_name(ctx, i, &lens[i]);
        offsets[i] = hz_input_packed_offset(ctx, i);
        widths[i] = (uint32_t)hz_input_packed_width(ctx, i);
    }
    MiShape shape;
    shape.n_tx = (uint32_t)cs.n_tx, shape.n_levels = (uint32_t)cs.n_levels, shape.max_l1 = (uint32_t)cs.max_l1, shape.max_fee = (uint32_t)cs.max_fee;
    std::vector<MiSignal> sig;
    const std::string err = mi_plan((size_t)n, names.data(), offsets.data(), widths.data(), lens.data(), packed, shape, k.flags, sig);
    if (!err.empty()) return set_err(HZ_ERR_ARG, "%s: the context's packed layout: %s", who, err.c_str());
    // one upload: the descriptors | old_last_idx, chain id, current_num_batch | fee_idxs | fee_plan_tokens as elements | the keys
    const size_t F = k.F, at_glob = ((size_t)n * sizeof(MainInputsDesc) + 31) & ~(size_t)31, at_idx = at_glob + 96, at_tok = at_idx + F * 32, at_keys = at_tok + F * 32;
    const size_t up = at_keys + k.keys.size();
    HZ_HIP(hipSetDevice(l->device));
    HZ_HIP(l->h_mi.grow(up));
    HZ_HIP(l->mi_in.grow(up));
    uint8_t* h = (uint8_t*)l->h_mi.p;
    const uint8_t* dv = (const uint8_t*)l->mi_in.p;
    memset(h + at_glob, 0, at_keys - at_glob);
    memcpy(h + at_glob, &old_last_idx, 8);
    memcpy(h + at_glob + 32, &k.chain_id, 4);
    memcpy(h + at_glob + 64, &k.current_num_batch, 4);
    for (size_t j = 0; j < F; j++) {
        memcpy(h + at_idx + j * 32, &k.fee_idxs[j], 8);
        memcpy(h + at_tok + j * 32, &k.plan_tokens[j], 4);
    }
    if (!k.keys.empty()) memcpy(h + at_keys, k.keys.data(), k.keys.size());
    MainInputsDesc* hd = (MainInputsDesc*)h;
    uint32_t blocks = 0;
    for (int32_t i = 0; i < n; i++) {
        const MiSignal& d = sig[i];
        MainInputsDesc o{};
        o.dst_off = offsets[i];
        o.src = ledger_mi_source(l, d, dv + at_glob, dv + at_idx, dv + at_tok);
        o.kind = d.kind, o.ebytes = d.width, o.outer = (uint32_t)d.rows, o.inner = d.inner, o.first_block = blocks;
        if ((d.kind == HZ_MI_KIND_COPY || d.kind == HZ_MI_KIND_BROADCAST) && !o.src) return set_err(HZ_ERR_ARG, "%s: signal %s has no source", who, names[i]);
        hd[i] = o;
        blocks += mi_blocks(d);
    }
    hipStream_t s = ledger_stream(l);
    HZ_HIP(hipMemcpyAsync(l->mi_in.p, h, up, hipMemcpyHostToDevice, s));
    {   // what no signal covers: the layout's alignment gaps and its tail
        std::vector<std::pair<uint64_t, uint64_t>> range;
        for (int32_t i = 0; i < n; i++) range.push_back({offsets[i], offsets[i] + lens[i] * widths[i]});
        std::sort(range.begin(), range.end());
        uint64_t at = 0;
        for (size_t q = 0; q <= range.size(); q++) {
            const uint64_t next = q < range.size() ? range[q].first : packed;
            if (next > at) HZ_HIP(hipMemsetAsync((uint8_t*)d_packed + at, 0, next - at, s));
            if (q < range.size()) at = std::max(at, range[q].second);
        }
    }
    const uint8_t* db = (const uint8_t*)l->ints.p;
    HZ_HIP(l->t_mi.begin(s));
    if (blocks) {
        hipLaunchKernelGGL(k_ledger_main_inputs, dim3(blocks), dim3(256), 0, s, (const MainInputsDesc*)dv, (uint32_t)n, (uint8_t*)d_packed, k.tx.dev((void*)db),
                           k.l1.dev((void*)db), (k.flags & HZ_MI_CREATES) ? k.crow.dev((void*)db) : nullptr, (const hz_l2sig*)l->sig_in.p,
                           (k.flags & HZ_MI_RQ) ? (const uint8_t*)l->rq_in.p : nullptr, k.keys.empty() ? nullptr : dv + at_keys, (uint32_t)k.n_l1, (uint32_t)k.m, k.chain_id);
        HZ_HIP(hipGetLastError());
    }
    HZ_HIP(l->t_mi.end(s));
    HZ_HIP(hipStreamSynchronize(s));
    HZ_HIP(l->t_mi.read(l->mi_ms));
    return HZ_OK;
}

// ---- marks, the undo journal, rollback (ledger_journal.h) ------------------------------------------------------------------------
extern "C" hz_status hz_ledger_journal(hz_ledger* l, uint32_t depth) {
    const char* who = "hz_ledger_journal";
    if (!l) return set_err(HZ_ERR_ARG, "%s: null ledger", who);
    if (hz_status e = journal_check_depth(who, depth)) return e;
    HZ_HIP(hipSetDevice(l->device));
    l->journal.reset();   // (no call is in flight: every one ends behind a synchronise)
    l->journal_ms = 0.0;
    if (depth == 0) return HZ_OK;
    std::unique_ptr<LedgerJournal> j(new LedgerJournal);
    j->ring.set_depth(depth);
    j->slab.reset(new DevBuf[j->ring.slots()]);
    j->undo.resize(j->ring.slots());
    j->has_undo.assign(j->ring.slots(), 0);
    for (DevSpan* t : {&j->t_tree, &j->t_planes, &j->t_rollback}) HZ_HIP(t->create());
    l->journal = std::move(j);
    return HZ_OK;
}

extern "C" hz_status hz_ledger_applied(const hz_ledger* l, uint64_t* mark) {
    if (!l || !mark) return set_err(HZ_ERR_ARG, "hz_ledger_applied: null argument");
    *mark = l->applied;
    return HZ_OK;
}

extern "C" hz_status hz_ledger_journal_stats(const hz_ledger* l, uint32_t* depth, size_t* records, uint64_t* oldest_mark, size_t* bytes_used, size_t* bytes_reserved) {
    if (!l) return set_err(HZ_ERR_ARG, "hz_ledger_journal_stats: null ledger");
    const LedgerJournal* j = l->journal.get();
    if (depth) *depth = j ? j->ring.depth : 0u;
    if (records) *records = j ? j->ring.records() : 0;
    if (oldest_mark) *oldest_mark = j ? j->ring.oldest_mark(l->applied) : l->applied;
    if (bytes_used) *bytes_used = j ? j->ring.bytes_used() : 0;
    if (bytes_reserved) *bytes_reserved = j ? j->cap * j->ring.slots() : 0;
    return HZ_OK;
}

extern "C" double hz_ledger_journal_ms(const hz_ledger* l) { return l ? l->journal_ms : 0.0; }
extern "C" double hz_ledger_rollback_ms(const hz_ledger* l) { return l ? l->rollback_ms : 0.0; }

// the exit trees kept after the mark was reached go, from the archive's end. Two steps, as hz_ledger_exit_keep works on `next`: plan -- how
// many snapshots stay, and the table of those uploaded on s, the archive itself untouched --, and once the rollback's synchronise has
// succeeded, commit: the snapshots popped, the counters of their slabs as a keep left them, the emptied slabs freed
static hz_status ledger_archive_cut_plan(const hz_ledger* l, bool has_kept, uint32_t last_kept, std::vector<ArchiveDesc>& host_table, hipStream_t s, size_t* stay) {
    const LedgerArchive* a = l->archive.get();
    *stay = a ? a->snaps.size() : 0;
    if (!a || a->snaps.empty()) return HZ_OK;
    std::vector<uint32_t> kept;
    for (const ArchiveSnap& sn : a->snaps) kept.push_back(sn.batch_num);
    *stay = journal_archive_keep(kept.data(), kept.size(), has_kept, last_kept);
    if (*stay == a->snaps.size()) return HZ_OK;
    const std::vector<ArchiveSnap> next(a->snaps.begin(), a->snaps.begin() + (ptrdiff_t)*stay);
    HZ_HIP(archive_upload_table(next, a->table.p, host_table, s));
    return HZ_OK;
}

static void ledger_archive_cut_commit(hz_ledger* l, size_t stay) {
    LedgerArchive* a = l->archive.get();
    if (!a || stay >= a->snaps.size()) return;
    while (a->snaps.size() > stay) {
        const ArchiveSnap& sn = a->snaps.back();   // the last snapshot of its slab: its bytes are the slab's last
        if (sn.slab) {
            sn.slab->live--;
            sn.slab->used -= sn.bytes;
        }
        a->snaps.pop_back();
    }
    archive_free_empty_slabs(a);
}

extern "C" hz_status hz_ledger_rollback(hz_ledger* l, uint64_t mark) {
    const char* who = "hz_ledger_rollback";
    if (hz_status e = ledger_ready(l, who)) return e;
    LedgerJournal* J = l->journal.get();
    if (hz_status e = journal_check_mark(who, l->applied, J ? J->ring.depth : 0u, J ? J->ring.records() : 0, mark)) return e;
    if (mark == l->applied) return HZ_OK;   // nothing changes, nothing is invalidated
    HZ_HIP(hipSetDevice(l->device));
    hipStream_t s = ledger_stream(l);
    const size_t n = J->ring.undone_by(mark);   // == applied - mark: the verdict says the ring reaches that far
    std::vector<ArchiveDesc> host_table;
    bool queued = false;
    size_t stay = 0;
    const hz_status st = [&]() -> hz_status {
        HZ_HIP(J->t_rollback.begin(s));
        for (size_t i = 0; i < n; i++) {   // newest first: where two batches touched an element the oldest saved value is written last
            const JournalRecord r = J->ring.rec.back();
            const JournalLayout lay = journal_layout(r.tree_entries, r.groups);
            const uint8_t* base = (const uint8_t*)J->slab[r.slot].p;
            if (r.groups) {
                const uint32_t G = (uint32_t)r.groups;
                queued = true;
                hipLaunchKernelGGL(k_ledger_journal_restore, dim3((4 * G + 255) / 256), dim3(256), 0, s, (const uint32_t*)(base + lay.planes.index), base + lay.planes.values,
                                   (uint8_t*)l->planes.p, l->N, G, (uint32_t)r.live);
                HZ_HIP(hipGetLastError());
            }
            if (l->smt && J->has_undo[r.slot]) {
                queued = true;
                if (hz_status e = smt_journal_restore(l->smt, base + lay.tree.values, (const uint32_t*)(base + lay.tree.index), r.tree_entries, J->undo[r.slot])) return e;
            } else if (l->tree && r.tree_entries) {
                queued = true;
                if (hz_status e = state_journal_restore(l->tree, base + lay.tree.values, (const uint32_t*)(base + lay.tree.index), r.tree_entries)) return e;
            }
            l->live = r.live;
            if (i + 1 == n)
                if (hz_status e = ledger_archive_cut_plan(l, r.has_kept, r.last_kept, host_table, s, &stay)) return e;
            J->ring.pop_newest();
        }
        HZ_HIP(J->t_rollback.end(s));
        HZ_HIP(hipStreamSynchronize(s));   // the one synchronise
        HZ_HIP(J->t_rollback.read(l->rollback_ms));
        return HZ_OK;
    }();
    if (st) {
        (void)hipStreamSynchronize(s);
        l->rollback_failed = queued;
        return st;
    }
    ledger_archive_cut_commit(l, stay);
    ledger_exit_reset(l);   // the batch's exit tree is empty, as after a load
    ledger_forget(l);
    l->applied = mark;
    return HZ_OK;
}

// ---- the hz_ledger_plan_* exports: the host half of a call alone, no ledger -- a shape check, the checks of ledger_checks.h, the planner, ------
// ---- the copies out ---------------------------------------------------------------------------------------------------------------------
// a planner's vector (its first n entries) to an output array the caller may have left out
template <class T, class V>
static void plan_out(T* out, const V& v, size_t n) {
    for (size_t i = 0; out && i < n; i++) out[i] = (T)v[i];
}
static void plan_out(size_t* out, size_t count) {
    if (out) *out = count;
}

extern "C" hz_status hz_ledger_plan_l2(size_t m, const hz_l2tx* txs, size_t F, const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs, int32_t k,
                                       uint64_t first_idx, int32_t* ev_sender_out, int32_t* ev_receiver_out, int32_t* fee_slot_out, int32_t* last_event_out,
                                       size_t* n_events_out, uint64_t* ev_account_out, int32_t* ev_prev_out) {
    const char* who = "hz_ledger_plan_l2";
    LedgerPlan p;
    if (hz_status e = ledger_check_k(who, k)) return e;
    if (hz_status e = ledger_check_plan(who, m, txs, F, fee_plan_tokens, fee_idxs, 1ull << k, first_idx, p)) return e;
    plan_out(ev_sender_out, p.ev_sender, m), plan_out(ev_receiver_out, p.ev_receiver, m), plan_out(fee_slot_out, p.fee_slot, m), plan_out(last_event_out, p.last_event, m);
    plan_out(n_events_out, p.account.size()), plan_out(ev_account_out, p.account, p.account.size()), plan_out(ev_prev_out, p.prev_same, p.account.size());
    return HZ_OK;
}

extern "C" hz_status hz_ledger_plan_batch(size_t n_l1, const hz_l1tx* l1, size_t m, const hz_l2tx* txs, size_t F, const uint32_t* fee_plan_tokens,
                                          const uint64_t* fee_idxs, int32_t k, uint64_t first_idx, int32_t* ev_sender_out, int32_t* ev_receiver_out,
                                          int32_t* fee_slot_out, int32_t* last_event_out, size_t* n_events_out, uint64_t* ev_account_out, int32_t* ev_prev_out,
                                          int32_t* l1_slot_sender_out, int32_t* l1_slot_receiver_out, size_t* n_slots_out, uint64_t* slot_account_out) {
    LedgerPlan p;
    if (hz_status e = ledger_check_plan_rows("hz_ledger_plan_batch", k, first_idx, false, 0, n_l1, l1, m, txs, F, fee_plan_tokens, fee_idxs, p)) return e;
    ledger_plan_batch(n_l1, l1, m, txs, F, fee_plan_tokens, fee_idxs, p);
    const size_t R = n_l1 + m, M = p.account.size();
    plan_out(ev_sender_out, p.ev_sender, R), plan_out(ev_receiver_out, p.ev_receiver, R), plan_out(fee_slot_out, p.fee_slot, R), plan_out(last_event_out, p.last_event, R);
    plan_out(n_events_out, M), plan_out(ev_account_out, p.account, M), plan_out(ev_prev_out, p.prev_same, M);
    plan_out(l1_slot_sender_out, p.l1_slot_sender, n_l1), plan_out(l1_slot_receiver_out, p.l1_slot_receiver, n_l1);
    plan_out(n_slots_out, p.slot_account.size()), plan_out(slot_account_out, p.slot_account, p.slot_account.size());
    return HZ_OK;
}

extern "C" hz_status hz_ledger_plan_exits(size_t n_l1, const hz_l1tx* l1, size_t m, const hz_l2tx* txs, size_t F, const uint32_t* fee_plan_tokens,
                                          const uint64_t* fee_idxs, int32_t k, uint64_t first_idx, size_t n_sib, int32_t* ev_sender_out, int32_t* ev_receiver_out,
                                          int32_t* last_event_out, size_t* n_events_out, uint64_t* ev_account_out, int32_t* ev_exit_out, int32_t* last_exit_out,
                                          size_t* n_exits_out, uint32_t* exit_row_out, uint64_t* exit_key_out, int32_t* exit_prev_out, uint32_t* exit_perm_out,
                                          uint8_t* exit_insert_out, uint8_t* exit_is_old0_out, uint64_t* exit_old_key_out) {
    const char* who = "hz_ledger_plan_exits";
    LedgerPlan p;
    if (hz_status e = ledger_check_plan_rows(who, k, first_idx, true, n_sib, n_l1, l1, m, txs, F, fee_plan_tokens, fee_idxs, p)) return e;
    ledger_plan_exits(n_l1, l1, m, txs, F, fee_plan_tokens, fee_idxs, p);
    const size_t R = n_l1 + m, X = p.exit_row.size();
    SmtShape sh;   // the exit tree of a batch starts empty
    sh.begin();
    for (size_t x = 0; x < X; x++)
        if (sh.add(p.exit_key[x], (uint32_t)n_sib) != SMT_PLAN_OK)
            return set_err(HZ_ERR_ARG, "%s: op %zu (key %llu) would have its leaf at depth >= n_sib = %zu: SMTProcessor(%zu) cannot express it", who, x,
                           (unsigned long long)p.exit_key[x], n_sib, n_sib);
    plan_out(ev_sender_out, p.ev_sender, R), plan_out(ev_receiver_out, p.ev_receiver, R), plan_out(last_event_out, p.last_event, R);
    plan_out(ev_exit_out, p.ev_exit, R), plan_out(last_exit_out, p.last_exit, R);
    plan_out(n_events_out, p.account.size()), plan_out(ev_account_out, p.account, p.account.size());
    plan_out(n_exits_out, X), plan_out(exit_row_out, p.exit_row, X), plan_out(exit_key_out, p.exit_key, X), plan_out(exit_prev_out, p.exit_prev, X);
    plan_out(exit_perm_out, p.exit_perm, X), plan_out(exit_insert_out, sh.fnc, X), plan_out(exit_is_old0_out, sh.is_old0, X), plan_out(exit_old_key_out, sh.old_key, X);
    return HZ_OK;
}

extern "C" hz_status hz_ledger_plan_creates(size_t n_l1, const hz_l1tx* l1, const uint8_t* from_bjj, size_t m, const hz_l2tx* txs, size_t F,
                                            const uint32_t* fee_plan_tokens, const uint64_t* fee_idxs, int32_t growing, uint64_t capacity, uint64_t first_idx,
                                            uint64_t size, uint64_t* aux_from_idx_out, uint64_t* out_idx_after_out, size_t* n_creates_out) {
    LedgerRows r;
    if (hz_status e = ledger_check_plan_creates("hz_ledger_plan_creates", LedgerShape{growing != 0, capacity, first_idx, size, 0}, n_l1, l1, from_bjj, m, txs, F, fee_plan_tokens,
                                                fee_idxs, r))
        return e;
    r.aux_from.resize(n_l1 + m, 0);   // an L2 row creates nothing and leaves the last idx where the L1 run left it
    r.idx_after.resize(n_l1 + m, first_idx + r.count - 1);
    plan_out(aux_from_idx_out, r.aux_from, n_l1 + m), plan_out(out_idx_after_out, r.idx_after, n_l1 + m), plan_out(n_creates_out, r.n_creates);
    return HZ_OK;
}

extern "C" hz_status hz_ledger_plan_atomic(size_t n_l1, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, const hz_l2rq* rq, int64_t* target_row_out,
                                           uint8_t* verdict_out) {
    if (hz_status e = ledger_check_plan_atomic("hz_ledger_plan_atomic", n_l1, m, txs, sigs, rq)) return e;
    for (size_t i = 0; i < m; i++) {
        int64_t row = -1;
        bool ok = true;
        if (rq && txs[i].from_idx != 0) {
            row = rq_target_row(n_l1 + i, rq[i].rq_offset, n_l1, n_l1 + m);
            if (row >= 0 && txs[row - n_l1].from_idx == 0) row = -1;   // a NOP: zeros
            Fc v2 = fc_zero(), eth = fc_zero(), ay = fc_zero();
            if (row >= 0) ledger_sig_link_fields_host(txs[row - n_l1], sigs[row - n_l1], &v2, &eth, &ay);
            ok = rq_fields_match(resolve_load32(rq[i].rq_tx_compressed_data_v2), resolve_load32(rq[i].rq_to_eth_addr), resolve_load32(rq[i].rq_to_bjj_ay), v2, eth, ay);
        }
        if (target_row_out) target_row_out[i] = row;
        if (verdict_out) verdict_out[i] = ok ? 0u : (uint8_t)HZ_RQ_REASON;
    }
    return HZ_OK;
}

extern "C" hz_status hz_ledger_plan_select(size_t n_l1, const hz_l1tx* l1, size_t m, const hz_l2tx* txs, const uint64_t* aux_to_idx, const int32_t* partner,
                                           const uint8_t* kept_in, int32_t* slot_sender_out, int32_t* slot_receiver_out, size_t* n_slots_out,
                                           uint64_t* slot_account_out, uint8_t* forced_out, uint8_t* rq_offset_out) {
    const char* who = "hz_ledger_plan_select";
    if (hz_status e = select_check_plan(who, n_l1, l1, m, txs, partner)) return e;
    std::vector<hz_l2tx> eff(txs, txs + m);
    for (size_t i = 0; i < m; i++)
        if (aux_to_idx && ledger_wants_receiver(eff[i])) eff[i].to_idx = aux_to_idx[i];
    LedgerPlan p;
    SelectPlan sp;
    if (hz_status e = select_plan(who, n_l1, l1, m, eff.data(), p, sp)) return e;
    plan_out(slot_sender_out, sp.slot_s, n_l1 + m), plan_out(slot_receiver_out, sp.slot_r, n_l1 + m);
    plan_out(n_slots_out, sp.slot_account.size()), plan_out(slot_account_out, sp.slot_account, sp.slot_account.size());
    if (kept_in) {   // the closure step alone, on the rows the kept transactions would have
        std::vector<uint32_t> row(m, HZ_SELECT_NO_ROW);
        uint32_t n_kept = 0;
        for (size_t i = 0; i < m; i++)
            if (kept_in[i] && txs[i].from_idx != 0) row[i] = n_kept++;
        for (size_t i = 0; i < m; i++) {
            uint32_t off = 0;
            bool forced = false;
            const int32_t q = partner && txs[i].from_idx != 0 ? partner[i] : -1;
            if (q >= 0 && row[i] != HZ_SELECT_NO_ROW) {
                off = select_link(row[q] != HZ_SELECT_NO_ROW, row[i], row[q]);
                forced = off == 0;
            }
            if (forced_out) forced_out[i] = forced;
            if (rq_offset_out) rq_offset_out[i] = (uint8_t)off;
        }
    }
    return HZ_OK;
}

extern "C" hz_status hz_ledger_plan_main_inputs(size_t n_signals, const char* const* names, const uint64_t* offsets, const uint32_t* widths, const uint64_t* flat_lens,
                                                uint64_t bytes, uint32_t n_tx, uint32_t n_levels, uint32_t max_l1_tx, uint32_t max_fee_tx, uint32_t flags,
                                                uint32_t* kind_out, uint32_t* source_out, uint64_t* first_row_out, uint64_t* rows_out) {
    const char* who = "hz_ledger_plan_main_inputs";
    if (!names || !offsets || !widths || !flat_lens) return set_err(HZ_ERR_ARG, "%s: null argument", who);
    MiShape shape;
    shape.n_tx = n_tx, shape.n_levels = n_levels, shape.max_l1 = max_l1_tx, shape.max_fee = max_fee_tx;
    std::vector<MiSignal> sig;
    const std::string err = mi_plan(n_signals, names, offsets, widths, flat_lens, bytes, shape, flags, sig);
    if (!err.empty()) return set_err(HZ_ERR_ARG, "%s: %s", who, err.c_str());
    for (size_t i = 0; i < n_signals; i++) {
        if (kind_out) kind_out[i] = sig[i].kind;
        if (source_out) source_out[i] = sig[i].source;
        if (first_row_out) first_row_out[i] = sig[i].r0;
        if (rows_out) rows_out[i] = sig[i].rows;
    }
    return HZ_OK;
}
