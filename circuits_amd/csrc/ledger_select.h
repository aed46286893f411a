// hz_ledger_select_batch: a batch chosen from a POOL of candidate L2 transactions. The pool is walked in order over the
// balances and nonces the L1 run left; a transaction the circuit would reject is DROPPED with a reason instead of refusing the call, and
// what is kept is exactly what a later hz_ledger_apply_batch_atomic accepts. Whether transaction i is kept decides what its receiver
// holds, and that whether a later transaction of that receiver is kept: the chain across accounts of ledger_l1.h, walked the same way --
// in LDS, in one workgroup, a parallel phase on each side:
//   1 parallel   a lane per local slot: the resident balance into LDS. A lane per L1 row: l1_static. A lane per pool transaction: amount,
//                fee, debit = amount + fee; the static verdict (the sender's token 1, the receiver's token 4, the verdict bytes of the
//                signature and link kernels 7 / 8 / 13, an unresolved destination 9, a fee of 2^128 or more 16); want = tx.nonce - resident nonce as a small
//                integer. The operands of every row go to a per-call buffer, 14 words a row
//   2 serial     rows are staged 64 at a time into an LDS tile by the first wavefront; one lane walks the tile: l1_step on an L1 row,
//                select_step / select_credit on a pool row, with the forced-out mask and the max_keep cap. LDS and registers only
//   3 parallel   a lane per linked transaction: the closure test select_link on the compacted rows. Anything forced out: the balances
//                are loaded again and phase 2 repeats with the forced set added, inside the same launch; else the verdict bytes, the
//                kept list and the offsets are written
// The nonce check needs no nonce in LDS: a slot keeps the number of transactions kept from it so far (16 bits), and a transaction is
// next in line when that number equals its want. Reason 12 falls out of the same two integers: when want equals the count, the
// sender's current nonce is the transaction's, and whether that is 2^40 - 1 is a bit of the want word.
// LDS (SelectLds below), limb-major: balances [7][4096] u32 (a balance stays below 2^193 + 2^138 in the L1 run and below 2^192 after
// it; a debit is below 2^204) = 114688 B, counts [4096] u16 = 8192 B, verdict and forced bytes and the compacted row of every pool
// transaction [4096] (1 + 1 + 2) = 16384 B, the staging tile [14][64] u32 = 3584 B, four words: 142864 B of the 163840 a gfx950
// workgroup may have.
// The per-transaction routines are HZ_HD: the kernel, hz_ledger_plan_select and tests/native/ledger_select_check.cpp share them.
#pragma once
#include <stdint.h>
#include "../../include/hermez_witness.h"
#include "ledger_fee.h"
#include "ledger_l1.h"
#include "u256.h"
#if defined(__HIPCC__)
#include "ledger_resolve.h"
#include "ledger_rq.h"
#endif

namespace hz {

#define HZ_SELECT_NO_ROW 0xFFFFu
#define HZ_SELECT_OP_WORDS 14u
enum : uint32_t { SELECT_WANT_NONE = 0x10000u, SELECT_NONCE_MAX = 0x20000u };   // the want word: 0 .. 65535, or NONE; bit 17: tx.nonce is 2^40 - 1
enum : uint32_t { SELECT_ACTIVE = 1u, SELECT_EXIT = 2u, SELECT_UNRESOLVED = 4u, SELECT_RECEIVER = 8u };   // SelectTxDev.flags

// one pool transaction as the kernel reads it: the planner's integers beside the transaction's own
struct SelectTxDev {
    uint64_t amount_f, nonce;
    uint32_t acct_s, acct_r;   // account - first_idx; acct_r is read only with SELECT_RECEIVER
    uint32_t token_id;
    uint16_t slot_s, slot_r;   // local slots; slot_r == HZ_L1_NO_SLOT: no receiver (a zero amount, an exit, an unresolved destination)
    uint8_t user_fee, flags;
};

// tx.nonce - resident nonce where that lies in 0 .. 65535 and tx.nonce is a leaf's (below 2^40), else NONE; SELECT_NONCE_MAX beside it
HZ_HD uint32_t select_want(uint64_t tx_nonce, uint64_t resident) {
    const uint64_t d = tx_nonce - resident;
    uint32_t w = tx_nonce >= resident && d <= 0xFFFFull && !(tx_nonce >> 40) ? (uint32_t)d : SELECT_WANT_NONE;
    if (tx_nonce == (1ull << 40) - 1) w |= SELECT_NONCE_MAX;
    return w;
}

// one step on the sender: its balance, the number of transactions kept from it so far, the debit, the want word -> 0, or the lowest of
// 2, 3 and 12 that holds. Nothing is changed: the caller debits, and judges the receiver (select_credit) before it does
HZ_HD uint32_t select_step(const Fc& bal, uint32_t kept, const Fc& debit, uint32_t want) {
    if ((want & 0x1FFFFu) != kept) return 2u;
    if (u256_less(bal, debit)) return 3u;
    if (want & SELECT_NONCE_MAX) return 12u;
    return 0u;
}

// the receiver's balance += amount; false: the new balance reaches 2^192 (reason 5), and `to` is left as it was
HZ_HD bool select_credit(Fc& to, const Fc& amount) {
    const Fc sum = u256_add(to, amount);
    if ((sum.v[6] | sum.v[7]) != 0u) return false;
    to = sum;
    return true;
}

// the lower of two verdicts of which 0 means none
HZ_HD uint32_t select_lower(uint32_t a, uint32_t b) { return a == 0u ? b : b == 0u ? a : a < b ? a : b; }

// the static verdict: 9 where it holds, else the lowest of 1, 4, the verdict byte of the signature and link kernels (0, 7, 8 or 13) and
// 16 for a fee of 2^128 or more (fee_over: ledger_fee_overflows, amount and selector alone; a caller that knows no fee leaves it out)
HZ_HD uint32_t select_static(uint32_t flags, uint32_t token_id, uint32_t tok_s, uint32_t tok_r, uint32_t sig_verdict, bool fee_over = false) {
    if (flags & SELECT_UNRESOLVED) return 9u;
    if (token_id != tok_s) return 1u;
    const uint32_t v = select_lower((flags & SELECT_RECEIVER) && token_id != tok_r ? 4u : 0u, sig_verdict);
    return select_lower(v, fee_over ? (uint32_t)HZ_LEDGER_FEE_OVERFLOW : 0u);
}

// the rqOffset that names a row d rows away, 0: none does
HZ_HD uint32_t select_offset(int64_t d) {
    if (d >= 1 && d <= 3) return (uint32_t)d;
    if (d >= -4 && d <= -1) return (uint32_t)(8 + d);
    return 0u;
}

// the closure test of a kept transaction on compacted row `row` whose partner, if kept, is on row `partner_row`: the offset it
// carries, or 0: it is forced out
HZ_HD uint32_t select_link(bool partner_kept, uint32_t row, uint32_t partner_row) {
    return partner_kept ? select_offset((int64_t)partner_row - (int64_t)row) : 0u;
}

#if defined(__HIPCC__)
struct SelectLds {
    uint32_t bal[7][HZ_SELECT_MAX_SLOTS];
    uint16_t cnt[HZ_SELECT_MAX_SLOTS];    // transactions kept from the slot in this walk
    uint16_t row[HZ_SELECT_MAX_POOL];     // the compacted row of a kept transaction, HZ_SELECT_NO_ROW otherwise
    uint8_t verdict[HZ_SELECT_MAX_POOL];
    uint8_t forced[HZ_SELECT_MAX_POOL];
    uint32_t tile[HZ_SELECT_OP_WORDS][64];
    uint32_t n_kept, changed, l1_fail, pad;
};
static_assert(sizeof(SelectLds) == 142864 && sizeof(SelectLds) <= 163840, "k_ledger_select's LDS");

__device__ __forceinline__ Fc select_lds_bal(const SelectLds& lds, uint32_t s) {
    Fc b;
#pragma unroll
    for (int q = 0; q < 7; q++) b.v[q] = lds.bal[q][s];
    b.v[7] = 0u;
    return b;
}

__device__ __forceinline__ void select_lds_put(SelectLds& lds, uint32_t s, const Fc& b) {
#pragma unroll
    for (int q = 0; q < 7; q++) lds.bal[q][s] = b.v[q];
}

// a lane per pool transaction, behind the signature kernels: the rq fields against the link fields of the transaction partner[i] names
// (k_ledger_rq's comparison with the partner in the offset's place); partner == NULL or an entry < 0: against zeros. 13 goes where the
// verdict is still 0: 7 and 8 stay
__global__ __launch_bounds__(64) void k_ledger_select_rq(const hz_l2tx* __restrict__ txs, const hz_l2sig* __restrict__ sigs, const uint8_t* __restrict__ rq,
                                                         const uint8_t* __restrict__ v2, const int32_t* __restrict__ partner, uint8_t* __restrict__ verdict,
                                                         uint32_t m) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    if (txs[i].from_idx == 0) return;
    const int32_t j = partner ? partner[i] : -1;
    Fc t_v2 = fc_zero(), t_eth = fc_zero(), t_ay = fc_zero();
    if (j >= 0 && (uint32_t)j < m && txs[j].from_idx != 0) {
        t_v2 = load_fr(v2 + (size_t)j * 32);
        t_eth = resolve_load32(sigs[j].to_eth_addr);
        t_ay = resolve_load32(sigs[j].to_bjj_ay);
    }
    const bool ok = rq_fields_match(load_fr(rq + (size_t)i * 32), load_fr(rq + ((size_t)m + i) * 32), load_fr(rq + ((size_t)2 * m + i) * 32), t_v2, t_eth, t_ay);
    if (!ok && verdict[i] == 0u) verdict[i] = (uint8_t)HZ_RQ_REASON;
}

// one workgroup; n_l1 <= HZ_L1_MAX_TX, m <= HZ_SELECT_MAX_POOL, n_slots <= HZ_SELECT_MAX_SLOTS (the host checks all three). ops:
// [n_l1 + m][14] words of this call. hdr: the kept count, the number of walks, the lowest L1 row that refuses the batch (~0: none)
__global__ __launch_bounds__(256) void k_ledger_select(const LedgerL1Dev* __restrict__ l1, const SelectTxDev* __restrict__ tx, const uint32_t* __restrict__ slot_acct,
                                                       const int32_t* __restrict__ partner, const uint8_t* __restrict__ sig_verdict,
                                                       const uint8_t* __restrict__ planes, uint32_t* __restrict__ ops, uint32_t* __restrict__ hdr,
                                                       uint32_t* __restrict__ kept_out, uint8_t* __restrict__ verdict_out, uint8_t* __restrict__ rq_offset_out, uint32_t N,
                                                       uint32_t n_l1, uint32_t m, uint32_t n_slots, uint32_t max_keep) {
    __shared__ SelectLds lds;
    const uint32_t R = n_l1 + m;
    // ---- 1: the operands of every row
    for (uint32_t i = threadIdx.x; i < n_l1; i += blockDim.x) {
        const LedgerL1Dev t = l1[i];
        const Fc e0_s = load_fr(planes + (size_t)t.acct_s * 32);
        const Fc eth_s = load_fr(planes + ((size_t)3 * N + t.acct_s) * 32);
        uint32_t tok_r = 0u;
        if (t.slot_r != HZ_L1_NO_SLOT) tok_r = load_fr(planes + (size_t)t.acct_r * 32).v[0];
        if (t.pos_x >= 0) tok_r = e0_s.v[0];   // the exit leaf holds the sender's token
        const L1Static st = l1_static(t.amount_f, t.load_amount_f, t.token_id, t.from_eth, e0_s.v[0], eth_s, tok_r);
        uint32_t* op = ops + (size_t)i * HZ_SELECT_OP_WORDS;
#pragma unroll
        for (int q = 0; q < 5; q++) {
            op[q] = st.eff_load.v[q];
            op[5 + q] = st.eff2.v[q];
        }
        op[10] = op[11] = op[12] = 0u;
        op[13] = (uint32_t)t.slot_s | (uint32_t)t.slot_r << 16;
    }
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
        const SelectTxDev t = tx[i];
        uint32_t* op = ops + (size_t)(n_l1 + i) * HZ_SELECT_OP_WORDS;
        Fc amount = fc_zero(), debit = fc_zero();
        uint32_t word = 0u;
        if (t.flags & SELECT_ACTIVE) {
            const Fc e0_s = load_fr(planes + (size_t)t.acct_s * 32);
            uint32_t tok_r = 0u;
            if (t.flags & SELECT_RECEIVER) tok_r = load_fr(planes + (size_t)t.acct_r * 32).v[0];
            const uint64_t resident = (uint64_t)e0_s.v[1] | ((uint64_t)(e0_s.v[2] & 0xFFu) << 32);
            amount = l1_float40(t.amount_f);
            const Fc fee = ledger_fee(amount, t.user_fee);
            const uint32_t st = select_static(t.flags, t.token_id, e0_s.v[0], tok_r, sig_verdict ? sig_verdict[i] : 0u, ledger_fee_overflows(fee));
            debit = u256_add(amount, fee);
            word = select_want(t.nonce, resident) << 8 | st;
        }
        lds.forced[i] = 0u;
#pragma unroll
        for (int q = 0; q < 7; q++) op[q] = debit.v[q];
#pragma unroll
        for (int q = 0; q < 5; q++) op[7 + q] = amount.v[q];
        op[12] = word | (t.flags & SELECT_ACTIVE ? 1u << 31 : 0u);
        op[13] = (uint32_t)t.slot_s | (uint32_t)t.slot_r << 16;
    }
    uint32_t rounds = 0;
    for (;;) {
        // the balances the batch starts from; nothing kept yet
        for (uint32_t s = threadIdx.x; s < n_slots; s += blockDim.x) {
            const Fc b = load_fr(planes + ((size_t)N + slot_acct[s]) * 32);
            select_lds_put(lds, s, b);
            lds.cnt[s] = 0u;
        }
        if (threadIdx.x == 0) {
            lds.n_kept = 0u;
            lds.changed = 0u;
            lds.l1_fail = 0xFFFFFFFFu;
        }
        rounds++;
        __syncthreads();   // (the first time round: phase 1's rows are in `ops`)
        // ---- 2: the walk, a tile of 64 rows at a time
        for (uint32_t base = 0; base < R; base += 64u) {
            if (threadIdx.x < 64u && base + threadIdx.x < R) {
                const uint32_t* op = ops + (size_t)(base + threadIdx.x) * HZ_SELECT_OP_WORDS;
#pragma unroll
                for (uint32_t q = 0; q < HZ_SELECT_OP_WORDS; q++) lds.tile[q][threadIdx.x] = op[q];
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                const uint32_t end = min(64u, R - base);
                uint32_t n_kept = lds.n_kept;
#pragma unroll 1
                for (uint32_t j = 0; j < end; j++) {
                    const uint32_t row = base + j;
                    const uint32_t s = lds.tile[13][j] & 0xFFFFu, r = lds.tile[13][j] >> 16;
                    Fc bal = select_lds_bal(lds, s);
                    if (row < n_l1) {
                        Fc eff_load = fc_zero(), amt = fc_zero();
#pragma unroll
                        for (int q = 0; q < 5; q++) {
                            eff_load.v[q] = lds.tile[q][j];
                            amt.v[q] = lds.tile[5 + q][j];
                        }
                        (void)l1_step(bal, eff_load, amt);
                        select_lds_put(lds, s, bal);
                        bool over = bal.v[6] != 0u;
                        if (r != HZ_L1_NO_SLOT) {   // after the sender's store: r == s reads the new balance
                            const Fc to = u256_add(select_lds_bal(lds, r), amt);
                            select_lds_put(lds, r, to);
                            over = over || to.v[6] != 0u;
                        }
                        if (over && lds.l1_fail == 0xFFFFFFFFu) lds.l1_fail = row;   // reason 5 through a load or a transfer: apply refuses here
                        continue;
                    }
                    const uint32_t i = row - n_l1, word = lds.tile[12][j];
                    lds.row[i] = (uint16_t)HZ_SELECT_NO_ROW;
                    if (!(word >> 31)) {   // a NOP: 0, not kept, not counted
                        lds.verdict[i] = 0u;
                        continue;
                    }
                    if (lds.forced[i]) {
                        lds.verdict[i] = (uint8_t)HZ_SELECT_PARTNER;
                        continue;
                    }
                    const uint32_t st = word & 0xFFu;
                    if (st == 9u || st == 1u) {   // nothing is lower
                        lds.verdict[i] = (uint8_t)st;
                        continue;
                    }
                    Fc debit, amount = fc_zero();
#pragma unroll
                    for (int q = 0; q < 7; q++) debit.v[q] = lds.tile[q][j];
                    debit.v[7] = 0u;
#pragma unroll
                    for (int q = 0; q < 5; q++) amount.v[q] = lds.tile[7 + q][j];
                    const uint32_t cnt = lds.cnt[s];
                    uint32_t v = select_step(bal, cnt, debit, (word >> 8) & 0x3FFFFu);
                    Fc to = fc_zero();
                    if (v == 0u || v == 12u) {   // 5 is lower than 12: the receiver is judged on the balance it would see
                        bal = u256_add(bal, u256_neg(debit));
                        if (r != HZ_L1_NO_SLOT) {
                            to = r == s ? bal : select_lds_bal(lds, r);
                            if (!select_credit(to, amount)) v = 5u;
                        }
                    }
                    v = select_lower(st, v);
                    if (v == 0u && n_kept >= max_keep) v = HZ_SELECT_FULL;
                    lds.verdict[i] = (uint8_t)v;
                    if (v != 0u) continue;
                    select_lds_put(lds, s, bal);
                    if (r != HZ_L1_NO_SLOT) select_lds_put(lds, r, to);   // r == s: `to` is the sender's new balance plus the amount
                    lds.cnt[s] = (uint16_t)(cnt + 1u);
                    lds.row[i] = (uint16_t)n_kept++;
                }
                lds.n_kept = n_kept;
            }
            __syncthreads();
        }
        // ---- 3: the closure over links
        if (partner) {
            for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
                const int32_t p = partner[i];
                if (p < 0 || lds.row[i] == HZ_SELECT_NO_ROW) continue;
                if (select_link(lds.row[p] != HZ_SELECT_NO_ROW, lds.row[i], lds.row[p]) == 0u) {
                    lds.forced[i] = 1u;
                    lds.changed = 1u;
                }
            }
        }
        __syncthreads();
        if (!lds.changed || lds.l1_fail != 0xFFFFFFFFu) break;
        __syncthreads();   // every lane has read `changed` before lane 0 clears it
    }
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
        const uint32_t row = lds.row[i];
        verdict_out[i] = lds.verdict[i];
        uint32_t off = 0u;
        if (row != HZ_SELECT_NO_ROW) {
            kept_out[row] = i;
            const int32_t p = partner ? partner[i] : -1;
            if (p >= 0) off = select_link(true, row, lds.row[p]);
        }
        rq_offset_out[i] = (uint8_t)off;
    }
    if (threadIdx.x == 0) {
        hdr[0] = lds.n_kept;
        hdr[1] = rounds;
        hdr[2] = lds.l1_fail;
    }
}
#endif

}  // namespace hz
