// hz_ledger's L1 run: deposits, depositTransfers and forceTransfers between existing accounts, NULLIFIED as the circuit
// does it (src/rollup-tx-states.circom:244-313, src/balance-updater.circom:56-100) instead of refused. The token and address nullifiers
// depend on leaf fields no batch changes; the underflow nullifier does not: effectiveAmount3 = underflowOk * effectiveAmount2, so what
// a receiver gets depends on its sender's balance at that moment, and that on whether earlier transfers into the sender were themselves
// nullified -- a dependency ACROSS accounts, which k_ledger_scan's lane per account over precomputed deltas cannot express.
// k_ledger_l1 resolves it before that scan runs, in one workgroup and three phases:
//   1 parallel   a lane per transaction: both float40s, the sender's token and ethAddr and the receiver's token from the resident
//                planes, the static nullifiers, eff_load and eff2 into LDS; a lane per local slot: the resident balance into LDS
//   2 serial     one lane walks the transactions in order over the LDS balances: underflow_ok, eff3, the two balance updates. Worst
//                case the dependence IS a chain (every transfer funded by the one before), so the phase is serial by nature; each
//                step touches LDS only, never HBM
//   3 parallel   a lane per transaction: the signed deltas eff_load - eff3 and + eff3 at the events' grouped positions of the delta
//                buffer k_ledger_scan reads, and the flag byte (bit 0 nullifyLoadAmount, bit 1 isAmountNullified)
// k_ledger_scan then treats the L1 events like any other: it carries the balance through the deltas (no token or nonce check; reason 5
// stays), so an L2 transaction sees exactly the balances the L1 run left.
// A forceExit (to_idx == 1) is a transfer whose receiver needs no slot: nothing ever depends on an exit leaf's balance. Its
// receiver's token is the sender's (the exit leaf is made of the sender's), so null_tok2 adds nothing; phase 3 leaves eff3 in the
// exit-amount buffer at pos_x, where k_ledger_tx leaves the amount of an L2 exit.
// LDS (L1Lds below), limb-major so that the parallel phases are free of bank conflicts: balances [8][1024] u32 = 32768 B; eff_load and
// eff2 / eff3 [5][512] u32 each (an amount is below 2^35 x 10^31 < 2^138) = 20480 B; the two slots of a transaction [512] u16 each =
// 2048 B; flags [512] = 512 B: 55808 B of the 65536 a workgroup may have.
// The per-transaction routines are HZ_HD: the kernel and tests/native/ledger_l1_check.cpp share them.
#pragma once
#include <stdint.h>
#include "u256.h"

namespace hz {

#define HZ_L1_MAX_TX 512u       // HZ_LEDGER_MAX_L1
#define HZ_L1_MAX_SLOTS 1024u   // two accounts per transaction
#define HZ_L1_NO_SLOT 0xFFFFu
enum : uint32_t { L1_NULL_LOAD = 1u, L1_NULL_AMOUNT = 2u };

// one L1 transaction as the kernel reads it: the planner's integers beside the transaction's own
struct LedgerL1Dev {
    uint64_t amount_f, load_amount_f;
    uint32_t token_id;
    uint32_t acct_s, acct_r;   // account - first_idx; acct_r is read only when the amount is not zero
    uint16_t slot_s, slot_r;   // local slots; slot_r == HZ_L1_NO_SLOT: no receiver event
    int32_t pos_s, pos_r;      // grouped positions of the two events in the delta buffer; pos_r < 0: none
    int32_t pos_x;             // a forceExit with an amount: the grouped position of its operation in the exit-amount buffer; else < 0
    uint32_t from_eth[5];      // 160 bits
};

// mantissa x 10^exponent (src/lib/decode-float.circom)
HZ_HD Fc l1_float40(uint64_t f) {
    Fc a = u256_u64(f & ((1ull << 35) - 1));
    const uint32_t e = (uint32_t)(f >> 35) & 31u;
    for (uint32_t s = 0; s < e; s++) a = u256_mul_u32(a, 10u);
    return a;
}

HZ_HD bool l1_is_zero(const Fc& a) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d |= a.v[i];
    return d == 0u;
}

struct L1Static {
    Fc eff_load, eff2;
    uint32_t flags;   // L1_NULL_LOAD | L1_NULL_AMOUNT
};

// the nullifiers that depend on nothing a batch changes. tok_r is looked at only when the amount is not zero
HZ_HD L1Static l1_static(uint64_t amount_f, uint64_t load_amount_f, uint32_t token_id, const uint32_t* from_eth, uint32_t tok_s, const Fc& eth_s,
                         uint32_t tok_r) {
    L1Static r;
    const Fc amount = l1_float40(amount_f), load = l1_float40(load_amount_f);
    const bool has_amount = !l1_is_zero(amount);
    uint32_t d = eth_s.v[5] | eth_s.v[6] | eth_s.v[7];
#pragma unroll
    for (int i = 0; i < 5; i++) d |= eth_s.v[i] ^ from_eth[i];
    const bool null_tok1 = token_id != tok_s;
    const bool null_load = null_tok1 && !l1_is_zero(load);
    const bool null_eth = has_amount && d != 0u;
    const bool null_tok2 = has_amount && token_id != tok_r;
    const bool null_amount = null_eth || null_tok2 || (null_tok1 && has_amount);
    r.eff_load = null_load ? fc_zero() : load;
    r.eff2 = null_amount ? fc_zero() : amount;
    r.flags = (null_load ? L1_NULL_LOAD : 0u) | (null_amount ? L1_NULL_AMOUNT : 0u);
    return r;
}

// one step of the recurrence on the sender: amt is eff2 on entry and eff3 on return, bal the sender's balance before and after;
// -> underflow_ok. The receiver's balance += amt is the caller's, AFTER it has stored bal (a self-transfer sees the new leaf)
HZ_HD bool l1_step(Fc& bal, const Fc& eff_load, Fc& amt) {
    const Fc funded = u256_add(bal, eff_load);   // below 2^193 + 2^138 while no refusal is pending
    const bool ok = !u256_less(funded, amt);
    if (!ok) amt = fc_zero();
    bal = u256_add(funded, u256_neg(amt));
    return ok;
}

// the sender event's delta, two's complement
HZ_HD Fc l1_sender_delta(const Fc& eff_load, const Fc& eff3) { return u256_add(eff_load, u256_neg(eff3)); }

#if defined(__HIPCC__)
struct L1Lds {
    uint32_t bal[8][HZ_L1_MAX_SLOTS];
    uint32_t load[5][HZ_L1_MAX_TX];
    uint32_t amt[5][HZ_L1_MAX_TX];   // eff2 after phase 1, eff3 after phase 2
    uint16_t slot_s[HZ_L1_MAX_TX], slot_r[HZ_L1_MAX_TX];
    uint8_t flag[HZ_L1_MAX_TX];      // L1_NULL_LOAD | L1_NULL_AMOUNT after phase 1; bit 1 is isAmountNullified after phase 2
};
static_assert(sizeof(L1Lds) == 55808 && sizeof(L1Lds) <= 65536, "k_ledger_l1's LDS");

// one workgroup; n <= HZ_L1_MAX_TX, n_slots <= HZ_L1_MAX_SLOTS (the host checks both)
__global__ __launch_bounds__(256) void k_ledger_l1(const LedgerL1Dev* __restrict__ l1, const uint32_t* __restrict__ slot_acct, const uint8_t* __restrict__ planes,
                                                   uint8_t* __restrict__ delta, uint8_t* __restrict__ exit_amt, uint8_t* __restrict__ flags_out, uint32_t N,
                                                   uint32_t n, uint32_t n_slots) {
    __shared__ L1Lds lds;
    // ---- 1: the static part of every transaction, the balance of every slot
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const LedgerL1Dev t = l1[i];
        const Fc e0_s = load_fr(planes + (size_t)t.acct_s * 32);
        const Fc eth_s = load_fr(planes + ((size_t)3 * N + t.acct_s) * 32);
        uint32_t tok_r = 0u;
        if (t.slot_r != HZ_L1_NO_SLOT) tok_r = load_fr(planes + (size_t)t.acct_r * 32).v[0];
        if (t.pos_x >= 0) tok_r = e0_s.v[0];   // the exit leaf holds the sender's token
        const L1Static st = l1_static(t.amount_f, t.load_amount_f, t.token_id, t.from_eth, e0_s.v[0], eth_s, tok_r);
#pragma unroll
        for (int q = 0; q < 5; q++) {
            lds.load[q][i] = st.eff_load.v[q];
            lds.amt[q][i] = st.eff2.v[q];
        }
        lds.slot_s[i] = t.slot_s;
        lds.slot_r[i] = t.slot_r;
        lds.flag[i] = (uint8_t)st.flags;
    }
    for (uint32_t s = threadIdx.x; s < n_slots; s += blockDim.x) {
        const Fc b = load_fr(planes + ((size_t)N + slot_acct[s]) * 32);
#pragma unroll
        for (int q = 0; q < 8; q++) lds.bal[q][s] = b.v[q];
    }
    __syncthreads();
    // ---- 2: the recurrence, in order, LDS only
    if (threadIdx.x == 0) {
#pragma unroll 1
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t s = lds.slot_s[i], r = lds.slot_r[i];
            Fc bal, eff_load = fc_zero(), amt = fc_zero();
#pragma unroll
            for (int q = 0; q < 8; q++) bal.v[q] = lds.bal[q][s];
#pragma unroll
            for (int q = 0; q < 5; q++) {
                eff_load.v[q] = lds.load[q][i];
                amt.v[q] = lds.amt[q][i];
            }
            const bool ok = l1_step(bal, eff_load, amt);
#pragma unroll
            for (int q = 0; q < 8; q++) lds.bal[q][s] = bal.v[q];
            if (r != HZ_L1_NO_SLOT) {   // after the sender's store: r == s reads the new balance
                Fc to;
#pragma unroll
                for (int q = 0; q < 8; q++) to.v[q] = lds.bal[q][r];
                to = u256_add(to, amt);
#pragma unroll
                for (int q = 0; q < 8; q++) lds.bal[q][r] = to.v[q];
            }
            if (!ok) {
#pragma unroll
                for (int q = 0; q < 5; q++) lds.amt[q][i] = 0u;
                lds.flag[i] = (uint8_t)(lds.flag[i] | L1_NULL_AMOUNT);
            }
        }
    }
    __syncthreads();
    // ---- 3: the deltas of the events, the flags
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        Fc eff_load = fc_zero(), eff3 = fc_zero();
#pragma unroll
        for (int q = 0; q < 5; q++) {
            eff_load.v[q] = lds.load[q][i];
            eff3.v[q] = lds.amt[q][i];
        }
        const int32_t pos_s = l1[i].pos_s, pos_r = l1[i].pos_r, pos_x = l1[i].pos_x;
        store_fr(delta + (size_t)pos_s * 32, l1_sender_delta(eff_load, eff3));
        if (pos_r >= 0) store_fr(delta + (size_t)pos_r * 32, eff3);
        if (pos_x >= 0) store_fr(exit_amt + (size_t)pos_x * 32, eff3);
        flags_out[i] = lds.flag[i];
    }
}
#endif

}  // namespace hz
