// hz_ledger's argument checks: what every ledger call and every hz_ledger_plan_* export decides about its arguments before anything is
// planned or launched -- which caller memory is read and how far, every status and every message, and the order in which errors win.
// No HIP, no device: the ledger is a LedgerShape, five integers. tests/native/ledger_checks_check.cpp drives these checks under the address
// and undefined-behaviour sanitizers with every input array in a heap block of exactly its size, on the cases of
// tests/golden/ledger_arg_errors.json.gz. Each check is written once: the call form selects what a row may be and, for the L1 run, the wording.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../../include/hermez_witness.h"
#include "ledger_create.h"
#include "ledger_plan.h"
#include "ledger_rq.h"
#if defined(__HIPCC__)
#include "hostutil.h"   // set_err, canon_lt_p
#endif

#define HZ_LEDGER_MAX_EVENTS 65536u
#define HZ_LEDGER_MAX_TX (1u << 20)
#define HZ_LEDGER_MAX_F 64u
#define HZ_LEDGER_MAX_CAPACITY (1ull << 24)
#define HZ_LEDGER_REASONS 17u   // refusal reasons 1 .. 13 and 16; 0 is none, 14 and 15 are verdicts of hz_ledger_select_batch

namespace hz {

#if !defined(__HIPCC__)
hz_status set_err(hz_status st, const char* fmt, ...);   // hostutil.h's, which needs HIP: the host check defines its own
inline bool canon_lt_p(const uint8_t* b) {               // canonical 32-byte LE integer < r ? (hostutil.h's)
    static const uint32_t P[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
    for (int i = 7; i >= 0; i--) {
        const uint32_t w = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
        if (w != P[i]) return w < P[i];
    }
    return false;
}
#endif

// what the checks need of a ledger. A dense one: capacity == live == 2^depth, depth its tree's k; a growing one: live of capacity accounts,
// depth its n_sib_max
struct LedgerShape {
    bool growing;
    uint64_t capacity, first_idx, live;
    uint32_t depth;
};
inline LedgerShape ledger_dense_shape(int32_t k, uint64_t first_idx) { return LedgerShape{false, 1ull << k, first_idx, 1ull << k, (uint32_t)k}; }

static const char* const LEDGER_REASON[HZ_LEDGER_REASONS] = {"", "the sender's token is not the transaction's", "the nonce is not the sender's current nonce",
                                             "the sender's balance is below amount + fee", "the receiver's token is not the transaction's",
                                             "a new balance reaches 2^192", "the fee account's token is not the slot's plan token",
                                             "the signature is rejected", "max_num_batch has expired",
                                              "no account holds the signed destination with the transaction's token",
                                              "the receiver's ethAddr is not the signed to_eth_addr", "the receiver's key is not the signed to_bjj_ay / to_bjj_sign",
                                              "the sender's nonce is 2^40 - 1: the next nonce is not a leaf field",
                                              "the rq fields are not the link fields of the row rq_offset names", "", "",
                                             "amount x fee factor does not fit 128 bits (src/compute-fee.circom:89-91)"};
static_assert(HZ_LEDGER_FEE_OVERFLOW == 16 && HZ_LEDGER_FEE_OVERFLOW > HZ_SELECT_FULL, "the reason behind the select verdicts");

// the one wording of a refusal: a fee slot (unit >= R), a row of a batch with an L1 run (L1 != 0), else a transaction
inline hz_status ledger_refused(const char* who, size_t unit, uint32_t reason, size_t R, size_t L1) {
    char what[64];
    if (unit >= R)
        snprintf(what, sizeof what, "fee slot %zu", unit - R);
    else if (L1)
        snprintf(what, sizeof what, "%s transaction %zu", unit < L1 ? "L1" : "L2", unit < L1 ? unit : unit - L1);
    else
        snprintf(what, sizeof what, "transaction %zu", unit);
    return set_err(HZ_ERR_INPUT, "%s: refused at index %zu (%s), reason %u: %s", who, unit, what, reason, LEDGER_REASON[reason < HZ_LEDGER_REASONS ? reason : 0]);
}

inline bool ledger_has(uint64_t first_idx, uint64_t N, uint64_t idx) { return idx >= first_idx && idx - first_idx < N; }

inline hz_status ledger_check_k(const char* who, int32_t k) { return k < 4 || k > 24 ? set_err(HZ_ERR_ARG, "%s: k = %d (4 .. 24)", who, k) : HZ_OK; }

inline hz_status ledger_check_flags(const char* who, uint32_t flags) {
    return flags & ~HZ_LEDGER_VERIFY_SIGS ? set_err(HZ_ERR_ARG, "%s: flags = %#x", who, flags) : HZ_OK;
}

// a dense ledger's tree has k levels; a growing one's depth is the planner's to judge (a leaf at depth >= n_sib is HZ_ERR_ARG there)
inline hz_status ledger_n_sib(const LedgerShape& g, const char* who, size_t n_sib) {
    if (g.growing) {
        if (n_sib < 1 || n_sib > 64 || n_sib > g.depth) return set_err(HZ_ERR_ARG, "%s: n_sib = %zu (1 .. %u, the ledger's n_sib_max)", who, n_sib, g.depth);
        return HZ_OK;
    }
    if (n_sib < g.depth || n_sib > 64) return set_err(HZ_ERR_ARG, "%s: n_sib = %zu (%u .. 64)", who, n_sib, g.depth);
    return HZ_OK;
}

// the per-transaction argument checks of every call that takes transactions; a NOP (from_idx == 0) is not looked at. by_addr: to_idx == 0
// (a receiver named by address or key) passes; exits: to_idx == 1 does
inline hz_status ledger_check_txs(const char* who, size_t m, const hz_l2tx* txs, uint64_t first_idx, uint64_t N, bool by_addr = false, bool exits = false) {
    const uint64_t last = first_idx + N - 1;
    for (size_t i = 0; i < m; i++) {
        const hz_l2tx& t = txs[i];
        if (t.from_idx == 0) continue;
        if (!ledger_has(first_idx, N, t.from_idx))
            return set_err(HZ_ERR_ARG, "%s: tx %zu: from_idx = %llu is outside the state (%llu .. %llu)", who, i, (unsigned long long)t.from_idx,
                           (unsigned long long)first_idx, (unsigned long long)last);
        const bool named = (t.to_idx == 0 && by_addr) || (t.to_idx == HZ_LEDGER_EXIT_IDX && exits);   // no receiver index to look at
        if (!named && t.to_idx <= 1)
            return set_err(HZ_ERR_ARG, "%s: tx %zu: to_idx = %llu (%s) is not supported yet", who, i, (unsigned long long)t.to_idx,
                           t.to_idx ? "an exit" : "a transfer to an address");
        if (!named && !ledger_has(first_idx, N, t.to_idx))
            return set_err(HZ_ERR_ARG, "%s: tx %zu: to_idx = %llu is outside the state (%llu .. %llu)", who, i, (unsigned long long)t.to_idx,
                           (unsigned long long)first_idx, (unsigned long long)last);
        if (t.amount_f >> 40) return set_err(HZ_ERR_ARG, "%s: tx %zu: amount_f has more than 40 bits", who, i);
    }
    return HZ_OK;
}

// the planners of the exports are given receivers: a transfer to an address has none before the lookup
inline hz_status ledger_check_receivers_given(const char* who, size_t m, const hz_l2tx* txs) {
    for (size_t i = 0; i < m; i++)
        if (txs[i].from_idx != 0 && txs[i].to_idx == 0) return set_err(HZ_ERR_ARG, "%s: tx %zu: to_idx = 0 (a transfer to an address) is not supported yet", who, i);
    return HZ_OK;
}

// the checks of an L1 row that do not depend on which accounts exist
inline hz_status ledger_check_l1_fields(const char* who, size_t i, const hz_l1tx& t) {
    if (t.amount_f >> 40) return set_err(HZ_ERR_ARG, "%s: L1 tx %zu: amount_f has more than 40 bits", who, i);
    if (t.load_amount_f >> 40) return set_err(HZ_ERR_ARG, "%s: L1 tx %zu: load_amount_f has more than 40 bits", who, i);
    for (int b = 20; b < 32; b++)
        if (t.from_eth_addr[b]) return set_err(HZ_ERR_ARG, "%s: L1 tx %zu: from_eth_addr has more than 160 bits", who, i);
    if (ledger_mantissa(t.amount_f) != 0 && t.to_idx == 0) return set_err(HZ_ERR_ARG, "%s: L1 tx %zu: an amount with to_idx = 0 (no receiver)", who, i);
    return HZ_OK;
}

// what the checks of a call with an L1 run or receivers by address leave: the rows as the pipeline takes them
struct LedgerRows {
    std::vector<hz_l1tx> eff_l1;   // a create row is a deposit on auxFromIdx, in from_idx's place
    std::vector<uint64_t> aux_from, idx_after;   // [n_l1] the running index; aux_from 0: the row creates nothing. Of a call form with creates
    const hz_l1tx* l1 = nullptr;   // eff_l1's, or the caller's where the call form creates nothing
    size_t n_creates = 0, l1_events = 0;
    std::vector<hz_l2sig> no_sigs;
    const hz_l2sig* sigs = nullptr;   // the caller's, or zero entries where no destination is signed
    std::vector<hz_l2tx> eff;      // the L2 rows with the effective receivers: what the plan is made of
    uint64_t count = 0;            // the accounts an L2 row or a fee slot may name: live plus created
};

// the argument checks of the L1 run, the one loop of every call form. creates: from_idx == 0 makes an account where the
// ledger grows, so an index exists from its row on and the messages say "at its row"; exits: to_idx == 1 passes. A form without creates
// takes the same loop with a constant last index. -> r.l1, the rows as the pipeline takes them, the events they make, the accounts the
// call makes, and of a form with creates auxFromIdx and the last idx after every row
inline hz_status ledger_effective_l1(const LedgerShape& g, const char* who, size_t n_l1, const hz_l1tx* l1, const uint8_t* from_bjj, bool creates, bool exits, LedgerRows& r) {
    r.l1 = l1;
    r.l1_events = r.n_creates = 0;
    if (n_l1 > HZ_LEDGER_MAX_L1) return set_err(HZ_ERR_ARG, "%s: n_l1 = %zu L1 transactions (at most %d)", who, n_l1, HZ_LEDGER_MAX_L1);
    if (n_l1 && !l1) return set_err(HZ_ERR_ARG, "%s: null l1", who);
    if (creates) {
        r.eff_l1.assign(l1, l1 + n_l1);
        r.aux_from.assign(n_l1, 0);
        r.idx_after.assign(n_l1, 0);
        r.l1 = r.eff_l1.data();
    }
    const uint64_t first = g.first_idx;
    uint64_t last = first + g.live - 1;   // first_idx - 1 on an empty ledger
    for (size_t i = 0; i < n_l1; i++) {
        const hz_l1tx& t = l1[i];
        // (each form's own test and wording: they differ only where first_idx + live wraps)
        auto missing = [&](const char* field, uint64_t idx) {
            if (creates ? idx >= first && idx <= last && last >= first : ledger_has(first, g.live, idx)) return HZ_OK;
            return creates ? set_err(HZ_ERR_ARG, "%s: L1 tx %zu: %s = %llu does not exist at its row (%llu .. %lld)", who, i, field, (unsigned long long)idx,
                                     (unsigned long long)first, (long long)last)
                           : set_err(HZ_ERR_ARG, "%s: L1 tx %zu: %s = %llu is outside the state (%llu .. %llu)", who, i, field, (unsigned long long)idx,
                                     (unsigned long long)first, (unsigned long long)last);
        };
        if (t.from_idx == 0) {
            if (!creates) return set_err(HZ_ERR_ARG, "%s: L1 tx %zu: from_idx = 0 (creates an account) is not supported yet", who, i);
            if (!g.growing) return set_err(HZ_ERR_ARG, "%s: L1 tx %zu: from_idx = 0 (creates an account) on a ledger that cannot grow (hz_ledger_create_growing)", who, i);
            if (!from_bjj) return set_err(HZ_ERR_ARG, "%s: L1 tx %zu: from_idx = 0 (creates an account) with from_bjj == NULL", who, i);
            if (g.live + r.n_creates + 1 > g.capacity)
                return set_err(HZ_ERR_ARG, "%s: L1 tx %zu: the ledger is full (capacity %llu accounts)", who, i, (unsigned long long)g.capacity);
            r.n_creates += 1;
            last = create_next_idx(last, true);
            r.aux_from[i] = last;
            r.eff_l1[i].from_idx = last;
            if (t.to_idx == HZ_LEDGER_EXIT_IDX) return set_err(HZ_ERR_ARG, "%s: L1 tx %zu: a row that creates an account with to_idx = 1 (an exit)", who, i);
        } else if (hz_status e = missing("from_idx", t.from_idx)) {
            return e;
        }
        if (creates) r.idx_after[i] = last;
        if (t.to_idx == HZ_LEDGER_EXIT_IDX && !exits) return set_err(HZ_ERR_ARG, "%s: L1 tx %zu: to_idx = 1 (an exit) is not supported yet", who, i);
        if (t.to_idx > HZ_LEDGER_EXIT_IDX)
            if (hz_status e = missing("to_idx", t.to_idx)) return e;
        if (hz_status e = ledger_check_l1_fields(who, i, t)) return e;
        r.l1_events += 1 + (ledger_mantissa(t.amount_f) != 0);
    }
    r.count = g.live + r.n_creates;
    return HZ_OK;
}

// the argument checks hz_ledger_apply_l2 and hz_ledger_plan_l2 share; on success the plan is made. by_addr (hz_ledger_apply_l2_addr): the
// checks alone -- the plan is made later, on the effective receivers
inline hz_status ledger_check_plan(const char* who, size_t m, const hz_l2tx* txs, size_t F, const uint32_t* plan_tokens, const uint64_t* fee_idxs, uint64_t N,
                                   uint64_t first_idx, LedgerPlan& plan, bool by_addr = false, size_t l1_events = 0, bool exits = false) {
    if ((m && !txs) || (F && (!plan_tokens || !fee_idxs))) return set_err(HZ_ERR_ARG, "%s: null argument", who);
    if (F > HZ_LEDGER_MAX_F) return set_err(HZ_ERR_ARG, "%s: F = %zu fee slots (at most %u)", who, F, HZ_LEDGER_MAX_F);
    if (m > HZ_LEDGER_MAX_TX) return set_err(HZ_ERR_ARG, "%s: %zu transactions in one call (at most %u)", who, m, HZ_LEDGER_MAX_TX);
    if (hz_status e = ledger_check_txs(who, m, txs, first_idx, N, by_addr, exits)) return e;
    for (size_t j = 0; j < F; j++)
        if (fee_idxs[j] != 0 && !ledger_has(first_idx, N, fee_idxs[j]))
            return set_err(HZ_ERR_ARG, "%s: fee_idxs[%zu] = %llu is outside the state (%llu .. %llu)", who, j, (unsigned long long)fee_idxs[j],
                           (unsigned long long)first_idx, (unsigned long long)(first_idx + N - 1));
    size_t events = l1_events;
    for (size_t i = 0; i < m; i++)
        if (txs[i].from_idx != 0) events += 1 + (ledger_mantissa(txs[i].amount_f) != 0);
    for (size_t j = 0; j < F; j++) events += fee_idxs[j] != 0;
    if (events > HZ_LEDGER_MAX_EVENTS) return set_err(HZ_ERR_ARG, "%s: %zu updates in one call (at most %u)", who, events, HZ_LEDGER_MAX_EVENTS);
    if (!by_addr) ledger_plan_l2(m, txs, F, plan_tokens, fee_idxs, plan);
    return HZ_OK;
}

// the head hz_ledger_plan_batch and hz_ledger_plan_exits (exits: with its n_sib) share: a dense ledger of 2^k accounts, an L1 run, the plan's
// checks, receivers given
inline hz_status ledger_check_plan_rows(const char* who, int32_t k, uint64_t first_idx, bool exits, size_t n_sib, size_t n_l1, const hz_l1tx* l1, size_t m,
                                        const hz_l2tx* txs, size_t F, const uint32_t* plan_tokens, const uint64_t* fee_idxs, LedgerPlan& p) {
    if (hz_status e = ledger_check_k(who, k)) return e;
    const LedgerShape g = ledger_dense_shape(k, first_idx);
    if (exits)
        if (hz_status e = ledger_n_sib(g, who, n_sib)) return e;
    LedgerRows r;
    if (hz_status e = ledger_effective_l1(g, who, n_l1, l1, nullptr, false, exits, r)) return e;
    if (hz_status e = ledger_check_plan(who, m, txs, F, plan_tokens, fee_idxs, g.live, first_idx, p, true, r.l1_events, exits)) return e;
    return ledger_check_receivers_given(who, m, txs);
}

// hz_ledger_plan_creates: the ledger as the caller states it, the L1 run, the plan's checks -> r: the running index
inline hz_status ledger_check_plan_creates(const char* who, const LedgerShape& g, size_t n_l1, const hz_l1tx* l1, const uint8_t* from_bjj, size_t m, const hz_l2tx* txs,
                                           size_t F, const uint32_t* plan_tokens, const uint64_t* fee_idxs, LedgerRows& r) {
    if (g.capacity < 1 || g.capacity > HZ_LEDGER_MAX_CAPACITY || g.live > g.capacity || g.first_idx < 2)
        return set_err(HZ_ERR_ARG, "%s: capacity = %llu, size = %llu, first_idx = %llu", who, (unsigned long long)g.capacity, (unsigned long long)g.live,
                       (unsigned long long)g.first_idx);
    if (hz_status e = ledger_effective_l1(g, who, n_l1, l1, from_bjj, true, true, r)) return e;
    LedgerPlan p;
    return ledger_check_plan(who, m, txs, F, plan_tokens, fee_idxs, r.count, g.first_idx, p, true, r.l1_events, true);
}

// the argument checks of the signed calls beyond those of the transactions; a NOP's entry is not looked at. verify == false
// (hz_ledger_apply_l2_addr without HZ_LEDGER_VERIFY_SIGS): the destination fields alone, s, r8x, r8y and chain_id are not read
inline hz_status ledger_check_sigs(const char* who, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, uint32_t chain_id, bool verify = true) {
    if (m && !sigs) return set_err(HZ_ERR_ARG, "%s: null sigs", who);
    if (verify && chain_id >> 16) return set_err(HZ_ERR_ARG, "%s: chain_id = %u has more than 16 bits", who, chain_id);
    for (size_t i = 0; i < m; i++) {
        if (txs[i].from_idx == 0) continue;
        const hz_l2sig& g = sigs[i];
        if (g.to_bjj_sign > 1) return set_err(HZ_ERR_ARG, "%s: tx %zu: to_bjj_sign = %u", who, i, (unsigned)g.to_bjj_sign);
        for (int b = 20; b < 32; b++)
            if (g.to_eth_addr[b]) return set_err(HZ_ERR_ARG, "%s: tx %zu: to_eth_addr has more than 160 bits", who, i);
        const uint8_t* f[4] = {g.s, g.r8x, g.r8y, g.to_bjj_ay};
        static const char* const name[4] = {"s", "r8x", "r8y", "to_bjj_ay"};
        for (int q = verify ? 0 : 3; q < 4; q++)
            if (!canon_lt_p(f[q])) return set_err(HZ_ERR_INPUT, "%s: tx %zu: %s is not below the field's modulus", who, i, name[q]);
    }
    return HZ_OK;
}

// sigs == NULL without verification: no destination is signed, zero entries stand in (the link fields of such rows are V2 and two zeros)
inline hz_status ledger_stand_in_sigs(const char* who, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, bool verify, LedgerRows& r) {
    r.sigs = sigs;
    if (sigs || !m || verify) return HZ_OK;
    for (size_t i = 0; i < m; i++)
        if (txs[i].from_idx != 0 && txs[i].to_idx == 0) return set_err(HZ_ERR_ARG, "%s: null sigs with tx %zu to an address", who, i);
    r.no_sigs.assign(m, hz_l2sig{});
    r.sigs = r.no_sigs.data();
    return HZ_OK;
}

// the argument checks of the atomic links; a NOP's entry is not looked at
inline hz_status ledger_check_rq(const char* who, size_t m, const hz_l2tx* txs, const hz_l2rq* rq) {
    if (!rq) return HZ_OK;
    for (size_t i = 0; i < m; i++) {
        if (txs[i].from_idx == 0) continue;
        const hz_l2rq& q = rq[i];
        if (q.rq_offset > HZ_RQ_MAX_OFFSET) return set_err(HZ_ERR_ARG, "%s: tx %zu: rq_offset = %u (0 .. 7)", who, i, (unsigned)q.rq_offset);
        const uint8_t* f[3] = {q.rq_tx_compressed_data_v2, q.rq_to_eth_addr, q.rq_to_bjj_ay};
        static const char* const name[3] = {"rq_tx_compressed_data_v2", "rq_to_eth_addr", "rq_to_bjj_ay"};
        for (int a = 0; a < 3; a++)
            if (!canon_lt_p(f[a])) return set_err(HZ_ERR_INPUT, "%s: tx %zu: %s is not below the field's modulus", who, i, name[a]);
    }
    return HZ_OK;
}

// hz_ledger_plan_atomic's
inline hz_status ledger_check_plan_atomic(const char* who, size_t n_l1, size_t m, const hz_l2tx* txs, const hz_l2sig* sigs, const hz_l2rq* rq) {
    if (m && (!txs || !sigs)) return set_err(HZ_ERR_ARG, "%s: null argument", who);
    if (n_l1 > HZ_LEDGER_MAX_L1) return set_err(HZ_ERR_ARG, "%s: n_l1 = %zu L1 transactions (at most %d)", who, n_l1, HZ_LEDGER_MAX_L1);
    if (m > HZ_LEDGER_MAX_TX) return set_err(HZ_ERR_ARG, "%s: %zu transactions in one call (at most %u)", who, m, HZ_LEDGER_MAX_TX);
    return ledger_check_rq(who, m, txs, rq);
}

// any byte set from `from` to the end of a 32-byte little-endian element
inline bool ledger_bytes_from(const uint8_t* p, int from) {
    uint8_t d = 0;
    for (int b = from; b < 32; b++) d |= p[b];
    return d != 0;
}

// the first account whose fields are not a leaf's, named
inline hz_status ledger_check_leaves(const char* who, uint64_t first_idx, size_t n, const uint8_t* e0, const uint8_t* balance, const uint8_t* eth_addr) {
    for (size_t i = 0; i < n; i++) {
        const char* bad = nullptr;
        if (ledger_bytes_from(balance + i * 32, 24)) bad = "balance >= 2^192";
        else if (ledger_bytes_from(e0 + i * 32, 10) || e0[i * 32 + 9] > 1) bad = "e0 >= 2^73";
        else if (ledger_bytes_from(eth_addr + i * 32, 20)) bad = "ethAddr >= 2^160";
        if (bad) return set_err(HZ_ERR_INPUT, "%s: account %llu (row %zu) is not a leaf: %s", who, (unsigned long long)(first_idx + i), i, bad);
    }
    return HZ_OK;
}

// ---- a batch selected from a pool ----------------------------------------------------------------------------------------
// the local slots of hz_ledger_select_batch: the distinct accounts the L1 rows and the pool touch, numbered by first appearance -- the
// groups ledger_plan_rows makes, L1's first. Per row (L1 rows, then the pool): the sender's and the receiver's slot, -1: none
struct SelectPlan {
    std::vector<int32_t> slot_s, slot_r;
    std::vector<uint64_t> slot_account;
};

inline hz_status select_check_pool(const char* who, size_t m) {
    if (m > HZ_SELECT_MAX_POOL)
        return set_err(HZ_ERR_ARG, "%s: tx %d does not fit: a pool holds at most %d candidates (HZ_SELECT_MAX_POOL)", who, HZ_SELECT_MAX_POOL, HZ_SELECT_MAX_POOL);
    return HZ_OK;
}

// partner[i] names another transaction of the pool or none; a NOP's entry is not looked at
inline hz_status select_check_partner(const char* who, size_t m, const hz_l2tx* txs, const int32_t* partner) {
    if (!partner) return HZ_OK;
    for (size_t i = 0; i < m; i++) {
        if (txs[i].from_idx == 0) continue;
        if (partner[i] < -1 || (partner[i] >= 0 && (size_t)partner[i] >= m))
            return set_err(HZ_ERR_ARG, "%s: tx %zu: partner = %d is outside the pool (-1 .. %zu)", who, i, partner[i], m ? m - 1 : 0);
        if (partner[i] >= 0 && (size_t)partner[i] == i) return set_err(HZ_ERR_ARG, "%s: tx %zu: partner = %d is the transaction itself", who, i, partner[i]);
    }
    return HZ_OK;
}

// hz_ledger_plan_select's: its L1 rows carry auxFromIdx in from_idx's place already, and no state is given to hold them against
inline hz_status select_check_plan(const char* who, size_t n_l1, const hz_l1tx* l1, size_t m, const hz_l2tx* txs, const int32_t* partner) {
    if ((n_l1 && !l1) || (m && !txs)) return set_err(HZ_ERR_ARG, "%s: null argument", who);
    if (n_l1 > HZ_LEDGER_MAX_L1) return set_err(HZ_ERR_ARG, "%s: n_l1 = %zu L1 transactions (at most %d)", who, n_l1, HZ_LEDGER_MAX_L1);
    for (size_t i = 0; i < n_l1; i++) {
        if (l1[i].from_idx == 0) return set_err(HZ_ERR_ARG, "%s: L1 tx %zu: from_idx = 0: the planner takes a create row with its auxFromIdx in from_idx's place", who, i);
        if (hz_status e = ledger_check_l1_fields(who, i, l1[i])) return e;
    }
    if (hz_status e = select_check_pool(who, m)) return e;
    return select_check_partner(who, m, txs, partner);
}

// eff: the pool with the effective receivers; a row whose to_idx is still 0 has none (an unresolved destination, or none asked for).
// More candidates or slots than k_ledger_select's LDS holds is an argument error that names the first pool index that does not fit
inline hz_status select_plan(const char* who, size_t n_l1, const hz_l1tx* l1, size_t m, const hz_l2tx* eff, LedgerPlan& p, SelectPlan& sp) {
    if (hz_status e = select_check_pool(who, m)) return e;
    std::vector<hz_l2tx> rows(eff, eff + m);
    for (size_t i = 0; i < m; i++)
        if (rows[i].from_idx != 0 && rows[i].to_idx == 0) rows[i].amount_f = 0;   // no receiver event
    ledger_plan_rows(n_l1, l1, m, rows.data(), 0, nullptr, nullptr, true, p);
    const size_t R = n_l1 + m, G = p.seg_start.size() - 1;
    std::vector<uint32_t> group_of(p.account.size());
    for (size_t g = 0; g < G; g++)
        for (uint32_t q = p.seg_start[g]; q < p.seg_start[g + 1]; q++) group_of[p.perm[q]] = (uint32_t)g;
    sp.slot_s.assign(R, -1);
    sp.slot_r.assign(R, -1);
    for (size_t r = 0; r < R; r++) {
        if (p.ev_sender[r] >= 0) sp.slot_s[r] = (int32_t)group_of[p.ev_sender[r]];
        if (p.ev_receiver[r] >= 0) sp.slot_r[r] = (int32_t)group_of[p.ev_receiver[r]];
        if (sp.slot_s[r] >= (int32_t)HZ_SELECT_MAX_SLOTS || sp.slot_r[r] >= (int32_t)HZ_SELECT_MAX_SLOTS)   // (an L1 run alone has at most 1024)
            return set_err(HZ_ERR_ARG, "%s: tx %zu does not fit: the L1 rows and the pool touch more than %d distinct accounts (HZ_SELECT_MAX_SLOTS)", who, r - n_l1,
                           HZ_SELECT_MAX_SLOTS);
    }
    sp.slot_account.resize(G);
    for (size_t g = 0; g < G; g++) sp.slot_account[g] = p.account[p.perm[p.seg_start[g]]];
    return HZ_OK;
}

}  // namespace hz
