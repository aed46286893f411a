// hz_ledger's host planner: the integer work of a batch of L2 transfers -- which update events the batch makes, on which accounts,
// in which order, and where each fee goes. No field arithmetic, no hash, no HIP: hz_ledger_plan_l2 runs it without a device and the
// CPU suite checks it against a Python restatement.
//
// Events. Active transaction i (from_idx != 0) makes a SENDER event and, when its amount is not zero (the float40's 35-bit mantissa is
// not zero: integer work), a RECEIVER event right after it; after the last transaction every fee slot j with fee_idxs[j] != 0 makes a
// FEE event, in slot order. The events in that order are the updates of one hz_state apply. Events of one account are grouped, in order
// (perm / seg_start): a device lane walks a group and carries the account's balance and nonce through it.
// A batch (ledger_plan_batch) puts n_l1 L1 transactions in front: row i < n_l1 is L1 transaction i, row n_l1 + i is L2
// transaction i, and "transaction" above reads "row". An L1 row makes an L1_SENDER event and, when its amount is not zero, an
// L1_RECEIVER event; it has no fee slot. The accounts the L1 run touches are numbered as dense local slots by first appearance
// (sender before receiver) -- the first groups of the grouping, since the L1 events come first: the L1 kernel keeps one balance per
// slot in LDS.
// Exits (ledger_plan_exits). A row with to_idx == 1 is an exit: an L2 exit or an L1 forceExit. It makes its sender event
// as any other row and NO receiver event -- last_event keeps counting state events only, and a forceExit has no receiver slot. When
// its amount is not zero it makes one operation on the batch's exit tree instead, at key from_idx. Those operations, in row order, are
// a second list: the row and the key of each, grouped by key as the events are by account (exit_perm / exit_seg_start, groups numbered
// by first appearance), and the first operation of a group is the INSERT of its key, every later one an UPDATE. A device lane walks a
// group and carries the exit leaf's balance through it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../include/hermez_witness.h"

namespace hz {

enum : uint8_t { LEDGER_EV_SENDER = 0, LEDGER_EV_RECEIVER = 1, LEDGER_EV_FEE = 2, LEDGER_EV_L1_SENDER = 3, LEDGER_EV_L1_RECEIVER = 4 };

struct LedgerPlan {
    // per row (transaction)
    std::vector<int32_t> ev_sender, ev_receiver;   // event numbers, -1: none
    std::vector<int32_t> fee_slot;                  // first slot whose plan token is the transaction's, -1: none (or a NOP)
    std::vector<int32_t> last_event;                // the last event made by transactions 0 .. i, -1: none yet
    // per fee slot
    std::vector<int32_t> ev_fee, last_event_fee;    // the slot's event (-1: fee_idxs[j] == 0); the last event up to and including slot j
    // per event
    std::vector<uint64_t> account;
    std::vector<int32_t> prev_same;                 // the previous event on the same account, -1: none
    std::vector<uint32_t> unit;                     // transaction i, or m + j for the event of fee slot j
    std::vector<uint8_t> kind;
    // grouping: the events of group g are perm[seg_start[g] .. seg_start[g + 1]), ascending
    std::vector<uint32_t> perm, seg_start;
    // the L1 run: the local slot of every L1 transaction's sender and receiver (-1: no receiver), the account of every slot
    std::vector<int32_t> l1_slot_sender, l1_slot_receiver;
    std::vector<uint64_t> slot_account;
    // exits: per row the exit operation it makes (-1: none) and the last one made by rows 0 .. i (-1: none yet); per operation its row,
    // its key, the previous operation on the same key (-1: none, the operation is the insert); the grouping by key
    std::vector<int32_t> ev_exit, last_exit;
    std::vector<uint32_t> exit_row;
    std::vector<uint64_t> exit_key;
    std::vector<int32_t> exit_prev;
    std::vector<uint32_t> exit_perm, exit_seg_start;
};

#define HZ_LEDGER_EXIT_IDX 1ull

// stable grouping of `key` (all below ~0): groups numbered by first appearance, the members of group g are perm[seg_start[g] ..
// seg_start[g + 1]), ascending; prev_same[e] is the previous member of e's group (-1: none), group_of[e] the group
inline void ledger_group(const std::vector<uint64_t>& key, std::vector<int32_t>& prev_same, std::vector<uint32_t>& perm, std::vector<uint32_t>& seg_start,
                         std::vector<uint32_t>& group_of) {
    const uint32_t M = (uint32_t)key.size();
    uint32_t cap = 16;
    while (cap < 2 * M) cap <<= 1;
    std::vector<uint64_t> slot_key(cap, ~0ull);
    std::vector<uint32_t> group(cap), tail;
    group_of.assign(M, 0);
    prev_same.assign(M, -1);
    seg_start.assign(1, 0);
    for (uint32_t e = 0; e < M; e++) {
        uint32_t s = (uint32_t)((key[e] * 0x9E3779B97F4A7C15ull) >> 40) & (cap - 1);
        while (slot_key[s] != ~0ull && slot_key[s] != key[e]) s = (s + 1) & (cap - 1);
        if (slot_key[s] == ~0ull) {
            slot_key[s] = key[e];
            group[s] = (uint32_t)tail.size();
            tail.push_back(e);
            seg_start.push_back(0);
        } else {
            prev_same[e] = (int32_t)tail[group[s]];
            tail[group[s]] = e;
        }
        group_of[e] = group[s];
        seg_start[group_of[e] + 1]++;
    }
    for (size_t g = 1; g < seg_start.size(); g++) seg_start[g] += seg_start[g - 1];
    std::vector<uint32_t> at(seg_start.begin(), seg_start.end() - 1);
    perm.resize(M);
    for (uint32_t e = 0; e < M; e++) perm[at[group_of[e]]++] = e;
}

inline uint64_t ledger_mantissa(uint64_t amount_f) { return amount_f & ((1ull << 35) - 1); }

// exits == false: no row has to_idx == 1 (the callers refuse it) and the exit lists stay empty
inline void ledger_plan_rows(size_t n_l1, const hz_l1tx* l1, size_t m, const hz_l2tx* txs, size_t F, const uint32_t* plan_tokens, const uint64_t* fee_idxs,
                             bool exits, LedgerPlan& p) {
    const size_t R = n_l1 + m;
    p.ev_sender.assign(R, -1);
    p.ev_receiver.assign(R, -1);
    p.fee_slot.assign(R, -1);
    p.last_event.assign(R, -1);
    p.l1_slot_sender.assign(n_l1, -1);
    p.l1_slot_receiver.assign(n_l1, -1);
    p.slot_account.clear();
    p.ev_fee.assign(F, -1);
    p.last_event_fee.assign(F, -1);
    p.account.clear();
    p.unit.clear();
    p.kind.clear();
    p.ev_exit.assign(R, -1);
    p.last_exit.assign(R, -1);
    p.exit_row.clear();
    p.exit_key.clear();
    auto event = [&](uint64_t account, size_t unit, uint8_t kind) {
        p.account.push_back(account);
        p.unit.push_back((uint32_t)unit);
        p.kind.push_back(kind);
        return (int32_t)(p.account.size() - 1);
    };
    // processor 2 of a row with an amount: an operation on the exit tree for an exit, else the receiver's event
    auto second = [&](uint64_t from_idx, uint64_t to_idx, size_t row, uint8_t kind) {
        if (exits && to_idx == HZ_LEDGER_EXIT_IDX) {
            p.ev_exit[row] = (int32_t)p.exit_row.size();
            p.exit_row.push_back((uint32_t)row);
            p.exit_key.push_back(from_idx);
        } else {
            p.ev_receiver[row] = event(to_idx, row, kind);
        }
    };
    for (size_t i = 0; i < n_l1; i++) {
        const hz_l1tx& t = l1[i];
        p.ev_sender[i] = event(t.from_idx, i, LEDGER_EV_L1_SENDER);
        if (ledger_mantissa(t.amount_f) != 0) second(t.from_idx, t.to_idx, i, LEDGER_EV_L1_RECEIVER);
        p.last_event[i] = (int32_t)p.account.size() - 1;
        p.last_exit[i] = (int32_t)p.exit_row.size() - 1;
    }
    for (size_t i = 0; i < m; i++) {
        const hz_l2tx& t = txs[i];
        const size_t row = n_l1 + i;
        if (t.from_idx != 0) {
            p.ev_sender[row] = event(t.from_idx, row, LEDGER_EV_SENDER);
            if (ledger_mantissa(t.amount_f) != 0) second(t.from_idx, t.to_idx, row, LEDGER_EV_RECEIVER);
            for (size_t s = 0; s < F; s++)
                if (plan_tokens[s] == t.token_id) {
                    p.fee_slot[row] = (int32_t)s;
                    break;
                }
        }
        p.last_event[row] = (int32_t)p.account.size() - 1;
        p.last_exit[row] = (int32_t)p.exit_row.size() - 1;
    }
    for (size_t j = 0; j < F; j++) {
        if (fee_idxs[j] != 0) p.ev_fee[j] = event(fee_idxs[j], R + j, LEDGER_EV_FEE);
        p.last_event_fee[j] = (int32_t)p.account.size() - 1;
    }

    // stable grouping by account, groups numbered by first appearance
    std::vector<uint32_t> ev_group;
    ledger_group(p.account, p.prev_same, p.perm, p.seg_start, ev_group);
    // the L1 events come first: the groups of the L1 run are its local slots
    for (size_t i = 0; i < n_l1; i++) {
        p.l1_slot_sender[i] = (int32_t)ev_group[p.ev_sender[i]];
        if (p.ev_receiver[i] >= 0) p.l1_slot_receiver[i] = (int32_t)ev_group[p.ev_receiver[i]];
    }
    size_t n_slots = 0;
    for (int32_t e = 0; n_l1 && e <= p.last_event[n_l1 - 1]; e++)
        if (ev_group[e] + 1 > n_slots) n_slots = ev_group[e] + 1;
    for (size_t q = 0; q < n_slots; q++) p.slot_account.push_back(p.account[p.perm[p.seg_start[q]]]);
    // the exit operations by key: the first of a group inserts
    std::vector<uint32_t> exit_group;
    ledger_group(p.exit_key, p.exit_prev, p.exit_perm, p.exit_seg_start, exit_group);
}

inline void ledger_plan_batch(size_t n_l1, const hz_l1tx* l1, size_t m, const hz_l2tx* txs, size_t F, const uint32_t* plan_tokens, const uint64_t* fee_idxs,
                              LedgerPlan& p) {
    ledger_plan_rows(n_l1, l1, m, txs, F, plan_tokens, fee_idxs, false, p);
}

inline void ledger_plan_exits(size_t n_l1, const hz_l1tx* l1, size_t m, const hz_l2tx* txs, size_t F, const uint32_t* plan_tokens, const uint64_t* fee_idxs,
                              LedgerPlan& p) {
    ledger_plan_rows(n_l1, l1, m, txs, F, plan_tokens, fee_idxs, true, p);
}

inline void ledger_plan_l2(size_t m, const hz_l2tx* txs, size_t F, const uint32_t* plan_tokens, const uint64_t* fee_idxs, LedgerPlan& p) {
    ledger_plan_batch(0, nullptr, m, txs, F, plan_tokens, fee_idxs, p);
}

}  // namespace hz
