// hz_ledger's integer tables: the blocks of typed arrays a call uploads in one copy -- their layout and their contents, made of the
// planner's integers (ledger_plan.h) and the rows. No HIP, no field arithmetic: tests/native/ledger_tables_check.cpp fills them into a
// heap block of exactly the layout's size under the address sanitizer and recomputes what they must hold.
// A Span is an array's offset and count inside a block; from a base pointer it yields the array, so one layout object serves the pinned
// block the host fills (host) and the device block the kernels read (dev). A layout is made by one function, in a fixed order, with
// Carve: every array starts at a multiple of 16 bytes and `end` is the block's size.
#pragma once
#include <assert.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/hermez_witness.h"
#include "ledger_archive.h"
#include "ledger_create.h"
#include "ledger_exit.h"
#include "ledger_l1.h"
#include "ledger_plan.h"
#include "ledger_resolve.h"
#include "ledger_select.h"
#if defined(__HIPCC__)
#include "hostutil.h"   // Carve
#endif

#define HZ_LEDGER_CHUNK 64u   // transactions per lane of the fee scan

namespace hz {

#if !defined(__HIPCC__)
struct Carve {   // hostutil.h's, which needs HIP: the host check's copy
    size_t end = 0;
    size_t take(size_t bytes) { const size_t at = end; end = (end + bytes + 15) & ~(size_t)15; return at; }
};
#endif

template <class T>
struct Span {
    size_t at = 0, n = 0;   // byte offset in the block, elements
    T* host(void* base) const { return (T*)((uint8_t*)base + at); }
    T* dev(void* base) const { return (T*)((uint8_t*)base + at); }
    size_t bytes() const { return n * sizeof(T); }
    void take(Carve& c, size_t count) { at = c.take(count * sizeof(T)), n = count; }   // the next array of the block
};

// one event in grouped order
struct LedgerPos {
    uint32_t ev, unit, kind, acct;
};

// a transfer to an address or key that needs its receiver found: processor 2 of a zero amount is a NOP
inline bool ledger_wants_receiver(const hz_l2tx& t) { return t.from_idx != 0 && t.to_idx == 0 && ledger_mantissa(t.amount_f) != 0; }

// an L1 row as k_ledger_l1 and k_ledger_select read it. slot_r < 0: no receiver event; pos_*: grouped positions, < 0: none
inline LedgerL1Dev ledger_l1_dev_row(const hz_l1tx& t, uint64_t first_idx, int32_t slot_s, int32_t slot_r, int32_t pos_s, int32_t pos_r, int32_t pos_x) {
    LedgerL1Dev d{};
    d.amount_f = t.amount_f;
    d.load_amount_f = t.load_amount_f;
    d.token_id = t.token_id;
    d.acct_s = (uint32_t)(t.from_idx - first_idx);
    d.slot_s = (uint16_t)slot_s;
    d.slot_r = HZ_L1_NO_SLOT;
    d.pos_s = pos_s;
    d.pos_r = pos_r;
    d.pos_x = pos_x;
    if (slot_r >= 0) {
        d.acct_r = (uint32_t)(t.to_idx - first_idx);
        d.slot_r = (uint16_t)slot_r;
    }
    memcpy(d.from_eth, t.from_eth_addr, 20);
    return d;
}

// ---- an apply call (R = n_l1 + m rows, F fee slots, M events in G groups, X exit operations on GX keys) ----------------------------------
struct LedgerTables {
    Span<hz_l2tx> tx;                                                   // [R]: an L1 row as the per-row kernels read it, then the L2 rows
    Span<int32_t> pos_s, pos_r, ev_s, ev_r, slot, last, ev_fee, pos_fee;   // last: [R + F]
    Span<uint32_t> plan_tok, acct;
    Span<LedgerPos> pos;
    Span<uint32_t> seg;
    Span<LedgerL1Dev> l1;
    Span<uint32_t> slot_acct;
    Span<int32_t> ev_x, pos_x, last_x;   // [R] where the batch has exit operations, else empty
    Span<LedgerExitPos> xpos;
    Span<uint32_t> xseg;
    Span<LedgerExitOp> xop;
    Span<LedgerCreateRow> crow;          // [R] where the call may create accounts
    size_t end = 0;                      // (G + 1 >= 1: never empty)

    void layout(size_t R, size_t F, size_t M, size_t G, size_t X, size_t GX, size_t n_l1, size_t n_slots, bool creates) {
        Carve c;
        const size_t XR = X ? R : 0;
        tx.take(c, R), pos_s.take(c, R), pos_r.take(c, R), ev_s.take(c, R), ev_r.take(c, R), slot.take(c, R), last.take(c, R + F), ev_fee.take(c, F), pos_fee.take(c, F);
        plan_tok.take(c, F), acct.take(c, M), pos.take(c, M), seg.take(c, G + 1), l1.take(c, n_l1), slot_acct.take(c, n_slots), ev_x.take(c, XR), pos_x.take(c, XR);
        last_x.take(c, XR), xpos.take(c, X), xseg.take(c, X ? GX + 1 : 0), xop.take(c, X), crow.take(c, creates ? R : 0);
        end = c.end;
    }

    // everything but the create rows. l1: the n_l1 rows as the pipeline takes them, txs: the m L2 rows as signed; x_*: the integers of the
    // exit tree's planner, [X] each (not read where the plan has no exit operation)
    void fill(void* hb, const LedgerPlan& p, const hz_l1tx* l1_rows, const hz_l2tx* txs, const uint32_t* plan_tokens, uint64_t first_idx,
              const uint64_t* x_old_key, const uint8_t* x_fnc, const uint8_t* x_is_old0) const {
        const size_t n_l1 = l1.n, R = tx.n, F = ev_fee.n, M = acct.n, X = xop.n;
        std::vector<uint32_t> pos_of(M), xpos_of(X);
        for (uint32_t q = 0; q < M; q++) pos_of[p.perm[q]] = q;
        for (uint32_t q = 0; q < X; q++) xpos_of[p.exit_perm[q]] = q;
        auto at = [](const std::vector<uint32_t>& of, int32_t e) { return e >= 0 ? (int32_t)of[e] : -1; };
        for (size_t i = 0; i < n_l1; i++) {
            hz_l2tx row{};
            row.from_idx = l1_rows[i].from_idx;
            row.to_idx = l1_rows[i].to_idx;
            row.amount_f = l1_rows[i].amount_f;
            row.token_id = l1_rows[i].token_id;
            tx.host(hb)[i] = row;
            l1.host(hb)[i] = ledger_l1_dev_row(l1_rows[i], first_idx, p.l1_slot_sender[i], p.l1_slot_receiver[i], at(pos_of, p.ev_sender[i]), at(pos_of, p.ev_receiver[i]),
                                               at(xpos_of, p.ev_exit[i]));
        }
        for (size_t q = 0; q < slot_acct.n; q++) slot_acct.host(hb)[q] = (uint32_t)(p.slot_account[q] - first_idx);
        if (R > n_l1) memcpy(tx.host(hb) + n_l1, txs, (R - n_l1) * sizeof(hz_l2tx));
        for (size_t i = 0; i < R; i++) {
            pos_s.host(hb)[i] = at(pos_of, p.ev_sender[i]);
            pos_r.host(hb)[i] = at(pos_of, p.ev_receiver[i]);
            ev_s.host(hb)[i] = p.ev_sender[i];
            ev_r.host(hb)[i] = p.ev_receiver[i];
            slot.host(hb)[i] = p.fee_slot[i];
            last.host(hb)[i] = p.last_event[i];
        }
        for (size_t j = 0; j < F; j++) {
            last.host(hb)[R + j] = p.last_event_fee[j];
            ev_fee.host(hb)[j] = p.ev_fee[j];
            pos_fee.host(hb)[j] = at(pos_of, p.ev_fee[j]);
            plan_tok.host(hb)[j] = plan_tokens[j];
        }
        for (uint32_t e = 0; e < M; e++) acct.host(hb)[e] = (uint32_t)(p.account[e] - first_idx);
        for (uint32_t q = 0; q < M; q++) {
            const uint32_t e = p.perm[q];
            pos.host(hb)[q] = LedgerPos{e, p.unit[e], p.kind[e], (uint32_t)(p.account[e] - first_idx)};
        }
        for (size_t g = 0; g < seg.n; g++) seg.host(hb)[g] = p.seg_start[g];
        if (!X) return;
        for (size_t i = 0; i < R; i++) {
            ev_x.host(hb)[i] = p.ev_exit[i];
            pos_x.host(hb)[i] = at(xpos_of, p.ev_exit[i]);
            last_x.host(hb)[i] = p.last_exit[i];
        }
        for (uint32_t q = 0; q < X; q++) {
            const uint32_t x = p.exit_perm[q];
            xpos.host(hb)[q] = LedgerExitPos{x, p.exit_row[x], (uint32_t)(p.exit_key[x] - first_idx)};
        }
        for (uint32_t x = 0; x < X; x++)
            xop.host(hb)[x] = LedgerExitOp{x_old_key[x], (uint32_t)(p.exit_key[x] - first_idx), (x_fnc[x] ? EXIT_OP_INSERT : 0u) | (x_is_old0[x] ? EXIT_OP_IS_OLD0 : 0u)};
        for (size_t g = 0; g < xseg.n; g++) xseg.host(hb)[g] = p.exit_seg_start[g];
    }

    // the create arrays' integers, once the state tree's planner has spoken: the running index (idx_after / aux_from: [n_l1], new_last
    // behind them), and of a create row's sender event -- the insert -- what the planner says (t_*: per event)
    void fill_creates(void* hb, const LedgerPlan& p, const uint64_t* aux_from, const uint64_t* idx_after, uint64_t new_last, const uint64_t* t_old_key,
                      const uint8_t* t_is_old0) const {
        for (size_t i = 0; i < crow.n; i++) {
            LedgerCreateRow row{};
            row.idx_after = i < l1.n ? idx_after[i] : new_last;
            row.ev = p.ev_sender[i];
            if (i < l1.n && aux_from[i]) {
                row.aux_from = aux_from[i];
                row.old_key = t_old_key[row.ev];
                row.flags = CREATE_ROW | (t_is_old0[row.ev] ? CREATE_IS_OLD0 : 0u);
            }
            crow.host(hb)[i] = row;
        }
    }
};

// the work buffer of an apply call: fee[R] | chunk sums | delta[M] | before[M][2] | the failure word | exit amounts[X] | exit before[X][2].
// Every piece is a multiple of 32 bytes, so Carve's rounding to 16 leaves none of them where a sum by hand would not
struct LedgerWork {
    Span<uint8_t> fee, chunk, delta, before, fail, xamt, xbefore;
    size_t end = 0;
    void layout(size_t R, size_t F, size_t M, size_t X) {
        const size_t n_chunks = R ? (R + HZ_LEDGER_CHUNK - 1) / HZ_LEDGER_CHUNK : 1, m1 = M ? M : 1;
        Carve c;
        fee.take(c, (R ? R : 1) * 32), chunk.take(c, n_chunks * (F ? F : 1) * 32), delta.take(c, m1 * 32), before.take(c, m1 * 64), fail.take(c, 64);
        xamt.take(c, X * 32), xbefore.take(c, X * 64);
        end = c.end;
        assert(end == fee.n + chunk.n + delta.n + before.n + fail.n + xamt.n + xbefore.n && xbefore.at + xbefore.n == end);
    }
};

// ---- hz_ledger_select_batch (n_l1 L1 rows in front of a pool of m, n_slots local slots) -------------------------------------------------
struct SelectTables {
    Span<hz_l2tx> tx;   // [m], room for one where m == 0
    Span<SelectTxDev> sel;
    Span<LedgerL1Dev> l1;
    Span<uint32_t> slot_acct;
    Span<int32_t> partner;   // [m] where the call has partners
    size_t end = 0;
    void layout(size_t n_l1, size_t m, size_t n_slots, bool partners) {
        Carve c;
        tx.take(c, m ? m : 1), sel.take(c, m), l1.take(c, n_l1), slot_acct.take(c, n_slots), partner.take(c, partners ? m : 0);
        end = c.end;
    }
    // txs: the pool as signed; eff: with the effective receivers, to_idx still 0 where the destination is unresolved; slot_s / slot_r:
    // [n_l1 + m], -1: none; partner_in: [m] or null
    void fill(void* hb, const hz_l1tx* l1_rows, const hz_l2tx* txs, const hz_l2tx* eff, const int32_t* slot_s, const int32_t* slot_r, const uint64_t* slot_account,
              const int32_t* partner_in, uint64_t first_idx) const {
        const size_t n_l1 = l1.n, m = sel.n;
        if (m) memcpy(tx.host(hb), txs, m * sizeof(hz_l2tx));
        for (size_t i = 0; i < m; i++) {
            SelectTxDev d{};
            const hz_l2tx& t = txs[i];
            if (t.from_idx != 0) {
                const bool has_amount = ledger_mantissa(t.amount_f) != 0, exit = t.to_idx == HZ_LEDGER_EXIT_IDX, unresolved = ledger_wants_receiver(t) && eff[i].to_idx == 0;
                d.amount_f = t.amount_f;
                d.nonce = t.nonce;
                d.token_id = t.token_id;
                d.user_fee = t.user_fee;
                d.acct_s = (uint32_t)(t.from_idx - first_idx);
                d.slot_s = (uint16_t)slot_s[n_l1 + i];
                d.slot_r = HZ_L1_NO_SLOT;
                d.flags = (uint8_t)(SELECT_ACTIVE | (exit ? SELECT_EXIT : 0u) | (unresolved ? SELECT_UNRESOLVED : 0u));
                if (has_amount && !exit && !unresolved) {
                    d.flags |= SELECT_RECEIVER;
                    d.acct_r = (uint32_t)(eff[i].to_idx - first_idx);
                    d.slot_r = (uint16_t)slot_r[n_l1 + i];
                }
            }
            sel.host(hb)[i] = d;
            if (partner.n) partner.host(hb)[i] = t.from_idx != 0 ? partner_in[i] : -1;
        }
        for (size_t i = 0; i < n_l1; i++) {   // a forceExit with an amount: the exit leaf's token is the sender's
            const hz_l1tx& t = l1_rows[i];
            l1.host(hb)[i] = ledger_l1_dev_row(t, first_idx, slot_s[i], slot_r[i], -1, -1, t.to_idx == HZ_LEDGER_EXIT_IDX && ledger_mantissa(t.amount_f) != 0 ? 0 : -1);
        }
        for (size_t q = 0; q < slot_acct.n; q++) slot_acct.host(hb)[q] = (uint32_t)(slot_account[q] - first_idx);
    }
};

// its work buffer: ops[R][14] words | header | kept[m] | verdict[m] | rq_offset[m]; from the header on it comes back to the host
struct SelectWork {
    Span<uint32_t> ops, hdr, kept;
    Span<uint8_t> verdict, off;
    size_t end = 0;
    void layout(size_t R, size_t m) {
        Carve c;
        ops.take(c, (R ? R : 1) * HZ_SELECT_OP_WORDS), hdr.take(c, 4), kept.take(c, m), verdict.take(c, m), off.take(c, m);
        end = c.end;
    }
};

// ---- the lookup of receivers by address or key: up to `up` the host's, the results behind it ----------------------------------------------
struct ResolveTables {
    Span<ResolveKey> table;
    Span<uint32_t> result;
    Span<int32_t> slot;
    Span<uint64_t> out;
    size_t up = 0, end = 0;
    static bool asks(const hz_l2tx& t, bool skip_zero) { return t.from_idx != 0 && t.to_idx == 0 && !(skip_zero && ledger_mantissa(t.amount_f) == 0); }
    void layout(size_t slots, size_t m) {
        Carve c;
        table.take(c, slots), result.take(c, slots), slot.take(c, m);
        up = c.end;
        out.take(c, m);
        end = c.end;
    }
    void fill(void* hb, const hz_l2tx* txs, const hz_l2sig* sigs, bool skip_zero) const {
        memset(table.host(hb), 0, table.bytes());
        memset(result.host(hb), 0xFF, result.bytes());
        for (size_t i = 0; i < slot.n; i++)
            slot.host(hb)[i] = !asks(txs[i], skip_zero) ? -1 : resolve_insert(table.host(hb), (uint32_t)table.n, resolve_key(txs[i].token_id, resolve_load32(sigs[i].to_eth_addr),
                                                                                                                        resolve_load32(sigs[i].to_bjj_ay), sigs[i].to_bjj_sign));
    }
};

// ---- hz_ledger_withdraw_rows: snapshot [n] | idx [n], the host's, then meta [n] | sources [n][S] ------------------------------------------
struct WithdrawTables {
    Span<int32_t> snap;
    Span<uint64_t> idx;
    Span<WithdrawMeta> meta;
    Span<uint32_t> src;
    size_t up = 0, end = 0;
    void layout(size_t n, size_t S) {
        Carve c;
        snap.take(c, n), idx.take(c, n);
        up = c.end;
        meta.take(c, n), src.take(c, n * S);
        end = c.end;
    }
    // find(batch) -> the snapshot's place in the descriptor table, -1: not kept (queries on one batch mostly come in runs)
    template <class Find>
    void fill(void* hb, const uint32_t* batch_num, const uint64_t* idx_in, Find find) const {
        uint32_t last_batch = 0;
        int64_t last_at = -2;
        for (size_t i = 0; i < snap.n; i++) {
            if (last_at == -2 || batch_num[i] != last_batch) last_batch = batch_num[i], last_at = find(last_batch);
            snap.host(hb)[i] = (int32_t)last_at;
            idx.host(hb)[i] = idx_in[i];
        }
    }
};

}  // namespace hz
