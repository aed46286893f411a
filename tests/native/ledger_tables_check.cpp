// host build of the ledger's integer tables (circuits_amd/csrc/ledger_tables.h): batches from stdin, one record per line, every field in hex --
//   b first_idx exits creates partners   a new batch: what the call accepts, whether the selection has partners
//   f token fee_idx                      a fee slot
//   l from to amount_f load_f token from_eth aux_from idx_after
//                                        an L1 row as the pipeline takes it (auxFromIdx in from_idx's place), its running index
//   t from to amount_f nonce token user_fee eff_to partner flags
//                                        an L2 row as signed; its effective receiver (0: none, or unresolved); partner + 1 (0: none);
//                                        the SelectTxDev flags it must get
//   e                                    the batch ends: ledger_plan_rows, then every block is laid out and filled into a heap block of
//                                        exactly its size -- an overrun is the sanitizer's -- and compared with a plain recomputation
// -- and prints "cases=N mismatches=K", a case being one check of one batch.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include "../../circuits_amd/csrc/ledger_tables.h"
using namespace hz;

static size_t cases = 0, bad = 0;
static void check(bool ok, const char* what, size_t batch) {
    cases++;
    if (!ok) {
        bad++;
        fprintf(stderr, "batch %zu: %s differs\n", batch, what);
    }
}

typedef std::vector<std::pair<size_t, size_t>> Extents;   // (offset, bytes) of every span of a block
template <class T>
static void add(Extents& x, const Span<T>& s) { x.push_back({s.at, s.bytes()}); }

// disjoint, at multiples of `align`, inside the block, in the order they were taken
static bool spans_ok(Extents x, size_t end, size_t align = 16) {
    bool ok = std::is_sorted(x.begin(), x.end(), [](const std::pair<size_t, size_t>& a, const std::pair<size_t, size_t>& b) { return a.first < b.first || (a.first == b.first && a.second < b.second); });
    for (size_t i = 0; i < x.size(); i++) ok = ok && x[i].first % align == 0 && x[i].first + x[i].second <= (i + 1 < x.size() ? x[i + 1].first : end);
    return ok && end % 16 == 0;
}

struct Batch {
    uint64_t first_idx = 0;
    bool exits = false, creates = false, partners = false;
    std::vector<uint32_t> tokens;
    std::vector<uint64_t> fee_idxs, aux_from, idx_after, eff_to;
    std::vector<hz_l1tx> l1;
    std::vector<hz_l2tx> txs;
    std::vector<int32_t> partner;
    std::vector<uint32_t> flags;
};

static std::unique_ptr<uint8_t[]> block(size_t bytes) { return std::unique_ptr<uint8_t[]>(new uint8_t[bytes]); }
static bool same_l1(const LedgerL1Dev& a, const LedgerL1Dev& b) {
    return a.amount_f == b.amount_f && a.load_amount_f == b.load_amount_f && a.token_id == b.token_id && a.acct_s == b.acct_s && a.acct_r == b.acct_r && a.slot_s == b.slot_s &&
           a.slot_r == b.slot_r && a.pos_s == b.pos_s && a.pos_r == b.pos_r && a.pos_x == b.pos_x && memcmp(a.from_eth, b.from_eth, 20) == 0;
}

// the apply call's block and its work buffer
static void check_apply(const Batch& b, size_t at) {
    const size_t n_l1 = b.l1.size(), m = b.txs.size(), R = n_l1 + m, F = b.tokens.size();
    std::vector<hz_l2tx> eff(b.txs);
    for (size_t i = 0; i < m; i++)
        if (ledger_wants_receiver(b.txs[i])) eff[i].to_idx = b.eff_to[i];
    LedgerPlan p;
    ledger_plan_rows(n_l1, b.l1.data(), m, eff.data(), F, b.tokens.data(), b.fee_idxs.data(), b.exits, p);
    const size_t M = p.account.size(), G = p.seg_start.size() - 1, X = p.exit_row.size(), GX = p.exit_seg_start.size() - 1;
    LedgerTables T;
    T.layout(R, F, M, G, X, GX, n_l1, p.slot_account.size(), b.creates);
    Extents x;
    add(x, T.tx), add(x, T.pos_s), add(x, T.pos_r), add(x, T.ev_s), add(x, T.ev_r), add(x, T.slot), add(x, T.last), add(x, T.ev_fee), add(x, T.pos_fee), add(x, T.plan_tok);
    add(x, T.acct), add(x, T.pos), add(x, T.seg), add(x, T.l1), add(x, T.slot_acct), add(x, T.ev_x), add(x, T.pos_x), add(x, T.last_x), add(x, T.xpos), add(x, T.xseg);
    add(x, T.xop), add(x, T.crow);
    check(spans_ok(x, T.end) && T.tx.n == R && T.last.n == R + F && T.seg.n == G + 1 && T.crow.n == (b.creates ? R : 0) && T.ev_x.n == (X ? R : 0), "the apply layout", at);
    LedgerWork W;
    W.layout(R, F, M, X);
    Extents w;
    add(w, W.fee), add(w, W.chunk), add(w, W.delta), add(w, W.before), add(w, W.fail), add(w, W.xamt), add(w, W.xbefore);
    const size_t chunks = R ? (R + 63) / 64 : 1;
    check(spans_ok(w, W.end, 32) && W.end == ((R ? R : 1) + chunks * (F ? F : 1) + (M ? M : 1) * 3 + 2 + X * 3) * 32 && W.fail.n == 64, "the work layout", at);
    // the integers of the two trees' planners: stand-ins, told apart by their values
    std::vector<uint64_t> x_old(X), t_old(M);
    std::vector<uint8_t> x_fnc(X), x_is0(X), t_is0(M);
    for (size_t q = 0; q < X; q++) x_old[q] = 0x5000 + q, x_fnc[q] = p.exit_prev[q] < 0, x_is0[q] = q % 3 == 0;
    for (size_t e = 0; e < M; e++) t_old[e] = 0x7000 + e, t_is0[e] = e % 2;
    const std::unique_ptr<uint8_t[]> mem = block(T.end);
    void* hb = mem.get();
    T.fill(hb, p, b.l1.data(), b.txs.data(), b.tokens.data(), b.first_idx, x_old.data(), x_fnc.data(), x_is0.data());
    const uint64_t new_last = 0x9999;
    T.fill_creates(hb, p, b.aux_from.data(), b.idx_after.data(), new_last, t_old.data(), t_is0.data());
    // positions: the inverse of the grouping, -1 where there is no event
    auto inverse = [](const std::vector<uint32_t>& perm, const int32_t* pos, const std::vector<int32_t>& ev) {
        bool ok = true;
        for (size_t i = 0; i < ev.size(); i++) ok = ok && (ev[i] < 0 ? pos[i] == -1 : pos[i] >= 0 && (size_t)pos[i] < perm.size() && perm[pos[i]] == (uint32_t)ev[i]);
        return ok;
    };
    check(inverse(p.perm, T.pos_s.host(hb), p.ev_sender) && inverse(p.perm, T.pos_r.host(hb), p.ev_receiver) && inverse(p.perm, T.pos_fee.host(hb), p.ev_fee) &&
              (!X || inverse(p.exit_perm, T.pos_x.host(hb), p.ev_exit)),
          "pos_s / pos_r / pos_fee / pos_x", at);
    bool ok = true;
    for (size_t q = 0; q < M; q++) {
        const LedgerPos g = T.pos.host(hb)[q];
        const uint32_t e = p.perm[q];
        ok = ok && g.ev == e && g.unit == p.unit[e] && g.kind == p.kind[e] && g.acct == p.account[e] - b.first_idx && T.acct.host(hb)[e] == p.account[e] - b.first_idx;
    }
    check(ok, "pos / acct", at);
    check(std::equal(p.seg_start.begin(), p.seg_start.end(), T.seg.host(hb)) && (!X || std::equal(p.exit_seg_start.begin(), p.exit_seg_start.end(), T.xseg.host(hb))), "seg / xseg", at);
    ok = true;
    for (size_t i = 0; i < R; i++) {
        ok = ok && T.ev_s.host(hb)[i] == p.ev_sender[i] && T.ev_r.host(hb)[i] == p.ev_receiver[i] && T.slot.host(hb)[i] == p.fee_slot[i] && T.last.host(hb)[i] == p.last_event[i];
        if (X) ok = ok && T.ev_x.host(hb)[i] == p.ev_exit[i] && T.last_x.host(hb)[i] == p.last_exit[i];
        const hz_l2tx& t = T.tx.host(hb)[i];
        if (i >= n_l1) ok = ok && memcmp(&t, &b.txs[i - n_l1], sizeof t) == 0;
        else ok = ok && t.from_idx == b.l1[i].from_idx && t.to_idx == b.l1[i].to_idx && t.amount_f == b.l1[i].amount_f && t.token_id == b.l1[i].token_id && t.nonce == 0 && t.user_fee == 0;
    }
    for (size_t j = 0; j < F; j++) ok = ok && T.last.host(hb)[R + j] == p.last_event_fee[j] && T.ev_fee.host(hb)[j] == p.ev_fee[j] && T.plan_tok.host(hb)[j] == b.tokens[j];
    check(ok, "the per-row and per-slot tables", at);
    // the L1 rows: slots by first appearance, positions by a search of the grouping
    std::map<uint64_t, int32_t> slot;
    auto slot_of = [&](uint64_t a) { return slot.emplace(a, (int32_t)slot.size()).first->second; };
    auto find = [](const std::vector<uint32_t>& perm, int32_t e) { return e < 0 ? -1 : (int32_t)(std::find(perm.begin(), perm.end(), (uint32_t)e) - perm.begin()); };
    ok = true;
    for (size_t i = 0; i < n_l1; i++) {
        const hz_l1tx& t = b.l1[i];
        const bool amount = ledger_mantissa(t.amount_f) != 0, receiver = amount && !(b.exits && t.to_idx == HZ_LEDGER_EXIT_IDX);
        LedgerL1Dev d{};
        d.amount_f = t.amount_f, d.load_amount_f = t.load_amount_f, d.token_id = t.token_id;
        d.acct_s = (uint32_t)(t.from_idx - b.first_idx), d.slot_s = (uint16_t)slot_of(t.from_idx), d.slot_r = HZ_L1_NO_SLOT;
        d.pos_s = find(p.perm, p.ev_sender[i]), d.pos_r = find(p.perm, p.ev_receiver[i]), d.pos_x = find(p.exit_perm, p.ev_exit[i]);
        if (receiver) d.acct_r = (uint32_t)(t.to_idx - b.first_idx), d.slot_r = (uint16_t)slot_of(t.to_idx);
        memcpy(d.from_eth, t.from_eth_addr, 20);
        ok = ok && same_l1(d, T.l1.host(hb)[i]) && (receiver == (p.ev_receiver[i] >= 0)) && ((amount && !receiver) == (p.ev_exit[i] >= 0));
    }
    ok = ok && slot.size() == T.slot_acct.n;
    for (const auto& s : slot) ok = ok && (size_t)s.second < T.slot_acct.n && T.slot_acct.host(hb)[s.second] == s.first - b.first_idx;
    check(ok, "the L1 rows", at);
    ok = true;
    for (size_t q = 0; q < X; q++) {
        const LedgerExitPos g = T.xpos.host(hb)[q];
        const uint32_t e = p.exit_perm[q];
        const LedgerExitOp o = T.xop.host(hb)[q];
        ok = ok && g.op == e && g.row == p.exit_row[e] && g.acct == p.exit_key[e] - b.first_idx;
        ok = ok && o.old_key == x_old[q] && o.acct == p.exit_key[q] - b.first_idx && o.flags == ((x_fnc[q] ? EXIT_OP_INSERT : 0u) | (x_is0[q] ? EXIT_OP_IS_OLD0 : 0u));
    }
    check(ok, "xpos / xop", at);
    ok = true;
    for (size_t i = 0; i < T.crow.n; i++) {
        const LedgerCreateRow r = T.crow.host(hb)[i];
        const bool made = i < n_l1 && b.aux_from[i] != 0;
        ok = ok && r.ev == p.ev_sender[i] && r.idx_after == (i < n_l1 ? b.idx_after[i] : new_last) && r.aux_from == (made ? b.aux_from[i] : 0) &&
             r.old_key == (made ? t_old[r.ev] : 0) && r.flags == (made ? CREATE_ROW | (t_is0[r.ev] ? CREATE_IS_OLD0 : 0u) : 0u);
    }
    check(ok, "the create rows", at);
}

// the selection call's block: local slots by first appearance, an unresolved destination has no receiver
static void check_select(const Batch& b, size_t at) {
    const size_t n_l1 = b.l1.size(), m = b.txs.size(), R = n_l1 + m;
    std::vector<hz_l2tx> eff(b.txs);
    std::vector<int32_t> slot_s(R, -1), slot_r(R, -1);
    std::vector<uint64_t> slot_account;
    auto slot_of = [&](uint64_t a) {
        const size_t s = std::find(slot_account.begin(), slot_account.end(), a) - slot_account.begin();
        if (s == slot_account.size()) slot_account.push_back(a);
        return (int32_t)s;
    };
    for (size_t i = 0; i < n_l1; i++) {
        slot_s[i] = slot_of(b.l1[i].from_idx);
        if (ledger_mantissa(b.l1[i].amount_f) != 0 && b.l1[i].to_idx != HZ_LEDGER_EXIT_IDX) slot_r[i] = slot_of(b.l1[i].to_idx);
    }
    for (size_t i = 0; i < m; i++) {
        if (ledger_wants_receiver(b.txs[i])) eff[i].to_idx = b.eff_to[i];
        if (b.txs[i].from_idx == 0) continue;
        slot_s[n_l1 + i] = slot_of(b.txs[i].from_idx);
        if (ledger_mantissa(b.txs[i].amount_f) != 0 && eff[i].to_idx > HZ_LEDGER_EXIT_IDX) slot_r[n_l1 + i] = slot_of(eff[i].to_idx);
    }
    SelectTables T;
    T.layout(n_l1, m, slot_account.size(), b.partners);
    Extents x;
    add(x, T.tx), add(x, T.sel), add(x, T.l1), add(x, T.slot_acct), add(x, T.partner);
    SelectWork W;
    W.layout(R, m);
    Extents w;
    add(w, W.ops), add(w, W.hdr), add(w, W.kept), add(w, W.verdict), add(w, W.off);
    check(spans_ok(x, T.end) && spans_ok(w, W.end) && T.tx.n == (m ? m : 1) && T.partner.n == (b.partners ? m : 0) && W.hdr.bytes() == 16, "the select layouts", at);
    const std::unique_ptr<uint8_t[]> mem = block(T.end);
    void* hb = mem.get();
    T.fill(hb, b.l1.data(), b.txs.data(), eff.data(), slot_s.data(), slot_r.data(), slot_account.data(), b.partners ? b.partner.data() : nullptr, b.first_idx);
    bool ok = m == 0 || memcmp(T.tx.host(hb), b.txs.data(), m * sizeof(hz_l2tx)) == 0, flags_ok = true;
    for (size_t i = 0; i < m; i++) {
        const SelectTxDev d = T.sel.host(hb)[i];
        const hz_l2tx& t = b.txs[i];
        flags_ok = flags_ok && d.flags == b.flags[i];
        if (b.partners) ok = ok && T.partner.host(hb)[i] == (t.from_idx ? b.partner[i] : -1);
        if (t.from_idx == 0) {
            ok = ok && d.amount_f == 0 && d.nonce == 0 && d.acct_s == 0 && d.acct_r == 0 && d.token_id == 0 && d.slot_s == 0 && d.slot_r == 0 && d.user_fee == 0;
            continue;
        }
        const bool rec = (d.flags & SELECT_RECEIVER) != 0;
        ok = ok && d.amount_f == t.amount_f && d.nonce == t.nonce && d.token_id == t.token_id && d.user_fee == t.user_fee && d.acct_s == t.from_idx - b.first_idx &&
             d.slot_s == (uint16_t)slot_s[n_l1 + i] && d.slot_r == (rec ? (uint16_t)slot_r[n_l1 + i] : HZ_L1_NO_SLOT) && d.acct_r == (rec ? eff[i].to_idx - b.first_idx : 0) &&
             rec == (slot_r[n_l1 + i] >= 0);
    }
    check(flags_ok, "the SelectTxDev flags", at);
    for (size_t i = 0; i < n_l1; i++) {
        const hz_l1tx& t = b.l1[i];
        const bool amount = ledger_mantissa(t.amount_f) != 0, exit = t.to_idx == HZ_LEDGER_EXIT_IDX;
        LedgerL1Dev d{};
        d.amount_f = t.amount_f, d.load_amount_f = t.load_amount_f, d.token_id = t.token_id;
        d.acct_s = (uint32_t)(t.from_idx - b.first_idx), d.slot_s = (uint16_t)slot_s[i], d.slot_r = HZ_L1_NO_SLOT, d.pos_s = d.pos_r = -1, d.pos_x = amount && exit ? 0 : -1;
        if (amount && !exit) d.acct_r = (uint32_t)(t.to_idx - b.first_idx), d.slot_r = (uint16_t)slot_r[i];
        memcpy(d.from_eth, t.from_eth_addr, 20);
        ok = ok && same_l1(d, T.l1.host(hb)[i]);
    }
    for (size_t q = 0; q < slot_account.size(); q++) ok = ok && T.slot_acct.host(hb)[q] == slot_account[q] - b.first_idx;
    check(ok, "the select rows", at);
}

// the lookup's and the withdraw call's blocks: the layouts, which rows ask, runs of one batch number
static void check_lookups(const Batch& b, size_t at) {
    const size_t m = b.txs.size();
    std::vector<hz_l2sig> sigs(m, hz_l2sig{});
    size_t queries = 0;
    for (size_t i = 0; i < m; i++) {
        memcpy(sigs[i].to_eth_addr, &b.txs[i].token_id, 4);   // a destination per token: rows of one token share a query
        queries += ResolveTables::asks(b.txs[i], true);
    }
    ResolveTables T;
    const uint32_t slots = resolve_slots(queries ? queries : 1);
    T.layout(slots, m);
    Extents x;
    add(x, T.table), add(x, T.result), add(x, T.slot), add(x, T.out);
    const std::unique_ptr<uint8_t[]> mem = block(T.end);
    T.fill(mem.get(), b.txs.data(), sigs.data(), true);
    bool ok = spans_ok(x, T.end) && T.up == T.out.at && T.up % 16 == 0;
    for (size_t i = 0; i < m; i++) {
        const int32_t s = T.slot.host(mem.get())[i];
        ok = ok && (s >= 0) == ledger_wants_receiver(b.txs[i]) && s < (int32_t)slots;
        for (size_t j = 0; j < i && s >= 0; j++)
            if (T.slot.host(mem.get())[j] >= 0) ok = ok && (T.slot.host(mem.get())[j] == s) == (b.txs[j].token_id == b.txs[i].token_id);
    }
    for (uint32_t s = 0; s < slots; s++) ok = ok && T.result.host(mem.get())[s] == HZ_RESOLVE_NONE;
    check(ok, "the lookup's block", at);
    // a query per row on the row's token as its batch number: even ones are kept, at place token / 2
    WithdrawTables V;
    const size_t S = 1 + at % 5;
    V.layout(m, S);
    Extents v;
    add(v, V.snap), add(v, V.idx), add(v, V.meta), add(v, V.src);
    std::vector<uint32_t> batch(m);
    std::vector<uint64_t> idx(m);
    for (size_t i = 0; i < m; i++) batch[i] = b.txs[i].token_id, idx[i] = b.txs[i].from_idx;
    const std::unique_ptr<uint8_t[]> host = block(V.up);   // the host's part alone
    size_t asked = 0;
    V.fill(host.get(), batch.data(), idx.data(), [&](uint32_t n) { return asked++, n % 2 ? (int64_t)-1 : (int64_t)(n / 2); });
    ok = spans_ok(v, V.end) && V.up == V.meta.at && V.src.n == m * S && asked <= m;
    for (size_t i = 0; i < m; i++) ok = ok && V.snap.host(host.get())[i] == (batch[i] % 2 ? -1 : (int32_t)(batch[i] / 2)) && V.idx.host(host.get())[i] == idx[i];
    check(ok, "the withdraw block", at);
}

int main() {
    Batch b;
    size_t batches = 0;
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        std::vector<std::string> f;
        for (char* p = strtok(line, " \t\r\n"); p; p = strtok(nullptr, " \t\r\n")) f.push_back(p);
        if (f.empty()) continue;
        auto u = [&](size_t i) { return strtoull(f[i].c_str(), nullptr, 16); };
        const char op = f[0][0];
        if (op == 'b' && f.size() == 5) {
            b = Batch();
            b.first_idx = u(1), b.exits = u(2) != 0, b.creates = u(3) != 0, b.partners = u(4) != 0;
        } else if (op == 'f' && f.size() == 3) {
            b.tokens.push_back((uint32_t)u(1));
            b.fee_idxs.push_back(u(2));
        } else if (op == 'l' && f.size() == 9) {
            hz_l1tx t{};
            t.from_idx = u(1), t.to_idx = u(2), t.amount_f = u(3), t.load_amount_f = u(4), t.token_id = (uint32_t)u(5);
            for (size_t i = 0; i < 40 && i < f[6].size(); i++) {   // from_eth_addr: 32 bytes, little-endian
                const char c = f[6][f[6].size() - 1 - i];
                t.from_eth_addr[i / 2] |= (uint8_t)((c <= '9' ? c - '0' : (c | 32) - 'a' + 10) << (4 * (i % 2)));
            }
            b.l1.push_back(t);
            b.aux_from.push_back(u(7));
            b.idx_after.push_back(u(8));
        } else if (op == 't' && f.size() == 10) {
            hz_l2tx t{};
            t.from_idx = u(1), t.to_idx = u(2), t.amount_f = u(3), t.nonce = u(4), t.token_id = (uint32_t)u(5), t.user_fee = (uint8_t)u(6);
            b.txs.push_back(t);
            b.eff_to.push_back(u(7));
            b.partner.push_back((int32_t)u(8) - 1);
            b.flags.push_back((uint32_t)u(9));
        } else if (op == 'e' && f.size() == 1) {
            bool unresolved = false;
            for (uint32_t fl : b.flags) unresolved = unresolved || (fl & SELECT_UNRESOLVED);
            if (!unresolved) check_apply(b, batches);   // (an apply call refuses an unresolved destination before it plans)
            check_select(b, batches);
            check_lookups(b, batches);
            batches++;
        } else {
            fprintf(stderr, "bad line: %s with %zu fields\n", f[0].c_str(), f.size());
            return 2;
        }
    }
    printf("cases=%zu mismatches=%zu\n", cases, bad);
    return bad != 0;
}
