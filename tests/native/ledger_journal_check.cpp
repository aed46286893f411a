// The undo journal's host half (csrc/ledger_journal.h) and the shape's undo (csrc/smt_plan.h: commit_undo / revert) built for the host and
// run under the address and undefined-behaviour sanitizers. The program checks itself: every CHECK that fails prints its line and the
// program ends with status 1; "ok checks=<n>" on stderr otherwise. With the argument "spoil" one expectation is altered on purpose and the
// program must fail: the checks do judge.
//   ring   depth 1, 2 and 64: push, eviction, the slot a record gets, which records a mark undoes and in what order, every accepted and
//          refused mark at the ring's two edges with status and message, the stats; the byte layout of a record
//   cut    the archive cut with none, one and several kept batches, after an exit_forget from below
//   shape  an SmtShape taken through three calls -- inserts that push an existing leaf deeper, updates, a call that only updates --,
//          reverted three at once, then one by one; after each, root, child and leaf_key equal those of a shape rebuilt from scratch that
//          never saw the reverted calls, and the shape takes the next call as the rebuilt one does
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../circuits_amd/csrc/ledger_journal.h"
#include "../../circuits_amd/csrc/smt_plan.h"

static char g_err[1024];
namespace hz {
hz_status set_err(hz_status st, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return st;
}
}  // namespace hz
using namespace hz;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        g_checks++;                                                       \
        if (!(cond)) {                                                    \
            g_failed++;                                                   \
            fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #cond); \
        }                                                                 \
    } while (0)

// ---- ring ----------------------------------------------------------------------------------------------------------------------------------
// `applies` applies on a ledger with a journal of `depth`, the way ledger.hip drives the ring: take the free slot, write, push (which evicts)
static void run_ring(uint32_t depth, uint64_t applies, bool spoil) {
    JournalRing ring;
    ring.set_depth(depth);
    uint64_t applied = 0;
    std::vector<uint64_t> slot_mark(depth + 1, ~0ull);   // which record's bytes a slab holds
    for (uint64_t a = 0; a < applies; a++) {
        const size_t before = ring.records();
        const int32_t slot = ring.free_slot();   // beside every record held: an apply that fails later has lost none
        CHECK(slot >= 0 && (uint32_t)slot <= depth && ring.records() == before);
        if (slot < 0) return;
        for (const JournalRecord& r : ring.rec) CHECK(r.slot != (uint32_t)slot);   // no live record loses its slab
        JournalRecord r;
        r.mark = applied, r.live = 16 + a, r.slot = (uint32_t)slot, r.tree_entries = 5 + a, r.groups = 3, r.bytes = journal_layout(5 + a, 3).bytes;
        ring.push(r);
        slot_mark[slot] = applied;
        applied++;
        CHECK(ring.records() == (size_t)(applied < depth ? applied : depth));
        CHECK(ring.oldest_mark(applied) == applied - ring.records());
    }
    const size_t held = ring.records();
    CHECK(held == (size_t)(applies < depth ? applies : depth));
    for (size_t i = 0; i < held; i++) {   // oldest first, consecutive marks, each in the slab that holds its bytes
        CHECK(ring.rec[i].mark == applied - held + i);
        CHECK(slot_mark[ring.rec[i].slot] == ring.rec[i].mark);
    }
    // the two edges: the current mark and one beyond; the oldest mark and one below
    const uint64_t oldest = applied - held;
    CHECK(journal_mark_verdict(applied, held, applied) == HZ_JOURNAL_OK && ring.undone_by(applied) == 0);
    CHECK(journal_mark_verdict(applied, held, applied + 1) == HZ_JOURNAL_FUTURE);
    CHECK(journal_mark_verdict(applied, held, oldest) == HZ_JOURNAL_OK && ring.undone_by(oldest) == held);
    if (oldest > 0) CHECK(journal_mark_verdict(applied, held, oldest - 1) == HZ_JOURNAL_GONE);
    CHECK(journal_mark_verdict(applied, held, ~0ull) == HZ_JOURNAL_FUTURE);
    for (uint64_t mark = oldest; mark <= applied; mark++) CHECK(ring.undone_by(mark) == (size_t)(applied - mark));   // every accepted mark
    // the messages name both numbers
    CHECK(journal_check_mark("f", applied, depth, held, applied) == HZ_OK);
    CHECK(journal_check_mark("f", applied, depth, held, applied + 1) == HZ_ERR_ARG);
    char want[256];
    snprintf(want, sizeof want, "f: mark = %llu lies ahead of the ledger (applied = %llu)", (unsigned long long)(applied + 1), (unsigned long long)applied);
    CHECK(std::string(g_err) == want);
    if (oldest > 0) {
        CHECK(journal_check_mark("f", applied, depth, held, oldest - 1) == HZ_ERR_ARG);
        snprintf(want, sizeof want, "f: mark = %llu is older than the journal reaches: applied = %llu, %zu records of depth %u (oldest mark %llu)",
                 (unsigned long long)(oldest - 1), (unsigned long long)applied, held, depth, (unsigned long long)(spoil ? oldest + 1 : oldest));
        CHECK(std::string(g_err) == want);
    }
    // a rollback to the middle: newest first, then the ring takes applies again from there
    const uint64_t mid = oldest + held / 2;
    const size_t n = ring.undone_by(mid);
    uint64_t expect = applied;
    for (size_t i = 0; i < n; i++) {
        expect--;
        CHECK(ring.rec.back().mark == expect);
        ring.pop_newest();
    }
    applied = mid;
    CHECK(expect == mid && ring.records() == held - n && ring.oldest_mark(applied) == oldest);
    CHECK(ring.bytes_used() <= held * journal_layout(5 + applies, 3).bytes);
    CHECK(ring.free_slot() >= 0 && ring.slots() == depth + 1);
    ring.clear();   // a load
    CHECK(ring.records() == 0 && ring.oldest_mark(0) == 0 && ring.free_slot() == 0 && ring.bytes_used() == 0);
}

static void ring_cases(bool spoil) {
    for (uint32_t depth : {1u, 2u, 64u})
        for (uint64_t applies : {0ull, 1ull, 2ull, 3ull, 63ull, 64ull, 65ull, 200ull}) run_ring(depth, applies, spoil);
    // the journal off: only the current mark
    CHECK(journal_mark_verdict(7, 0, 7) == HZ_JOURNAL_OK && journal_mark_verdict(7, 0, 6) == HZ_JOURNAL_GONE && journal_mark_verdict(0, 0, 0) == HZ_JOURNAL_OK);
    CHECK(journal_check_mark("g", 7, 0, 0, 6) == HZ_ERR_ARG && std::string(g_err) == "g: mark = 6, applied = 7, and the journal is off (hz_ledger_journal)");
    CHECK(journal_check_depth("h", 0) == HZ_OK && journal_check_depth("h", HZ_LEDGER_JOURNAL_MAX) == HZ_OK);
    CHECK(journal_check_depth("h", HZ_LEDGER_JOURNAL_MAX + 1) == HZ_ERR_ARG && std::string(g_err) == "h: depth = 65 (0 .. 64)");
    // the byte layout: the parts do not overlap, every element is 32-byte aligned, the entries lie behind their elements
    for (size_t t : {0u, 1u, 7u, 8u, 9u, 255u, 256u, 257u})
        for (size_t g : {0u, 1u, 63u, 64u, 65u}) {
            const JournalLayout l = journal_layout(t, g);
            CHECK(l.tree.values == 0 && l.tree.index == t * 32 && l.tree.end >= l.tree.index + t * 4 && l.tree.end % 32 == 0);
            CHECK(l.planes.values == l.tree.end && l.planes.index == l.planes.values + 4 * g * 32 && l.planes.end >= l.planes.index + g * 4);
            CHECK(l.bytes == l.planes.end && l.bytes % 32 == 0 && l.bytes < (t + 4 * g) * 36 + 64);
        }
    CHECK(journal_grown_cap(0, 1) == 4096 && journal_grown_cap(4096, 4096) == 4096 && journal_grown_cap(4096, 4097) == 8192 && journal_grown_cap(0, 100000) == 131072);
}

// ---- the archive cut -------------------------------------------------------------------------------------------------------------------------
static void cut_cases() {
    const uint32_t none[1] = {0};
    CHECK(journal_archive_keep(none, 0, false, 0) == 0 && journal_archive_keep(none, 0, true, 9) == 0);
    const uint32_t one[1] = {5};
    CHECK(journal_archive_keep(one, 1, false, 0) == 0);   // kept after the mark, nothing kept then
    CHECK(journal_archive_keep(one, 1, true, 5) == 1);    // kept before
    CHECK(journal_archive_keep(one, 1, true, 4) == 0 && journal_archive_keep(one, 1, true, 6) == 1);
    const uint32_t many[5] = {1, 2, 4, 8, 0xFFFFFFFFu};
    CHECK(journal_archive_keep(many, 5, false, 0) == 0 && journal_archive_keep(many, 5, true, 0) == 0);
    CHECK(journal_archive_keep(many, 5, true, 1) == 1 && journal_archive_keep(many, 5, true, 3) == 2 && journal_archive_keep(many, 5, true, 4) == 3);
    CHECK(journal_archive_keep(many, 5, true, 0xFFFFFFFEu) == 4 && journal_archive_keep(many, 5, true, 0xFFFFFFFFu) == 5);
    // after an exit_forget from below: the record noted batch 2 as the highest kept, 1 and 2 are forgotten since -- 4 and 8 were kept later
    const uint32_t forgotten[2] = {4, 8};
    CHECK(journal_archive_keep(forgotten, 2, true, 2) == 0 && journal_archive_keep(forgotten, 2, true, 4) == 1 && journal_archive_keep(forgotten, 2, true, 9) == 2);
}

// ---- the shape -----------------------------------------------------------------------------------------------------------------------------
static const uint32_t N_SIB = 64;
typedef std::vector<uint64_t> Call;

static bool apply(SmtShape& sh, const Call& c, SmtShape::UndoLog* undo) {
    sh.begin();
    for (uint64_t key : c)
        if (sh.add(key, N_SIB) != SMT_PLAN_OK) {
            sh.rollback();
            return false;
        }
    if (undo)
        sh.commit_undo(*undo);
    else
        sh.commit();
    return true;
}

static SmtShape rebuilt(const std::vector<Call>& calls, size_t n) {
    SmtShape sh;
    sh.begin();
    for (size_t i = 0; i < n; i++) (void)apply(sh, calls[i], nullptr);
    return sh;
}

// field by field, and the per-call marks as a committed shape leaves them
static void same_shape(const SmtShape& a, const SmtShape& b) {
    CHECK(a.root == b.root);
    CHECK(a.child.size() == b.child.size() && a.child == b.child);
    CHECK(a.leaf_key.size() == b.leaf_key.size() && a.leaf_key == b.leaf_key);
    CHECK(a.node_ver == b.node_ver && a.leaf_op == b.leaf_op);
    CHECK(a.nodes0 == b.nodes0 && a.leaves0 == b.leaves0 && a.root_src == b.root_src && a.undo.empty() && a.touched_nodes.empty() && a.touched_leaves.empty());
}

static void shape_cases() {
    // call 0 is the load: 16 consecutive keys. Call 1 inserts keys that meet an existing leaf and push it deeper (256 + 2^10 shares ten low bits
    // with 256, 257 + 2^20 twenty with 257), a key below an internal node, and updates 258 twice and 260. Call 2 inserts beside call 1's new
    // leaves (another push), a far key, and updates old and new leaves. Call 3 only updates
    std::vector<Call> calls;
    Call load;
    for (uint64_t j = 0; j < 16; j++) load.push_back(256 + j);
    calls.push_back(load);
    calls.push_back({256 + (1ull << 10), 258, 257 + (1ull << 20), 272, 258, 260, 256 + (1ull << 10)});
    calls.push_back({256 + (1ull << 10) + (1ull << 30), 1000000007ull, 256, 257 + (1ull << 20), 273, (1ull << 47) + 256});
    calls.push_back({256, 258, 1000000007ull, 256 + (1ull << 10), 271, 256});
    SmtShape sh = rebuilt(calls, 1);
    same_shape(sh, rebuilt(calls, 1));
    SmtShape::UndoLog u[4];
    for (size_t i = 1; i <= 3; i++) CHECK(apply(sh, calls[i], &u[i]));
    same_shape(sh, rebuilt(calls, 4));
    CHECK(sh.nodes() > rebuilt(calls, 1).nodes() + 20);   // the pushes made nodes: the inserts did move leaves
    CHECK(u[3].undo.empty() && u[3].nodes0 == sh.nodes() && u[3].leaves0 == sh.leaves());   // a call that only updates changes no reference
    CHECK(!u[1].undo.empty() && !u[2].undo.empty());
    // three at once, newest first
    for (size_t i = 3; i >= 1; i--) sh.revert(u[i]);
    same_shape(sh, rebuilt(calls, 1));
    // and the reverted shape takes the calls again as the rebuilt one does
    for (size_t i = 1; i <= 3; i++) CHECK(apply(sh, calls[i], &u[i]));
    same_shape(sh, rebuilt(calls, 4));
    // one by one
    for (size_t i = 3; i >= 1; i--) {
        sh.revert(u[i]);
        same_shape(sh, rebuilt(calls, i));
    }
    // a different call on the reverted shape: what call 1 left behind is gone
    const Call other = {999, 256 + (1ull << 11), 258};
    std::vector<Call> alt = {calls[0], other};
    CHECK(apply(sh, other, &u[1]));
    same_shape(sh, rebuilt(alt, 2));
    sh.revert(u[1]);
    same_shape(sh, rebuilt(calls, 1));
    // a refused call in between keeps rollback()'s meaning
    sh.begin();
    CHECK(sh.add(300, N_SIB) == SMT_PLAN_OK && sh.add(1ull << 48, N_SIB) == SMT_PLAN_KEY);
    sh.rollback();
    same_shape(sh, rebuilt(calls, 1));
    // down to the empty tree
    SmtShape empty;
    empty.begin();
    SmtShape::UndoLog u0;
    CHECK(apply(empty, calls[0], &u0));
    same_shape(empty, rebuilt(calls, 1));
    empty.revert(u0);
    same_shape(empty, rebuilt(calls, 0));
    CHECK(empty.root == 0 && empty.nodes() == 0 && empty.leaves() == 0);
}

int main(int argc, char** argv) {
    const bool spoil = argc > 1 && strcmp(argv[1], "spoil") == 0;
    ring_cases(spoil);
    cut_cases();
    shape_cases();
    if (g_failed) {
        fprintf(stderr, "FAILED %d of %d checks\n", g_failed, g_checks);
        return 1;
    }
    fprintf(stderr, "ok checks=%d\n", g_checks);
    return 0;
}
