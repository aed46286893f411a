// hz_ledger's undo journal: the bookkeeping of the ring of undo records -- push and evict, which records a mark undoes and
// in what order, the argument verdicts and their messages, the cut of the exit archive, the byte layout of a record. No HIP, integers only:
// ledger.hip keeps the bytes in device slabs and runs the kernels, tests/native/ledger_journal_check.cpp drives everything here on the host
// under the address and undefined-behaviour sanitizers.
//
// A mark is the number of successful apply calls since the ledger's last load. The record of the apply that took the ledger from mark a to
// a + 1 carries `a`; the ring holds the records of the last `depth` applies in depth + 1 slots, each slot a slab of device memory of one
// common capacity: one slot is always free, so an apply writes its record beside the `depth` held and the oldest goes only once the apply
// stands. Rolling back to `mark` undoes the records that carry mark .. applied - 1, newest first.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../../include/hermez_witness.h"
#if defined(__HIPCC__)
#include "hostutil.h"   // set_err
#endif

namespace hz {

#if !defined(__HIPCC__)
hz_status set_err(hz_status st, const char* fmt, ...);   // hostutil.h's, which needs HIP: the host check defines its own
#endif

// ---- the byte layout of a record in its slab -------------------------------------------------------------------------------------------
// Two parts behind each other, the state tree's and the planes': each the saved 32-byte elements, then the uint32 entries that name where
// they belong (a tree entry: the pool or level array in the top three bits, the element's index there below; a plane entry: the account),
// rounded up to 32 bytes so that every element stays aligned for 16-byte accesses. A plane part of G accounts saves 4 G elements -- plane f
// of group g at element f * G + g -- under G entries.
struct JournalPart {
    size_t values = 0, index = 0, end = 0;   // byte offsets in the slab: the elements, the entries, the first byte behind the part
};
inline size_t journal_round32(size_t n) { return (n + 31) & ~(size_t)31; }
inline JournalPart journal_part(size_t at, size_t n_values, size_t n_index) {
    JournalPart p;
    p.values = at;
    p.index = at + n_values * 32;
    p.end = p.index + journal_round32(n_index * 4);
    return p;
}
struct JournalLayout {
    JournalPart tree, planes;
    size_t bytes = 0;
};
inline JournalLayout journal_layout(size_t tree_entries, size_t groups) {
    JournalLayout l;
    l.tree = journal_part(0, tree_entries, tree_entries);
    l.planes = journal_part(l.tree.end, 4 * groups, groups);
    l.bytes = l.planes.end;
    return l;
}

// ---- the ring ------------------------------------------------------------------------------------------------------------------------------
// what the ledger notes of an apply besides the device bytes. The tree's own host part (an hz_smt's shape undo) is the owner's, kept per
// `slot` (JournalRing knows no tree type)
struct JournalRecord {
    uint64_t mark = 0;          // `applied` when the apply began
    uint64_t live = 0;          // accounts then
    bool has_kept = false;      // the archive cut: was any batch kept when the apply began,
    uint32_t last_kept = 0;     // and the highest kept batch_num
    uint32_t slot = 0;          // the slab that holds its bytes
    size_t tree_entries = 0, groups = 0;
    size_t bytes = 0;
};

struct JournalRing {
    uint32_t depth = 0;
    std::vector<JournalRecord> rec;   // oldest first, at most depth
    std::vector<uint8_t> slot_used;   // [slots()]

    uint32_t slots() const { return depth ? depth + 1 : 0; }
    void set_depth(uint32_t d) {
        depth = d;
        rec.clear();
        slot_used.assign(slots(), 0);
    }
    void clear() {
        rec.clear();
        slot_used.assign(slots(), 0);
    }
    size_t records() const { return rec.size(); }
    uint64_t oldest_mark(uint64_t applied) const { return rec.empty() ? applied : rec.front().mark; }
    size_t bytes_used() const {
        size_t n = 0;
        for (const JournalRecord& r : rec) n += r.bytes;
        return n;
    }
    // the ring is full: the oldest record goes, its slot is free. Nothing happens otherwise
    void evict_if_full() {
        if (depth == 0 || rec.size() < depth) return;
        slot_used[rec.front().slot] = 0;
        rec.erase(rec.begin());
    }
    // a free slot for the next record: there always is one while at most `depth` records are held (-1: the journal is off)
    int32_t free_slot() const {
        for (uint32_t s = 0; s < slots(); s++)
            if (!slot_used[s]) return (int32_t)s;
        return -1;
    }
    // the apply stands: its record, written into a free slot, joins the ring, and the oldest goes where that makes depth + 1
    void push(const JournalRecord& r) {
        evict_if_full();
        slot_used[r.slot] = 1;
        rec.push_back(r);
    }
    // rolling back to `mark`: how many records go, from the back of `rec` (newest first): rec.size() - 1 down to rec.size() - n
    size_t undone_by(uint64_t mark) const {
        size_t n = 0;
        while (n < rec.size() && rec[rec.size() - 1 - n].mark >= mark) n++;
        return n;
    }
    void pop_newest() {
        slot_used[rec.back().slot] = 0;
        rec.pop_back();
    }
};

// ---- the argument verdicts ---------------------------------------------------------------------------------------------------------------
#define HZ_JOURNAL_OK 0
#define HZ_JOURNAL_FUTURE 1   // mark > applied
#define HZ_JOURNAL_GONE 2     // mark < applied - records: the journal is off, or the ring has moved on
inline int journal_mark_verdict(uint64_t applied, size_t records, uint64_t mark) {
    if (mark > applied) return HZ_JOURNAL_FUTURE;
    if (applied - mark > (uint64_t)records) return HZ_JOURNAL_GONE;
    return HZ_JOURNAL_OK;
}

inline hz_status journal_check_depth(const char* who, uint32_t depth) {
    return depth > HZ_LEDGER_JOURNAL_MAX ? set_err(HZ_ERR_ARG, "%s: depth = %u (0 .. %u)", who, depth, (unsigned)HZ_LEDGER_JOURNAL_MAX) : HZ_OK;
}

// the message names both numbers
inline hz_status journal_check_mark(const char* who, uint64_t applied, uint32_t depth, size_t records, uint64_t mark) {
    const int v = journal_mark_verdict(applied, records, mark);
    if (v == HZ_JOURNAL_FUTURE)
        return set_err(HZ_ERR_ARG, "%s: mark = %llu lies ahead of the ledger (applied = %llu)", who, (unsigned long long)mark, (unsigned long long)applied);
    if (v == HZ_JOURNAL_GONE) {
        if (depth == 0)
            return set_err(HZ_ERR_ARG, "%s: mark = %llu, applied = %llu, and the journal is off (hz_ledger_journal)", who, (unsigned long long)mark,
                           (unsigned long long)applied);
        return set_err(HZ_ERR_ARG, "%s: mark = %llu is older than the journal reaches: applied = %llu, %zu records of depth %u (oldest mark %llu)", who,
                       (unsigned long long)mark, (unsigned long long)applied, records, depth, (unsigned long long)(applied - records));
    }
    return HZ_OK;
}

// ---- the archive cut -----------------------------------------------------------------------------------------------------------------------
// kept[n]: the kept batch numbers, ascending (what hz_ledger_exit_forget left of them). The snapshots that stay when the oldest undone
// record noted (has_kept, last_kept): those kept before its apply began -- batch_num <= last_kept, none where nothing was kept then
inline size_t journal_archive_keep(const uint32_t* kept, size_t n, bool has_kept, uint32_t last_kept) {
    if (!has_kept) return 0;
    size_t stay = 0;
    while (stay < n && kept[stay] <= last_kept) stay++;
    return stay;
}

// the slabs' common capacity once a record of `need` bytes has to fit: doubled, at least 4 KiB
inline size_t journal_grown_cap(size_t cap, size_t need) {
    size_t c = cap ? cap : 4096;
    while (c < need) c *= 2;
    return c;
}

}  // namespace hz
