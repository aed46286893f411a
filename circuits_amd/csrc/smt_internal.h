// hz_smt from the inside: the ordered inserts and updates of hz_smt_apply for callers in this library whose leaf fields are already in
// device memory (ledger.hip's exit tree). The counterpart of state_internal.h; smt_tree.hip defines everything declared here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/hermez_witness.h"
#include "smt_plan.h"

namespace hz {

// device buffers of one apply, valid until the tree's next call: the [M][4][32] records the update reads, and what it leaves behind
struct SmtCallBufs {
    uint8_t* fields;      // in:  [M][4][32], written by the caller between prepare and launch; the launch must be ordered behind that write
    uint8_t* siblings;    // out: [M][n_sib][32], zero-padded (NULL when the caller asked for none)
    uint8_t* roots;       // out: [M + 1][32], the root before operation j (so [j + 1]: after it)
    uint8_t* old_value;   // out: [M][32]
    // the planner's integers of the M operations, the host's: valid until finish / abort
    const uint64_t* old_key;
    const uint8_t *is_old0, *fnc;
};

// Plans the M keys on the host (SmtShape::add), grows pools and buffers, and queues the upload of the call's integer tables on the
// tree's stream. A key the planner refuses leaves the tree as it was: HZ_ERR_INPUT, or depth_status for a leaf at depth >= n_sib.
// The tree must be usable and 1 <= M <= 65536, 1 <= n_sib <= n_sib_max (the callers check).
hz_status smt_apply_prepare(hz_smt* t, const char* who, hz_status depth_status, uint32_t M, const uint64_t* key, uint32_t n_sib, bool want_siblings, SmtCallBufs* out);
// Undo for an owner that journals its applies (ledger.hip). A prepared call tells how many resident pool entries its
// write-back will replace (entries at or above the pools' old counts are new and are not counted); the owner gives room for them -- n
// 32-byte elements and n uint32 entries, pool kind << 29 | index -- and the launch saves them there, between the level kernels and the
// write-back, under `span`. Entries, never addresses: a pool reallocated later does not matter
struct DevSpan;
struct SmtJournalDst {
    uint8_t* values;
    uint32_t* index;
    DevSpan* span;
};
hz_status smt_journal_entries(hz_smt* t, size_t* n);
// the kernels, on the tree's stream: leaf, one level launch per depth, gather, (the journal's save,) write-back
hz_status smt_apply_launch(hz_smt* t, uint32_t M, uint32_t n_sib, bool want_siblings, const SmtJournalDst* journal = nullptr);
// synchronises the tree's stream, records the device time of the launch and lets the call stand; undo: what it changed of the shape
hz_status smt_apply_finish(hz_smt* t, SmtShape::UndoLog* undo = nullptr);
// the call that left (values, index, undo) did not happen: the n saved elements back into the pools on the tree's stream -- no
// synchronise --, the shape reverted at once. Every later call has been restored already
hz_status smt_journal_restore(hz_smt* t, const uint8_t* values, const uint32_t* index, size_t n, const SmtShape::UndoLog& undo);
// the prepared call did not happen, or failed: nothing stays in flight, the shape is rolled back; after a queued write-back the tree
// is poisoned (hz_smt_apply's rule)
void smt_apply_abort(hz_smt* t);
// the empty tree again without a synchronise: for an owner whose every call on the tree ended in finish or abort
void smt_clear(hz_smt* t);
hipStream_t smt_stream(const hz_smt* t);
// the tree as it stands, read-only, for an owner that freezes it (ledger_archive.h): the shape's integers on the host, the digest pools
// on the device. Valid until the tree's next call; nothing may be in flight on the tree's stream
struct SmtView {
    int32_t root;                // 0 empty, n + 1 node n, -(l + 1) leaf l
    size_t nodes, leaves;
    const int32_t* child;        // host, [2 * nodes]
    const uint64_t* leaf_key;    // host, [leaves]
    const uint8_t* node_digest;  // device, [nodes][32]
    const uint8_t* leaf_hash;    // device, [leaves][32]
};
SmtView smt_view(const hz_smt* t);
// a call failed on the device behind its queued write-back: every public call answers HZ_ERR_HIP until hz_smt_reset
bool smt_poisoned(const hz_smt* t);

}  // namespace hz
