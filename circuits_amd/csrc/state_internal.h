// hz_state from the inside: the tree update of hz_state_apply for callers in this library whose leaf fields are already in device
// memory (ledger.hip). state.hip defines everything declared here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/hermez_witness.h"

namespace hz {

// device buffers of one apply, valid until the state's next call: the [M][4][32] records the update reads, and what it leaves behind
struct StateCallBufs {
    uint8_t* fields;      // in:  [M][4][32], written by the caller between prepare and launch, on the state's stream
    uint8_t* siblings;    // out: [M][n_sib][32]
    uint8_t* old_value;   // out: [M][32]
    uint8_t* old_root;    // out: [M][32], the root before update j
    uint8_t* new_root;    // out: [M][32], the root after update j (old_root + 32)
};

// idx[M] must lie inside the state and the state must be loaded (the callers check); 1 <= M <= 65536, k <= n_sib <= 64
hz_status state_apply_prepare(hz_state* st, uint32_t M, const uint64_t* idx, uint32_t n_sib, StateCallBufs* out);
// Undo for an owner that journals its applies (ledger.hip). A prepared call tells how many resident elements its write-back
// will replace -- the touched level nodes, then the touched state hashes, each once --; the owner gives room for them -- n 32-byte elements
// and n uint32 entries (1 << 29 | account for a state hash, else the node's element in the level buffer) -- and the launch saves them there,
// between the level kernels and the write-back, under `span`
struct DevSpan;
struct StateJournalDst {
    uint8_t* values;
    uint32_t* index;
    DevSpan* span;
};
hz_status state_journal_entries(hz_state* st, uint32_t M, size_t* n);
hz_status state_apply_launch(hz_state* st, uint32_t M, uint32_t n_sib, bool clear_siblings, const StateJournalDst* journal = nullptr);
hz_status state_apply_finish(hz_state* st);   // synchronises and records the device time of the launch
// the call that left (values, index) did not happen: the n saved elements back into levels and state hashes, on the state's stream, no synchronise
hz_status state_journal_restore(hz_state* st, const uint8_t* values, const uint32_t* index, size_t n);
hipStream_t state_stream(const hz_state* st);
const uint8_t* state_root_dev(const hz_state* st);
bool state_loaded(const hz_state* st);

}  // namespace hz
