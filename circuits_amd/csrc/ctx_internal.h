// The context beside the public C ABI: struct hz_ctx itself, shared by ctx.hip (creation, inputs, check, reads, symbols) and
// ctx_step.hip (the kernel schedule of a step), and what export.hip (the witness in the compiler's variable order, on the device),
// ledger.hip and shard.hip need from a context: the geometry of the physical buffer and the context's own stream. Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/hermez_witness.h"
#include "../../include/hz_layout.h"
#include "hostutil.h"

namespace hz {
// section of the witness: virtual element v of instance i (v - vbase = sig * upi + unit) lives at physical element
// base + sig * n_units + i * upi + unit
struct SecMap { uint64_t vbase, base; uint32_t upi, n_units; };
struct CtxGeom {
    SecMap sec[4];
    uint32_t nsec = 0, n_inst = 0;
    uint64_t per_instance = 0, total = 0;
    int device = 0;
    hipStream_t s_main = nullptr;
    const void* wit = nullptr;
};
void ctx_geometry(const hz_ctx* c, CtxGeom& g);
// what ledger.hip (hz_ledger_main_inputs) asks of a context before it writes a packed input buffer for it: the template and its parameters
struct CtxShape {
    int tmpl = 0, n_tx = 0, n_levels = 0, max_l1 = 0, max_fee = 0, device = 0;
};
void ctx_shape(const hz_ctx* c, CtxShape& s);
// The export's scratch belongs to the CONTEXT, not to the map: two contexts that export through one map (each on its own stream) must
// not share the derived-value buffer or the staging vector of the host deliveries (a map's device plan holds tables only).
struct ExportScratch {
    DevBuf dval;              // derived values of the instances exported together: [instances][D] elements
    uint64_t dval_elems = 0;
    DevBuf xbuf;              // one exported vector, the source of a host delivery (released after deliveries above 64 MB)
};
ExportScratch* ctx_export_scratch(hz_ctx* c);

// The idle CU-masked streams of the process and the count of partitioned contexts alive per device (ctx.hip "masked-stream pool"):
// ONE pool, defined in ctx.hip; the schedule reads `alive` to choose the form of a flagged context's chain launch.
struct MaskedPool {
    std::mutex mu;
    std::vector<hipStream_t> idle[16][4];
    int alive[16] = {};   // partitioned contexts per device
};
MaskedPool& masked_pool();
}  // namespace hz

struct hz_ctx {
    // optional per-kernel timing (HIP events on the launch stream)
    bool profiling = false;
    // chain: the SMT chain of a k_smt launch (ctx_step.hip SmtChain: which skip counter of zm_skip it wrote), -1 for every other record
    struct Prof { std::string name; uint64_t bytes; uint64_t units; hipEvent_t e0, e1; float ms; int chain; };
    std::vector<Prof> prof;
    size_t prof_used = 0;
    hzl::Layout lo;
    int device = 0;
    hz::DevBuf wit, sc_tx, sc_fee, err, msg, chain, stage;
    hz::DevBuf ed_side;   // the small-launch signature ladder's parked numerators (eddsa_side_bytes), allocated by the first launch that needs it
    // per-instance failure report (hz_witness_failures): every instance's lowest failing key, kept by report_fail beside the
    // launch-wide minimum, and -- allocated by the first call that finds failures -- the operands of each
    hz::DevBuf inst_min, inst_rec;
    bool inst_min_dirty = false;          // a failure was seen (or no check told otherwise) since inst_min was last reset
    unsigned long long last_minkey = ~0ull;
    bool checked = false;                 // hz_witness_check has completed for the last enqueue
    std::vector<uint8_t> input_set;
    std::vector<uint8_t> host_stage;
    hipStream_t last_stream = nullptr;
    // multi-GPU intra-batch shard (RollupMain): this context evaluates transactions [sh_first, sh_first + sh_count);
    // only meaningful when `sharded`. The fee transactions and HashInputs of a sharded context run in hz_witness_enqueue_tail.
    uint32_t sh_first = 0, sh_count = 0;
    bool sharded = false;   // hz_ctx_set_shard with count >= 0 (an empty range is a legal shard: more ranks than transactions)
    bool sh_tail = true;
    // device-side input writes (hz_set_input_dev, hz_copy_instance_inputs, hz_inputs_upload) are asynchronous on the stream they were
    // given; the next enqueue waits for this event on ITS stream, whichever that is
    hipEvent_t ev_inputs = nullptr;
    bool inputs_pending = false;
    // bulk upload (hz_inputs_upload): one packed buffer per instance -> device staging -> k_unpack_inputs into the witness layout
    hz::DevBuf upl, upl_desc, upl_bad;
    uint64_t upl_bytes = 0;                 // packed bytes of one instance
    std::vector<uint64_t> upl_off;          // per input: byte offset inside the packed buffer
    uint32_t upl_blocks = 0;
    bool upl_used = false;                  // hz_witness_check also reads the range-check flag of the unpack kernel
    // hz_inputs_stage: the H2D half alone, ahead of time (while the previous step still computes on the old inputs); the unpack
    // kernels of the staged instances run at the head of the next enqueue
    std::vector<uint8_t> staged;
    bool any_staged = false;
    hipStream_t stage_stream = nullptr;     // the stream of the stage calls since the last enqueue (ev_staged is recorded on it)
    hipStream_t s_copy = nullptr;
    hipEvent_t ev_staged = nullptr, ev_unpacked = nullptr;
    // independent chains of one batch run concurrently: the EdDSA ladders and the fee transactions on
    // their own streams, joined by events before HashInputs (DESIGN.md "Kernel schedule"). The streams are set by hz_ctx_create and by
    // nobody after it: a step resolves which stream plays which role once per enqueue (ctx_step.hip StepStreams)
    bool exclusive = false;   // hz_ctx_set_profiling(ctx, 2)
    bool partitioned = false; // latency-bound context: CU-masked internal streams (hz_ctx_create)
    hipEvent_t ev_user_in = nullptr, ev_user_out = nullptr;
    hipStream_t s_ed = nullptr, s_fee = nullptr, s_main = nullptr;   // s_main replaces a NULL caller stream
    hipEvent_t ev_reset = nullptr, ev_front = nullptr, ev_ed = nullptr, ev_fee = nullptr, ev_fix = nullptr;
    hipEvent_t ev_sha[9] = {};   // HashInputs: chain group g done (0..7), expansion done (8)
    hipStream_t s_fix = nullptr;   // the fixed-base half of the signature check
    hipStream_t s_sha = nullptr;   // SHA-256 expansion groups behind the chain when HashInputs runs early on the fee stream
    // Constant marks. The witness buffer is persistent: what the previous step left in it is still there when the next one starts,
    // and more than a third of what a step of the headline shape used to store does not depend on its inputs -- the S-box block of
    // Poseidon(0, 0) in the hash slots of every SMT level above a proof's leaf (HZ_POSEIDON3_ZERO_WIT, 243 signals per level and
    // chain: 36.7 of 100 GB per step), zeros in the switcher / state-machine signals of those levels. k_smt keeps two bytes per
    // (chain, unit) -- from which level up the buffer holds that content -- stores an empty level only below the mark and leaves
    // the mark of what the buffer holds after the step (smt_kernels.hip). Nothing but k_smt writes those slots; the marks are cleared
    // (0xFF: "nothing held") at creation and by hz_clear_inputs. HZ_NO_ZMARK=1: no marks, every level stored every step.
    hz::DevBuf zm_tx, zm_fee;
    hz::DevBuf zm_skip;            // profiling: elements not stored by [0] the transaction launch, [1] the fee launch, [2] the early-tail launch
    bool zm_reset = false;         // hz_clear_inputs: the next enqueue clears the marks first
    hz::ExportScratch exp_scratch; // export.hip's per-context buffers
    hz::DevBuf smt_trace;          // experiments: HZ_SMT_TRACE=<file> -- per-wavefront start / end / placement of the transaction k_smt launch
    hz::DevBuf pos3;               // poseidon_quad.h's constants (C, M R, M R^2): the latency form of k_smt
    bool smt_lat = false;          // this context's chain launches take the latency form (hz_ctx_create)
    bool smt_lat_few = false;      // ... while at most two partitioned contexts are alive on the device (HZ_FLAG_LATENCY, one batch)
    hipEvent_t ev_hash4 = nullptr, ev_tail = nullptr, ev_sighash = nullptr;
    void release_masked();
    ~hz_ctx();
    unsigned long long filter_stage = ~0ull;
    bool enqueued = false;
    // symbol enumeration index: cumulative symbol counts per (section, block)
    struct BlkRef { int sec, blk; uint64_t first; uint32_t units; };
    std::vector<BlkRef> sym_index;
    uint64_t sym_total = 0;
    std::string sym_name;
};

namespace hz {
inline uint8_t* sec_ptr(hz_ctx* c, int sec) { return (uint8_t*)c->wit.p + c->lo.sections[sec].base * 32; }
// ctx.hip: the unpack kernels of the instances staged since the last enqueue (hz_inputs_stage), at the head of a step; records ev_unpacked on `s`
hz_status scatter_staged_inputs(hz_ctx* c, hipStream_t s);
// ctx_step.hip: one step on `stream`. filter != ~0: a second pass over the SAME inputs for the operands of failures the first pass
// found (hz_witness_check after an overflow of the record list; hz_witness_failures)
hz_status enqueue_impl(hz_ctx* c, void* stream, unsigned long long filter);
}  // namespace hz
