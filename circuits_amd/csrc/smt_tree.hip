// hz_smt: a circomlib sparse Merkle tree resident in HBM that accepts INSERTS as well as updates -- the exit tree of a batch, the state
// tree under create-account deposits. hz_state (state.hip) keeps a perfect tree of 2^k consecutive keys in level arrays; here the shape
// changes with every insert, so the digests live in POOLS (internal nodes, leaf hashes, leaf values: 32 B each, grown on demand) and
// the host owns the shape (smt_plan.h: which slot is which pool entry). No field arithmetic and no hash on the host.
//
// Ordered operations keep hz_state_apply's NODE VERSIONS: operation j makes version j of the internal slots on its path (depths
// 0 .. D_j - 1, D_j the depth of its leaf) and leaf hash j. The planner compacts, per depth d, the operations with D_j > d and tells
// every hash where its two inputs lie as (kind, index) -- this call's leaf hashes or versions, the resident pools, or zero. The
// dependent device work is max D + 2 launches whatever m is: leaf (state hash + leaf hash), one level launch per depth from max D - 1
// down to 0, write-back; one gather launch (roots and old values, read before the write-back replaces them) rides between.
// Buffers and block offsets are hostutil.h's, stream, timing and the constants' upload resident.h's, the hashes state_dev.h's: state.hip's.
#define HZ_FR_INLINE 1
#include <hip/hip_runtime.h>
#include <memory>
#include <vector>
#include "../../include/hermez_witness.h"
#include "devcommon.h"
#include "resident.h"
#include "smt_internal.h"
#include "smt_plan.h"
#include "state_dev.h"

#define HZ_SMT_MAX_M 65536u
#define HZ_SMT_MAX_PROOFS ((size_t)1 << 20)

namespace hz {

// ---- kernels ------------------------------------------------------------------------------------------------------------------------
// the element a source names; `bases` is the table of the SMT_KINDS buffers in device memory (an index into a kernel argument would
// make the compiler keep the table in private memory)
__device__ __forceinline__ Fc smt_load(const uint8_t* const* __restrict__ bases, uint32_t src) {
    Fc r = fc_zero();
    const uint32_t kind = src >> 29;
    if (kind != SMT_ZERO) r = load_fr(bases[kind] + (size_t)(src & 0x1FFFFFFFu) * 32);
    return r;
}

// leaf: value j = state hash of operation j's fields, leaf hash j = SMTHash1(key j, value j)
__global__ __launch_bounds__(64) void k_smt_leaf(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ fields, uint8_t* __restrict__ lv,
                                                 uint8_t* __restrict__ lh, uint32_t m) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const Fc v = state_value_hash(fields + (size_t)j * 128, 1);
    store_fr(lv + (size_t)j * 32, v);
    store_fr(lh + (size_t)j * 32, state_leaf_hash(keys[j], v));
}

// level: hash e of this depth's list, a quad of lanes each; ver_out is this depth's part of the version buffer. Where the other child
// is a sibling of the operation's proof it goes to sib_out (NULL: nobody asked for siblings).
__global__ __launch_bounds__(64) void k_smt_level(const SmtLevelOp* __restrict__ ops, const uint8_t* const* __restrict__ bases, uint8_t* __restrict__ ver_out,
                                                  uint8_t* __restrict__ sib_out, const Fr* __restrict__ pos3, uint32_t n_sib, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t e = t >> 2;
    if (e >= n) return;   // (whole quads leave together)
    const SmtLevelOp op = ops[e];
    const Fc sib = smt_load(bases, op.other);
    const Fr h = state_level_hash(smt_load(bases, op.own), sib, op.meta >> 31, pos3, t & 3u);
    if ((t & 3u) == 0) {
        if (sib_out && (op.meta >> 30 & 1u)) store_fr(sib_out + ((size_t)(op.meta & 0xFFFFu) * n_sib + (op.meta >> 16 & 63u)) * 32, sib);
        store_fr(ver_out + (size_t)e * 32, fr_to_canon(h));
    }
}

// gather: out[dst] = the element src names (roots and old values of a call; siblings and values of proofs)
struct SmtCopy { uint32_t src, dst; };
__global__ __launch_bounds__(256) void k_smt_gather(const SmtCopy* __restrict__ list, const uint8_t* const* __restrict__ bases, uint8_t* __restrict__ out, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const SmtCopy c = list[t];
    store_fr(out + (size_t)c.dst * 32, smt_load(bases, c.src));
}

// write-back: the last version of every touched node, the last leaf hash and value of every touched key, into the pools; dst is a
// source too (SMT_NODE / SMT_LEAF / SMT_VALUE), every destination appears once
__global__ __launch_bounds__(256) void k_smt_writeback(const SmtCopy* __restrict__ list, const uint8_t* const* __restrict__ bases, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const SmtCopy c = list[t];
    store_fr(const_cast<uint8_t*>(bases[c.dst >> 29]) + (size_t)(c.dst & 0x1FFFFFFFu) * 32, smt_load(bases, c.src));
}

// the undo journal of an owner (smt_internal.h): a lane per 32-byte element, moved as 16-byte accesses, consecutive lanes on consecutive
// journal addresses; the entry names the pool (SMT_NODE / SMT_LEAF / SMT_VALUE) and the element's index there
template <class T>   // uint8_t to restore, const uint8_t to save
__device__ __forceinline__ T* smt_journal_at(uint32_t e, T* node, T* leaf, T* value) {
    const uint32_t kind = e >> 29;
    T* pool = kind == SMT_NODE ? node : kind == SMT_LEAF ? leaf : value;
    return pool + (size_t)(e & 0x1FFFFFFFu) * 32;
}
__global__ __launch_bounds__(256) void k_smt_journal_save(const uint32_t* __restrict__ index, const uint8_t* node, const uint8_t* leaf, const uint8_t* value,
                                                          uint8_t* __restrict__ out, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    store_fr(out + (size_t)t * 32, load_fr(smt_journal_at(index[t], node, leaf, value)));
}
// the write-back run the other way: every destination appears once in a record
__global__ __launch_bounds__(256) void k_smt_journal_restore(const uint32_t* __restrict__ index, const uint8_t* __restrict__ saved, uint8_t* node, uint8_t* leaf,
                                                             uint8_t* value, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    store_fr(smt_journal_at(index[t], node, leaf, value), load_fr(saved + (size_t)t * 32));
}

}  // namespace hz

using namespace hz;

struct hz_smt {
    uint32_t n_sib_max = 0;
    SmtShape shape;
    DevBuf node, leaf, value, pos3;                      // resident pools, the quad form's constants
    DevBuf fields, lv, lh, ver, out, sib, ints;          // per call, grown on demand
    PinnedBuf h_ints, h_journal;                         // h_journal: the entries of a journalled call, made only for an owner that asks
    size_t n_journal = 0;
    std::vector<SmtCopy> copies;
    Resident r;               // device, stream, device time of the last apply
    bool wb_queued = false;   // the call in progress has queued its write-back: the pools may have changed
    bool poisoned = false;    // a call failed after that point: shape and pools may disagree until hz_smt_reset
    // the prepared call (smt_internal.h): where its tables lie in the integer block
    size_t o_keys = 0, o_ops = 0, o_gather = 0, o_wb = 0, n_gather = 0, n_wb = 0;
    uint32_t first[HZ_SMT_MAX_DEPTH] = {};
};

// a pool that holds `used` entries gets room for `want`: a larger buffer and a device-to-device copy
static hz_status smt_pool(hz_smt* t, DevBuf& pool, size_t used, size_t want) {
    if (want * 32 <= pool.bytes) return HZ_OK;
    size_t cap = pool.bytes ? pool.bytes : (size_t)4096 * 32;
    while (cap < want * 32) cap *= 2;
    DevBuf grown;
    HZ_HIP(grown.alloc(cap));
    if (used) HZ_HIP(hipMemcpyAsync(grown.p, pool.p, used * 32, hipMemcpyDeviceToDevice, t->r.s));
    HZ_HIP(hipStreamSynchronize(t->r.s));
    pool.release();
    pool.p = grown.p;
    pool.bytes = grown.bytes;
    grown.p = nullptr;
    grown.bytes = 0;
    return HZ_OK;
}

// the kinds' buffers as the kernels index them
static void smt_bases(const hz_smt* t, const void** b) {
    b[SMT_ZERO] = nullptr;
    b[SMT_CALL_LH] = t->lh.p;
    b[SMT_LEAF] = t->leaf.p;
    b[SMT_VER] = t->ver.p;
    b[SMT_NODE] = t->node.p;
    b[SMT_CALL_LV] = t->lv.p;
    b[SMT_VALUE] = t->value.p;
    b[7] = nullptr;
}

static hz_status smt_n_sib(const hz_smt* t, const char* who, size_t n_sib) {
    if (n_sib < 1 || n_sib > HZ_SMT_MAX_DEPTH || n_sib > t->n_sib_max)
        return set_err(HZ_ERR_ARG, "%s: n_sib = %zu (1 .. %u, the tree's n_sib_max)", who, n_sib, t->n_sib_max);
    return HZ_OK;
}

static hz_status smt_usable(const hz_smt* t, const char* who) {
    if (!t) return set_err(HZ_ERR_ARG, "%s: null tree", who);
    if (t->poisoned) return set_err(HZ_ERR_HIP, "%s: an earlier call failed on the device after its write-back was queued; hz_smt_reset makes the tree usable again", who);
    return HZ_OK;
}

static hz_status smt_plan_err(const char* who, SmtPlanError e, size_t j, uint64_t key, size_t n_sib, hz_status depth_status = HZ_ERR_INPUT) {
    if (e == SMT_PLAN_KEY) return set_err(HZ_ERR_INPUT, "%s: key[%zu] = %llu >= 2^48 (the circuits' idx has 48 bits)", who, j, (unsigned long long)key);
    if (e == SMT_PLAN_DEPTH)
        return set_err(depth_status, "%s: op %zu (key %llu) would have its leaf at depth >= n_sib = %zu: SMTProcessor(%zu) cannot express it", who, j,
                       (unsigned long long)key, n_sib, n_sib);
    return set_err(HZ_ERR_ARG, "%s: op %zu: the tree is full (2^28 keys)", who, j);
}

extern "C" hz_status hz_smt_create(int32_t device, int32_t n_sib_max, hz_smt** out) {
    if (!out) return set_err(HZ_ERR_ARG, "hz_smt_create: null argument");
    *out = nullptr;
    if (n_sib_max < 1 || n_sib_max > HZ_SMT_MAX_DEPTH) return set_err(HZ_ERR_ARG, "hz_smt_create: n_sib_max = %d (1 .. %d)", n_sib_max, HZ_SMT_MAX_DEPTH);
    std::unique_ptr<hz_smt> t(new hz_smt);
    if (hz_status e = t->r.open("hz_smt_create", device)) return e;
    t->n_sib_max = (uint32_t)n_sib_max;
    t->shape.begin();
    if (hz_status e = pos3_dense_create(t->pos3)) return e;
    *out = t.release();
    return HZ_OK;
}

extern "C" void hz_smt_destroy(hz_smt* t) {
    if (!t) return;
    (void)hipSetDevice(t->r.device);
    if (t->r.s) (void)hipStreamSynchronize(t->r.s);
    delete t;
}

extern "C" hz_status hz_smt_reset(hz_smt* t) {
    if (!t) return set_err(HZ_ERR_ARG, "hz_smt_reset: null tree");
    (void)hipSetDevice(t->r.device);
    if (t->r.s) (void)hipStreamSynchronize(t->r.s);
    t->shape.clear();
    t->poisoned = false;
    return HZ_OK;
}

extern "C" uint64_t hz_smt_size(const hz_smt* t) { return t ? t->shape.leaves() : 0; }

extern "C" double hz_smt_device_ms(const hz_smt* t) { return t ? t->r.device_ms : 0.0; }

extern "C" hz_status hz_smt_root(hz_smt* t, uint8_t* out32) {
    if (hz_status e = smt_usable(t, "hz_smt_root")) return e;
    if (!out32) return set_err(HZ_ERR_ARG, "hz_smt_root: null argument");
    const uint32_t src = t->shape.hash_src(t->shape.root);
    if (src >> 29 == SMT_ZERO) {
        for (int i = 0; i < 32; i++) out32[i] = 0;
        return HZ_OK;
    }
    HZ_HIP(hipSetDevice(t->r.device));
    const uint8_t* pool = (const uint8_t*)(src >> 29 == SMT_LEAF ? t->leaf.p : t->node.p);
    HZ_HIP(hipMemcpyAsync(out32, pool + (size_t)(src & 0x1FFFFFFFu) * 32, 32, hipMemcpyDeviceToHost, t->r.s));
    HZ_HIP(hipStreamSynchronize(t->r.s));
    return HZ_OK;
}

// ---- one apply in three steps (smt_internal.h): hz_smt_apply below, and the ledger's exit tree ---------------------------------------------
hz_status hz::smt_apply_prepare(hz_smt* t, const char* who, hz_status depth_status, uint32_t M, const uint64_t* key, uint32_t n_sib, bool want_siblings,
                                SmtCallBufs* bufs) {
    SmtShape& sh = t->shape;
    sh.begin();
    for (uint32_t j = 0; j < M; j++)
        if (const SmtPlanError e = sh.add(key[j], n_sib)) {
            sh.rollback();
            return smt_plan_err(who, e, j, key[j], n_sib, depth_status);
        }
    t->wb_queued = false;
    const hz_status st = [&]() -> hz_status {
        HZ_HIP(hipSetDevice(t->r.device));
        if (hz_status e = smt_pool(t, t->node, sh.nodes0, sh.nodes())) return e;
        if (hz_status e = smt_pool(t, t->leaf, sh.leaves0, sh.leaves())) return e;
        if (hz_status e = smt_pool(t, t->value, sh.leaves0, sh.leaves())) return e;
        uint32_t* first = t->first;
        sh.firsts(first);
        const size_t V = sh.versions();
        // what the gather reads: roots [m + 1] | old values [m]; what the write-back scatters
        const size_t G = (size_t)2 * M + 1, W = sh.touched_nodes.size() + 2 * sh.touched_leaves.size();
        // the integer tables of the call, one pinned block: bases [8] (at offset 0) | keys u64[m] | level ops [V] | gather list [G] | write-back list [W]
        Carve c;
        c.take(64);
        const size_t o_keys = c.take((size_t)M * 8), o_ops = c.take(V * sizeof(SmtLevelOp)), o_gather = c.take(G * sizeof(SmtCopy)), o_wb = c.take(W * sizeof(SmtCopy));
        const size_t ints_bytes = c.end;
        t->o_keys = o_keys, t->o_ops = o_ops, t->o_gather = o_gather, t->o_wb = o_wb, t->n_gather = G, t->n_wb = W;
        HZ_HIP(t->h_ints.grow(ints_bytes));
        HZ_HIP(t->ints.grow(ints_bytes));
        HZ_HIP(t->fields.grow((size_t)M * 128));
        HZ_HIP(t->lv.grow((size_t)M * 32));
        HZ_HIP(t->lh.grow((size_t)M * 32));
        HZ_HIP(t->ver.grow((V + 1) * 32));
        HZ_HIP(t->out.grow(G * 32));
        if (want_siblings) HZ_HIP(t->sib.grow((size_t)M * n_sib * 32));
        uint8_t* hb = (uint8_t*)t->h_ints.p;
        smt_bases(t, (const void**)hb);
        uint64_t* h_keys = (uint64_t*)(hb + o_keys);
        for (uint32_t j = 0; j < M; j++) h_keys[j] = key[j];
        SmtLevelOp* h_ops = (SmtLevelOp*)(hb + o_ops);
        for (uint32_t d = 0; d < sh.max_depth; d++)
            for (size_t i = 0; i < sh.level[d].size(); i++) {
                const SmtLevelOp& o = sh.level[d][i];
                h_ops[first[d] + i] = {sh.flat_src(o.own, first), sh.flat_src(o.other, first), o.meta};
            }
        SmtCopy* h_gather = (SmtCopy*)(hb + o_gather);
        for (uint32_t j = 0; j <= M; j++) h_gather[j] = {sh.flat_src(sh.root_src[j], first), j};
        for (uint32_t j = 0; j < M; j++) h_gather[M + 1 + j] = {sh.old_value_src[j], M + 1 + j};
        SmtCopy* h_wb = (SmtCopy*)(hb + o_wb);
        size_t w = 0;
        for (uint32_t n : sh.touched_nodes) h_wb[w++] = {smt_src(SMT_VER, sh.global_ver((uint32_t)sh.node_ver[n], first)), smt_src(SMT_NODE, n)};
        for (uint32_t l : sh.touched_leaves) {
            h_wb[w++] = {smt_src(SMT_CALL_LH, (uint32_t)sh.leaf_op[l]), smt_src(SMT_LEAF, l)};
            h_wb[w++] = {smt_src(SMT_CALL_LV, (uint32_t)sh.leaf_op[l]), smt_src(SMT_VALUE, l)};
        }
        HZ_HIP(hipMemcpyAsync(t->ints.p, t->h_ints.p, ints_bytes, hipMemcpyHostToDevice, t->r.s));
        return HZ_OK;
    }();
    if (st) {
        smt_apply_abort(t);
        return st;
    }
    bufs->fields = (uint8_t*)t->fields.p;
    bufs->siblings = want_siblings ? (uint8_t*)t->sib.p : nullptr;
    bufs->roots = (uint8_t*)t->out.p;
    bufs->old_value = (uint8_t*)t->out.p + ((size_t)M + 1) * 32;
    bufs->old_key = sh.old_key.data();
    bufs->is_old0 = sh.is_old0.data();
    bufs->fnc = sh.fnc.data();
    return HZ_OK;
}

// the resident entries the prepared call's write-back replaces, into the pinned entry list
hz_status hz::smt_journal_entries(hz_smt* t, size_t* n_out) {
    const SmtShape& sh = t->shape;
    t->n_journal = 0;
    size_t n = 0;
    for (uint32_t x : sh.touched_nodes) n += x < sh.nodes0;
    for (uint32_t l : sh.touched_leaves) n += l < sh.leaves0 ? 2 : 0;
    *n_out = n;
    if (n == 0) return HZ_OK;
    HZ_HIP(t->h_journal.grow(n * 4));
    uint32_t* h = (uint32_t*)t->h_journal.p;
    size_t w = 0;
    for (uint32_t x : sh.touched_nodes)
        if (x < sh.nodes0) h[w++] = smt_src(SMT_NODE, x);
    for (uint32_t l : sh.touched_leaves)
        if (l < sh.leaves0) {
            h[w++] = smt_src(SMT_LEAF, l);
            h[w++] = smt_src(SMT_VALUE, l);
        }
    t->n_journal = n;
    return HZ_OK;
}

hz_status hz::smt_apply_launch(hz_smt* t, uint32_t M, uint32_t n_sib, bool want_siblings, const SmtJournalDst* journal) {
    const SmtShape& sh = t->shape;
    const uint32_t* first = t->first;
    const size_t G = t->n_gather, W = t->n_wb;
    HZ_HIP(hipSetDevice(t->r.device));
    const uint8_t* db = (const uint8_t*)t->ints.p;
    const uint8_t* const* d_bases = (const uint8_t* const*)db;
    hipStream_t s = t->r.s;
    if (want_siblings) HZ_HIP(hipMemsetAsync(t->sib.p, 0, (size_t)M * n_sib * 32, s));
    HZ_HIP(t->r.begin());
    hipLaunchKernelGGL(k_smt_leaf, dim3((M + 63) / 64), dim3(64), 0, s, (const uint64_t*)(db + t->o_keys), (const uint8_t*)t->fields.p, (uint8_t*)t->lv.p, (uint8_t*)t->lh.p, M);
    HZ_HIP(hipGetLastError());
    for (uint32_t d = sh.max_depth; d-- > 0;) {
        const uint32_t n = (uint32_t)sh.level[d].size();
        hipLaunchKernelGGL(k_smt_level, dim3((4 * n + 63) / 64), dim3(64), 0, s, (const SmtLevelOp*)(db + t->o_ops) + first[d], d_bases,
                           (uint8_t*)t->ver.p + (size_t)first[d] * 32, want_siblings ? (uint8_t*)t->sib.p : (uint8_t*)nullptr, (const Fr*)t->pos3.p, n_sib, n);
        HZ_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_smt_gather, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s, (const SmtCopy*)(db + t->o_gather), d_bases, (uint8_t*)t->out.p, (uint32_t)G);
    HZ_HIP(hipGetLastError());
    if (journal && t->n_journal) {   // what the write-back is about to replace
        const uint32_t n = (uint32_t)t->n_journal;
        HZ_HIP(hipMemcpyAsync(journal->index, t->h_journal.p, (size_t)n * 4, hipMemcpyHostToDevice, s));
        HZ_HIP(journal->span->begin(s));
        hipLaunchKernelGGL(k_smt_journal_save, dim3((n + 255) / 256), dim3(256), 0, s, (const uint32_t*)journal->index, (const uint8_t*)t->node.p, (const uint8_t*)t->leaf.p,
                           (const uint8_t*)t->value.p, journal->values, n);
        HZ_HIP(hipGetLastError());
        HZ_HIP(journal->span->end(s));
    }
    t->wb_queued = true;
    hipLaunchKernelGGL(k_smt_writeback, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, s, (const SmtCopy*)(db + t->o_wb), d_bases, (uint32_t)W);
    HZ_HIP(hipGetLastError());
    HZ_HIP(t->r.end());
    return HZ_OK;
}

hz_status hz::smt_apply_finish(hz_smt* t, SmtShape::UndoLog* undo) {
    if (hz_status e = t->r.finish()) return e;
    if (undo)
        t->shape.commit_undo(*undo);
    else
        t->shape.commit();
    return HZ_OK;
}

hz_status hz::smt_journal_restore(hz_smt* t, const uint8_t* values, const uint32_t* index, size_t n, const SmtShape::UndoLog& undo) {
    HZ_HIP(hipSetDevice(t->r.device));
    if (n) {
        hipLaunchKernelGGL(k_smt_journal_restore, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, t->r.s, index, values, (uint8_t*)t->node.p, (uint8_t*)t->leaf.p,
                           (uint8_t*)t->value.p, (uint32_t)n);
        HZ_HIP(hipGetLastError());
    }
    t->shape.revert(undo);
    return HZ_OK;
}

// nothing of the call stays in flight (its copies read the pinned block and the caller's buffers). Before the write-back was queued the
// pools are as they were and the roll-back is exact; after it they may not be, and the tree says so from now on
void hz::smt_apply_abort(hz_smt* t) {
    (void)hipStreamSynchronize(t->r.s);
    t->shape.rollback();
    t->poisoned = t->wb_queued;
    t->wb_queued = false;
}

void hz::smt_clear(hz_smt* t) {
    t->shape.clear();
    t->poisoned = false;
}

hipStream_t hz::smt_stream(const hz_smt* t) { return t->r.s; }
SmtView hz::smt_view(const hz_smt* t) {
    const SmtShape& sh = t->shape;
    return SmtView{sh.root, sh.nodes(), sh.leaves(), sh.child.data(), sh.leaf_key.data(), (const uint8_t*)t->node.p, (const uint8_t*)t->leaf.p};
}
bool hz::smt_poisoned(const hz_smt* t) { return t->poisoned; }

extern "C" hz_status hz_smt_apply(hz_smt* t, size_t m, const uint64_t* key, const uint8_t* fields, size_t n_sib, uint8_t* siblings_out, uint64_t* old_key_out,
                                  uint8_t* old_value_out, uint8_t* is_old0_out, uint8_t* fnc_out, uint8_t* old_root_out, uint8_t* new_root_out) {
    if (hz_status e = smt_usable(t, "hz_smt_apply")) return e;
    if (hz_status e = smt_n_sib(t, "hz_smt_apply", n_sib)) return e;
    if (m == 0) return HZ_OK;
    if (!key || !fields) return set_err(HZ_ERR_ARG, "hz_smt_apply: null argument");
    if (m > HZ_SMT_MAX_M) return set_err(HZ_ERR_ARG, "hz_smt_apply: %zu ops in one call (at most %u)", m, HZ_SMT_MAX_M);
    for (size_t i = 0; i < m * 4; i++)
        if (!canon_lt_p(fields + i * 32)) return set_err(HZ_ERR_INPUT, "hz_smt_apply: field %zu of op %zu >= r", i & 3, i >> 2);
    const uint32_t M = (uint32_t)m;
    SmtCallBufs b{};
    if (hz_status e = smt_apply_prepare(t, "hz_smt_apply", HZ_ERR_INPUT, M, key, (uint32_t)n_sib, siblings_out != nullptr, &b)) return e;
    const hz_status st = [&]() -> hz_status {
        hipStream_t s = t->r.s;
        HZ_HIP(hipMemcpyAsync(b.fields, fields, (size_t)M * 128, hipMemcpyHostToDevice, s));
        if (hz_status e = smt_apply_launch(t, M, (uint32_t)n_sib, siblings_out != nullptr)) return e;
        if (old_root_out) HZ_HIP(hipMemcpyAsync(old_root_out, b.roots, (size_t)M * 32, hipMemcpyDeviceToHost, s));
        if (new_root_out) HZ_HIP(hipMemcpyAsync(new_root_out, b.roots + 32, (size_t)M * 32, hipMemcpyDeviceToHost, s));
        if (old_value_out) HZ_HIP(hipMemcpyAsync(old_value_out, b.old_value, (size_t)M * 32, hipMemcpyDeviceToHost, s));
        if (siblings_out) HZ_HIP(hipMemcpyAsync(siblings_out, b.siblings, (size_t)M * n_sib * 32, hipMemcpyDeviceToHost, s));
        HZ_HIP(hipStreamSynchronize(s));
        return HZ_OK;
    }();
    if (st) {
        smt_apply_abort(t);
        return st;
    }
    for (size_t j = 0; j < m; j++) {
        if (old_key_out) old_key_out[j] = b.old_key[j];
        if (is_old0_out) is_old0_out[j] = b.is_old0[j];
        if (fnc_out) fnc_out[j] = b.fnc[j];
    }
    return smt_apply_finish(t);
}

// the device's part of hz_smt_proofs: the gather over t->copies and the copies out
static hz_status smt_proofs_device(hz_smt* t, size_t n, size_t n_sib, uint8_t* siblings_out, uint8_t* value_out, uint8_t* not_found_value_out) {
    const std::vector<SmtCopy>& list = t->copies;
    const size_t o_value = n * n_sib, o_nf = o_value + n, total = o_nf + n;
    HZ_HIP(hipSetDevice(t->r.device));
    const size_t ints_bytes = 64 + list.size() * sizeof(SmtCopy);
    HZ_HIP(t->h_ints.grow(ints_bytes));
    HZ_HIP(t->ints.grow(ints_bytes));
    HZ_HIP(t->out.grow(total * 32));
    uint8_t* hb = (uint8_t*)t->h_ints.p;
    smt_bases(t, (const void**)hb);
    for (size_t i = 0; i < list.size(); i++) ((SmtCopy*)(hb + 64))[i] = list[i];
    hipStream_t s = t->r.s;
    HZ_HIP(hipMemcpyAsync(t->ints.p, t->h_ints.p, ints_bytes, hipMemcpyHostToDevice, s));
    HZ_HIP(hipMemsetAsync(t->out.p, 0, total * 32, s));
    if (!list.empty()) {
        hipLaunchKernelGGL(k_smt_gather, dim3((unsigned)((list.size() + 255) / 256)), dim3(256), 0, s, (const SmtCopy*)((const uint8_t*)t->ints.p + 64),
                           (const uint8_t* const*)t->ints.p, (uint8_t*)t->out.p, (uint32_t)list.size());
        HZ_HIP(hipGetLastError());
    }
    const uint8_t* out = (const uint8_t*)t->out.p;
    if (siblings_out) HZ_HIP(hipMemcpyAsync(siblings_out, out, o_value * 32, hipMemcpyDeviceToHost, s));
    if (value_out) HZ_HIP(hipMemcpyAsync(value_out, out + o_value * 32, n * 32, hipMemcpyDeviceToHost, s));
    if (not_found_value_out) HZ_HIP(hipMemcpyAsync(not_found_value_out, out + o_nf * 32, n * 32, hipMemcpyDeviceToHost, s));
    HZ_HIP(hipStreamSynchronize(s));
    return HZ_OK;
}

extern "C" hz_status hz_smt_proofs(hz_smt* t, size_t n, const uint64_t* key, size_t n_sib, uint8_t* siblings_out, uint8_t* found_out, uint8_t* value_out,
                                   uint64_t* not_found_key_out, uint8_t* not_found_value_out, uint8_t* is_old0_out) {
    if (hz_status e = smt_usable(t, "hz_smt_proofs")) return e;
    if (hz_status e = smt_n_sib(t, "hz_smt_proofs", n_sib)) return e;
    if (n == 0) return HZ_OK;
    if (!key) return set_err(HZ_ERR_ARG, "hz_smt_proofs: null argument");
    if (n > HZ_SMT_MAX_PROOFS) return set_err(HZ_ERR_ARG, "hz_smt_proofs: %zu proofs in one call (at most 2^20)", n);
    const SmtShape& sh = t->shape;
    // every key is looked at before anything is written: a refused call leaves the caller's buffers as they were
    for (size_t i = 0; i < n; i++) {
        if (key[i] >> HZ_SMT_KEY_BITS) return smt_plan_err("hz_smt_proofs", SMT_PLAN_KEY, i, key[i], n_sib);
        int32_t met = 0;
        const uint32_t f = sh.find(key[i], &met, nullptr);
        if (f >= n_sib)
            return set_err(HZ_ERR_INPUT, "hz_smt_proofs: key[%zu] = %llu is looked up at depth %u >= n_sib = %zu", i, (unsigned long long)key[i], f, n_sib);
    }
    // out: siblings [n][n_sib] | value [n] | not-found value [n], zero where the gather writes nothing
    const size_t o_value = n * n_sib, o_nf = o_value + n;
    std::vector<SmtCopy>& list = t->copies;
    list.clear();
    uint32_t sib[HZ_SMT_MAX_DEPTH];
    for (size_t i = 0; i < n; i++) {
        int32_t met = 0;
        const uint32_t f = sh.find(key[i], &met, sib);
        for (uint32_t d = 0; d < f; d++)
            if (sib[d] >> 29 != SMT_ZERO) list.push_back({sib[d], (uint32_t)(i * n_sib + d)});
        const bool found = met < 0 && sh.leaf_key[(size_t)(-met - 1)] == key[i];
        if (met < 0) list.push_back({smt_src(SMT_VALUE, (uint32_t)(-met - 1)), (uint32_t)((found ? o_value : o_nf) + i)});
    }
    if (siblings_out || value_out || not_found_value_out)
        if (hz_status e = smt_proofs_device(t, n, n_sib, siblings_out, value_out, not_found_value_out)) {
            (void)hipStreamSynchronize(t->r.s);   // nothing stays in flight over the pinned block or the caller's buffers
            return e;
        }
    for (size_t i = 0; i < n; i++) {
        int32_t met = 0;
        (void)sh.find(key[i], &met, nullptr);
        if (found_out) found_out[i] = met < 0 && sh.leaf_key[(size_t)(-met - 1)] == key[i];
        if (not_found_key_out) not_found_key_out[i] = met < 0 ? sh.leaf_key[(size_t)(-met - 1)] : key[i];
        if (is_old0_out) is_old0_out[i] = met == 0;
    }
    return HZ_OK;
}

extern "C" hz_status hz_smt_plan(size_t m, const uint64_t* key, size_t n_sib, uint32_t* depth_out, uint8_t* fnc_out, uint64_t* old_key_out, uint8_t* is_old0_out) {
    if (n_sib < 1 || n_sib > HZ_SMT_MAX_DEPTH) return set_err(HZ_ERR_ARG, "hz_smt_plan: n_sib = %zu (1 .. %d)", n_sib, HZ_SMT_MAX_DEPTH);
    if (m == 0) return HZ_OK;
    if (!key) return set_err(HZ_ERR_ARG, "hz_smt_plan: null argument");
    if (m > HZ_SMT_MAX_M) return set_err(HZ_ERR_ARG, "hz_smt_plan: %zu ops in one call (at most %u)", m, HZ_SMT_MAX_M);
    SmtShape sh;
    sh.begin();
    for (size_t j = 0; j < m; j++)
        if (const SmtPlanError e = sh.add(key[j], (uint32_t)n_sib)) return smt_plan_err("hz_smt_plan", e, j, key[j], n_sib);
    for (size_t j = 0; j < m; j++) {
        if (depth_out) depth_out[j] = sh.depth[j];
        if (fnc_out) fnc_out[j] = sh.fnc[j];
        if (old_key_out) old_key_out[j] = sh.old_key[j];
        if (is_old0_out) is_old0_out[j] = sh.is_old0[j];
    }
    return HZ_OK;
}
