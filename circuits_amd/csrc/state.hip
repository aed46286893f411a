// hz_state: the account tree of a pre-populated state resident in HBM -- built, updated and asked for proofs on the device.
//
// Geometry (builder.DenseState's): N = 2^k consecutive accounts first_idx .. first_idx + N - 1, so every residue class modulo 2^k holds
// one key and circomlib's tree (key bits LSB first) is the perfect binary tree of depth k. Node (d, p) covers the keys = p (mod 2^d);
// its children are (d + 1, p) and (d + 1, p + 2^d); leaves sit at depth k. Level d is an array of 2^d digests indexed by p; the
// k + 1 levels lie behind each other in one buffer (level d at element 2^d - 1), the N state hashes (indexed by account
// j = idx - first_idx) in another.
//
// Ordered updates (hz_state_apply) are level-parallel by NODE VERSIONS. Update j makes version j of the k + 1 nodes on its path. The
// level-d launch gives thread group j its own child (version j at depth d + 1, made by the launch before) and the OTHER child: the
// latest version with a sequence number below j, or the resident array's entry when no earlier update touched it. Which version that
// is -- m x k integers -- is plain integer work on the keys and is done by the host while nothing runs (no field arithmetic, no
// hash there); the dependent work is k + 2 launches whatever m is: state hash, leaf hash, k levels. One more launch scatters the
// highest version of every touched node into the resident arrays.
//
// The level hash is the quad-lane Poseidon(3) of poseidon_quad.h: a call is a few dozen wavefronts and k dependent hashes long, so it
// costs the length of one hash, not the number of hashes.
//
// Shared with smt_tree.hip and ledger.hip: the growing device and pinned buffers and the block offsets (hostutil.h), the stream, the
// timing events and the upload of the level hash's constants (resident.h), the leaf hashes and the level hash (state_dev.h).
#define HZ_FR_INLINE 1
#include <hip/hip_runtime.h>
#include <memory>
#include <vector>
#include "../../include/hermez_witness.h"
#include "devcommon.h"
#include "resident.h"
#include "state_dev.h"
#include "state_internal.h"

#define HZ_STATE_MIN_K 4
#define HZ_STATE_MAX_K 24
#define HZ_STATE_MAX_M 65536u

namespace hz {

// ---- kernels ------------------------------------------------------------------------------------------------------------------------
// state hash of `n` leaves: Poseidon(5) of (e0, balance, ay, ethAddr) (reference src/lib/hash-state.circom:14-40). Field f of leaf i
// is element i * elem_stride + f * field_stride of `fields`: four planes of n (load) or records of four (apply).
__global__ __launch_bounds__(256) void k_state_value(const uint8_t* __restrict__ fields, size_t elem_stride, size_t field_stride,
                                                      uint8_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_fr(out + (size_t)i * 32, state_value_hash(fields + (size_t)i * elem_stride * 32, field_stride));
}

// load: the leaf of residue p belongs to account (p - first_idx) mod N
__global__ __launch_bounds__(256) void k_state_leaf_load(const uint8_t* __restrict__ value, uint8_t* __restrict__ leaves, uint64_t first_idx, uint32_t N) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N) return;
    const uint32_t a = (uint32_t)((uint64_t)p - first_idx) & (N - 1);
    store_fr(leaves + (size_t)p * 32, state_leaf_hash(first_idx + a, load_fr(value + (size_t)a * 32)));
}

// apply: version j of leaf (k, p_j), and the state hash update j replaces: the latest earlier update of the same account, or the resident one
__global__ __launch_bounds__(64) void k_state_leaf_apply(const uint64_t* __restrict__ keys, const int32_t* __restrict__ prev_same, const uint8_t* __restrict__ uval,
                                                         const uint8_t* __restrict__ value, uint8_t* __restrict__ ver_k, uint8_t* __restrict__ old_value,
                                                         uint64_t first_idx, uint32_t m) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint64_t key = keys[j];
    const int32_t prev = prev_same[j];
    store_fr(old_value + (size_t)j * 32, prev >= 0 ? load_fr(uval + (size_t)prev * 32) : load_fr(value + (size_t)(key - first_idx) * 32));
    store_fr(ver_k + (size_t)j * 32, state_leaf_hash(key, load_fr(uval + (size_t)j * 32)));
}

// load: node (d, q) from its children in level d + 1; a quad of lanes per node
__global__ __launch_bounds__(256) void k_state_level_load(const uint8_t* __restrict__ below, uint8_t* __restrict__ out, const Fr* __restrict__ pos3, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t q = t >> 2;
    if (q >= n) return;   // (whole quads leave together)
    const Fr h = state_level_hash(load_fr(below + (size_t)q * 32), load_fr(below + ((size_t)q + n) * 32), false, pos3, t & 3u);
    if ((t & 3u) == 0) store_fr(out + (size_t)q * 32, fr_to_canon(h));
}

// apply, level d: version j of node (d, p_j mod 2^d) from version j of its child on the path and the latest earlier version of the
// other child (sib_src[j] >= 0: that update's version; -1: the resident array). The other child is sibling d of update j's proof.
__global__ __launch_bounds__(64) void k_state_level_apply(const uint32_t* __restrict__ res, const int32_t* __restrict__ sib_src, const uint8_t* __restrict__ ver_below,
                                                          const uint8_t* __restrict__ level_below, uint8_t* __restrict__ ver_out, uint8_t* __restrict__ sib_out,
                                                          const Fr* __restrict__ pos3, uint32_t d, uint32_t n_sib, uint32_t m) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t j = t >> 2;
    if (j >= m) return;
    const uint32_t p = res[j];
    const uint32_t q = (p & ((2u << d) - 1u)) ^ (1u << d);
    const int32_t src = sib_src[j];
    const Fc sib = src >= 0 ? load_fr(ver_below + (size_t)src * 32) : load_fr(level_below + (size_t)q * 32);
    const Fr h = state_level_hash(load_fr(ver_below + (size_t)j * 32), sib, (p >> d) & 1u, pos3, t & 3u);
    if ((t & 3u) == 0) {
        store_fr(sib_out + ((size_t)j * n_sib + d) * 32, sib);
        store_fr(ver_out + (size_t)j * 32, fr_to_canon(h));
    }
}

// write-back: the highest version of every touched node into the resident level arrays, the last state hash per account into `value`
__global__ __launch_bounds__(256) void k_state_writeback(const uint32_t* __restrict__ res, const uint64_t* __restrict__ keys, const uint8_t* __restrict__ last,
                                                         const uint8_t* __restrict__ ver, const uint8_t* __restrict__ uval, uint8_t* __restrict__ levels,
                                                         uint8_t* __restrict__ value, uint64_t first_idx, uint32_t k, uint32_t m) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (k + 1) * m) return;
    const uint32_t d = t / m, j = t - d * m;
    if (!last[t]) return;
    const uint32_t node = res[j] & ((1u << d) - 1u);
    store_fr(levels + (((size_t)1 << d) - 1 + node) * 32, load_fr(ver + (size_t)t * 32));
    if (d == k) store_fr(value + (size_t)(keys[j] - first_idx) * 32, load_fr(uval + (size_t)j * 32));
}

// the undo journal of an owner (state_internal.h): a lane per 32-byte element, moved as 16-byte accesses, consecutive lanes on consecutive
// journal addresses. The entry names the element: 1 << 29 | account in the state hashes, else the node's element in the level buffer
#define HZ_STATE_JOURNAL_VALUE (1u << 29)
static_assert(2ull << HZ_STATE_MAX_K <= 1ull << 29, "a level-buffer element, up to 2N - 2, and an account fit below the entry's kind bit");
__global__ __launch_bounds__(256) void k_state_journal_save(const uint32_t* __restrict__ index, const uint8_t* levels, const uint8_t* value, uint8_t* __restrict__ out,
                                                            uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t e = index[t];
    store_fr(out + (size_t)t * 32, load_fr((e >> 29 ? value : levels) + (size_t)(e & 0x1FFFFFFFu) * 32));
}
// the write-back run the other way: every destination appears once in a record
__global__ __launch_bounds__(256) void k_state_journal_restore(const uint32_t* __restrict__ index, const uint8_t* __restrict__ saved, uint8_t* levels, uint8_t* value,
                                                               uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t e = index[t];
    store_fr((e >> 29 ? value : levels) + (size_t)(e & 0x1FFFFFFFu) * 32, load_fr(saved + (size_t)t * 32));
}

// proofs: a pure gather. Thread (i, d): sibling d of key i; thread (i, k): its state hash
__global__ __launch_bounds__(256) void k_state_proofs(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ levels, const uint8_t* __restrict__ value,
                                                      uint8_t* __restrict__ sib_out, uint8_t* __restrict__ value_out, uint64_t first_idx, uint32_t k,
                                                      uint32_t n_sib, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (k + 1) * n) return;
    const uint32_t i = t / (k + 1), d = t - i * (k + 1);
    const uint64_t key = keys[i];
    if (d == k) {
        store_fr(value_out + (size_t)i * 32, load_fr(value + (size_t)(key - first_idx) * 32));
        return;
    }
    const uint32_t p = (uint32_t)key & ((1u << k) - 1u);
    const uint32_t q = (p & ((2u << d) - 1u)) ^ (1u << d);
    store_fr(sib_out + ((size_t)i * n_sib + d) * 32, load_fr(levels + (((size_t)2 << d) - 1 + q) * 32));
}

// ---- host: which earlier update made the version a thread reads ------------------------------------------------------------------------
// node -> sequence number of its latest version so far; open addressing over twice the updates, emptied per depth
struct NodeTable {
    std::vector<uint32_t> key;
    std::vector<int32_t> val;
    uint32_t mask = 0;
    void reset(uint32_t m) {
        uint32_t cap = 16;
        while (cap < 2 * m) cap <<= 1;
        mask = cap - 1;
        key.assign(cap, 0xFFFFFFFFu);
        val.resize(cap);
    }
    uint32_t slot(uint32_t node) const {
        uint32_t s = (node * 2654435761u) >> 7 & mask;
        while (key[s] != 0xFFFFFFFFu && key[s] != node) s = (s + 1) & mask;
        return s;
    }
    int32_t get(uint32_t node) const {
        const uint32_t s = slot(node);
        return key[s] == node ? val[s] : -1;
    }
    int32_t swap(uint32_t node, int32_t v) {   // returns the previous entry (-1: none)
        const uint32_t s = slot(node);
        const int32_t old = key[s] == node ? val[s] : -1;
        key[s] = node;
        val[s] = v;
        return old;
    }
};

// the integer tables of an apply, one block (pinned, then uploaded): keys u64[m] | residues u32[m] | prev_same i32[m] | sib_src i32[k][m] |
// last u8[k + 1][m]. The keys lie at offset 0.
struct StateInts {
    size_t res, prev, src, last, bytes;
    StateInts(uint32_t k, uint32_t M) {
        Carve c;
        c.take((size_t)M * 8);
        res = c.take((size_t)M * 4);
        prev = c.take((size_t)M * 4);
        src = c.take((size_t)k * M * 4);
        last = c.take((size_t)(k + 1) * M);
        bytes = c.end;
    }
};

}  // namespace hz

using namespace hz;

struct hz_state {
    uint32_t k = 0, N = 0;
    uint64_t first_idx = 0;
    bool loaded = false;
    DevBuf levels, value, pos3;                  // resident: (2N - 1) x 32, N x 32, the quad form's constants
    DevBuf fields, uval, oldval, ver, sib, ints;  // per call, grown on demand
    PinnedBuf h_ints, h_journal;   // h_journal: the entries of a journalled call, made only for an owner that asks
    size_t n_journal = 0;
    NodeTable table;
    Resident r;   // device, stream, device time of the last load / apply
    uint8_t* level(uint32_t d) const { return (uint8_t*)levels.p + (((size_t)1 << d) - 1) * 32; }
};

static hz_status state_ready(const hz_state* st, const char* who) {
    if (!st) return set_err(HZ_ERR_ARG, "%s: null state", who);
    if (!st->loaded) return set_err(HZ_ERR_ARG, "%s: the state holds no tree yet (hz_state_load)", who);
    return HZ_OK;
}

static hz_status state_keys(const hz_state* st, const char* who, const uint64_t* idx, size_t n) {
    for (size_t j = 0; j < n; j++)
        if (idx[j] < st->first_idx || idx[j] - st->first_idx >= st->N)
            return set_err(HZ_ERR_ARG, "%s: idx[%zu] = %llu is outside the state (%llu .. %llu)", who, j, (unsigned long long)idx[j],
                           (unsigned long long)st->first_idx, (unsigned long long)(st->first_idx + st->N - 1));
    return HZ_OK;
}

extern "C" hz_status hz_state_create(int32_t device, int32_t k, uint64_t first_idx, hz_state** out) {
    if (!out) return set_err(HZ_ERR_ARG, "hz_state_create: null argument");
    *out = nullptr;
    if (k < HZ_STATE_MIN_K || k > HZ_STATE_MAX_K) return set_err(HZ_ERR_ARG, "hz_state_create: k = %d (%d .. %d)", k, HZ_STATE_MIN_K, HZ_STATE_MAX_K);
    if (first_idx > (1ull << 48)) return set_err(HZ_ERR_ARG, "hz_state_create: first_idx beyond 2^48 (the circuits' idx has 48 bits)");
    std::unique_ptr<hz_state> st(new hz_state);
    if (hz_status e = st->r.open("hz_state_create", device)) return e;
    st->k = (uint32_t)k;
    st->N = 1u << k;
    st->first_idx = first_idx;
    HZ_HIP(st->levels.alloc(((size_t)2 * st->N - 1) * 32));
    HZ_HIP(st->value.alloc((size_t)st->N * 32));
    if (hz_status e = pos3_dense_create(st->pos3)) return e;
    *out = st.release();
    return HZ_OK;
}

extern "C" void hz_state_destroy(hz_state* st) {
    if (!st) return;
    (void)hipSetDevice(st->r.device);
    if (st->r.s) (void)hipStreamSynchronize(st->r.s);
    delete st;
}

extern "C" hz_status hz_state_load(hz_state* st, const uint8_t* e0, const uint8_t* balance, const uint8_t* ay, const uint8_t* eth_addr) {
    if (!st || !e0 || !balance || !ay || !eth_addr) return set_err(HZ_ERR_ARG, "hz_state_load: null argument");
    const uint32_t N = st->N, k = st->k;
    const uint8_t* src[4] = {e0, balance, ay, eth_addr};
    for (int f = 0; f < 4; f++)
        for (size_t i = 0; i < N; i++)
            if (!canon_lt_p(src[f] + i * 32)) return set_err(HZ_ERR_INPUT, "hz_state_load: field %d of account %zu >= r", f, i);
    HZ_HIP(hipSetDevice(st->r.device));
    st->loaded = false;
    // the upload: the four field planes behind each other in one buffer, dropped again when the tree stands
    DevBuf planes;
    HZ_HIP(planes.alloc((size_t)4 * N * 32));
    for (int f = 0; f < 4; f++) HZ_HIP(hipMemcpyAsync((uint8_t*)planes.p + (size_t)f * N * 32, src[f], (size_t)N * 32, hipMemcpyHostToDevice, st->r.s));
    HZ_HIP(st->r.begin());
    hipLaunchKernelGGL(k_state_value, dim3((N + 255) / 256), dim3(256), 0, st->r.s, (const uint8_t*)planes.p, (size_t)1, (size_t)N, (uint8_t*)st->value.p, N);
    HZ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_state_leaf_load, dim3((N + 255) / 256), dim3(256), 0, st->r.s, (const uint8_t*)st->value.p, st->level(k), st->first_idx, N);
    HZ_HIP(hipGetLastError());
    for (uint32_t d = k; d-- > 0;) {
        const uint32_t n = 1u << d;
        hipLaunchKernelGGL(k_state_level_load, dim3((4 * n + 255) / 256), dim3(256), 0, st->r.s, (const uint8_t*)st->level(d + 1), st->level(d), (const Fr*)st->pos3.p, n);
        HZ_HIP(hipGetLastError());
    }
    HZ_HIP(st->r.end());
    if (hz_status e = st->r.finish()) return e;
    st->loaded = true;
    return HZ_OK;
}

extern "C" hz_status hz_state_root(hz_state* st, uint8_t* out32) {
    if (hz_status e = state_ready(st, "hz_state_root")) return e;
    if (!out32) return set_err(HZ_ERR_ARG, "hz_state_root: null argument");
    HZ_HIP(hipSetDevice(st->r.device));
    HZ_HIP(hipMemcpyAsync(out32, st->level(0), 32, hipMemcpyDeviceToHost, st->r.s));
    HZ_HIP(hipStreamSynchronize(st->r.s));
    return HZ_OK;
}

extern "C" double hz_state_device_ms(const hz_state* st) { return st ? st->r.device_ms : 0.0; }

// The body of an apply in two halves, so that a caller whose fields are already in device memory (ledger.hip) runs the same tree update
// as hz_state_apply. prepare: the integer tables of the call (which earlier update made the version a thread reads), the per-call
// buffers grown, the tables queued for upload. launch: state hash, leaf hash, k levels, write-back; siblings, old values and roots
// stay in the buffers `prepare` named. Nothing here synchronises.
hz_status hz::state_apply_prepare(hz_state* st, uint32_t M, const uint64_t* idx, uint32_t n_sib, StateCallBufs* out) {
    const uint32_t k = st->k;
    HZ_HIP(hipSetDevice(st->r.device));
    const StateInts o(k, M);
    HZ_HIP(st->h_ints.grow(o.bytes));
    uint8_t* hb = (uint8_t*)st->h_ints.p;
    uint64_t* h_keys = (uint64_t*)hb;
    uint32_t* h_res = (uint32_t*)(hb + o.res);
    int32_t* h_prev = (int32_t*)(hb + o.prev);
    int32_t* h_src = (int32_t*)(hb + o.src);
    uint8_t* h_last = hb + o.last;
    for (uint32_t j = 0; j < M; j++) {
        h_keys[j] = idx[j];
        h_res[j] = (uint32_t)idx[j] & (st->N - 1);
    }
    for (uint32_t dd = 0; dd <= k; dd++) {   // nodes of depth dd
        st->table.reset(M);
        const uint32_t pre = (1u << dd) - 1u;
        uint8_t* last = h_last + (size_t)dd * M;
        int32_t* src = dd ? h_src + (size_t)(dd - 1) * M : nullptr;   // read by the launch that hashes depth dd - 1
        for (uint32_t j = 0; j < M; j++) {
            const uint32_t node = h_res[j] & pre;
            if (src) src[j] = st->table.get(node ^ (1u << (dd - 1)));
            const int32_t before = st->table.swap(node, (int32_t)j);
            if (dd == k) h_prev[j] = before;
            if (before >= 0) last[before] = 0;
            last[j] = 1;
        }
    }

    HZ_HIP(st->ints.grow(o.bytes));
    HZ_HIP(st->fields.grow((size_t)M * 128));
    HZ_HIP(st->uval.grow((size_t)M * 32));
    HZ_HIP(st->oldval.grow((size_t)M * 32));
    HZ_HIP(st->ver.grow(((size_t)(k + 1) * M + 1) * 32));   // one element ahead of version 0 of the root: the root the call found
    HZ_HIP(st->sib.grow((size_t)M * n_sib * 32));
    HZ_HIP(hipMemcpyAsync(st->ints.p, st->h_ints.p, o.bytes, hipMemcpyHostToDevice, st->r.s));
    if (out) {
        out->fields = (uint8_t*)st->fields.p;
        out->siblings = (uint8_t*)st->sib.p;
        out->old_value = (uint8_t*)st->oldval.p;
        out->old_root = (uint8_t*)st->ver.p;
        out->new_root = (uint8_t*)st->ver.p + 32;
    }
    return HZ_OK;
}

// the resident elements the prepared call's write-back replaces, from the call's own `last` flags, into the pinned entry list
hz_status hz::state_journal_entries(hz_state* st, uint32_t M, size_t* n_out) {
    const uint32_t k = st->k;
    const StateInts o(k, M);
    const uint8_t* hb = (const uint8_t*)st->h_ints.p;
    const uint64_t* h_keys = (const uint64_t*)hb;
    const uint32_t* h_res = (const uint32_t*)(hb + o.res);
    const uint8_t* h_last = hb + o.last;
    st->n_journal = 0;
    size_t n = 0;
    for (size_t t = 0; t < (size_t)(k + 1) * M; t++) n += h_last[t] ? (t >= (size_t)k * M ? 2 : 1) : 0;
    *n_out = n;
    if (n == 0) return HZ_OK;
    HZ_HIP(st->h_journal.grow(n * 4));
    uint32_t* h = (uint32_t*)st->h_journal.p;
    size_t w = 0;
    for (uint32_t d = 0; d <= k; d++)
        for (uint32_t j = 0; j < M; j++)
            if (h_last[(size_t)d * M + j]) h[w++] = ((1u << d) - 1u) + (h_res[j] & ((1u << d) - 1u));
    for (uint32_t j = 0; j < M; j++)
        if (h_last[(size_t)k * M + j]) h[w++] = HZ_STATE_JOURNAL_VALUE | (uint32_t)(h_keys[j] - st->first_idx);
    st->n_journal = n;
    return HZ_OK;
}

hz_status hz::state_apply_launch(hz_state* st, uint32_t M, uint32_t n_sib, bool clear_siblings, const StateJournalDst* journal) {
    const uint32_t k = st->k;
    const StateInts o(k, M);
    uint8_t* db = (uint8_t*)st->ints.p;
    const uint64_t* d_keys = (const uint64_t*)db;
    const uint32_t* d_res = (const uint32_t*)(db + o.res);
    const int32_t* d_prev = (const int32_t*)(db + o.prev);
    const int32_t* d_src = (const int32_t*)(db + o.src);
    const uint8_t* d_last = db + o.last;
    uint8_t* ver = (uint8_t*)st->ver.p + 32;   // [k + 1][m], depth 0 first
    hipStream_t s = st->r.s;
    if (clear_siblings && n_sib > k) HZ_HIP(hipMemsetAsync(st->sib.p, 0, (size_t)M * n_sib * 32, s));
    HZ_HIP(st->r.begin());
    hipLaunchKernelGGL(k_state_value, dim3((M + 63) / 64), dim3(64), 0, s, (const uint8_t*)st->fields.p, (size_t)4, (size_t)1, (uint8_t*)st->uval.p, M);
    HZ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_state_leaf_apply, dim3((M + 63) / 64), dim3(64), 0, s, d_keys, d_prev, (const uint8_t*)st->uval.p, (const uint8_t*)st->value.p,
                       ver + (size_t)k * M * 32, (uint8_t*)st->oldval.p, st->first_idx, M);
    HZ_HIP(hipGetLastError());
    for (uint32_t d = k; d-- > 0;) {
        hipLaunchKernelGGL(k_state_level_apply, dim3((4 * M + 63) / 64), dim3(64), 0, s, d_res, d_src + (size_t)d * M, (const uint8_t*)(ver + (size_t)(d + 1) * M * 32),
                           (const uint8_t*)st->level(d + 1), ver + (size_t)d * M * 32, (uint8_t*)st->sib.p, (const Fr*)st->pos3.p, d, n_sib, M);
        HZ_HIP(hipGetLastError());
    }
    // the root before the first update is set aside before the write-back replaces it: old roots = (that, versions 0 .. m - 2 of the root)
    HZ_HIP(hipMemcpyAsync(st->ver.p, st->level(0), 32, hipMemcpyDeviceToDevice, s));
    if (journal && st->n_journal) {   // what the write-back is about to replace
        const uint32_t n = (uint32_t)st->n_journal;
        HZ_HIP(hipMemcpyAsync(journal->index, st->h_journal.p, (size_t)n * 4, hipMemcpyHostToDevice, s));
        HZ_HIP(journal->span->begin(s));
        hipLaunchKernelGGL(k_state_journal_save, dim3((n + 255) / 256), dim3(256), 0, s, (const uint32_t*)journal->index, (const uint8_t*)st->levels.p,
                           (const uint8_t*)st->value.p, journal->values, n);
        HZ_HIP(hipGetLastError());
        HZ_HIP(journal->span->end(s));
    }
    const uint32_t wb = (k + 1) * M;
    hipLaunchKernelGGL(k_state_writeback, dim3((wb + 255) / 256), dim3(256), 0, s, d_res, d_keys, d_last, (const uint8_t*)ver, (const uint8_t*)st->uval.p,
                       (uint8_t*)st->levels.p, (uint8_t*)st->value.p, st->first_idx, k, M);
    HZ_HIP(hipGetLastError());
    HZ_HIP(st->r.end());
    return HZ_OK;
}

hz_status hz::state_apply_finish(hz_state* st) { return st->r.finish(); }

hz_status hz::state_journal_restore(hz_state* st, const uint8_t* values, const uint32_t* index, size_t n) {
    HZ_HIP(hipSetDevice(st->r.device));
    if (n == 0) return HZ_OK;
    hipLaunchKernelGGL(k_state_journal_restore, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st->r.s, index, values, (uint8_t*)st->levels.p, (uint8_t*)st->value.p,
                       (uint32_t)n);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

hipStream_t hz::state_stream(const hz_state* st) { return st->r.s; }
const uint8_t* hz::state_root_dev(const hz_state* st) { return st->level(0); }
bool hz::state_loaded(const hz_state* st) { return st->loaded; }

extern "C" hz_status hz_state_apply(hz_state* st, size_t m, const uint64_t* idx, const uint8_t* fields, size_t n_sib, uint8_t* siblings_out,
                                    uint8_t* old_value_out, uint8_t* old_root_out, uint8_t* new_root_out) {
    if (hz_status e = state_ready(st, "hz_state_apply")) return e;
    if (m == 0) return HZ_OK;
    if (!idx || !fields) return set_err(HZ_ERR_ARG, "hz_state_apply: null argument");
    if (m > HZ_STATE_MAX_M) return set_err(HZ_ERR_ARG, "hz_state_apply: %zu updates in one call (at most %u)", m, HZ_STATE_MAX_M);
    const uint32_t k = st->k, M = (uint32_t)m;
    if (n_sib < k || n_sib > 64) return set_err(HZ_ERR_ARG, "hz_state_apply: n_sib = %zu (%u .. 64)", n_sib, k);
    if (hz_status e = state_keys(st, "hz_state_apply", idx, m)) return e;
    for (size_t i = 0; i < m * 4; i++)
        if (!canon_lt_p(fields + i * 32)) return set_err(HZ_ERR_INPUT, "hz_state_apply: field %zu of update %zu >= r", i & 3, i >> 2);
    StateCallBufs b;
    if (hz_status e = state_apply_prepare(st, M, idx, (uint32_t)n_sib, &b)) return e;
    hipStream_t s = st->r.s;
    HZ_HIP(hipMemcpyAsync(b.fields, fields, (size_t)M * 128, hipMemcpyHostToDevice, s));
    if (hz_status e = state_apply_launch(st, M, (uint32_t)n_sib, siblings_out != nullptr)) return e;
    if (old_root_out) HZ_HIP(hipMemcpyAsync(old_root_out, b.old_root, (size_t)M * 32, hipMemcpyDeviceToHost, s));
    if (new_root_out) HZ_HIP(hipMemcpyAsync(new_root_out, b.new_root, (size_t)M * 32, hipMemcpyDeviceToHost, s));
    if (old_value_out) HZ_HIP(hipMemcpyAsync(old_value_out, b.old_value, (size_t)M * 32, hipMemcpyDeviceToHost, s));
    if (siblings_out) HZ_HIP(hipMemcpyAsync(siblings_out, b.siblings, (size_t)M * n_sib * 32, hipMemcpyDeviceToHost, s));
    return state_apply_finish(st);
}

extern "C" hz_status hz_state_proofs(hz_state* st, size_t n, const uint64_t* idx, size_t n_sib, uint8_t* siblings_out, uint8_t* value_out) {
    if (hz_status e = state_ready(st, "hz_state_proofs")) return e;
    if (n == 0) return HZ_OK;
    if (!idx) return set_err(HZ_ERR_ARG, "hz_state_proofs: null argument");
    const uint32_t k = st->k;
    if (n > ((size_t)1 << 24)) return set_err(HZ_ERR_ARG, "hz_state_proofs: %zu proofs in one call (at most 2^24)", n);
    if (n_sib < k || n_sib > 64) return set_err(HZ_ERR_ARG, "hz_state_proofs: n_sib = %zu (%u .. 64)", n_sib, k);
    if (hz_status e = state_keys(st, "hz_state_proofs", idx, n)) return e;
    HZ_HIP(hipSetDevice(st->r.device));
    const uint32_t n32 = (uint32_t)n;
    HZ_HIP(st->ints.grow(n * 8));
    HZ_HIP(st->sib.grow(n * n_sib * 32));
    HZ_HIP(st->oldval.grow(n * 32));
    hipStream_t s = st->r.s;
    HZ_HIP(hipMemcpyAsync(st->ints.p, idx, n * 8, hipMemcpyHostToDevice, s));
    if (n_sib > k) HZ_HIP(hipMemsetAsync(st->sib.p, 0, n * n_sib * 32, s));
    const size_t threads = (size_t)(k + 1) * n32;
    hipLaunchKernelGGL(k_state_proofs, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, (const uint64_t*)st->ints.p, (const uint8_t*)st->levels.p,
                       (const uint8_t*)st->value.p, (uint8_t*)st->sib.p, (uint8_t*)st->oldval.p, st->first_idx, k, (uint32_t)n_sib, n32);
    HZ_HIP(hipGetLastError());
    if (siblings_out) HZ_HIP(hipMemcpyAsync(siblings_out, st->sib.p, n * n_sib * 32, hipMemcpyDeviceToHost, s));
    if (value_out) HZ_HIP(hipMemcpyAsync(value_out, st->oldval.p, n * 32, hipMemcpyDeviceToHost, s));
    HZ_HIP(hipStreamSynchronize(s));
    return HZ_OK;
}

extern "C" hz_status hz_state_download(hz_state* st, uint8_t* const* levels_out, uint8_t* value_out) {
    if (hz_status e = state_ready(st, "hz_state_download")) return e;
    HZ_HIP(hipSetDevice(st->r.device));
    if (levels_out)
        for (uint32_t d = 0; d <= st->k; d++)
            if (levels_out[d]) HZ_HIP(hipMemcpyAsync(levels_out[d], st->level(d), ((size_t)32) << d, hipMemcpyDeviceToHost, st->r.s));
    if (value_out) HZ_HIP(hipMemcpyAsync(value_out, st->value.p, (size_t)st->N * 32, hipMemcpyDeviceToHost, st->r.s));
    HZ_HIP(hipStreamSynchronize(st->r.s));
    return HZ_OK;
}
