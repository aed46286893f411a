// hz_ledger's archive of exit trees: a withdrawal is made against the exit tree of an EARLIER batch, so the tree a batch
// leaves behind is frozen (hz_ledger_exit_keep) before the next batch empties it, and the inputs of Withdraw(nLevels) come out of the
// frozen trees in bulk (hz_ledger_withdraw_rows). A finished exit tree never changes again, so its SNAPSHOT is immutable and compact,
// one run of bytes inside a slab of the ledger's arena:
//   child [2 * nodes] int32 | leaf_key [leaves] u64 | leaf_place [leaves] u32 | node digests [nodes][32] | leaf hashes [leaves][32] |
//   leaf fields [4][leaves][32]
// each part at a multiple of 32 bytes. The first two are smt_plan.h's shape as it is (a reference: 0 empty, n + 1 node n, -(l + 1) leaf
// l), the digests are device-to-device copies of the tree's pools, the fields a copy of the ledger's final exit leaves (plane-major: e0,
// balance, ay, ethAddr; leaf l lies at place leaf_place[l]). The root digest is the pool entry the root reference names. A DESCRIPTOR
// per snapshot (ArchiveDesc, a table in device memory) holds the six addresses, the counts and the root reference.
// Two kernels answer n queries (snapshot, idx), hz_smt_proofs' own split:
//   k_withdraw_walk   a lane per query: SmtShape::find over the snapshot's integers, a dependent chain of 8-byte loads. It leaves the
//                     status, the depth, the leaf number and one 32-bit SOURCE per depth: zero, node n or leaf l of the query's snapshot
//   k_withdraw_fill   a lane per 16 bytes of output: (query, element, half), elements 0 .. S - 1 the siblings, S .. S + 6 the seven
//                     single rows. The 32 * S bytes of a query's siblings leave as contiguous stores; tokenID and sign are unpacked
//                     from e0 here. A query whose status is not 0 gets zeros
// The walk and the unpacking are HZ_HD: the kernels, the host and tests/native/exit_archive_check.cpp share them.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "fr.h"

namespace hz {

#define HZ_ARCHIVE_MAX_DEPTH 64u   // HZ_SMT_MAX_DEPTH
#define HZ_ARCHIVE_KEY_BITS 48     // HZ_SMT_KEY_BITS

// what a query found
enum : uint32_t { WITHDRAW_FOUND = 0u, WITHDRAW_NOT_KEPT = 1u, WITHDRAW_ABSENT = 2u, WITHDRAW_DEEP = 3u };
// where a 32-byte digest of a snapshot lies: kind in the top two bits, pool index below (a pool holds at most 2^28 entries)
enum : uint32_t { ARC_ZERO = 0u, ARC_NODE = 1u, ARC_LEAF = 2u };
// the seven single rows behind the siblings, in hz_withdraw_rows_out's order
enum : uint32_t { WR_ROOT_EXIT = 0u, WR_ETH_ADDR = 1u, WR_TOKEN_ID = 2u, WR_BALANCE = 3u, WR_IDX = 4u, WR_SIGN = 5u, WR_AY = 6u, WR_ROWS = 7u };

// the memory a walk reads: device memory in a kernel (cast to the global address space at the access), plain memory on the host
#if defined(__HIP_DEVICE_COMPILE__)
#define HZ_ARC_MEM(T) __attribute__((address_space(1))) T
#else
#define HZ_ARC_MEM(T) T
#endif

HZ_HD uint32_t arc_src(int32_t ref) {
    if (ref == 0) return ARC_ZERO;
    return ref > 0 ? (ARC_NODE << 30 | (uint32_t)(ref - 1)) : (ARC_LEAF << 30 | (uint32_t)(-ref - 1));
}

struct ArchiveWalk {
    uint32_t status, depth, leaf;   // depth: the siblings the walk passed; leaf: the leaf's number where status is FOUND or DEEP
};

// SmtShape::find over a snapshot's integers, for a proof of n_sib siblings (hz_smt_proofs' n_sib = nLevels + 1). src[d], d < min(depth,
// n_sib), is the sibling of depth d; nothing else of src is written. A key of 2^48 or more, a walk that ends in an empty slot or at
// another key's leaf: ABSENT. The key's leaf behind n_sib or more siblings: DEEP (hz_smt_proofs' depth rule)
HZ_HD ArchiveWalk archive_walk(int32_t root, const int32_t* child, const uint64_t* leaf_key, uint64_t key, uint32_t n_sib, uint32_t* src) {
    ArchiveWalk w;
    w.status = WITHDRAW_ABSENT;
    w.depth = 0;
    w.leaf = 0;
    if (key >> HZ_ARCHIVE_KEY_BITS) return w;
    const HZ_ARC_MEM(int32_t)* c = (const HZ_ARC_MEM(int32_t)*)child;
    int32_t ref = root;
    uint32_t f = 0;
    while (ref > 0 && f < HZ_ARCHIVE_MAX_DEPTH) {   // (a tree holds no node at depth 64: the bound only keeps a lane from running away)
        const size_t n = (size_t)(ref - 1);
        const int32_t left = c[n * 2], right = c[n * 2 + 1];
        const bool bit = ((key >> f) & 1u) != 0u;
        if (f < n_sib) ((HZ_ARC_MEM(uint32_t)*)src)[f] = arc_src(bit ? left : right);
        ref = bit ? right : left;
        f++;
    }
    w.depth = f;
    if (ref >= 0) return w;
    const uint32_t leaf = (uint32_t)(-ref - 1);
    if (((const HZ_ARC_MEM(uint64_t)*)leaf_key)[leaf] != key) return w;
    w.leaf = leaf;
    w.status = f >= n_sib ? WITHDRAW_DEEP : WITHDRAW_FOUND;
    return w;
}

// tokenID and sign of an exit leaf from the limbs 0 and 2 of its e0 = tokenID | nonce << 32 | sign << 72
HZ_HD uint32_t withdraw_token_id(uint32_t e0_limb0) { return e0_limb0; }
HZ_HD uint32_t withdraw_sign(uint32_t e0_limb2) { return (e0_limb2 >> 8) & 1u; }

// the offsets of a snapshot's parts, each a multiple of 32 bytes, and its size
struct ArchiveLayout {
    size_t child, leaf_key, leaf_place, node, leaf, fields, bytes;
};
inline ArchiveLayout archive_layout(size_t nodes, size_t leaves) {
    ArchiveLayout a;
    size_t end = 0;
    auto take = [&end](size_t bytes) {
        const size_t at = end;
        end = (end + bytes + 31) & ~(size_t)31;
        return at;
    };
    a.child = take(nodes * 2 * sizeof(int32_t));
    a.leaf_key = take(leaves * sizeof(uint64_t));
    a.leaf_place = take(leaves * sizeof(uint32_t));
    a.node = take(nodes * 32);
    a.leaf = take(leaves * 32);
    a.fields = take(leaves * 4 * 32);
    a.bytes = end;
    return a;
}

// one snapshot as the kernels index it: 64 bytes
struct ArchiveDesc {
    const int32_t* child;
    const uint64_t* leaf_key;
    const uint32_t* leaf_place;
    const uint8_t* node;
    const uint8_t* leaf;
    const uint8_t* fields;
    int32_t root;
    uint32_t leaves, nodes, batch_num;
};
static_assert(sizeof(ArchiveDesc) == 64, "a descriptor is 64 bytes");

// what the walk leaves per query
struct WithdrawMeta {
    uint32_t status_depth;   // status | depth << 8
    uint32_t leaf;
};

#if defined(__HIPCC__)
typedef __attribute__((address_space(1))) const ArchiveDesc g_arc_desc;

// a lane per query. snap[q]: the query's place in the descriptor table, -1: its batch is not kept
__global__ __launch_bounds__(64) void k_withdraw_walk(const ArchiveDesc* __restrict__ descs, const int32_t* __restrict__ snap, const uint64_t* __restrict__ idx,
                                                      WithdrawMeta* __restrict__ meta, uint32_t* __restrict__ srcs, uint8_t* __restrict__ status, uint32_t n_sib,
                                                      uint32_t n) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const int32_t s = snap[q];
    ArchiveWalk w;
    w.status = WITHDRAW_NOT_KEPT;
    w.depth = 0;
    w.leaf = 0;
    if (s >= 0) {
        g_arc_desc* d = (g_arc_desc*)(descs + s);
        w = archive_walk(d->root, d->child, d->leaf_key, idx[q], n_sib, srcs + (size_t)q * n_sib);
    }
    WithdrawMeta m;
    m.status_depth = w.status | w.depth << 8;
    m.leaf = w.leaf;
    meta[q] = m;
    status[q] = (uint8_t)w.status;
}

// 16 bytes of a digest a source names
__device__ __forceinline__ hz_u32x4 withdraw_digest(const uint8_t* node, const uint8_t* leaf, uint32_t src, uint32_t half) {
    hz_u32x4 v = {0u, 0u, 0u, 0u};
    const uint32_t kind = src >> 30;
    if (kind != ARC_ZERO) v = *(const hz_g_u32x4*)((kind == ARC_NODE ? node : leaf) + (size_t)(src & 0x3FFFFFFFu) * 32 + half * 16);
    return v;
}

// a lane per 16 bytes: t = ((q * (n_sib + 7)) + e) * 2 + half. rows: the seven single arrays behind each other, [7][n][32]
__global__ __launch_bounds__(256) void k_withdraw_fill(const ArchiveDesc* __restrict__ descs, const int32_t* __restrict__ snap, const uint64_t* __restrict__ idx,
                                                       const WithdrawMeta* __restrict__ meta, const uint32_t* __restrict__ srcs, uint8_t* __restrict__ rows,
                                                       uint8_t* __restrict__ sib, uint32_t n_sib, uint32_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t per = n_sib + WR_ROWS;
    if (t >= (size_t)n * per * 2) return;
    const uint32_t half = (uint32_t)(t & 1u);
    const size_t unit = t >> 1;
    const uint32_t q = (uint32_t)(unit / per), e = (uint32_t)(unit - (size_t)q * per);
    uint8_t* dst = (e < n_sib ? sib + ((size_t)q * n_sib + e) * 32 : rows + ((size_t)(e - n_sib) * n + q) * 32) + half * 16;
    hz_u32x4 v = {0u, 0u, 0u, 0u};
    const WithdrawMeta m = meta[q];
    if ((m.status_depth & 0xFFu) == WITHDRAW_FOUND) {
        g_arc_desc* d = (g_arc_desc*)(descs + snap[q]);
        if (e < n_sib) {
            if (e < m.status_depth >> 8) v = withdraw_digest(d->node, d->leaf, srcs[(size_t)q * n_sib + e], half);
        } else {
            const uint32_t row = e - n_sib;
            if (row == WR_ROOT_EXIT) {
                v = withdraw_digest(d->node, d->leaf, arc_src(d->root), half);
            } else if (row == WR_IDX) {
                const uint64_t key = idx[q];
                if (half == 0u) v.x = (uint32_t)key, v.y = (uint32_t)(key >> 32);
            } else {
                const size_t G = d->leaves, place = ((const HZ_ARC_MEM(uint32_t)*)d->leaf_place)[m.leaf];
                const size_t plane = row == WR_BALANCE ? 1u : row == WR_AY ? 2u : row == WR_ETH_ADDR ? 3u : 0u;   // tokenID and sign: e0
                const hz_u32x4 f = *(const hz_g_u32x4*)(d->fields + (plane * G + place) * 32 + (plane ? half * 16 : 0u));
                if (plane) v = f;
                else if (half == 0u) v.x = row == WR_TOKEN_ID ? withdraw_token_id(f.x) : withdraw_sign(f.z);
            }
        }
    }
    *(hz_g_u32x4*)dst = v;
}
#endif

}  // namespace hz
