// The hashes of an account tree, shared by the dense tree (state.hip) and the sparse one (smt_tree.hip): the two leaf-side ones and the
// level hash.
#pragma once
#include "devcommon.h"
#include "poseidon_quad.h"

namespace hz {

// state hash: Poseidon(5) of (e0, balance, ay, ethAddr) (reference src/lib/hash-state.circom:14-40). Field f of the leaf is element
// f * field_stride behind `fields`.
__device__ __forceinline__ Fc state_value_hash(const uint8_t* __restrict__ fields, size_t field_stride) {
    Fr x[4];
#pragma unroll
    for (int f = 0; f < 4; f++) x[f] = fr_from_canon(load_fr(fields + (size_t)f * field_stride * 32));
    NoSink sink;
    return fr_to_canon(poseidon_hash<5>(x, poseidon_consts<5>(), sink));
}

// leaf hash: Poseidon(4) of (key, value, 1) (circomlib SMTHash1)
__device__ __forceinline__ Fc state_leaf_hash(uint64_t key, const Fc& value) {
    const Fr x[3] = {fr_from_u64(key), fr_from_canon(value), fr_one()};
    NoSink sink;
    return fr_to_canon(poseidon_hash<4>(x, poseidon_consts<4>(), sink));
}

// level hash: the node above two canonical children, by a quad of lanes (poseidon_quad.h; pos3: the dense constants). `right`: the
// path goes right, so `other` is the left input. Every lane of the quad passes the same values and gets the digest in MONTGOMERY form:
// only the lane that stores it pays for fr_to_canon (a reduction on the dependent chain of every level otherwise).
__device__ __forceinline__ Fr state_level_hash(const Fc& own, const Fc& other, bool right, const Fr* __restrict__ pos3, uint32_t lane_in_quad) {
    const Fr o = fr_from_canon(own), s = fr_from_canon(other);
    return poseidon3_quad_digest(fr_select(right, s, o), fr_select(right, o, s), pos3_dense_view(pos3), lane_in_quad);
}

}  // namespace hz
