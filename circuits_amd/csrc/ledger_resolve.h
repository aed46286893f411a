// hz_ledger's receiver lookup: a transaction with to_idx == 0 names its receiver by a 160-bit address, or by the "any"
// address 2^160 - 1 plus a BabyJubjub key (ay, sign); the receiver is the LOWEST account that holds that address (or that key under the
// "any" address) and the transaction's token. Every account has exactly one such key, so the lookup is one pass over the resident planes:
// the host puts the batch's distinct queries into an open-addressing table (integers of the transactions only), a lane per account forms
// the account's key, probes the table and lowers the slot's result with atomicMin.
// The key, its hash, the comparison and the probe are HZ_HD: the host builder, the kernel and tests/native/ledger_addr_check.cpp share them.
// The slot count is an argument (a power of two); the library uses at least twice the number of queries.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "fr.h"

namespace hz {

enum : uint32_t { RESOLVE_EMPTY = 0u, RESOLVE_ADDR = 1u, RESOLVE_KEY = 2u /* | sign */ };
#define HZ_RESOLVE_NONE 0xFFFFFFFFu

// w[0]: 0 an empty slot, 1 an address, 2 | sign a key; w[1]: the token; w[2 .. 9]: the address or ay, eight 32-bit limbs
struct ResolveKey {
    uint32_t w[10];
};

// 32 bytes of a hz_l2sig member: the struct is 4-byte aligned, not 16
HZ_HD Fc resolve_load32(const uint8_t* p) {
    const uint32_t* q = (const uint32_t*)p;
    Fc r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = q[i];
    return r;
}

HZ_HD bool resolve_is_any(const Fc& eth) {
    return (eth.v[0] & eth.v[1] & eth.v[2] & eth.v[3] & eth.v[4]) == 0xFFFFFFFFu && (eth.v[5] | eth.v[6] | eth.v[7]) == 0u;
}

HZ_HD bool resolve_fc_same(const Fc& a, const Fc& b) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d |= a.v[i] ^ b.v[i];
    return d == 0u;
}

// the key of an account, or of a transaction's signed destination: by address, or by (ay, sign) when the address is the "any" address
HZ_HD ResolveKey resolve_key(uint32_t token, const Fc& eth, const Fc& ay, uint32_t sign) {
    const bool any = resolve_is_any(eth);
    ResolveKey k;
    k.w[0] = any ? (RESOLVE_KEY | (sign & 1u)) : RESOLVE_ADDR;
    k.w[1] = token;
#pragma unroll
    for (int i = 0; i < 8; i++) k.w[2 + i] = any ? ay.v[i] : eth.v[i];
    return k;
}

// FNV-1a over the ten words, one xor-shift at the end: the low bits choose the slot
HZ_HD uint32_t resolve_hash(const ResolveKey& k) {
    uint32_t h = 0x811C9DC5u;
#pragma unroll
    for (int i = 0; i < 10; i++) h = (h ^ k.w[i]) * 0x01000193u;
    return h ^ (h >> 15);
}

HZ_HD bool resolve_same(const ResolveKey& a, const ResolveKey& b) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) d |= a.w[i] ^ b.w[i];
    return d == 0u;
}

// the slot that holds k, or -1: linear probing from the hash, ended by an empty slot or after `slots` steps (a full table)
HZ_HD int32_t resolve_probe(const ResolveKey* table, uint32_t slots, const ResolveKey& k) {
    uint32_t s = resolve_hash(k) & (slots - 1u);
    for (uint32_t step = 0; step < slots; step++) {
        const uint32_t kind = table[s].w[0];
        if (kind == RESOLVE_EMPTY) return -1;
        if (kind == k.w[0]) {
            ResolveKey c;
#pragma unroll
            for (int i = 0; i < 10; i++) c.w[i] = table[s].w[i];
            if (resolve_same(c, k)) return (int32_t)s;
        }
        s = (s + 1u) & (slots - 1u);
    }
    return -1;
}

// host: the slot of k, entered at the first empty slot of its probe sequence when it is new; -1 when the table is full without it
inline int32_t resolve_insert(ResolveKey* table, uint32_t slots, const ResolveKey& k) {
    uint32_t s = resolve_hash(k) & (slots - 1u);
    for (uint32_t step = 0; step < slots; step++) {
        if (table[s].w[0] == RESOLVE_EMPTY) {
            table[s] = k;
            return (int32_t)s;
        }
        if (resolve_same(table[s], k)) return (int32_t)s;
        s = (s + 1u) & (slots - 1u);
    }
    return -1;
}

// the smallest power of two that is at least 2 x queries (and at least 2)
inline uint32_t resolve_slots(size_t queries) {
    uint32_t s = 2;
    while (s < 2 * queries) s <<= 1;
    return s;
}

}  // namespace hz
