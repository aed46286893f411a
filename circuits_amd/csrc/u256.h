// Plain 256-bit integers in the Fc container of fr.h (eight 32-bit limbs, nothing is reduced modulo r), for the ledger's balances and
// fees (ledger.hip) and the packed words and comparisons of its signature check (ledger_sig.h). HZ_HD: device and host builds alike.
#pragma once
#include "fr.h"

namespace hz {

HZ_HD Fc u256_add(const Fc& a, const Fc& b) {
    Fc r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)a.v[i] + b.v[i];
        r.v[i] = (uint32_t)c;
        c >>= 32;
    }
    return r;
}
HZ_HD Fc u256_neg(const Fc& a) {
    Fc r;
    uint64_t c = 1;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)(~a.v[i]);
        r.v[i] = (uint32_t)c;
        c >>= 32;
    }
    return r;
}
HZ_HD Fc u256_mul_u32(const Fc& a, uint32_t w) {
    Fc r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)a.v[i] * w;
        r.v[i] = (uint32_t)c;
        c >>= 32;
    }
    return r;
}
HZ_HD Fc u256_mul_u64(const Fc& a, uint64_t t) {
    const Fc lo = u256_mul_u32(a, (uint32_t)t), hi = u256_mul_u32(a, (uint32_t)(t >> 32));
    Fc sh;
    sh.v[0] = 0u;
#pragma unroll
    for (int i = 1; i < 8; i++) sh.v[i] = hi.v[i - 1];
    return u256_add(lo, sh);
}
HZ_HD Fc u256_shr60(const Fc& a) {
    Fc r;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t lo = i + 1 < 8 ? a.v[i + 1] : 0u, hi = i + 2 < 8 ? a.v[i + 2] : 0u;
        r.v[i] = (lo >> 28) | (hi << 4);
    }
    return r;
}
HZ_HD Fc u256_u64(uint64_t x) {
    Fc r = fc_zero();
    r.v[0] = (uint32_t)x;
    r.v[1] = (uint32_t)(x >> 32);
    return r;
}
// r |= v << sh (sh a constant once inlined)
HZ_HD void u256_or_shl(Fc& r, uint64_t v, int sh) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int lo = 32 * i - sh;   // the bit of v that lands on bit 0 of limb i
        uint32_t w = 0;
        if (lo >= 0 && lo < 64) w = (uint32_t)(v >> lo);
        if (lo < 0 && lo > -32) w = (uint32_t)(v << (-lo));
        r.v[i] |= w;
    }
}
HZ_HD bool u256_less(const Fc& a, const Fc& b) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) br = (((uint64_t)a.v[i] - b.v[i] - br) >> 63) & 1;
    return br != 0;
}

}  // namespace hz
