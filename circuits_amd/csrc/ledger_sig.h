// Verify-only EdDSA-Poseidon for the ledger: the message of an L2 transaction (src/decode-tx.circom:249-283) and the
// verdict of EdDSAPoseidonVerifier on it, without a single witness signal. Everything here is HZ_HD: the kernels of ledger_sig.hip
// and the stand-alone host build (tests/native/ledger_sig_check.cpp, tools/ledger_sig_bench.py) share the routines.
//
// The verdict is a group-law statement: S < l, Ax recovered from (ay, sign) as AySign2Ax does, hm = Poseidon(R8, A, M) as the full
// integer, Q8 = 8 A with x != 0, and BabyAdd(R8, hm Q8) == S B8 with the AFFINE formula on R8 as given (R8 is not checked to be on
// the curve) and both denominators nonzero. hm Q8 and S B8 are in extended coordinates, so the comparison needs no inversion:
//     x3 = (x1 Yq + y1 Xq) / (Zq + d x1 y1 Tq),  y3 = (y1 Yq - a x1 Xq) / (Zq - d x1 y1 Tq)   against   Xl / Zl, Yl / Zl.
// hm Q8 is a binary ladder with a dedicated doubling (4M + 4S) and a 9-product addition; S B8 takes no doubling at all: 64 mixed
// additions from a table of d * 16^w * B8 (d < 16, w < 64) that the host builds once with these same routines (sig_b8_table).
#pragma once
#include "../../include/hermez_witness.h"
#include "babyjub.h"
#include "poseidon.h"
#include "u256.h"

namespace hz {

#define HZ_SIG_CONST 3322668559u   // SIGNATURE_CONSTANT of decode-tx.circom
#define HZ_SIG_B8_WINDOWS 64
#define HZ_SIG_B8_FRS (HZ_SIG_B8_WINDOWS * 16 * 3)   // Fr per table: [window][digit][x, y, d x y]

// the suborder l and (r - 1) / 2, plain integers
HZ_HD constexpr uint32_t sig_l(int i) {
    constexpr uint32_t k[8] = {0x392126f1u, 0x677297dcu, 0x3920ee0au, 0xab3eedb8u, 0xd0302b0bu, 0x370a08b6u, 0x5c263405u, 0x060c89ceu};
    return k[i];
}
HZ_HD constexpr uint32_t sig_half(int i) {
    constexpr uint32_t k[8] = {0xf8000000u, 0xa1f0fac9u, 0x3cdcb848u, 0x9419f424u, 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u};
    return k[i];
}
// Base8 and the square root's constants as gen/bjj_consts.inc has them (Montgomery form; the exponent is a plain integer)
HZ_HD constexpr uint32_t sig_b8x(int i) {
    constexpr uint32_t k[9] = {0x013f50b3u, 0x1bfbf801u, 0x09836037u, 0x104a5e1cu, 0x0f079f09u, 0x06241221u, 0x047dc05eu, 0x1a102c70u, 0x001f07f1u};
    return k[i];
}
HZ_HD constexpr uint32_t sig_b8y(int i) {
    constexpr uint32_t k[9] = {0x10403537u, 0x1bb5c071u, 0x1e18f6e8u, 0x1668dae4u, 0x0a95f960u, 0x0f8d13a8u, 0x1281e883u, 0x15d13959u, 0x000be9f1u};
    return k[i];
}
HZ_HD constexpr uint32_t sig_sqrt_root(int i) {   // a generator of the 2^28 roots of unity
    constexpr uint32_t k[9] = {0x1a27b370u, 0x1d788b88u, 0x0a3c6e0bu, 0x1fd3f9dau, 0x0f541c23u, 0x1e4ddf15u, 0x093d0e83u, 0x0ae32ca7u, 0x0005d90bu};
    return k[i];
}
HZ_HD constexpr uint32_t sig_sqrt_zexp(int i) {   // (q - 1) / 2 with r - 1 = 2^28 q
    constexpr uint32_t k[8] = {0x1f0fac9fu, 0xcdcb848au, 0x419f4243u, 0x0c0ac2e9u, 0xc2822db4u, 0x098d014du, 0x83227397u, 0x00000001u};
    return k[i];
}

// ---- the two bounds as plain 256-bit integers (the arithmetic is u256.h's) ------------------------------------------------------------------
HZ_HD Fc sig_l_c() {
    Fc r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = sig_l(i);
    return r;
}
HZ_HD Fc sig_half_c() {
    Fc r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = sig_half(i);
    return r;
}

// the fields of one transaction the message is made of; a NOP is all zeros
struct SigTx {
    uint64_t from_idx, to_idx, amount_f, nonce;
    uint32_t token_id, user_fee, to_bjj_sign, max_num_batch;
    Fc to_eth_addr, to_bjj_ay;
};
// 32 bytes of a hz_l2sig member (the struct is 4-byte aligned, not 16), or zero. (Masking the limbs of a SigTx member in a loop of
// their own, inside an inlined routine, keeps the struct in private memory on the device: 40 bytes of scratch a lane.)
HZ_HD Fc sig_load32_if(const uint8_t* p, bool active) {
    const uint32_t* q = (const uint32_t*)p;
    Fc r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = active ? q[i] : 0u;
    return r;
}
// the fields of a transaction as uploaded, zero for a NOP: the one place that says what the message and the V2 row are made of, for the
// kernels of ledger_sig.hip and for the host's hz_ledger_plan_atomic
HZ_HD SigTx sig_load_tx(const hz_l2tx& x, const hz_l2sig& g, bool active) {
    SigTx t;
    t.from_idx = active ? x.from_idx : 0;
    t.to_idx = active ? x.to_idx : 0;
    t.amount_f = active ? x.amount_f : 0;
    t.nonce = active ? x.nonce : 0;
    t.token_id = active ? x.token_id : 0u;
    t.user_fee = active ? x.user_fee : 0u;
    t.to_bjj_sign = active ? g.to_bjj_sign : 0u;
    t.max_num_batch = active ? g.max_num_batch : 0u;
    t.to_eth_addr = sig_load32_if(g.to_eth_addr, active);
    t.to_bjj_ay = sig_load32_if(g.to_bjj_ay, active);
    return t;
}
HZ_HD Fc sig_tx_compressed_data(const SigTx& t, uint32_t chain_id) {
    Fc r = fc_zero();
    u256_or_shl(r, HZ_SIG_CONST, 0);
    u256_or_shl(r, chain_id & 0xFFFFu, 32);
    u256_or_shl(r, t.from_idx & 0xFFFFFFFFFFFFull, 48);
    u256_or_shl(r, t.to_idx & 0xFFFFFFFFFFFFull, 96);
    u256_or_shl(r, t.token_id, 144);
    u256_or_shl(r, t.nonce & 0xFFFFFFFFFFull, 176);
    u256_or_shl(r, t.user_fee & 0xFFu, 216);
    u256_or_shl(r, t.to_bjj_sign & 1u, 224);
    return r;
}
HZ_HD Fc sig_tx_compressed_data_v2(const SigTx& t) {
    Fc r = fc_zero();
    u256_or_shl(r, t.from_idx & 0xFFFFFFFFFFFFull, 0);
    u256_or_shl(r, t.to_idx & 0xFFFFFFFFFFFFull, 48);
    u256_or_shl(r, t.amount_f & 0xFFFFFFFFFFull, 96);
    u256_or_shl(r, t.token_id, 136);
    u256_or_shl(r, t.nonce & 0xFFFFFFFFFFull, 168);
    u256_or_shl(r, t.user_fee & 0xFFu, 208);
    u256_or_shl(r, t.to_bjj_sign & 1u, 216);
    return r;
}
HZ_HD Fc sig_e1(const SigTx& t) {   // toEthAddr | amountF << 160 | maxNumBatch << 200
    Fc r = t.to_eth_addr;
    u256_or_shl(r, t.amount_f & 0xFFFFFFFFFFull, 160);
    u256_or_shl(r, t.max_num_batch, 200);
    return r;
}
// M = Poseidon(6)(txCompressedData, e1, toBjjAy, rqTxCompressedDataV2, rqToEthAddr, rqToBjjAy): the transaction's own rq fields, canonical
// (DESIGN.md 8i). K7: the digest-only constant block of t = 7
HZ_HD Fc sig_message(const Fc& tcd, const SigTx& t, const Fc& rq_v2, const Fc& rq_eth, const Fc& rq_ay, const Fr* K7) {
    Fr in[6];
    in[0] = fr_from_canon(tcd);
    in[1] = fr_from_canon(sig_e1(t));
    in[2] = fr_from_canon(t.to_bjj_ay);
    in[3] = fr_from_canon(rq_v2);
    in[4] = fr_from_canon(rq_eth);
    in[5] = fr_from_canon(rq_ay);
    NoSink sink;
    return fr_to_canon(poseidon_hash<7>(in, K7, sink));
}
// the message of a transaction that links to nothing: the rq fields are zero
HZ_HD Fc sig_message(const Fc& tcd, const SigTx& t, const Fr* K7) { return sig_message(tcd, t, fc_zero(), fc_zero(), fc_zero(), K7); }
// src/decode-tx.circom:360-368
HZ_HD bool sig_batch_expired(uint32_t max_num_batch, uint32_t current_num_batch) { return max_num_batch != 0 && max_num_batch < current_num_batch; }

// ---- the curve ----------------------------------------------------------------------------------------------------------------------------
HZ_HD Fr sig_b8x_m() {
    Fr r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = sig_b8x(i);
    return r;
}
HZ_HD Fr sig_b8y_m() {
    Fr r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = sig_b8y(i);
    return r;
}
// 2 P (dbl-2008-hwcd): 4 squarings, 4 products and a A; every point of the curve, T of the operand is not read
HZ_HD PtE sig_dbl(const PtE& p, const Fr& a) {
    const Fr A = fr_sqr(p.X), B = fr_sqr(p.Y), C = fr_dbl(fr_sqr(p.Z)), D = fr_mul(a, A);
    const Fr E = fr_sub(fr_sub(fr_sqr(fr_add(p.X, p.Y)), A), B);
    const Fr G = fr_add(D, B), F = fr_sub(G, C), H = fr_sub(D, B);
    PtE r;
    r.X = fr_mul(E, F); r.Y = fr_mul(G, H); r.T = fr_mul(E, H); r.Z = fr_mul(F, G);
    return r;
}
// P + Q for Q = (X, Y, Z, d T): pte_add with the product by d taken out of the loop
HZ_HD PtE sig_add_dt(const PtE& p, const PtE& q, const Fr& a) {
    const Fr A = fr_mul(p.X, q.X), B = fr_mul(p.Y, q.Y), C = fr_mul(p.T, q.T), D = fr_mul(p.Z, q.Z);
    const Fr E = fr_sub(fr_sub(fr_mul(fr_add(p.X, p.Y), fr_add(q.X, q.Y)), A), B);
    const Fr F = fr_sub(D, C), G = fr_add(D, C), H = fr_sub(B, fr_mul(a, A));
    PtE r;
    r.X = fr_mul(E, F); r.Y = fr_mul(G, H); r.T = fr_mul(E, H); r.Z = fr_mul(F, G);
    return r;
}
// P + (x, y) for an affine table entry (x, y, d x y); the entry (0, 1, 0) leaves the point as it is
HZ_HD PtE sig_add_affine(const PtE& p, const Fr& x, const Fr& y, const Fr& dxy, const Fr& a) {
    const Fr A = fr_mul(p.X, x), B = fr_mul(p.Y, y), C = fr_mul(p.T, dxy);
    const Fr E = fr_sub(fr_sub(fr_mul(fr_add(p.X, p.Y), fr_add(x, y)), A), B);
    const Fr F = fr_sub(p.Z, C), G = fr_add(p.Z, C), H = fr_sub(B, fr_mul(a, A));
    PtE r;
    r.X = fr_mul(E, F); r.Y = fr_mul(G, H); r.T = fr_mul(E, H); r.Z = fr_mul(F, G);
    return r;
}
// k Q over the low 254 bits of k, most significant first
HZ_HD PtE sig_mul_var(const PtE& q, const Fc& k, const Fr& a, const Fr& d) {
    PtE qd = q;
    qd.T = fr_mul(q.T, d);
    PtE acc = pte_identity();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 253; i >= 0; i--) {
        acc = sig_dbl(acc, a);
        uint32_t w = 0;   // k.v[i >> 5] without indexing the limbs at run time
#pragma unroll
        for (int j = 0; j < 8; j++) w = (i >> 5) == j ? k.v[j] : w;
        if ((w >> (i & 31)) & 1u) acc = sig_add_dt(acc, qd, a);
    }
    return acc;
}
// S B8 from the table: one mixed addition per 4-bit digit of S, no doubling
HZ_HD PtE sig_mul_b8(const Fc& s, const Fr* table, const Fr& a) {
    PtE acc = pte_identity();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int w = 0; w < HZ_SIG_B8_WINDOWS; w++) {
        uint32_t limb = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) limb = (w >> 3) == j ? s.v[j] : limb;
        const uint32_t digit = (limb >> (4 * (w & 7))) & 15u;
        const Fr* e = table + ((size_t)w * 16 + digit) * 3;
        acc = sig_add_affine(acc, e[0], e[1], e[2], a);
    }
    return acc;
}
// the table of sig_mul_b8, [64][16][3] Fr: (x, y, d x y) of digit * 16^w * B8. Host only: a thousand inversions, once per process
inline void sig_b8_table(Fr* out) {
    const Fr a = bj_a(), d = bj_d();
    PtE base = pte_from_affine(sig_b8x_m(), sig_b8y_m());
    for (int w = 0; w < HZ_SIG_B8_WINDOWS; w++) {
        PtE e = pte_identity();
        for (int digit = 0; digit < 16; digit++) {
            Fr x, y;
            pte_to_affine(e, x, y);
            Fr* o = out + ((size_t)w * 16 + digit) * 3;
            o[0] = x;
            o[1] = y;
            o[2] = fr_mul(fr_mul(x, y), d);
            e = pte_add(e, base, a, d);
        }
        base = e;
    }
}

// a square root of n (Tonelli-Shanks, r - 1 = 2^28 q), false for a non-residue
HZ_HD bool sig_sqrt(const Fr& n, Fr& root) {
    root = fr_zero();
    if (fr_is_zero(n)) return true;
    const Fr one = fr_one();
    Fr z = n;   // n^((q - 1) / 2): the exponent has 225 bits, the top one set
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 223; i >= 0; i--) {
        z = fr_sqr(z);
        if ((sig_sqrt_zexp(i >> 5) >> (i & 31)) & 1u) z = fr_mul(z, n);
    }
    Fr r = fr_mul(z, n), t = fr_mul(r, z), c;
#pragma unroll
    for (int i = 0; i < 9; i++) c.v[i] = sig_sqrt_root(i);
    int m = 28;
    while (!fr_eq(t, one)) {
        Fr sq = fr_sqr(t);
        int i = 1;
        while (i < m && !fr_eq(sq, one)) {
            sq = fr_sqr(sq);
            i++;
        }
        if (i >= m) return false;
        Fr b = c;
        for (int j = 0; j < m - i - 1; j++) b = fr_sqr(b);
        m = i;
        c = fr_sqr(b);
        t = fr_mul(t, c);
        r = fr_mul(r, b);
    }
    root = r;
    return true;
}
// AySign2Ax (src/lib/utils-bjj.circom with Bits2Point_Strict): the root of (1 - ay^2) / (a - d ay^2) that lies above (r - 1) / 2 iff
// sign. false: there is no root, or the only root is 0 and sign is set
HZ_HD bool sig_recover_ax(const Fr& ay, uint32_t sign, const Fr& a, const Fr& d, Fr& ax) {
    const Fr y2 = fr_sqr(ay);
    const Fr n = fr_mul(fr_sub(fr_one(), y2), fr_inv(fr_sub(a, fr_mul(d, y2))));
    Fr x;
    const bool has = sig_sqrt(n, x);
    const Fc xc = fr_to_canon(x);
    const bool zero = fc_is_zero(xc);
    const bool above = u256_less(sig_half_c(), xc);
    ax = (above != (sign != 0)) ? fr_neg(x) : x;
    return has && !(zero && sign != 0);
}

// EdDSAPoseidonVerifier's verdict on (S, R8) for the key (ay, sign) and the message M; every value canonical. K6: the digest-only
// constant block of t = 6, table: sig_b8_table's. No early exit: the lanes of a wavefront walk the same code.
HZ_HD bool sig_verify(const Fc& s, const Fc& r8x, const Fc& r8y, const Fc& ay_c, uint32_t sign, const Fc& msg, const Fr* K6, const Fr* table) {
    const Fr a = bj_a(), d = bj_d();
    bool ok = u256_less(s, sig_l_c());   // the malleability guard
    const Fr ay = fr_from_canon(ay_c), x1 = fr_from_canon(r8x), y1 = fr_from_canon(r8y);
    Fr ax;
    ok = sig_recover_ax(ay, sign, a, d, ax) && ok;
    Fc hm;
    {
        Fr in[5];
        in[0] = x1;
        in[1] = y1;
        in[2] = ax;
        in[3] = ay;
        in[4] = fr_from_canon(msg);
        NoSink sink;
        hm = fr_to_canon(poseidon_hash<6>(in, K6, sink));
    }
    PtE q = pte_from_affine(ax, ay);
    q = sig_dbl(sig_dbl(sig_dbl(q, a), a), a);
    ok = ok && !fr_is_zero(q.X);   // Z is never zero on the curve: x = 0 iff X = 0
    const PtE p = sig_mul_var(q, hm, a, d);
    const PtE l = sig_mul_b8(s, table, a);
    const Fr t = fr_mul(fr_mul(fr_mul(x1, y1), d), p.T);
    const Fr dx = fr_add(p.Z, t), dy = fr_sub(p.Z, t);
    const Fr nx = fr_add(fr_mul(x1, p.Y), fr_mul(y1, p.X)), ny = fr_sub(fr_mul(y1, p.Y), fr_mul(a, fr_mul(x1, p.X)));
    ok = ok && !fr_is_zero(dx) && !fr_is_zero(dy);
    ok = ok && fr_eq(fr_mul(nx, l.Z), fr_mul(l.X, dx)) && fr_eq(fr_mul(ny, l.Z), fr_mul(l.Y, dy));
    return ok;
}

}  // namespace hz
