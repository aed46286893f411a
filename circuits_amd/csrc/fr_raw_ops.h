// hz_fr_raw_ops (include/hermez_witness.h): ONE routine of fr.h per op code, on raw limbs -- the self test of the routines'
// contracts (tests/fr_contract_common.py). This is the one body that three builds share:
//   fr_raw_inline.hip    the kernels with HZ_FR_INLINE, as every kernel of the step has it      (form 0)
//   fr_raw_outline.hip   the kernels without it: fr_mul / fr_sqr / fr_to_canon / fr_inv out of line (form 1)
//   tests/native/fr_contract_host.cpp   fr_raw_apply on the host, the CPU suite's runner of the same table
// A .hip file defines HZ_FR_RAW_FORM (and, for form 0, HZ_FR_INLINE) before it includes this.
#pragma once
#include <type_traits>
#include "../../include/hermez_witness.h"
#include "fr.h"

namespace hz {

// operands of an op; -1 for a code that is none
constexpr int fr_raw_operands(int op) {
    if (op < 0 || op >= HZ_FRR_COUNT) return -1;
    if (op >= HZ_FRR_DOT1 && op < HZ_FRR_DOT1_ADD) return 2 * (op - HZ_FRR_DOT1 + 1);
    if (op >= HZ_FRR_DOT1_ADD && op < HZ_FRR_FROM_CANON) return 2 * (op - HZ_FRR_DOT1_ADD + 1) + 1;
    switch (op) {
        case HZ_FRR_NEG: case HZ_FRR_DBL: case HZ_FRR_DBL_LAZY: case HZ_FRR_COND_SUB_2P: case HZ_FRR_COND_SUB_4P: case HZ_FRR_COND_SUB_P:
        case HZ_FRR_COND_SUB_P_RARE: case HZ_FRR_IS_ZERO: case HZ_FRR_SQR: case HZ_FRR_FROM_CANON: case HZ_FRR_FROM_U64: case HZ_FRR_TO_CANON:
        case HZ_FRR_CANON_LIMBS: case HZ_FRR_PACK_CANON: case HZ_FRR_INV: case HZ_FRR_INV_FERMAT: return 1;
        case HZ_FRR_SUB2_LAZY: case HZ_FRR_3A_B_C_LAZY: case HZ_FRR_SUB_A_2X: case HZ_FRR_MULADD: return 3;
        case HZ_FRR_SUB3: return 4;
        case HZ_FRR_MULADD2: return 5;
        default: return 2;
    }
}

// o[0..8] = the routine OP on the operands ld(0), ld(1), ... (each an Fr of 9 raw words); nothing else is computed on the way
template <int OP, class L>
HZ_HD void fr_raw_apply(const L& ld, uint32_t* o) {
    static_assert(OP >= 0 && OP < HZ_FRR_COUNT, "fr_raw_apply: no such op");
    Fr r = fr_zero();
    if constexpr (OP == HZ_FRR_ADD) r = fr_add(ld(0), ld(1));
    else if constexpr (OP == HZ_FRR_SUB) r = fr_sub(ld(0), ld(1));
    else if constexpr (OP == HZ_FRR_NEG) r = fr_neg(ld(0));
    else if constexpr (OP == HZ_FRR_DBL) r = fr_dbl(ld(0));
    else if constexpr (OP == HZ_FRR_SUB_LAZY) r = fr_sub_lazy(ld(0), ld(1));
    else if constexpr (OP == HZ_FRR_DBL_LAZY) r = fr_dbl_lazy(ld(0));
    else if constexpr (OP == HZ_FRR_ADD_LAZY) r = fr_add_lazy(ld(0), ld(1));
    else if constexpr (OP == HZ_FRR_SUB2_LAZY) r = fr_sub2_lazy(ld(0), ld(1), ld(2));
    else if constexpr (OP == HZ_FRR_3A_B_C_LAZY) r = fr_3a_b_c_lazy(ld(0), ld(1), ld(2));
    else if constexpr (OP == HZ_FRR_SUB3) r = fr_sub3(ld(0), ld(1), ld(2), ld(3));
    else if constexpr (OP == HZ_FRR_SUB_A_2X) r = fr_sub_a_2x(ld(0), ld(1), ld(2));
    else if constexpr (OP == HZ_FRR_COND_SUB_2P) { r = ld(0); fr_cond_sub_2p(r.v); }
    else if constexpr (OP == HZ_FRR_COND_SUB_4P) r = fr_cond_sub_4p(ld(0));
    else if constexpr (OP == HZ_FRR_COND_SUB_P) r = fr_cond_sub_p(ld(0));
    else if constexpr (OP == HZ_FRR_COND_SUB_P_RARE) r = fr_cond_sub_p_rare(ld(0));
    else if constexpr (OP == HZ_FRR_IS_ZERO) r.v[0] = fr_is_zero(ld(0)) ? 1u : 0u;
    else if constexpr (OP == HZ_FRR_EQ) r.v[0] = fr_eq(ld(0), ld(1)) ? 1u : 0u;
    else if constexpr (OP == HZ_FRR_MUL) r = fr_mul(ld(0), ld(1));
    else if constexpr (OP == HZ_FRR_SQR) r = fr_sqr(ld(0));
    else if constexpr (OP == HZ_FRR_MULADD) r = fr_muladd(ld(0), ld(1), ld(2));
    else if constexpr (OP == HZ_FRR_MULADD2) r = fr_muladd2(ld(0), ld(1), ld(2), ld(3), ld(4));
    else if constexpr (OP >= HZ_FRR_DOT1 && OP < HZ_FRR_FROM_CANON) {
        constexpr bool kAdd = OP >= HZ_FRR_DOT1_ADD;
        constexpr int N = OP - (kAdd ? HZ_FRR_DOT1_ADD : HZ_FRR_DOT1) + 1;
        Fr a[N], b[N];
#pragma unroll
        for (int n = 0; n < N; n++) { a[n] = ld(2 * n); b[n] = ld(2 * n + 1); }
        if constexpr (kAdd) {
            const Fr addend = ld(2 * N);
            r = fr_dot<N>(a, b, &addend);
        } else {
            r = fr_dot<N>(a, b);
        }
    } else if constexpr (OP == HZ_FRR_FROM_CANON || OP == HZ_FRR_FROM_U64) {
        const Fr x = ld(0);
        if constexpr (OP == HZ_FRR_FROM_U64) {
            r = fr_from_u64((uint64_t)x.v[0] | ((uint64_t)x.v[1] << 32));
        } else {
            Fc c;
#pragma unroll
            for (int i = 0; i < 8; i++) c.v[i] = x.v[i];
            r = fr_from_canon(c);
        }
    } else if constexpr (OP == HZ_FRR_TO_CANON || OP == HZ_FRR_PACK_CANON) {
        Fc c;
        if constexpr (OP == HZ_FRR_TO_CANON) c = fr_to_canon(ld(0));
        else c = fr_pack_canon(ld(0));
#pragma unroll
        for (int i = 0; i < 8; i++) r.v[i] = c.v[i];
    } else if constexpr (OP == HZ_FRR_CANON_LIMBS) r = fr_canon_limbs(ld(0));
    else if constexpr (OP == HZ_FRR_INV) r = fr_inv(ld(0));
    else if constexpr (OP == HZ_FRR_INV_FERMAT) r = fr_inv_fermat(ld(0));
    else {   // HZ_FRR_POW: every element has its own exponent
        const Fr e = ld(1);
        r = fr_pow(ld(0), e.v);
    }
#pragma unroll
    for (int i = 0; i < 9; i++) o[i] = r.v[i];
}

// f(std::integral_constant<int, OP>) for the run-time op; false for a code that is none (host side)
template <int OP = 0, class F>
inline bool fr_raw_dispatch(int op, F&& f) {
    if constexpr (OP < HZ_FRR_COUNT) {
        if (op == OP) {
            f(std::integral_constant<int, OP>{});
            return true;
        }
        return fr_raw_dispatch<OP + 1>(op, f);
    } else {
        return false;
    }
}

#if defined(__HIPCC__) && defined(HZ_FR_RAW_FORM)
// one instantiation per op and form. Element i is thread i of the launch: the grid-stride loop iterates only beyond 2048 workgroups.
template <int OP, int FORM>
__global__ __launch_bounds__(256) void fr_raw_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const auto ld = [&](int k) {
            Fr x;
#pragma unroll
            for (int j = 0; j < 9; j++) x.v[j] = in[((size_t)k * n + i) * 9 + j];
            return x;
        };
        uint32_t o[9];
        fr_raw_apply<OP>(ld, o);
#pragma unroll
        for (int j = 0; j < 9; j++) out[i * 9 + j] = o[j];
    }
}

#define HZ_FR_RAW_CAT2(a, b) a##b
#define HZ_FR_RAW_CAT(a, b) HZ_FR_RAW_CAT2(a, b)
// d_in: uint32[fr_raw_operands(op)][n][9], d_out: uint32[n][9]; the caller has checked op and n > 0
hipError_t HZ_FR_RAW_CAT(fr_raw_launch_form, HZ_FR_RAW_FORM)(int op, size_t n, const uint32_t* d_in, uint32_t* d_out, hipStream_t s) {
    size_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    const bool known = fr_raw_dispatch(op, [&](auto c) {
        hipLaunchKernelGGL((fr_raw_kernel<decltype(c)::value, HZ_FR_RAW_FORM>), dim3((unsigned)blocks), dim3(256), 0, s, d_in, d_out, n);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}
#endif

}  // namespace hz
