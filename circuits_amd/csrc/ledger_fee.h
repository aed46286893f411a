// The fee of an L2 transfer (src/compute-fee.circom) on plain 256-bit integers: amount x table[selector], shifted right by 60 below
// selector 192 (the table holds 2^60 x the factor there, the factor itself from 192 on). An amount is below 2^35 x 10^31 < 2^138 and an
// entry below 2^64, so the product has at most 201 bits. HZ_HD: k_ledger_tx (ledger.hip) and tests/native/u256_check.cpp share it.
#pragma once
#include "u256.h"
#if defined(__HIPCC__)
#include "devcommon.h"   // the device's copy of HZ_FEE_TABLE
#endif

namespace hz {

#if !defined(__HIPCC__)
#define HZ_CONST_ARR static const
#include "gen/fee_table.inc"
#undef HZ_CONST_ARR
#endif

HZ_HD Fc ledger_fee(const Fc& amount, uint32_t sel) {
    Fc fee = u256_mul_u64(amount, HZ_FEE_TABLE[sel]);
    if (sel < 192u) fee = u256_shr60(fee);
    return fee;
}

}  // namespace hz
