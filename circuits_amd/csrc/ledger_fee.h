// The fee of an L2 transfer (src/compute-fee.circom) on plain 256-bit integers: amount x table[selector], shifted right by 60 below
// selector 192 (the table holds 2^60 x the factor there, the factor itself from 192 on). An amount is below 2^35 x 10^31 < 2^138 and an
// entry below 2^64, so the product has at most 201 bits. HZ_HD: k_ledger_tx (ledger.hip), k_ledger_select
// (ledger_select.h), tests/native/u256_check.cpp and tests/native/ledger_select_check.cpp share it.
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

// src/compute-fee.circom:89-91 ("checks overflow of 128 bits"): the circuit rejects a fee of 2^128 or more -- amount x table[selector]
// below 2^188 under selector 192, below 2^128 from there on. On ledger_fee's result, after the shift, that is one rule for both
// branches: a bit at or above 128. (The 201-bit product never reaches the template's other bound, 2^253.)
HZ_HD bool ledger_fee_overflows(const Fc& fee) { return (fee.v[4] | fee.v[5] | fee.v[6] | fee.v[7]) != 0u; }

}  // namespace hz
