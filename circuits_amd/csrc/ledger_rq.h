// The atomic link of an L2 transaction (src/rq-tx-verifier.circom:91-93 fed by src/rollup-main.circom:286-309). Row r of a
// batch of n_rows rows, the n_l1 L1 rows first, names with rqOffset k the row whose three link fields -- txCompressedDataV2, the signed
// toEthAddr, the signed toBjjAy -- its own rq fields must equal as full field elements:
//   k = 0        nothing: the multiplexer's input 0 is the constant 0, the comparison is against (0, 0, 0)
//   k = 1 .. 3   row r + k
//   k = 4 .. 7   row r - (8 - k)   (7: the previous row, 4: four back)
// A position outside 0 .. n_rows - 1, an L1 row and an L2 NOP have link fields (0, 0, 0). Everything here is HZ_HD: k_ledger_rq, the
// host's hz_ledger_plan_atomic and tests/native/ledger_atomic_check.cpp share the routines.
#pragma once
#include <stdint.h>
#include "fr.h"

namespace hz {

#define HZ_RQ_REASON 13u
#define HZ_RQ_MAX_OFFSET 7u

// the row transaction r is linked to, or -1 where the link fields are zero whatever the batch holds: offset 0, a position before row 0
// or past the last row, an L1 row. (An L2 NOP compares against zeros too: the caller's to see, it takes the transaction.)
HZ_HD int64_t rq_target_row(uint64_t r, uint32_t k, uint64_t n_l1, uint64_t n_rows) {
    k &= HZ_RQ_MAX_OFFSET;
    if (k == 0u) return -1;
    const int64_t t = (int64_t)r + (k < 4u ? (int64_t)k : (int64_t)k - 8);
    if (t < (int64_t)n_l1 || t >= (int64_t)n_rows) return -1;
    return t;
}

// all three fields equal, limb for limb: no reduction, an rq field is compared as the integer it was given as
HZ_HD bool rq_fields_match(const Fc& rq_v2, const Fc& rq_eth, const Fc& rq_ay, const Fc& v2, const Fc& eth, const Fc& ay) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d |= (rq_v2.v[i] ^ v2.v[i]) | (rq_eth.v[i] ^ eth.v[i]) | (rq_ay.v[i] ^ ay.v[i]);
    return d == 0u;
}

}  // namespace hz
