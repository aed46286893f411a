// The ledger's signature kernels: a lane per transaction, verify-only -- no witness signal is written.
//   k_ledger_sig_msg     txCompressedData, txCompressedDataV2 and e1 packed as plain 256-bit integers, M = Poseidon(6) of the message,
//                        the three per-transaction output rows, the maxNumBatch check (reason 8)
//   k_ledger_sig_verify  Ax from the sender's RESIDENT ay and sign, hm = Poseidon(5), hm * 8A by a doubling ladder, S * B8 from the
//                        fixed-base table, the inversion-free comparison (reason 7)
// A failure lowers the failure word of the semantic kernels ((unit << 8) | reason, atomicMin) or, for hz_ledger_verify_l2, is written
// to the transaction's verdict byte; the verify kernel runs after the message kernel on the same stream, so 7 replaces 8 there as the
// minimum does in the word. The arithmetic is ledger_sig.h's, shared with the host build.
// The atomic calls hand the message kernel the transactions' own rq fields; k_ledger_rq (ledger.hip) reads the V2 rows
// behind it on the same stream. For a call that does not verify,
//   k_ledger_sig_v2      the V2 rows alone: the packing of the message kernel without its Poseidon
// The rq fields lie plane-major, [3][m][32] (V2, toEthAddr, toBjjAy), then the m offset bytes: the host lays hz_l2rq out so.
#define HZ_FR_INLINE 1
#include <hip/hip_runtime.h>
#include "../../include/hermez_witness.h"
#include "devcommon.h"
#include "ledger_sig.h"

namespace hz {

// 32 bytes of a hz_l2sig member: the struct is 4-byte aligned, not 16
__device__ __forceinline__ Fc sig_load32(const uint8_t* p) {
    const uint32_t* q = (const uint32_t*)p;
    Fc r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = q[i];
    return r;
}

// rq field f of transaction i, zero without an rq array and for a NOP
__device__ __forceinline__ Fc sig_load_rq(const uint8_t* __restrict__ rq, uint32_t f, uint32_t i, uint32_t m, bool active) {
    Fc r = fc_zero();
    if (rq && active) r = load_fr(rq + ((size_t)f * m + i) * 32);
    return r;
}

__global__ __launch_bounds__(64) void k_ledger_sig_msg(const hz_l2tx* __restrict__ txs, const hz_l2sig* __restrict__ sigs, const uint8_t* __restrict__ rq, uint32_t chain_id,
                                                       uint32_t current_num_batch, uint8_t* __restrict__ out_tcd, uint8_t* __restrict__ out_v2, uint8_t* __restrict__ out_hash,
                                                       uint32_t* __restrict__ fail_word, uint8_t* __restrict__ verdict, uint32_t m, uint32_t unit_base) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const bool active = txs[i].from_idx != 0;
    const SigTx t = sig_load_tx(txs[i], sigs[i], active);
    const Fc tcd = sig_tx_compressed_data(t, chain_id);
    store_fr(out_tcd + (size_t)i * 32, tcd);
    store_fr(out_v2 + (size_t)i * 32, sig_tx_compressed_data_v2(t));
    store_fr(out_hash + (size_t)i * 32,
             sig_message(tcd, t, sig_load_rq(rq, 0, i, m, active), sig_load_rq(rq, 1, i, m, active), sig_load_rq(rq, 2, i, m, active), poseidon_consts<7>()));
    const bool expired = active && sig_batch_expired(t.max_num_batch, current_num_batch);
    if (verdict) verdict[i] = expired ? 8u : 0u;
    if (expired && fail_word) atomicMin(fail_word, ((unit_base + i) << 8) | 8u);
}

// the V2 rows alone: what k_ledger_rq reads when the call verifies no signature
__global__ __launch_bounds__(64) void k_ledger_sig_v2(const hz_l2tx* __restrict__ txs, const hz_l2sig* __restrict__ sigs, uint8_t* __restrict__ out_v2, uint32_t m) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    store_fr(out_v2 + (size_t)i * 32, sig_tx_compressed_data_v2(sig_load_tx(txs[i], sigs[i], txs[i].from_idx != 0)));
}

__global__ __launch_bounds__(64) void k_ledger_sig_verify(const hz_l2tx* __restrict__ txs, const hz_l2sig* __restrict__ sigs, const uint8_t* __restrict__ msg_hash,
                                                          const uint8_t* __restrict__ planes, const Fr* __restrict__ b8_table, uint32_t N, uint64_t first_idx,
                                                          uint32_t* __restrict__ fail_word, uint8_t* __restrict__ verdict, uint32_t m, uint32_t unit_base) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t from = txs[i].from_idx;
    if (from == 0 || from < first_idx || from - first_idx >= N) return;   // a NOP is not verified (the host has refused an index outside the state)
    const uint32_t acct = (uint32_t)(from - first_idx);
    const Fc e0 = load_fr(planes + (size_t)acct * 32);
    const Fc ay = load_fr(planes + ((size_t)2 * N + acct) * 32);
    const uint32_t sign = (e0.v[2] >> 8) & 1u;
    const bool ok = sig_verify(sig_load32(sigs[i].s), sig_load32(sigs[i].r8x), sig_load32(sigs[i].r8y), ay, sign, load_fr(msg_hash + (size_t)i * 32),
                               poseidon_consts<6>(), b8_table);
    if (!ok) {
        if (verdict) verdict[i] = 7u;
        if (fail_word) atomicMin(fail_word, ((unit_base + i) << 8) | 7u);
    }
}

hipError_t launch_ledger_sig(const hz_l2tx* d_txs, const hz_l2sig* d_sigs, uint32_t chain_id, uint32_t current_num_batch, uint8_t* d_tcd, uint8_t* d_v2, uint8_t* d_hash,
                             const uint8_t* planes, const void* b8_table, uint32_t N, uint64_t first_idx, uint32_t* d_fail_word, uint8_t* d_verdict, uint32_t m,
                             hipStream_t s, uint32_t unit_base, const uint8_t* d_rq) {
    if (m == 0) return hipSuccess;
    const dim3 grid((m + 63) / 64), block(64);
    hipLaunchKernelGGL(k_ledger_sig_msg, grid, block, 0, s, d_txs, d_sigs, d_rq, chain_id, current_num_batch, d_tcd, d_v2, d_hash, d_fail_word, d_verdict, m, unit_base);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_ledger_sig_verify, grid, block, 0, s, d_txs, d_sigs, (const uint8_t*)d_hash, planes, (const Fr*)b8_table, N, first_idx, d_fail_word, d_verdict, m, unit_base);
    return hipGetLastError();
}

// the V2 rows of a call that verifies nothing, for the link check
hipError_t launch_ledger_sig_v2(const hz_l2tx* d_txs, const hz_l2sig* d_sigs, uint8_t* d_v2, uint32_t m, hipStream_t s) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ledger_sig_v2, dim3((m + 63) / 64), dim3(64), 0, s, d_txs, d_sigs, d_v2, m);
    return hipGetLastError();
}

// the link fields of an L2 row on the host, through the packing the kernels use (hz_ledger_plan_atomic); zero for a NOP
void ledger_sig_link_fields_host(const hz_l2tx& tx, const hz_l2sig& sig, Fc* v2, Fc* eth, Fc* ay) {
    const SigTx t = sig_load_tx(tx, sig, tx.from_idx != 0);
    *v2 = sig_tx_compressed_data_v2(t);
    *eth = t.to_eth_addr;
    *ay = t.to_bjj_ay;
}

// the fixed-base table, built on the host with the routines the kernel uses
void ledger_sig_b8_table_host(void* out) { sig_b8_table((Fr*)out); }
size_t ledger_sig_b8_table_bytes() { return (size_t)HZ_SIG_B8_FRS * sizeof(Fr); }

}  // namespace hz
