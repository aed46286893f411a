// The ledger's signature kernels: a lane per transaction, verify-only -- no witness signal is written.
//   k_ledger_sig_msg     txCompressedData, txCompressedDataV2 and e1 packed as plain 256-bit integers, M = Poseidon(6) of the message,
//                        the three per-transaction output rows, the maxNumBatch check (reason 8)
//   k_ledger_sig_verify  Ax from the sender's RESIDENT ay and sign, hm = Poseidon(5), hm * 8A by a doubling ladder, S * B8 from the
//                        fixed-base table, the inversion-free comparison (reason 7)
// A failure lowers the failure word of the semantic kernels ((unit << 8) | reason, atomicMin) or, for hz_ledger_verify_l2, is written
// to the transaction's verdict byte; the verify kernel runs after the message kernel on the same stream, so 7 replaces 8 there as the
// minimum does in the word. The arithmetic is ledger_sig.h's, shared with the host build.
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

__global__ __launch_bounds__(64) void k_ledger_sig_msg(const hz_l2tx* __restrict__ txs, const hz_l2sig* __restrict__ sigs, uint32_t chain_id, uint32_t current_num_batch,
                                                       uint8_t* __restrict__ out_tcd, uint8_t* __restrict__ out_v2, uint8_t* __restrict__ out_hash,
                                                       uint32_t* __restrict__ fail_word, uint8_t* __restrict__ verdict, uint32_t m, uint32_t unit_base) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const bool active = txs[i].from_idx != 0;
    SigTx t;
    t.from_idx = active ? txs[i].from_idx : 0;
    t.to_idx = active ? txs[i].to_idx : 0;
    t.amount_f = active ? txs[i].amount_f : 0;
    t.nonce = active ? txs[i].nonce : 0;
    t.token_id = active ? txs[i].token_id : 0u;
    t.user_fee = active ? txs[i].user_fee : 0u;
    t.to_bjj_sign = active ? sigs[i].to_bjj_sign : 0u;
    t.max_num_batch = active ? sigs[i].max_num_batch : 0u;
    t.to_eth_addr = sig_load32(sigs[i].to_eth_addr);
    t.to_bjj_ay = sig_load32(sigs[i].to_bjj_ay);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        t.to_eth_addr.v[q] = active ? t.to_eth_addr.v[q] : 0u;
        t.to_bjj_ay.v[q] = active ? t.to_bjj_ay.v[q] : 0u;
    }
    const Fc tcd = sig_tx_compressed_data(t, chain_id);
    store_fr(out_tcd + (size_t)i * 32, tcd);
    store_fr(out_v2 + (size_t)i * 32, sig_tx_compressed_data_v2(t));
    store_fr(out_hash + (size_t)i * 32, sig_message(tcd, t, poseidon_consts<7>()));
    const bool expired = active && sig_batch_expired(t.max_num_batch, current_num_batch);
    if (verdict) verdict[i] = expired ? 8u : 0u;
    if (expired && fail_word) atomicMin(fail_word, ((unit_base + i) << 8) | 8u);
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
                             hipStream_t s, uint32_t unit_base) {
    if (m == 0) return hipSuccess;
    const dim3 grid((m + 63) / 64), block(64);
    hipLaunchKernelGGL(k_ledger_sig_msg, grid, block, 0, s, d_txs, d_sigs, chain_id, current_num_batch, d_tcd, d_v2, d_hash, d_fail_word, d_verdict, m, unit_base);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_ledger_sig_verify, grid, block, 0, s, d_txs, d_sigs, (const uint8_t*)d_hash, planes, (const Fr*)b8_table, N, first_idx, d_fail_word, d_verdict, m, unit_base);
    return hipGetLastError();
}

// the fixed-base table, built on the host with the routines the kernel uses
void ledger_sig_b8_table_host(void* out) { sig_b8_table((Fr*)out); }
size_t ledger_sig_b8_table_bytes() { return (size_t)HZ_SIG_B8_FRS * sizeof(Fr); }

}  // namespace hz
