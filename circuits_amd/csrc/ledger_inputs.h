// RollupMain's packed inputs of an applied batch (hz_ledger_main_inputs): the descriptor table -- one descriptor per input
// signal of the context's packed layout, made by mi_plan from the signal's name, the shape and what kind of call was applied -- and the
// packing of the signals that are computed from the uploaded rows. The planner is plain C++ (hz_ledger_plan_main_inputs runs it without a
// device); the packing routines are HZ_HD, shared by k_ledger_main_inputs (ledger.hip) and the stand-alone host build
// (tests/native/ledger_main_inputs_check.cpp). txCompressedData / txCompressedDataV2 of an L2 row are ledger_sig.h's own routines, so the
// rows equal those k_ledger_sig_msg / k_ledger_sig_v2 write whether or not the call verified.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/hermez_witness.h"
#include "ledger_l1.h"
#include "ledger_sig.h"

namespace hz {

// ---- the packing (device and host) ------------------------------------------------------------------------------------------------------
// txCompressedData of an L1 row, as the coordinator writes it: no nonce, no fee, no sign
HZ_HD Fc mi_l1_tx_compressed_data(uint32_t chain_id, uint64_t from_idx, uint64_t to_idx, uint32_t token_id) {
    Fc r = fc_zero();
    u256_or_shl(r, HZ_SIG_CONST, 0);
    u256_or_shl(r, chain_id & 0xFFFFu, 32);
    u256_or_shl(r, from_idx & 0xFFFFFFFFFFFFull, 48);
    u256_or_shl(r, to_idx & 0xFFFFFFFFFFFFull, 96);
    u256_or_shl(r, token_id, 144);
    return r;
}

HZ_HD Fc mi_eth160(const uint32_t* eth5) {
    Fc r = fc_zero();
#pragma unroll
    for (int i = 0; i < 5; i++) r.v[i] = eth5[i];
    return r;
}

// 16 bits as 16 bytes, bit b of `half` in byte b: word q of the result holds bits 4 q .. 4 q + 3
HZ_HD uint32_t mi_bits4(uint32_t half, int q) {
    const uint32_t n = (half >> (4 * q)) & 15u;
    return (n & 1u) | ((n & 2u) << 7) | ((n & 4u) << 14) | ((n & 8u) << 21);
}

// bits 16 g .. 16 g + 15 of a compressed key, g = 0 .. 15: the half of limb g / 2 they lie in (the kernel loads that limb alone)
HZ_HD uint32_t mi_half(uint32_t limb, uint32_t g) { return (limb >> (16 * (g & 1u))) & 0xFFFFu; }
HZ_HD uint32_t mi_key_half(const Fc& key, uint32_t g) {
    uint32_t w = 0;   // key.v[g >> 1] without indexing the limbs at run time
#pragma unroll
    for (int j = 0; j < 8; j++) w = (g >> 1) == (uint32_t)j ? key.v[j] : w;
    return mi_half(w, g);
}

// a computed signal of an L1 row. x: the row as the per-row kernels read it (from_idx is auxFromIdx on a create row), r: the L1 kernel's;
// the caller's fromIdx of a create row is 0
HZ_HD Fc mi_l1_value(uint32_t kind, uint32_t chain_id, const hz_l2tx& x, const LedgerL1Dev& r, bool create) {
    const uint64_t from = create ? 0ull : x.from_idx;
    switch (kind) {
        case HZ_MI_KIND_TX_COMPRESSED_DATA: return mi_l1_tx_compressed_data(chain_id, from, x.to_idx, x.token_id);
        case HZ_MI_KIND_AMOUNT_F: return u256_u64(x.amount_f);
        case HZ_MI_KIND_FROM_IDX: return u256_u64(from);
        case HZ_MI_KIND_TO_IDX: return u256_u64(x.to_idx);
        case HZ_MI_KIND_ON_CHAIN: return u256_u64(1);
        case HZ_MI_KIND_NEW_ACCOUNT: return u256_u64(create ? 1 : 0);
        case HZ_MI_KIND_LOAD_AMOUNT_F: return u256_u64(r.load_amount_f);
        case HZ_MI_KIND_FROM_ETH_ADDR: return mi_eth160(r.from_eth);
        default: return fc_zero();   // txCompressedDataV2, the signed destination, the links and the signature: L2's
    }
}

// a computed signal of L2 row j of m. rq: the links as uploaded -- the three fields plane-major, [3][m][32], then the m offsets -- or null.
// A NOP (from_idx == 0) is zero but for the constant and the chain id of txCompressedData; its sig and rq entries are not looked at
HZ_HD Fc mi_l2_value(uint32_t kind, uint32_t chain_id, const hz_l2tx& x, const hz_l2sig& g, const uint8_t* rq, uint32_t j, uint32_t m) {
    const bool active = x.from_idx != 0;
    const bool linked = active && rq != nullptr;
    switch (kind) {
        case HZ_MI_KIND_TX_COMPRESSED_DATA: return sig_tx_compressed_data(sig_load_tx(x, g, active), chain_id);
        case HZ_MI_KIND_TX_COMPRESSED_DATA_V2: return sig_tx_compressed_data_v2(sig_load_tx(x, g, active));
        case HZ_MI_KIND_AMOUNT_F: return u256_u64(active ? x.amount_f : 0);
        case HZ_MI_KIND_FROM_IDX: return u256_u64(active ? x.from_idx : 0);
        case HZ_MI_KIND_TO_IDX: return u256_u64(active ? x.to_idx : 0);
        case HZ_MI_KIND_TO_BJJ_AY: return sig_load32_if(g.to_bjj_ay, active);
        case HZ_MI_KIND_TO_ETH_ADDR: return sig_load32_if(g.to_eth_addr, active);
        case HZ_MI_KIND_MAX_NUM_BATCH: return u256_u64(active ? g.max_num_batch : 0u);
        case HZ_MI_KIND_S: return sig_load32_if(g.s, active);
        case HZ_MI_KIND_R8X: return sig_load32_if(g.r8x, active);
        case HZ_MI_KIND_R8Y: return sig_load32_if(g.r8y, active);
        case HZ_MI_KIND_RQ_OFFSET: return u256_u64(linked ? rq[(size_t)3 * m * 32 + j] : 0u);
        case HZ_MI_KIND_RQ_V2: return linked ? sig_load32_if(rq + (size_t)j * 32, true) : fc_zero();
        case HZ_MI_KIND_RQ_TO_ETH_ADDR: return linked ? sig_load32_if(rq + ((size_t)m + j) * 32, true) : fc_zero();
        case HZ_MI_KIND_RQ_TO_BJJ_AY: return linked ? sig_load32_if(rq + ((size_t)2 * m + j) * 32, true) : fc_zero();
        default: return fc_zero();   // onChain, newAccount, loadAmountF, fromEthAddr: L1's
    }
}

// ---- the table (host) --------------------------------------------------------------------------------------------------------------------
struct MiShape {
    uint32_t n_tx = 0, n_levels = 0, max_l1 = 0, max_fee = 0;
};

// one signal's descriptor before it has addresses: rows x inner elements of `width` bytes; COPY / BROADCAST read `source` from row r0
struct MiSignal {
    uint32_t kind = HZ_MI_KIND_ZERO, source = HZ_MI_SRC_NONE, width = 32, inner = 1;
    uint64_t r0 = 0, rows = 0;
};

// the rule of one input signal of RollupMain (src/rollup-main.circom's signal inputs); false: no such signal
inline bool mi_signal(const char* name, const MiShape& s, uint32_t flags, MiSignal& d) {
    const std::string n(name);
    const uint64_t T = s.n_tx, F = s.max_fee;
    const bool exits = flags & HZ_MI_EXITS, creates = flags & HZ_MI_CREATES, sigs = flags & HZ_MI_SIGS, rq = flags & HZ_MI_RQ, aux = flags & HZ_MI_AUX;
    d = MiSignal{};
    auto copy = [&](uint32_t source, uint64_t r0, uint64_t rows, uint32_t inner = 1) {
        d.kind = HZ_MI_KIND_COPY, d.source = source, d.r0 = r0, d.rows = rows, d.inner = inner;
        return true;
    };
    auto copy_if = [&](bool have, uint32_t source, uint64_t rows) {
        if (have) return copy(source, 0, rows);
        d.rows = rows;   // zeros
        return true;
    };
    auto rows_kind = [&](bool have, uint32_t kind, uint64_t rows) {
        d.rows = rows;
        if (have) d.kind = kind, d.source = HZ_MI_SRC_ROWS;
        return true;
    };
    // the globals
    if (n == "oldLastIdx") return copy(HZ_MI_SRC_GLOBALS, 0, 1);
    if (n == "globalChainID") return copy(HZ_MI_SRC_GLOBALS, 1, 1);
    if (n == "currentNumBatch") return copy(HZ_MI_SRC_GLOBALS, 2, 1);
    if (n == "oldStateRoot") return copy(HZ_MI_SRC_OUT + 25, 0, 1);
    if (n == "imInitStateRootFee") return copy(HZ_MI_SRC_OUT + 14, T - 1, 1);
    // the intermediate signals: the first nTx - 1 rows
    if (n == "imOnChain") return rows_kind(true, HZ_MI_KIND_ON_CHAIN, T - 1);
    if (n == "imStateRoot") return copy(HZ_MI_SRC_OUT + 14, 0, T - 1);
    if (n == "imAccFeeOut") return copy(HZ_MI_SRC_OUT + 15, 0, T - 1, (uint32_t)F);
    if (n == "imExitRoot") return copy_if(exits, HZ_MI_SRC_EXIT + 4, T - 1);
    if (n == "imOutIdx") {
        if (creates) return copy(HZ_MI_SRC_CREATE + 4, 0, T - 1);
        d.kind = HZ_MI_KIND_BROADCAST, d.source = HZ_MI_SRC_GLOBALS, d.rows = T - 1;
        return true;
    }
    // per transaction: packed from the rows
    static const struct { const char* name; uint32_t kind; int needs; /* 0 nothing, 1 sigs, 2 rq */ } computed[] = {
        {"txCompressedData", HZ_MI_KIND_TX_COMPRESSED_DATA, 0}, {"txCompressedDataV2", HZ_MI_KIND_TX_COMPRESSED_DATA_V2, 0}, {"amountF", HZ_MI_KIND_AMOUNT_F, 0},
        {"fromIdx", HZ_MI_KIND_FROM_IDX, 0}, {"toIdx", HZ_MI_KIND_TO_IDX, 0}, {"toBjjAy", HZ_MI_KIND_TO_BJJ_AY, 1}, {"toEthAddr", HZ_MI_KIND_TO_ETH_ADDR, 1},
        {"maxNumBatch", HZ_MI_KIND_MAX_NUM_BATCH, 1}, {"onChain", HZ_MI_KIND_ON_CHAIN, 0}, {"newAccount", HZ_MI_KIND_NEW_ACCOUNT, 0},
        {"rqOffset", HZ_MI_KIND_RQ_OFFSET, 2}, {"rqTxCompressedDataV2", HZ_MI_KIND_RQ_V2, 2}, {"rqToEthAddr", HZ_MI_KIND_RQ_TO_ETH_ADDR, 2},
        {"rqToBjjAy", HZ_MI_KIND_RQ_TO_BJJ_AY, 2}, {"s", HZ_MI_KIND_S, 1}, {"r8x", HZ_MI_KIND_R8X, 1}, {"r8y", HZ_MI_KIND_R8Y, 1},
        {"loadAmountF", HZ_MI_KIND_LOAD_AMOUNT_F, 0}, {"fromEthAddr", HZ_MI_KIND_FROM_ETH_ADDR, 0}};
    for (const auto& c : computed)
        if (n == c.name) return rows_kind(c.needs == 0 || (c.needs == 1 && sigs) || (c.needs == 2 && rq), c.kind, T);
    if (n == "fromBjjCompressed") {
        d.kind = HZ_MI_KIND_KEY_BITS, d.source = HZ_MI_SRC_KEYS, d.width = 1, d.inner = 256, d.rows = T;
        return true;
    }
    // per transaction: where the apply left them
    if (n == "auxToIdx") return copy_if(aux, HZ_MI_SRC_AUX_TO_IDX, T);
    static const char* const create_names[4] = {"auxFromIdx", "isOld0_1", "oldKey1", "oldValue1"};
    static const char* const exit_names[4] = {"newExit", "isOld0_2", "oldKey2", "oldValue2"};
    for (uint32_t q = 0; q < 4; q++) {
        if (n == create_names[q]) return copy_if(creates, HZ_MI_SRC_CREATE + q, T);
        if (n == exit_names[q]) return copy_if(exits, HZ_MI_SRC_EXIT + q, T);
    }
    static const char* const leaf[7] = {"tokenID", "nonce", "sign", "balance", "ay", "ethAddr", "siblings"};
    for (uint32_t p = 0; p < 3; p++)   // processor 1, processor 2, the fee transactions
        for (uint32_t q = 0; q < 7; q++)
            if (n == std::string(leaf[q]) + (char)('1' + p)) return copy(HZ_MI_SRC_OUT + (p == 2 ? 16 : 7 * p) + q, 0, p == 2 ? F : T, q == 6 ? s.n_levels + 1 : 1);
    // per fee slot
    if (n == "feeIdxs") return copy(HZ_MI_SRC_FEE_IDXS, 0, F);
    if (n == "feePlanTokens") return copy(HZ_MI_SRC_FEE_PLAN_TOKENS, 0, F);
    if (n == "imStateRootFee") return copy(HZ_MI_SRC_OUT + 23, 0, F - 1);
    if (n == "imFinalAccFee") return copy(HZ_MI_SRC_OUT + 24, 0, F);
    return false;
}
#define HZ_MI_SIGNALS 64   // input signals of RollupMain

// the table of a layout; -> "" or what is wrong with it. Every signal of RollupMain exactly once, every range 32-byte aligned, inside
// [0, bytes) and clear of the others
inline std::string mi_plan(size_t n, const char* const* names, const uint64_t* offsets, const uint32_t* widths, const uint64_t* flat_lens, uint64_t bytes,
                           const MiShape& s, uint32_t flags, std::vector<MiSignal>& out) {
    out.assign(n, MiSignal{});
    if (s.n_tx < 1 || s.max_fee < 1 || s.max_l1 > s.n_tx) return "a shape with nTx = 0, maxFeeTx = 0 or maxL1Tx > nTx";
    if (flags >> 6) return "unknown flags";
    if (n != HZ_MI_SIGNALS) return "the layout has " + std::to_string(n) + " signals, RollupMain has " + std::to_string(HZ_MI_SIGNALS);
    std::vector<std::pair<uint64_t, size_t>> order;
    for (size_t i = 0; i < n; i++) {
        if (!names[i] || !mi_signal(names[i], s, flags, out[i])) return std::string("unknown signal ") + (names[i] ? names[i] : "(null)");
        for (size_t j = 0; j < i; j++)
            if (!strcmp(names[i], names[j])) return std::string("signal ") + names[i] + " twice";
        const MiSignal& d = out[i];
        if (widths[i] != d.width) return std::string(names[i]) + ": element width " + std::to_string(widths[i]) + ", not " + std::to_string(d.width);
        if (flat_lens[i] != d.rows * d.inner) return std::string(names[i]) + ": flat length " + std::to_string(flat_lens[i]) + ", not " + std::to_string(d.rows * d.inner);
        if (offsets[i] & 31u) return std::string(names[i]) + ": offset " + std::to_string(offsets[i]) + " is not 32-byte aligned";
        order.push_back({offsets[i], i});
    }
    std::sort(order.begin(), order.end());
    for (size_t q = 0; q < n; q++) {
        const size_t i = order[q].second;
        const uint64_t end = offsets[i] + flat_lens[i] * widths[i], next = q + 1 < n ? order[q + 1].first : bytes;
        if (end > next) return std::string(names[i]) + (q + 1 < n ? ": its range overlaps the next signal's" : ": its range ends beyond the buffer");
    }
    return "";
}

// ---- the descriptor as the kernel reads it -------------------------------------------------------------------------------------------------
// elements = outer x inner of ebytes each at dst_off; first_block: the signal's first block of the launch (256 elements a block; the
// bit signal 16 elements a lane); src: the first byte COPY / BROADCAST read (row r0 applied)
struct MainInputsDesc {
    uint64_t dst_off;
    const uint8_t* src;
    uint32_t kind, ebytes, outer, inner, first_block, pad;
};
inline uint32_t mi_blocks(const MiSignal& d) {
    const uint64_t lanes = d.width == 1 ? (d.rows * d.inner + 15) / 16 : d.rows * d.inner;
    return (uint32_t)((lanes + 255) / 256);
}

}  // namespace hz
