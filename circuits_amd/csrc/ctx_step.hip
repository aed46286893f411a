// The kernel schedule of a step: hz_witness_enqueue and what it launches, the tail of a tx-sharded step, per-kernel profiling.
// EVERY wait and record of a step is in this file -- the launchers of the kernel files take arguments and one stream and launch.
// Streams and events belong to the context (ctx_internal.h, made by hz_ctx_create in ctx.hip); which stream plays which role in this
// step is resolved once per enqueue (StepStreams). DESIGN.md section 5 describes the schedules in the order they read here:
// step_main_throughput, step_main_partitioned, step_main_sharded (+ enqueue_tail), step_rollup_tx, built from the pieces above them.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>
#include "hostutil.h"
#include "kernels.h"
#include "tx_dev.h"
#include "ctx_internal.h"

using namespace hz;
using namespace hzl;

#define HZ_TRY(expr)                          \
    do {                                      \
        const hz_status _st = (expr);         \
        if (_st != HZ_OK) return _st;         \
    } while (0)

// ---- profiling: one record per launch, in launch order ---------------------------------------------------------
// which kernel writes a block of the tx / fee / hash-inputs sections (for algorithmic byte counts)
static const char* block_owner(const Layout& lo, int sec, const Block& b) {
    const std::string& n = b.name;
    auto has = [&](const char* t) { return n.find(t) != std::string::npos; };
    if (sec == lo.sec_hi && lo.p.tmpl != T_WITHDRAW) return "hash_inputs";
    const bool fee = (sec == lo.sec_fee);
    if (has(".hash1Old.") || has(".hash1New.") || has("St1Hash.") || has("St2Hash.") || has("StFeePck.") || has("s1OldValue") || has("s2OldValue"))
        return fee ? "fee_hash" : "hash4";
    if (has(".topSwitcher.") || has(".checkOldInput.") || has(".areKeyEquals.") || has(".keysOk.") || (has(".processor") && n.size() > 8 && n.compare(n.size() - 8, 8, ".newRoot") == 0))
        return fee ? "fee_back" : "rtx_back";
    if (has(".processor")) return fee ? "fee_smt" : "smt";
    // the standalone SMTProcessor: the same signals without a ".processor" in their names, and the chain launch is recorded as "smt"
    if (lo.p.tmpl == T_SMT_PROCESSOR && (n == "main.enabled" || has("main.n2bOld") || has("main.n2bNew") || has("main.smtLevIns.") || has("main.xors[") ||
                                         has("main.sm[") || has("main.levels[")))
        return "smt";
    if (!fee && lo.p.tmpl == T_ROLLUP_MAIN && has(".hashSig.")) return "sig_hash";
    if (has(".sigVerifier.mulFix.") || has(".sigVerifier.snum2bits") || has(".sigVerifier.compConstant")) return "eddsa_fix";
    if (has(".sigVerifier.eqCheck")) return "eddsa_final";
    if (has(".getAx.") || has(".sigVerifier.")) return "eddsa";
    if (has(".s3.out") || has(".s4.out") || has(".s5.out") || n == "main.hasherInputs.L1L2TxsData") return "rtx_back";
    if (!fee && lo.p.tmpl == T_ROLLUP_MAIN && has(".feeAccumulator.")) return "fee_acc";   // (standalone RollupTx: part of its front kernel)
    return fee ? "fee_front" : "front";
}
static uint64_t owner_bytes(const hz_ctx* c, const char* owner) {
    uint64_t n = 0;
    const Layout& lo = c->lo;
    if (!strcmp(owner, "withdraw") || !strcmp(owner, "withdraw_sha")) {   // the SHA part owns the sha256 blocks and the bit decompositions
        uint64_t sha = 0;
        for (size_t si = 0; si < lo.sections.size(); si++)
            for (const Block& b : lo.sections[si].blocks)
                if (b.name.find("main.hasherInputs.") == 0) sha += (uint64_t)b.count * lo.sections[si].n_units;
        return (!strcmp(owner, "withdraw_sha") ? sha : lo.total - sha) * 32;
    }
    for (size_t si = 0; si < lo.sections.size(); si++)
        for (const Block& b : lo.sections[si].blocks)
            if (!strcmp(block_owner(lo, (int)si, b), owner)) n += (uint64_t)b.count * lo.sections[si].n_units;
    return n * 32;
}
// The SMT chain a k_smt launch walks. It names the mark buffer the launch keeps and the counter of zm_skip it adds what it left in
// place to (its value), and the profile record of the launch remembers it: hz_profile_get subtracts what the chain's launches counted.
enum SmtChain { CHAIN_TX = 0, CHAIN_FEE = 1, CHAIN_LAST_TX = 2 };
struct ProfScope {
    hz_ctx* c;
    hipStream_t s;
    bool on;
    ProfScope(hz_ctx* c_, hipStream_t s_, const char* name, uint64_t units, int chain = -1) : c(c_), s(s_), on(c_->profiling) {
        if (!on) return;
        if (c->prof_used == c->prof.size()) {
            hz_ctx::Prof p;
            p.name = name; p.bytes = owner_bytes(c, name); p.units = units; p.ms = 0; p.chain = chain;
            (void)hipEventCreate(&p.e0);
            (void)hipEventCreate(&p.e1);
            c->prof.push_back(p);
        }
        (void)hipEventRecord(c->prof[c->prof_used].e0, s);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(c->prof[c->prof_used].e1, s);
        c->prof_used++;
    }
};
// one launch on a stream with its profile record (a record that spans several launches opens a ProfScope itself)
#define HZ_PROF(c, s, name, units, launch)      \
    do {                                        \
        ProfScope _ps(c, s, name, units);       \
        HZ_HIP(launch);                         \
    } while (0)

// ---- argument blocks ------------------------------------------------------------------------------------------
static SmtProcDesc make_proc(const SmtProcOff& o, uint32_t siblings, int which /*0: p1, 1: p2, 2: fee, 3: SMTProcessor main*/) {
    SmtProcDesc d;
    d.o = o;
    d.siblings = siblings;
    if (which == 1) {
        d.sc_oldkey = SC_KEY_S2OLD; d.sc_newkey = SC_KEY_2; d.sc_fnc0 = SC_P2_FNC0; d.sc_fnc1 = SC_P2_FNC1; d.sc_isold0 = SC_ISOLD0_2;
        d.sc_leaf_old = SC_LEAF_P2OLD; d.sc_leaf_new = SC_LEAF_P2NEW; d.sc_root_old = SC_ROOT_P2OLD; d.sc_root_new = SC_ROOT_P2NEW;
        d.cid_alias_old = C_RTX_P2_ALIAS_OLD; d.cid_alias_new = C_RTX_P2_ALIAS_NEW; d.cid_levins = C_RTX_P2_LEVINS; d.cid_sm_final = C_RTX_P2_SM_FINAL;
    } else {
        d.sc_oldkey = SC_KEY_S1OLD; d.sc_newkey = SC_KEY_1; d.sc_fnc0 = SC_P1_FNC0; d.sc_fnc1 = SC_P1_FNC1; d.sc_isold0 = SC_ISOLD0_1;
        d.sc_leaf_old = SC_LEAF_P1OLD; d.sc_leaf_new = SC_LEAF_P1NEW; d.sc_root_old = SC_ROOT_P1OLD; d.sc_root_new = SC_ROOT_P1NEW;
        if (which == 0) {
            d.cid_alias_old = C_RTX_P1_ALIAS_OLD; d.cid_alias_new = C_RTX_P1_ALIAS_NEW; d.cid_levins = C_RTX_P1_LEVINS; d.cid_sm_final = C_RTX_P1_SM_FINAL;
        } else if (which == 3) {
            d.cid_alias_old = C_SMTP_ALIAS_OLD; d.cid_alias_new = C_SMTP_ALIAS_NEW; d.cid_levins = C_SMTP_LEVINS; d.cid_sm_final = C_SMTP_SM_FINAL;
        } else {
            d.cid_alias_old = C_FEE_P_ALIAS_OLD; d.cid_alias_new = C_FEE_P_ALIAS_NEW; d.cid_levins = C_FEE_P_LEVINS; d.cid_sm_final = C_FEE_P_SM_FINAL;
        }
    }
    return d;
}

static Hash4Args make_hash4_rtx(uint8_t* base, Fr* sc, uint32_t n_units, const RtxOff& r) {
    Hash4Args h;
    memset(&h, 0, sizeof h);
    h.base = base; h.scratch = sc; h.n_units = n_units; h.n_jobs = 4;
    const PoseidonOff hs[4] = {r.oldSt1Hash, r.oldSt2Hash, r.newSt1Hash, r.newSt2Hash};
    const PoseidonOff h1[4] = {r.p1.hash1Old, r.p2.hash1Old, r.p1.hash1New, r.p2.hash1New};
    const uint32_t key[4] = {SC_KEY_S1OLD, SC_KEY_S2OLD, SC_KEY_1, SC_KEY_2};
    const uint32_t leaf[4] = {SC_LEAF_P1OLD, SC_LEAF_P2OLD, SC_LEAF_P1NEW, SC_LEAF_P2NEW};
    for (int j = 0; j < 4; j++) {
        HashJob& J = h.job[j];
        J.hs = hs[j]; J.h1 = h1[j]; J.sc_in = SC_HS_IN + 4 * j; J.sc_key = key[j]; J.sc_leaf = leaf[j];
        J.mux_off = ~0u; J.sc_ins = 0; J.sc_oldvalue = 0; J.out_sig = ~0u;
    }
    h.job[0].mux_off = r.mux16 + MX_S1OLDVALUE; h.job[0].sc_ins = SC_ISP1INSERT; h.job[0].sc_oldvalue = SC_OLDVALUE1;
    h.job[1].mux_off = r.mux16 + MX_S2OLDVALUE; h.job[1].sc_ins = SC_ISP2INSERT; h.job[1].sc_oldvalue = SC_OLDVALUE2;
    return h;
}

// the kernels of the transactions of a step (RollupMain's transaction section, or standalone RollupTx): signature check, hash-state,
// SMT chains, back
struct TxArgs { EddsaArgs ea; Hash4Args h4; SmtArgs sa; RtxBackArgs ba; };
static TxArgs make_tx(hz_ctx* c, uint8_t* base, uint32_t n_units, bool is_main) {
    const Layout& lo = c->lo;
    Fr* sc = (Fr*)c->sc_tx.p;
    ErrBuf* err = (ErrBuf*)c->err.p;
    const uint32_t u0 = is_main ? c->sh_first : 0, ucnt = is_main ? c->sh_count : 0;
    const uint32_t upi = lo.sections[lo.sec_tx].upi;
    TxArgs T;
    memset(&T, 0, sizeof T);
    EddsaArgs& ea = T.ea;
    ea.base = base; ea.scratch = sc; ea.err = err; ea.n_units = n_units; ea.upi = upi; ea.ed = lo.rtx.ed;
    ea.u0 = u0; ea.ucnt = ucnt;
    ea.in_onChain = ~0u;
    if (is_main && !getenv("HZ_ED_NO_PRE_SPLIT")) {
        const auto& mi = lo.mi;
        ea.in_onChain = mi.onChain; ea.in_newAccount = mi.newAccount; ea.in_auxFromIdx = mi.auxFromIdx; ea.in_sign1 = mi.sign1; ea.in_ay1 = mi.ay1;
        ea.in_txCompressedData = mi.txCompressedData; ea.in_fromBjjCompressed = mi.fromBjjCompressed;
    }
    T.h4 = make_hash4_rtx(base, sc, n_units, lo.rtx);
    T.h4.u0 = u0; T.h4.ucnt = ucnt;
    SmtArgs& sa = T.sa;
    sa.base = base; sa.scratch = sc; sa.err = err; sa.n_units = n_units; sa.n_levels = (uint32_t)lo.p.L + 1; sa.n_proc = 2; sa.upi = upi;
    sa.p[0] = make_proc(lo.rtx.p1, is_main ? lo.mi.siblings1 : lo.rtxi.siblings1, 0);
    sa.p[1] = make_proc(lo.rtx.p2, is_main ? lo.mi.siblings2 : lo.rtxi.siblings2, 1);
    sa.u0 = u0; sa.ucnt = ucnt;
    RtxBackArgs& ba = T.ba;
    ba.base = base; ba.glob_base = is_main ? sec_ptr(c, lo.sec_glob) : nullptr; ba.scratch = sc; ba.err = err; ba.n_units = n_units; ba.L = (uint32_t)lo.p.L;
    ba.is_main = is_main ? 1 : 0;
    ba.upi = upi; ba.B = lo.n_inst;
    ba.u0 = u0; ba.ucnt = ucnt;
    ba.p[0] = sa.p[0]; ba.p[1] = sa.p[1];
    ba.s3 = lo.rtx.s3; ba.s4 = lo.rtx.s4; ba.s5 = lo.rtx.s5;
    if (is_main) {
        ba.im_stateroot = lo.mi.imStateRoot; ba.im_exitroot = lo.mi.imExitRoot; ba.g_initfeeroot = lo.g.imInitStateRootFee;
        ba.main_l1l2amt = lo.rtx.main_l1l2amt; ba.n2bAmount = lo.dec.n2bAmount;
    } else {
        ba.o_newStateRoot = lo.rtxi.o_newStateRoot; ba.o_newExitRoot = lo.rtxi.o_newExitRoot;
    }
    return T;
}

static MainFrontArgs make_main_front(hz_ctx* c) {
    const Layout& lo = c->lo;
    MainFrontArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.tx_base = sec_ptr(c, lo.sec_tx); fa.fee_base = sec_ptr(c, lo.sec_fee); fa.glob_base = sec_ptr(c, lo.sec_glob);
    fa.scratch = (Fr*)c->sc_tx.p; fa.err = (ErrBuf*)c->err.p; fa.nTx = (uint32_t)lo.p.nTx; fa.L = (uint32_t)lo.p.L; fa.F = (uint32_t)lo.p.F; fa.B = lo.n_inst;
    fa.g = lo.g; fa.mi = lo.mi; fa.fi = lo.fi; fa.dec = lo.dec; fa.rtx = lo.rtx;
    fa.u0 = c->sh_first; fa.ucnt = c->sh_count;
    return fa;
}

static HashInputsArgs make_hi(hz_ctx* c, bool is_main) {
    const Layout& lo = c->lo;
    HashInputsArgs a;
    memset(&a, 0, sizeof a);
    a.hi_base = sec_ptr(c, lo.sec_hi);
    a.err = (ErrBuf*)c->err.p;
    a.nTx = (uint32_t)lo.p.nTx; a.L = (uint32_t)lo.p.L; a.maxL1 = (uint32_t)lo.p.maxL1; a.F = (uint32_t)lo.p.F; a.is_main = is_main; a.B = lo.n_inst;
    a.hi = lo.hi;
    a.msg = (uint8_t*)c->msg.p; a.chain = (uint32_t*)c->chain.p;
    if (is_main) {
        a.glob_base = sec_ptr(c, lo.sec_glob); a.tx_base = sec_ptr(c, lo.sec_tx); a.fee_base = sec_ptr(c, lo.sec_fee);
        a.tx_scratch = (Fr*)c->sc_tx.p; a.fee_scratch = (Fr*)c->sc_fee.p;
        a.g = lo.g; a.mi_onChain = lo.mi.onChain; a.fi_feeIdxs = lo.fi.feeIdxs; a.dec = lo.dec; a.rtx_s5 = lo.rtx.s5; a.rtx_main_l1l2amt = lo.rtx.main_l1l2amt;
    }
    return a;
}

// ---- the pieces the schedules share ------------------------------------------------------------------------------
// Which of the context's streams plays which role in THIS step. Profiling mode 2 (`exclusive`): every kernel alone on the device --
// every role is the launch stream and nothing is piped. This is the one place of the schedule that reads c->exclusive.
struct StepStreams {
    hipStream_t main;   // front, hash-state, SMT chains, back; every other stream is joined to it before the step returns
    hipStream_t sig;    // variable-base half of the signature check, then the equality
    hipStream_t fix;    // fixed-base half (+ RollupMain's fee accumulators)
    hipStream_t fee;    // sigL2Hash, the fee chain, the early tail
    hipStream_t sha;    // the expansion groups of a HashInputs that runs on `fee`; NULL: not piped
};
static StepStreams step_streams(const hz_ctx* c, hipStream_t caller) {
    // partitioned contexts run their main sequence on the CU-masked stream, ordered after / before the caller's stream by two events
    hipStream_t m = c->partitioned ? c->s_main : caller;
    if (c->exclusive) return StepStreams{m, m, m, m, nullptr};
    return StepStreams{m, c->s_ed, c->s_fix, c->s_fee, c->s_sha};
}

// the SMT chain kernel: one launch, one profile entry under `name` (CHAIN_LAST_TX has no entry: NULL)
static hipError_t enqueue_smt_chain(hz_ctx* c, SmtChain chain, const SmtArgs& sa0, const char* name, hipStream_t s) {
    SmtArgs sa = sa0;
    sa.zmark = (uint16_t*)(chain == CHAIN_FEE ? c->zm_fee.p : c->zm_tx.p);   // (marks are per unit: the last transactions are nobody else's this step)
    sa.skipped = (c->profiling && c->zm_skip.p) ? (unsigned long long*)c->zm_skip.p + chain : nullptr;
    // the last transactions (4 lanes per batch beside the fee stream's other work): never the latency form, no trace, no record of
    // their own -- what they leave in place is subtracted from the transaction chain's record
    if (chain == CHAIN_LAST_TX) return launch_smt(sa, s);
    bool lat = c->smt_lat;
    if (!lat && c->smt_lat_few && c->partitioned && c->device >= 0 && c->device < 16) {
        MaskedPool& P = masked_pool();
        std::lock_guard<std::mutex> g(P.mu);
        lat = P.alive[c->device] <= 2;
    }
    sa.pos3_dense = lat ? (const Fr*)c->pos3.p : nullptr;
    if (chain == CHAIN_TX && getenv("HZ_SMT_TRACE")) {   // tools/experiments/smt_trace.py
        const uint32_t nl = sa.ucnt ? sa.ucnt : sa.n_units;
        const size_t waves = (size_t)((nl + 127) / 128) * 2 * 2 * sa.n_proc;
        if (c->smt_trace.bytes < waves * 32) { if (c->smt_trace.alloc(waves * 32) != hipSuccess) return hipErrorOutOfMemory; }
        (void)hipMemsetAsync(c->smt_trace.p, 0, waves * 32, s);
        sa.trace = (unsigned long long*)c->smt_trace.p;
    }
    ProfScope ps(c, s, name, sa.n_units, chain);
    return launch_smt(sa, s);
}

// The signature check: the two halves (S*B8 and R8 + h*8A) are independent -- two kernels on two streams beside the hash / SMT
// chain -- then the equality. Waits for ev_reset, ev_front and (feeacc: RollupMain) ev_sighash; RECORDS ev_ed on st.sig when the
// check is complete: the schedule joins it to the main stream.
static hz_status enqueue_sig_check(hz_ctx* c, const StepStreams& st, EddsaArgs ea, const MainFrontArgs* feeacc) {
    const uint32_t n_units = ea.n_units;
    {
        // the split form (launches of <= HZ_ED_SPLIT_MAX signatures) parks its numerators in a side buffer: 84.7 KB per signature,
        // allocated by the first launch that takes that form and sized for it (a shard: its own range, not the section); the throughput
        // form keeps the lane state of the fixed-base kernel there (1.7 KB per eight signatures)
        const size_t need = eddsa_side_bytes(ea.ucnt ? ea.ucnt : n_units);
        if (need > c->ed_side.bytes || (need && !c->ed_side.p)) {
            HZ_HIP(hipStreamSynchronize(st.sig));
            HZ_HIP(hipStreamSynchronize(st.fix));
            HZ_HIP(c->ed_side.alloc(need));
        }
    }
    ea.side = (uint32_t*)c->ed_side.p;
    HZ_HIP(hipStreamWaitEvent(st.fix, c->ev_front, 0));
    HZ_PROF(c, st.fix, "eddsa_fix", n_units, launch_eddsa_fix(ea, st.fix));
    // RollupMain's fee accumulators (k_main_feeacc) need the front step only and feed nothing downstream: they follow the fixed-base
    // half on its stream -- 10 + 1.5 ms against the 16.6 ms of the ladder beside it (one batch: 4.5 + 0.6 against 6.8) -- and are
    // joined with it (ev_fix -> the signature stream -> the launch stream)
    if (feeacc) HZ_PROF(c, st.fix, "fee_acc", n_units, launch_main_feeacc(*feeacc, st.fix));
    HZ_HIP(hipEventRecord(c->ev_fix, st.fix));
    HZ_HIP(hipStreamWaitEvent(st.sig, c->ev_reset, 0));   // the error buffer, the inputs' scatter
    {
        ProfScope ps(c, st.sig, "eddsa", n_units);
        // a RollupMain launch small enough for the split form starts the point half of its prologue BEFORE the front step is done
        // (k_eddsa_pre_a reads inputs only); the hash half, or the whole prologue of every other launch, reads the front step's
        // scratch and -- RollupMain -- DecodeTx's sigL2Hash, which k_main_sighash leaves at the head of the fee stream
        const bool point_first = eddsa_split_form(ea) && ea.in_onChain != ~0u;
        if (point_first) HZ_HIP(launch_eddsa_pre_point(ea, st.sig));
        HZ_HIP(hipStreamWaitEvent(st.sig, c->ev_front, 0));
        if (feeacc) HZ_HIP(hipStreamWaitEvent(st.sig, c->ev_sighash, 0));
        HZ_HIP(point_first ? launch_eddsa_pre_hash(ea, st.sig) : launch_eddsa_pre(ea, st.sig));
        HZ_HIP(launch_eddsa_ladder(ea, st.sig));
    }
    HZ_HIP(hipStreamWaitEvent(st.sig, c->ev_fix, 0));
    HZ_PROF(c, st.sig, "eddsa_final", n_units, launch_eddsa_final(ea, st.sig));
    HZ_HIP(hipEventRecord(c->ev_ed, st.sig));
    return HZ_OK;
}

// the transactions behind the front kernel, on one stream: hash-state, then the SMT chains and the back kernel
static hz_status enqueue_tx_hash4(hz_ctx* c, const TxArgs& T, hipStream_t s) {
    HZ_PROF(c, s, "hash4", T.h4.n_units, launch_hash4(T.h4, s));
    return HZ_OK;
}
static hz_status enqueue_tx_chains(hz_ctx* c, const TxArgs& T, hipStream_t s) {
    HZ_HIP(enqueue_smt_chain(c, CHAIN_TX, T.sa, "smt", s));
    HZ_PROF(c, s, "rtx_back", T.ba.n_units, launch_rtx_back(T.ba, s));
    return HZ_OK;
}
// The LAST transaction of every batch ahead of the others, on `s` (behind hash4): its four chains with root slots of their own, its
// back kernel, and phase H (k_da_mask) of every unit. T is changed: the main launches leave these units and phase H out (`skip_mod`,
// `skip_h`), so no signal is written twice and a failing constraint of that transaction is recorded once.
static hz_status enqueue_last_tx(hz_ctx* c, TxArgs& T, hipStream_t s) {
    const Layout& lo = c->lo;
    SmtArgs sl = T.sa;
    sl.u0 = (uint32_t)lo.p.nTx - 1; sl.ucnt = lo.n_inst; sl.ustride = (uint32_t)lo.p.nTx;
    sl.p[0].sc_root_old = SC_EROOT_P1OLD; sl.p[0].sc_root_new = SC_EROOT_P1NEW; sl.p[1].sc_root_old = SC_EROOT_P2OLD; sl.p[1].sc_root_new = SC_EROOT_P2NEW;
    HZ_HIP(enqueue_smt_chain(c, CHAIN_LAST_TX, sl, nullptr, s));
    RtxBackArgs bl = T.ba;
    bl.u0 = sl.u0; bl.ucnt = sl.ucnt; bl.ustride = sl.ustride;
    bl.p[0] = sl.p[0]; bl.p[1] = sl.p[1];
    bl.skip_h = 1;
    HZ_HIP(launch_rtx_back(bl, s));
    HZ_HIP(launch_da_mask(T.ba, s));
    T.sa.skip_mod = T.ba.skip_mod = (uint32_t)lo.p.nTx;
    T.ba.skip_h = 1;
    return HZ_OK;
}

// the fee transactions (RollupMain's fee section, or standalone FeeTx): front, hash-state, chain, back on one stream
static hz_status enqueue_fee(hz_ctx* c, uint8_t* base, uint32_t n_units, bool is_main, hipStream_t s) {
    const Layout& lo = c->lo;
    Fr* sc = (Fr*)c->sc_fee.p;
    ErrBuf* err = (ErrBuf*)c->err.p;
    FeeFrontArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.base = base; fa.glob_base = is_main ? sec_ptr(c, lo.sec_glob) : nullptr; fa.scratch = sc; fa.err = err; fa.n_units = n_units; fa.is_main = is_main;
    fa.upi = lo.sections[lo.sec_fee].upi; fa.B = lo.n_inst;
    fa.fee = lo.fee;
    uint32_t sib;
    if (is_main) {
        const MainFeeInOff& f = lo.fi;
        fa.in_feePlanToken = f.feePlanTokens; fa.in_feeIdx = f.feeIdxs; fa.in_accFee = f.imFinalAccFee; fa.in_tokenID = f.tokenID3; fa.in_nonce = f.nonce3;
        fa.in_sign = f.sign3; fa.in_balance = f.balance3; fa.in_ay = f.ay3; fa.in_ethAddr = f.ethAddr3; fa.im_stateRootFee = f.imStateRootFee;
        fa.g_initfeeroot = lo.g.imInitStateRootFee;
        sib = f.siblings3;
    } else {
        const FeeTxInOff& f = lo.feei;
        fa.in_feePlanToken = f.feePlanToken; fa.in_feeIdx = f.feeIdx; fa.in_accFee = f.accFee; fa.in_tokenID = f.tokenID; fa.in_nonce = f.nonce;
        fa.in_sign = f.sign; fa.in_balance = f.balance; fa.in_ay = f.ay; fa.in_ethAddr = f.ethAddr; fa.in_oldStateRoot = f.oldStateRoot;
        sib = f.siblings;
    }
    HZ_PROF(c, s, "fee_front", n_units, launch_fee_front(fa, s));
    Hash4Args h;
    memset(&h, 0, sizeof h);
    h.base = base; h.scratch = sc; h.n_units = n_units; h.n_jobs = 2;
    h.job[0] = HashJob{lo.fee.oldHash, lo.fee.p.hash1Old, SC_HS_IN + 0, SC_KEY_S1OLD, SC_LEAF_P1OLD, ~0u, 0, 0, ~0u};
    h.job[1] = HashJob{lo.fee.newHash, lo.fee.p.hash1New, SC_HS_IN + 8, SC_KEY_1, SC_LEAF_P1NEW, ~0u, 0, 0, ~0u};
    HZ_PROF(c, s, "fee_hash", n_units, launch_hash4(h, s));
    SmtArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.base = base; sa.scratch = sc; sa.err = err; sa.n_units = n_units; sa.n_levels = (uint32_t)lo.p.L + 1; sa.n_proc = 1; sa.upi = lo.sections[lo.sec_fee].upi;
    sa.p[0] = make_proc(lo.fee.p, sib, 2);
    HZ_HIP(enqueue_smt_chain(c, CHAIN_FEE, sa, "fee_smt", s));
    FeeBackArgs fb;
    memset(&fb, 0, sizeof fb);
    fb.base = base; fb.scratch = sc; fb.err = err; fb.n_units = n_units; fb.is_main = is_main; fb.upi = lo.sections[lo.sec_fee].upi; fb.p = sa.p[0];
    fb.im_stateRootFee = is_main ? lo.fi.imStateRootFee : 0; fb.o_newStateRoot = lo.fee.o_newStateRoot;
    HZ_PROF(c, s, "fee_back", n_units, launch_fee_back(fb, s));
    return HZ_OK;
}

// HashInputs on `s`: the message (`part`: HI_WHOLE, or HI_HEADER behind an HI_BODY launch), the SHA-256 chain, the expansion.
// The chain is sequential, the expansion (a 0.7 GB store stream per batch) is not. With a second stream `pipe` and a message of at
// least 64 blocks the blocks are split into HZ_SHA_GROUPS groups: group g's expansion runs on `pipe` (behind ev_sha[g]) while `s` chains
// group g + 1, and `s` joins at the end (ev_sha[last]). The tail of a step is then about chain + expansion / groups instead of
// chain + expansion. pipe == s or NULL, or a shorter message: one chain launch, one expansion, both on `s`.
#ifndef HZ_SHA_GROUPS
#define HZ_SHA_GROUPS 8
#endif
static hz_status enqueue_hash_inputs(hz_ctx* c, const HashInputsArgs& a, hipStream_t s, hipStream_t pipe, uint32_t part = HI_WHOLE) {
    constexpr uint32_t n_ev = sizeof(c->ev_sha) / sizeof(c->ev_sha[0]);
    static_assert(HZ_SHA_GROUPS >= 1 && HZ_SHA_GROUPS < n_ev, "one event per chain group and one for the end of the expansion");
    HZ_HIP(launch_hi_prep(a, part, s));
    const uint32_t nb = (uint32_t)a.hi.sha.nblocks;
    const bool piped = pipe && pipe != s && nb >= 64;
    const uint32_t groups = piped ? HZ_SHA_GROUPS : 1u;
    const uint32_t per = (nb + groups - 1) / groups;
    for (uint32_t g = 0, b0 = 0; b0 < nb; g++, b0 += per) {
        const uint32_t b1 = std::min(nb, b0 + per);
        HZ_HIP(launch_sha_chain(a, b0, b1, s));
        if (piped) {
            HZ_HIP(hipEventRecord(c->ev_sha[g], s));
            HZ_HIP(hipStreamWaitEvent(pipe, c->ev_sha[g], 0));
        }
        HZ_HIP(launch_sha_expand_range(a, b0, b1 - b0, piped ? pipe : s));
    }
    if (piped) {
        HZ_HIP(hipEventRecord(c->ev_sha[n_ev - 1], pipe));
        HZ_HIP(hipStreamWaitEvent(s, c->ev_sha[n_ev - 1], 0));
    }
    return HZ_OK;
}
// RollupMain's HashInputs, with its profile record
static hz_status enqueue_main_hash_inputs(hz_ctx* c, hipStream_t s, hipStream_t pipe, uint32_t part = HI_WHOLE) {
    ProfScope ps(c, s, "hash_inputs", (uint64_t)c->lo.hi.sha.nblocks);
    return enqueue_hash_inputs(c, make_hi(c, true), s, pipe, part);
}

// ---- the schedules ------------------------------------------------------------------------------
// Every schedule starts behind ev_reset (recorded on st.main by enqueue_impl) and returns with every stream it used joined to st.main.

// The head of every RollupMain step. DecodeTx's sigL2Hash (k_main_sighash: one Poseidon of width 7 over INPUTS; read by the signature
// prologue's hash half only) heads the fee stream -- beside the front kernel and the prologue's point half, in front of a chain that
// has time to spare; RECORDS ev_sighash. with_fee_chain: the fee transactions, independent of the transactions, follow it there;
// RECORDS ev_fee. The front kernel on st.main; RECORDS ev_front. Then the signature check on st.fix and st.sig (RECORDS ev_ed on st.sig:
// the schedule joins it to st.main) and the hash-state kernel on st.main. T: the transactions' argument blocks, for the chains and
// the back kernel the schedule orders itself.
static hz_status enqueue_main_head(hz_ctx* c, const StepStreams& st, bool with_fee_chain, TxArgs& T) {
    const Layout& lo = c->lo;
    const MainFrontArgs fa = make_main_front(c);
    HZ_HIP(hipStreamWaitEvent(st.fee, c->ev_reset, 0));
    HZ_PROF(c, st.fee, "sig_hash", (uint64_t)fa.nTx * fa.B, launch_main_sighash(fa, st.fee));
    HZ_HIP(hipEventRecord(c->ev_sighash, st.fee));
    if (with_fee_chain) {
        HZ_TRY(enqueue_fee(c, fa.fee_base, lo.sections[lo.sec_fee].n_units, true, st.fee));
        HZ_HIP(hipEventRecord(c->ev_fee, st.fee));
    }
    HZ_PROF(c, st.main, "front", (uint64_t)fa.nTx * fa.B, launch_main_front(fa, st.main));
    HZ_HIP(hipEventRecord(c->ev_front, st.main));
    T = make_tx(c, fa.tx_base, lo.sections[lo.sec_tx].n_units, true);
    HZ_TRY(enqueue_sig_check(c, st, T.ea, &fa));
    return enqueue_tx_hash4(c, T, st.main);
}

// RollupMain, whole batches, unmasked streams: the EARLY TAIL. HashInputs does not wait for the SMT chains of every transaction. Its
// SHA-256 message needs the data-availability bits (front kernel), the last fee transaction's root (fee chain, own stream from the
// start) and ONE value of the chains: the LAST transaction's exit root. That transaction's four chains are evaluated first, as a
// launch of their own (4 lanes per batch) on the fee stream right after the hash-state kernel, then the message, the sequential
// chain and the expansion follow there while the main stream hashes the other 2047 transactions of every batch.
// The 3.6 ms of one-wavefront chain latency and the expansion leave the end of the step.
static hz_status step_main_throughput(hz_ctx* c, const StepStreams& st) {
    TxArgs T;
    HZ_TRY(enqueue_main_head(c, st, true, T));
    HZ_HIP(hipEventRecord(c->ev_hash4, st.main));
    HZ_HIP(hipStreamWaitEvent(st.fee, c->ev_hash4, 0));   // the fee chain was enqueued on st.fee before: newStateRoot is ready when these run
    HZ_TRY(enqueue_last_tx(c, T, st.fee));
    HZ_TRY(enqueue_main_hash_inputs(c, st.fee, st.sha));
    HZ_HIP(hipEventRecord(c->ev_tail, st.fee));
    HZ_TRY(enqueue_tx_chains(c, T, st.main));   // (without the last transactions)
    HZ_HIP(hipStreamWaitEvent(st.main, c->ev_tail, 0));
    HZ_HIP(hipStreamWaitEvent(st.main, c->ev_ed, 0));   // join the signature stream
    return HZ_OK;
}

// RollupMain, CU-partitioned context (a few batches, latency): the tail stays on the main stream. The chain cannot start before the
// roots are known (they sit in the first block), but the rest of the message is laid out on the fee stream while the SMT chains run
// (EARLY PREP). HashInputs needs the roots and the data-availability bits, not the signatures: it runs beside the ladders, chain and
// expansion on the main stream, one launch each -- the expansion piped over the fee stream in eight groups, as the throughput
// schedule does, costs a single batch 1.25 ms: 9.1 against 7.86 ms.
static hz_status step_main_partitioned(hz_ctx* c, const StepStreams& st) {
    TxArgs T;
    HZ_TRY(enqueue_main_head(c, st, true, T));
    HZ_HIP(hipStreamWaitEvent(st.fee, c->ev_front, 0));
    HZ_HIP(launch_da_mask(T.ba, st.fee));
    T.ba.skip_h = 1;
    HZ_HIP(launch_hi_prep(make_hi(c, true), HI_BODY, st.fee));
    HZ_HIP(hipEventRecord(c->ev_tail, st.fee));
    HZ_TRY(enqueue_tx_chains(c, T, st.main));
    HZ_HIP(hipStreamWaitEvent(st.main, c->ev_fee, 0));
    HZ_HIP(hipStreamWaitEvent(st.main, c->ev_tail, 0));
    HZ_TRY(enqueue_main_hash_inputs(c, st.main, nullptr, HI_HEADER));
    HZ_HIP(hipStreamWaitEvent(st.main, c->ev_ed, 0));   // join the signature stream
    return HZ_OK;
}

// RollupMain, tx-sharded (multi-GPU): this rank's range of the transactions. The fee transactions and HashInputs run once the other
// ranks' records are imported: hz_witness_enqueue_tail / hz_witness_enqueue_tail_chain (enqueue_tail below).
static hz_status step_main_sharded(hz_ctx* c, const StepStreams& st) {
    TxArgs T;
    HZ_TRY(enqueue_main_head(c, st, false, T));
    HZ_TRY(enqueue_tx_chains(c, T, st.main));
    HZ_HIP(hipStreamWaitEvent(st.main, c->ev_ed, 0));   // join the signature stream
    return HZ_OK;
}

// standalone RollupTx: the signature ladders only need the front step and run beside the hash / SMT chain
static hz_status step_rollup_tx(hz_ctx* c, const StepStreams& st) {
    const Layout& lo = c->lo;
    RtxFrontArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.base = sec_ptr(c, 0); fa.scratch = (Fr*)c->sc_tx.p; fa.err = (ErrBuf*)c->err.p; fa.N = lo.sections[0].n_units; fa.L = (uint32_t)lo.p.L; fa.F = (uint32_t)lo.p.F;
    fa.in = lo.rtxi; fa.rtx = lo.rtx;
    HZ_PROF(c, st.main, "front", fa.N, launch_rtx_front(fa, st.main));
    HZ_HIP(hipEventRecord(c->ev_front, st.main));
    const TxArgs T = make_tx(c, fa.base, fa.N, false);
    HZ_TRY(enqueue_sig_check(c, st, T.ea, nullptr));
    HZ_TRY(enqueue_tx_hash4(c, T, st.main));
    HZ_TRY(enqueue_tx_chains(c, T, st.main));
    HZ_HIP(hipStreamWaitEvent(st.main, c->ev_ed, 0));   // join the signature stream
    return HZ_OK;
}

// the standalone mains that are one or two launches
static hz_status step_small_main(hz_ctx* c, const StepStreams& st) {
    const Layout& lo = c->lo;
    ErrBuf* err = (ErrBuf*)c->err.p;
    hipStream_t s = st.main;
    switch (lo.p.tmpl) {
        case T_DECODE_TX: {
            DecMainArgs da;
            memset(&da, 0, sizeof da);
            da.base = sec_ptr(c, 0); da.err = err; da.N = lo.sections[0].n_units; da.L = (uint32_t)lo.p.L; da.in = lo.deci; da.dec = lo.dec;
            HZ_HIP(launch_dec_main(da, s));
            break;
        }
        case T_FEE_TX:
            return enqueue_fee(c, sec_ptr(c, 0), lo.sections[0].n_units, false, s);
        case T_HASH_STATE:
            HZ_HIP(launch_hash_state_main(sec_ptr(c, 0), lo.sections[0].n_units, lo.hs, s));
            break;
        case T_WITHDRAW: {
            WithdrawArgs wa;
            memset(&wa, 0, sizeof wa);
            wa.base = sec_ptr(c, 0); wa.err = err; wa.N = lo.sections[0].n_units; wa.L = (uint32_t)lo.p.L; wa.wd = lo.wd;
            // the SHA-256 bit witness (store bound) runs beside the Poseidon / SMT part (integer bound) on a side stream
            HZ_HIP(hipStreamWaitEvent(st.sig, c->ev_reset, 0));
            HZ_PROF(c, st.sig, "withdraw_sha", wa.N, launch_withdraw_sha(wa, st.sig));
            HZ_HIP(hipEventRecord(c->ev_ed, st.sig));
            HZ_PROF(c, s, "withdraw", wa.N, launch_withdraw(wa, s));
            HZ_HIP(hipStreamWaitEvent(s, c->ev_ed, 0));
            break;
        }
        case T_HASH_INPUTS:
            return enqueue_hash_inputs(c, make_hi(c, false), s, st.fee);
        case T_SMT_PROCESSOR: case T_SMT_VERIFIER: {
            SmtMainArgs ma;
            memset(&ma, 0, sizeof ma);
            ma.base = sec_ptr(c, 0); ma.scratch = (Fr*)c->sc_fee.p; ma.err = err; ma.N = lo.sections[0].n_units; ma.n_levels = (uint32_t)lo.p.L;
            if (lo.p.tmpl == T_SMT_VERIFIER) {
                ma.vin = lo.smtvi; ma.ver = lo.smtv;
                HZ_HIP(launch_smtver_main(ma, s));
                break;
            }
            ma.pin = lo.smtpi; ma.proc = make_proc(lo.smtp, lo.smtpi.siblings, 3);
            HZ_HIP(launch_smtproc_front(ma, s));
            SmtArgs sa;
            memset(&sa, 0, sizeof sa);
            sa.base = ma.base; sa.scratch = ma.scratch; sa.err = err; sa.n_units = ma.N; sa.n_levels = ma.n_levels; sa.n_proc = 1; sa.upi = 1;
            sa.p[0] = ma.proc;
            HZ_HIP(enqueue_smt_chain(c, CHAIN_FEE, sa, "smt", s));   // (one chain per unit in the fee scratch: the fee chain's marks and counter)
            HZ_HIP(launch_smtproc_back(ma, s));
            break;
        }
        default: {   // the gadget mains
            GadgetArgs ga;
            memset(&ga, 0, sizeof ga);
            ga.base = sec_ptr(c, 0); ga.err = err; ga.N = lo.sections[0].n_units; ga.F = (uint32_t)lo.p.F; ga.io = lo.gad;
            ga.n2b40 = lo.rtx.n2bLoadAmountF; ga.df = lo.rtx.dfLoadAmount; ga.bu = lo.rtx.bu; ga.feeAcc = lo.rtx.feeAcc; ga.st = lo.rtx.st;
            ga.rq_n2b = lo.rtx.rq_n2b;
            for (int m = 0; m < 3; m++) ga.rq_mux[m] = lo.rtx.rq_mux[m];
            if (lo.p.tmpl == T_AYSIGN2AX) HZ_HIP(launch_ay_sign_2_ax_main(ga, lo.rtx.ed, s));
            else HZ_HIP(launch_gadget(lo.p.tmpl, ga, s));
            break;
        }
    }
    return HZ_OK;
}

// ---- the step -------------------------------------------------------------------------------------------------
// error buffer header: minkey = ~0, filter (= ~0 unless this is a second pass), count = 0
static hz_status reset_err(hz_ctx* c, hipStream_t s, unsigned long long filter) {
    HZ_HIP(hipMemsetAsync(c->err.p, 0xFF, 16, s));
    HZ_HIP(hipMemsetAsync((uint8_t*)c->err.p + 16, 0, 8, s));
    if (filter != ~0ull) {
        c->filter_stage = filter;
        HZ_HIP(hipMemcpyAsync((uint8_t*)c->err.p + 8, &c->filter_stage, 8, hipMemcpyHostToDevice, s));
    } else {
        // the per-instance minima are reset only when the last pass lowered one (or nobody checked): a clean serving loop pays nothing
        if (c->inst_min_dirty || !c->checked) HZ_HIP(hipMemsetAsync(c->inst_min.p, 0xFF, c->inst_min.bytes, s));
        c->inst_min_dirty = false;
        c->checked = false;
    }
    return HZ_OK;
}

// filter != ~0: a second pass over the SAME inputs (ctx_internal.h): inputs staged for the next step stay staged, the per-instance minima stay.
hz_status hz::enqueue_impl(hz_ctx* c, void* stream, unsigned long long filter) {
    const bool rerun = filter != ~0ull;
    if (!c) return set_err(HZ_ERR_ARG, "hz_witness_enqueue: null context");
    const Layout& lo = c->lo;
    for (size_t i = 0; i < c->input_set.size(); i++)
        if (!c->input_set[i]) return set_err(HZ_ERR_INPUT, "Not all inputs have been set: %s", lo.inputs[i].name.c_str());
    HZ_HIP(hipSetDevice(c->device));
    // the legacy default stream has implicit-synchronisation semantics that do not mix with the
    // context's non-blocking side streams: a NULL stream means "the context's own stream"
    hipStream_t s_user = stream ? (hipStream_t)stream : c->s_main;
    const StepStreams st = step_streams(c, s_user);
    hipStream_t s = st.main;
    if (c->any_staged && !rerun) HZ_TRY(scatter_staged_inputs(c, s_user));
    if (c->inputs_pending) {
        HZ_HIP(hipStreamWaitEvent(s_user, c->ev_inputs, 0));
        c->inputs_pending = false;
    }
    if (s != s_user) {
        HZ_HIP(hipEventRecord(c->ev_user_in, s_user));
        HZ_HIP(hipStreamWaitEvent(s, c->ev_user_in, 0));
    }
    HZ_TRY(reset_err(c, s, filter));
    if (c->zm_reset) {   // (before ev_reset: every side stream waits for it before its first kernel)
        if (c->zm_tx.p) HZ_HIP(hipMemsetAsync(c->zm_tx.p, 0xFF, c->zm_tx.bytes, s));
        if (c->zm_fee.p) HZ_HIP(hipMemsetAsync(c->zm_fee.p, 0xFF, c->zm_fee.bytes, s));
        c->zm_reset = false;
    }
    if (c->profiling && c->zm_skip.p) HZ_HIP(hipMemsetAsync(c->zm_skip.p, 0, c->zm_skip.bytes, s));
    HZ_HIP(hipEventRecord(c->ev_reset, s));
    c->prof_used = 0;
    if (lo.p.tmpl == T_ROLLUP_MAIN) {
        // sharded contexts run the tail separately (hz_witness_enqueue_tail); an empty shard (more ranks than transactions) evaluates nothing
        if (c->sharded) { if (c->sh_count != 0) HZ_TRY(step_main_sharded(c, st)); }
        else HZ_TRY(c->partitioned ? step_main_partitioned(c, st) : step_main_throughput(c, st));
    } else if (lo.p.tmpl == T_ROLLUP_TX) {
        HZ_TRY(step_rollup_tx(c, st));
    } else {
        HZ_TRY(step_small_main(c, st));
    }
    if (s != s_user) {
        HZ_HIP(hipEventRecord(c->ev_user_out, s));
        HZ_HIP(hipStreamWaitEvent(s_user, c->ev_user_out, 0));
    }
    c->last_stream = s_user;
    c->enqueued = true;
    return HZ_OK;
}

extern "C" hz_status hz_witness_enqueue(hz_ctx* c, void* stream) { return enqueue_impl(c, stream, ~0ull); }

// ---- multi-GPU intra-batch sharding: what a rank launches besides its step ------------------------------------------
static DaArgs make_da(hz_ctx* c, uint32_t first, uint32_t count, void* buf) {
    const Layout& lo = c->lo;
    DaArgs a;
    memset(&a, 0, sizeof a);
    a.tx_base = sec_ptr(c, lo.sec_tx); a.tx_scratch = (Fr*)c->sc_tx.p; a.buf = (uint8_t*)buf;
    a.nTx = (uint32_t)lo.p.nTx; a.L = (uint32_t)lo.p.L; a.u0 = first; a.ucnt = count;
    a.l1full = lo.dec.l1full; a.n2bData = lo.dec.n2bData; a.n2bFinalToIdx = lo.dec.n2bFinalToIdx; a.l1l2amt = lo.rtx.main_l1l2amt;
    a.l1l2Fee = lo.dec.l1l2Fee; a.s5 = lo.rtx.s5;
    return a;
}
extern "C" hz_status hz_da_export(hz_ctx* c, void* d_buf, void* stream) {
    if (!c || c->lo.p.tmpl != T_ROLLUP_MAIN || !d_buf) return set_err(HZ_ERR_ARG, "hz_da_export: bad argument");
    HZ_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->s_main;
    const uint32_t cnt = c->sharded ? c->sh_count : (uint32_t)c->lo.p.nTx;
    HZ_HIP(launch_da_export(make_da(c, c->sh_first, cnt, d_buf), s));
    return HZ_OK;
}
extern "C" hz_status hz_da_import(hz_ctx* c, int32_t first, int32_t count, const void* d_buf, void* stream) {
    if (!c || c->lo.p.tmpl != T_ROLLUP_MAIN || !d_buf || first < 0 || count < 0 || first > c->lo.p.nTx || count > c->lo.p.nTx - first)
        return set_err(HZ_ERR_ARG, "hz_da_import: bad argument");
    HZ_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->s_main;
    HZ_HIP(launch_da_import(make_da(c, (uint32_t)first, (uint32_t)count, const_cast<void*>(d_buf)), s));
    return HZ_OK;
}
// fee transactions + HashInputs of a sharded context on the caller's stream, after the other ranks' records were imported. expand:
// the whole HashInputs, its expansion piped over the context's fee stream; otherwise the message and the sequential chain alone
// (rank 0 of a step whose ranks share the expansion: hz_sha_export / hz_sha_expand)
static hz_status enqueue_tail(hz_ctx* c, void* stream, const char* who, bool expand) {
    if (!c || c->lo.p.tmpl != T_ROLLUP_MAIN) return set_err(HZ_ERR_ARG, "%s: RollupMain contexts only", who);
    HZ_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->s_main;
    const Layout& lo = c->lo;
    HZ_TRY(enqueue_fee(c, sec_ptr(c, lo.sec_fee), lo.sections[lo.sec_fee].n_units, true, s));
    if (expand) {
        HZ_TRY(enqueue_main_hash_inputs(c, s, c->s_fee));
    } else {
        const HashInputsArgs hi = make_hi(c, true);
        ProfScope ps(c, s, "hash_inputs", (uint64_t)lo.hi.sha.nblocks);
        HZ_HIP(launch_hi_prep(hi, HI_WHOLE, s));
        HZ_HIP(launch_sha_chain(hi, 0, (uint32_t)lo.hi.sha.nblocks, s));
    }
    c->last_stream = s;
    c->enqueued = true;
    return HZ_OK;
}
extern "C" hz_status hz_witness_enqueue_tail(hz_ctx* c, void* stream) { return enqueue_tail(c, stream, "hz_witness_enqueue_tail", true); }
extern "C" hz_status hz_witness_enqueue_tail_chain(hz_ctx* c, void* stream) { return enqueue_tail(c, stream, "hz_witness_enqueue_tail_chain", false); }

extern "C" hz_status hz_sha_export(hz_ctx* c, void* d_buf, void* stream) {
    if (!c || !d_buf || c->lo.sec_hi < 0) return set_err(HZ_ERR_ARG, "hz_sha_export: needs a context with a HashInputs section and a buffer");
    HZ_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->s_main;
    const size_t mb = (size_t)c->lo.hi.sha.nblocks * 64 * c->lo.n_inst, cb = ((size_t)c->lo.hi.sha.nblocks + 1) * 32 * c->lo.n_inst;
    HZ_HIP(hipMemcpyAsync(d_buf, c->msg.p, mb, hipMemcpyDeviceToDevice, s));
    HZ_HIP(hipMemcpyAsync((uint8_t*)d_buf + mb, c->chain.p, cb, hipMemcpyDeviceToDevice, s));
    return HZ_OK;
}
extern "C" hz_status hz_sha_expand(hz_ctx* c, int32_t first, int32_t count, const void* d_buf, void* stream) {
    if (!c || c->lo.sec_hi < 0) return set_err(HZ_ERR_ARG, "hz_sha_expand: needs a context with a HashInputs section");
    const int64_t nb = c->lo.hi.sha.nblocks;
    if (first < 0 || count < 0 || (int64_t)first + count > nb) return set_err(HZ_ERR_ARG, "hz_sha_expand: blocks %d..%d out of range (%lld blocks)", first, first + count - 1, (long long)nb);
    HZ_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->s_main;
    if (d_buf) {
        const size_t mb = (size_t)nb * 64 * c->lo.n_inst, cb = ((size_t)nb + 1) * 32 * c->lo.n_inst;
        HZ_HIP(hipMemcpyAsync(c->msg.p, d_buf, mb, hipMemcpyDeviceToDevice, s));
        HZ_HIP(hipMemcpyAsync(c->chain.p, (const uint8_t*)d_buf + mb, cb, hipMemcpyDeviceToDevice, s));
    }
    if (!c->enqueued) HZ_TRY(reset_err(c, s, ~0ull));   // a rank with an empty transaction shard has not reset its failure record this step
    HZ_HIP(launch_sha_expand_range(make_hi(c, true), (uint32_t)first, (uint32_t)count, s));
    c->last_stream = s;
    c->enqueued = true;
    return HZ_OK;
}

// ---- profiling ------------------------------------------------------------------------------------------------
extern "C" hz_status hz_ctx_set_profiling(hz_ctx* c, int32_t on) {
    if (!c) return set_err(HZ_ERR_ARG, "hz_ctx_set_profiling: null context");
    c->profiling = on != 0;
    c->exclusive = on == 2;
    return HZ_OK;
}
extern "C" int32_t hz_profile_count(const hz_ctx* c) { return c ? (int32_t)c->prof_used : 0; }
extern "C" hz_status hz_profile_get(hz_ctx* c, int32_t i, const char** kernel, float* ms, uint64_t* algorithmic_bytes, uint64_t* units) {
    if (!c || i < 0 || (size_t)i >= c->prof_used) return set_err(HZ_ERR_ARG, "hz_profile_get: bad index");
    hz_ctx::Prof& p = c->prof[i];
    HZ_HIP(hipSetDevice(c->device));
    HZ_HIP(hipEventSynchronize(p.e1));
    HZ_HIP(hipEventElapsedTime(&p.ms, p.e0, p.e1));
    if (kernel) *kernel = p.name.c_str();
    if (ms) *ms = p.ms;
    uint64_t bytes = p.bytes;
    if (c->zm_skip.p && p.chain >= 0) {
        // what the chain's launches left in place because the buffer held it already (constant marks) is not among the bytes the
        // record is responsible for. The transaction chain's record stands for the early launch of the last transactions as well.
        unsigned long long sk[3] = {0, 0, 0};
        HZ_HIP(hipMemcpy(sk, c->zm_skip.p, sizeof sk, hipMemcpyDeviceToHost));
        const uint64_t left = (uint64_t)(p.chain == CHAIN_FEE ? sk[CHAIN_FEE] : sk[CHAIN_TX] + sk[CHAIN_LAST_TX]) * 32ull;
        bytes = bytes > left ? bytes - left : 0;
    }
    if (algorithmic_bytes) *algorithmic_bytes = bytes;
    if (units) *units = p.units;
    return HZ_OK;
}
