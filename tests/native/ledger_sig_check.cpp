// host build of the ledger's signature routines (circuits_amd/csrc/ledger_sig.h): cases from stdin, one per line, every field in hex --
//   chain_id current_num_batch from_idx to_idx amount_f nonce token_id user_fee to_bjj_sign max_num_batch to_eth_addr to_bjj_ay
//   s r8x r8y ay sign expected_verdict expected_M expected_txCompressedData expected_txCompressedDataV2
// -- and for each the three packed values and the verdict (0, 7 or 8; 7 beside 8 is 7) against the expected ones.
//   ledger_sig_check             compare, print "cases=N mismatches=K"
//   ledger_sig_check --bench T   verify every case on T threads, print "bench_ms=..." (tools/ledger_sig_bench.py's host baseline)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <string>
#include <thread>
#include <vector>
#include "../../circuits_amd/csrc/ledger_sig.h"
using namespace hz;
#define HZ_CONST_ARR static const
#include "../../circuits_amd/csrc/gen/poseidon_consts.inc"
#undef HZ_CONST_ARR

struct Case {
    uint32_t chain_id, current;
    SigTx t;
    Fc s, r8x, r8y, ay;
    uint32_t sign, verdict;
    Fc m, tcd, v2;
};

static Fc parse_fc(const char* h) {
    Fc r = fc_zero();
    const size_t n = strlen(h);
    for (size_t i = 0; i < n && i < 64; i++) {
        const char c = h[n - 1 - i];
        const uint32_t d = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
        r.v[i / 8] |= d << (4 * (i % 8));
    }
    return r;
}
static bool same(const Fc& a, const Fc& b) { return memcmp(a.v, b.v, 32) == 0; }

static uint32_t verdict_of(const Case& c, const Fr* table, Fc* m, Fc* tcd, Fc* v2) {
    const Fr* K6 = reinterpret_cast<const Fr*>(&HZ_POSEIDON_K_T6[0][0]);
    const Fr* K7 = reinterpret_cast<const Fr*>(&HZ_POSEIDON_K_T7[0][0]);
    *tcd = sig_tx_compressed_data(c.t, c.chain_id);
    *v2 = sig_tx_compressed_data_v2(c.t);
    *m = sig_message(*tcd, c.t, K7);
    uint32_t v = sig_batch_expired(c.t.max_num_batch, c.current) ? 8u : 0u;
    if (!sig_verify(c.s, c.r8x, c.r8y, c.ay, c.sign, *m, K6, table)) v = 7u;
    return v;
}

int main(int argc, char** argv) {
    std::vector<Case> cases;
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        std::vector<std::string> f;
        for (char* p = strtok(line, " \t\r\n"); p; p = strtok(nullptr, " \t\r\n")) f.push_back(p);
        if (f.empty()) continue;
        if (f.size() != 21) {
            fprintf(stderr, "line with %zu fields\n", f.size());
            return 2;
        }
        auto u = [&](int i) { return (uint64_t)strtoull(f[i].c_str(), nullptr, 16); };
        Case c;
        c.chain_id = (uint32_t)u(0);
        c.current = (uint32_t)u(1);
        c.t.from_idx = u(2); c.t.to_idx = u(3); c.t.amount_f = u(4); c.t.nonce = u(5);
        c.t.token_id = (uint32_t)u(6); c.t.user_fee = (uint32_t)u(7); c.t.to_bjj_sign = (uint32_t)u(8); c.t.max_num_batch = (uint32_t)u(9);
        c.t.to_eth_addr = parse_fc(f[10].c_str());
        c.t.to_bjj_ay = parse_fc(f[11].c_str());
        c.s = parse_fc(f[12].c_str()); c.r8x = parse_fc(f[13].c_str()); c.r8y = parse_fc(f[14].c_str()); c.ay = parse_fc(f[15].c_str());
        c.sign = (uint32_t)u(16);
        c.verdict = (uint32_t)u(17);
        c.m = parse_fc(f[18].c_str()); c.tcd = parse_fc(f[19].c_str()); c.v2 = parse_fc(f[20].c_str());
        cases.push_back(c);
    }
    std::vector<Fr> table(HZ_SIG_B8_FRS);
    sig_b8_table(table.data());
    if (argc >= 3 && !strcmp(argv[1], "--bench")) {
        const int T = atoi(argv[2]) > 0 ? atoi(argv[2]) : 1;
        std::vector<uint32_t> got(cases.size());
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> th;
        for (int w = 0; w < T; w++)
            th.emplace_back([&, w] {
                Fc m, a, b;
                for (size_t i = w; i < cases.size(); i += T) got[i] = verdict_of(cases[i], table.data(), &m, &a, &b);
            });
        for (auto& x : th) x.join();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        size_t bad = 0;
        for (size_t i = 0; i < cases.size(); i++) bad += got[i] != cases[i].verdict;
        printf("cases=%zu threads=%d mismatches=%zu bench_ms=%.3f\n", cases.size(), T, bad, ms);
        return bad != 0;
    }
    size_t bad = 0;
    for (size_t i = 0; i < cases.size(); i++) {
        Fc m, tcd, v2;
        const uint32_t v = verdict_of(cases[i], table.data(), &m, &tcd, &v2);
        if (v != cases[i].verdict || !same(m, cases[i].m) || !same(tcd, cases[i].tcd) || !same(v2, cases[i].v2)) {
            bad++;
            fprintf(stderr, "case %zu: verdict %u (expected %u) M %s tcd %s v2 %s\n", i, v, cases[i].verdict, same(m, cases[i].m) ? "ok" : "DIFFERS",
                    same(tcd, cases[i].tcd) ? "ok" : "DIFFERS", same(v2, cases[i].v2) ? "ok" : "DIFFERS");
        }
    }
    printf("cases=%zu mismatches=%zu\n", cases.size(), bad);
    return bad != 0;
}
