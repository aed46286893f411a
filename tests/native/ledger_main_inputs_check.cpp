// host build of the packing routines of hz_ledger_main_inputs (circuits_amd/csrc/ledger_inputs.h): cases from stdin, one record per line,
// every field in hex --
//   1 kind chain from to token amountf loadf eth create expect                     mi_l1_value of an L1 row (from: the row's from_idx as the
//                                                                                  kernels read it, auxFromIdx on a create row)
//   2 kind chain from to amountf nonce token fee sign maxnb toeth toay s r8x r8y rqoff rqv2 rqeth rqay haverq expect
//                                                                                  mi_l2_value of L2 row 1 of 3; rows 0 and 2 hold other values
//   b key g expect                                                                 bits 16 g .. 16 g + 15 of the key as 16 bytes (32 hex digits,
//                                                                                  byte 0 first)
// -- and prints "cases=N mismatches=K".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../circuits_amd/csrc/ledger_inputs.h"
using namespace hz;

static Fc parse_fc(const std::string& s) {
    Fc r;
    memset(r.v, 0, sizeof r.v);
    const size_t n = s.size();
    for (size_t i = 0; i < n && i < 64; i++) {
        const char c = s[n - 1 - i];
        const uint32_t d = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
        r.v[i / 8] |= d << (4 * (i % 8));
    }
    return r;
}

static bool same(const Fc& a, const Fc& b) { return memcmp(a.v, b.v, sizeof a.v) == 0; }

int main() {
    size_t cases = 0, bad = 0;
    static char line[16384];
    while (fgets(line, sizeof line, stdin)) {
        std::vector<std::string> f;
        for (char* p = strtok(line, " \t\r\n"); p; p = strtok(nullptr, " \t\r\n")) f.push_back(p);
        if (f.empty()) continue;
        auto u = [&](size_t i) { return strtoull(f[i].c_str(), nullptr, 16); };
        auto fc = [&](size_t i) { return parse_fc(f[i]); };
        cases++;
        bool ok = false;
        if (f[0] == "1" && f.size() == 11) {
            hz_l2tx x{};
            x.from_idx = u(3), x.to_idx = u(4), x.token_id = (uint32_t)u(5), x.amount_f = u(6);
            LedgerL1Dev r{};
            r.amount_f = x.amount_f, r.load_amount_f = u(7), r.token_id = x.token_id;
            const Fc eth = fc(8);
            memcpy(r.from_eth, eth.v, 20);
            ok = same(mi_l1_value((uint32_t)u(1), (uint32_t)u(2), x, r, u(9) != 0), fc(10));
        } else if (f[0] == "2" && f.size() == 22) {
            const uint32_t m = 3, j = 1;
            // exactly m entries on the heap: a read beside row j is another value, a read beyond the arrays is the sanitizer's
            std::vector<hz_l2tx> txs(m);
            std::vector<hz_l2sig> sigs(m);
            std::vector<uint8_t> rq((size_t)m * 97);
            for (uint32_t i = 0; i < m; i++) {
                txs[i].from_idx = 0x1111 + i, txs[i].to_idx = 0x2222 + i, txs[i].amount_f = 0x333 + i, txs[i].nonce = 7 + i, txs[i].token_id = 9 + i, txs[i].user_fee = (uint8_t)(3 + i);
                memset(&sigs[i], 0x50 + (int)i, sizeof(hz_l2sig));
            }
            for (size_t q = 0; q < rq.size(); q++) rq[q] = (uint8_t)(0xA0 + q % 7);
            hz_l2tx& x = txs[j];
            x.from_idx = u(3), x.to_idx = u(4), x.amount_f = u(5), x.nonce = u(6), x.token_id = (uint32_t)u(7), x.user_fee = (uint8_t)u(8);
            hz_l2sig& g = sigs[j];
            g.to_bjj_sign = (uint8_t)u(9), g.max_num_batch = (uint32_t)u(10);
            const Fc parts[5] = {fc(11), fc(12), fc(13), fc(14), fc(15)};
            memcpy(g.to_eth_addr, parts[0].v, 32), memcpy(g.to_bjj_ay, parts[1].v, 32), memcpy(g.s, parts[2].v, 32), memcpy(g.r8x, parts[3].v, 32), memcpy(g.r8y, parts[4].v, 32);
            rq[(size_t)3 * m * 32 + j] = (uint8_t)u(16);
            const Fc links[3] = {fc(17), fc(18), fc(19)};
            for (uint32_t q = 0; q < 3; q++) memcpy(rq.data() + ((size_t)q * m + j) * 32, links[q].v, 32);
            ok = same(mi_l2_value((uint32_t)u(1), (uint32_t)u(2), txs[j], sigs[j], u(20) ? rq.data() : nullptr, j, m), fc(21));
        } else if (f[0] == "b" && f.size() == 4) {
            const Fc key = fc(1);
            const uint32_t g = (uint32_t)u(2), half = mi_key_half(key, g);
            uint8_t got[16], want[16];
            for (int q = 0; q < 4; q++) {
                const uint32_t w = mi_bits4(half, q);
                memcpy(got + 4 * q, &w, 4);
            }
            ok = f[3].size() == 32;
            for (int i = 0; ok && i < 16; i++) want[i] = (uint8_t)strtoul(f[3].substr(2 * i, 2).c_str(), nullptr, 16);
            ok = ok && memcmp(got, want, 16) == 0;
        } else {
            fprintf(stderr, "bad line: %s with %zu fields\n", f[0].c_str(), f.size());
            return 2;
        }
        if (!ok) {
            bad++;
            fprintf(stderr, "mismatch in case %zu (%s kind %s)\n", cases, f[0].c_str(), f[1].c_str());
        }
    }
    printf("cases=%zu mismatches=%zu\n", cases, bad);
    return bad ? 1 : 0;
}
