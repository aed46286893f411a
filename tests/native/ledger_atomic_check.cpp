// host build of the atomic link's routines (circuits_amd/csrc/ledger_rq.h): one record per line from stdin --
//   t r k n_l1 n_rows expect          rq_target_row(r, k, n_l1, n_rows), decimal; expect -1: the comparison is against zeros
//   m pos a b expect                  rq_fields_match with field `pos` (0 .. 2) of the rq side a and of the target side b, hex, the other
//                                     four fields equal and nonzero; expect 1: all three match
//   s from to amount_f nonce token fee sign max_num_batch eth ay rq_v2 rq_eth rq_ay M      (hex, chain_id 1) sig_message of ledger_sig.h with the
//                                     three rq fields must give M; with all three zero the three-argument form -- the path of the
//                                     calls that know no link -- must give the same digest
// -- and prints "cases=N mismatches=K".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../circuits_amd/csrc/ledger_rq.h"
#include "../../circuits_amd/csrc/ledger_sig.h"
using namespace hz;
#define HZ_CONST_ARR static const
#include "../../circuits_amd/csrc/gen/poseidon_consts.inc"
#undef HZ_CONST_ARR

static Fc parse_fc(const char* h) {
    Fc r;
    memset(r.v, 0, sizeof r.v);
    const size_t n = strlen(h);
    for (size_t i = 0; i < n && i < 64; i++) {
        const char c = h[n - 1 - i];
        const uint32_t d = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
        r.v[i / 8] |= d << (4 * (i % 8));
    }
    return r;
}

int main() {
    size_t cases = 0, bad = 0;
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        std::vector<std::string> f;
        for (char* p = strtok(line, " \t\r\n"); p; p = strtok(nullptr, " \t\r\n")) f.push_back(p);
        if (f.empty()) continue;
        const char op = f[0][0];
        cases++;
        bool ok = false;
        if (op == 't' && f.size() == 6) {
            const int64_t got = rq_target_row(strtoull(f[1].c_str(), nullptr, 10), (uint32_t)strtoul(f[2].c_str(), nullptr, 10), strtoull(f[3].c_str(), nullptr, 10),
                                              strtoull(f[4].c_str(), nullptr, 10));
            ok = got == strtoll(f[5].c_str(), nullptr, 10);
        } else if (op == 'm' && f.size() == 5) {
            const unsigned pos = (unsigned)strtoul(f[1].c_str(), nullptr, 10);
            Fc rq[3], tg[3];
            for (unsigned q = 0; q < 3; q++) rq[q] = tg[q] = parse_fc(q == 0 ? "abcdef0123456789" : q == 1 ? "ffffffffffffffffffffffffffffffffffffffff" : "1");
            if (pos > 2) return 2;
            rq[pos] = parse_fc(f[2].c_str());
            tg[pos] = parse_fc(f[3].c_str());
            ok = rq_fields_match(rq[0], rq[1], rq[2], tg[0], tg[1], tg[2]) == (strtoul(f[4].c_str(), nullptr, 10) != 0);
        } else if (op == 's' && f.size() == 15) {
            auto u = [&](int i) { return (uint64_t)strtoull(f[i].c_str(), nullptr, 16); };
            const Fr* K7 = reinterpret_cast<const Fr*>(&HZ_POSEIDON_K_T7[0][0]);
            SigTx t;
            t.from_idx = u(1); t.to_idx = u(2); t.amount_f = u(3); t.nonce = u(4);
            t.token_id = (uint32_t)u(5); t.user_fee = (uint32_t)u(6); t.to_bjj_sign = (uint32_t)u(7); t.max_num_batch = (uint32_t)u(8);
            t.to_eth_addr = parse_fc(f[9].c_str());
            t.to_bjj_ay = parse_fc(f[10].c_str());
            const Fc rq[3] = {parse_fc(f[11].c_str()), parse_fc(f[12].c_str()), parse_fc(f[13].c_str())}, want = parse_fc(f[14].c_str());
            const Fc tcd = sig_tx_compressed_data(t, 1);
            const Fc m = sig_message(tcd, t, rq[0], rq[1], rq[2], K7);
            ok = memcmp(m.v, want.v, 32) == 0;
            if (fc_is_zero(rq[0]) && fc_is_zero(rq[1]) && fc_is_zero(rq[2])) {
                const Fc old = sig_message(tcd, t, K7);
                ok = ok && memcmp(old.v, m.v, 32) == 0;
            }
        } else {
            fprintf(stderr, "bad line: %s with %zu fields\n", f[0].c_str(), f.size());
            return 2;
        }
        if (!ok) {
            bad++;
            fprintf(stderr, "case %zu (%c) differs\n", cases, op);
        }
    }
    printf("cases=%zu mismatches=%zu\n", cases, bad);
    return bad != 0;
}
