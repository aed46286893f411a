// host build of the ledger's L1 routines (circuits_amd/csrc/ledger_l1.h): runs of the recurrence from stdin, one record per line, every
// field in hex --
//   r slots                              a new run over that many local slots, balances zero
//   b slot balance                       the slot's balance before the run
//   t slot_s slot_r amount_f load_f token from_eth tok_s eth_s tok_r eff3 flags delta_s
//                                        the next transaction (slot_r ffff: no receiver): l1_static on the fields, l1_step on the
//                                        sender's balance, then the receiver's balance += eff3, as k_ledger_l1's serial phase does;
//                                        eff3, the flag byte and the sender's delta (two's complement) it must give
//   e slot balance                       the slot's balance after the run
// -- and prints "cases=N mismatches=K".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../circuits_amd/csrc/ledger_l1.h"
using namespace hz;

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

static bool same(const Fc& a, const Fc& b) { return memcmp(a.v, b.v, sizeof a.v) == 0; }

int main() {
    std::vector<Fc> bal;
    size_t cases = 0, bad = 0;
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        std::vector<std::string> f;
        for (char* p = strtok(line, " \t\r\n"); p; p = strtok(nullptr, " \t\r\n")) f.push_back(p);
        if (f.empty()) continue;
        auto u = [&](size_t i) { return strtoull(f[i].c_str(), nullptr, 16); };
        const char op = f[0][0];
        if (op == 'r' && f.size() == 2) {
            bal.assign(u(1), fc_zero());   // exactly `slots` balances: a slot past the end is the sanitizer's
            bal.shrink_to_fit();
            continue;
        }
        if (op == 'b' && f.size() == 3) {
            bal.at(u(1)) = parse_fc(f[2].c_str());
            continue;
        }
        cases++;
        bool ok = false;
        if (op == 't' && f.size() == 13) {
            const Fc from_eth = parse_fc(f[6].c_str());
            const L1Static st = l1_static(u(3), u(4), (uint32_t)u(5), from_eth.v, (uint32_t)u(7), parse_fc(f[8].c_str()), (uint32_t)u(9));
            const size_t s = u(1), r = u(2);
            Fc amt = st.eff2;
            const bool funded = l1_step(bal.at(s), st.eff_load, amt);
            if (r != HZ_L1_NO_SLOT) bal.at(r) = u256_add(bal.at(r), amt);
            const uint32_t flags = (st.flags & L1_NULL_LOAD) | ((st.flags & L1_NULL_AMOUNT) || !funded ? L1_NULL_AMOUNT : 0u);
            ok = same(amt, parse_fc(f[10].c_str())) && flags == u(11) && same(l1_sender_delta(st.eff_load, amt), parse_fc(f[12].c_str())) &&
                 (from_eth.v[5] | from_eth.v[6] | from_eth.v[7]) == 0u;
        } else if (op == 'e' && f.size() == 3) {
            ok = same(bal.at(u(1)), parse_fc(f[2].c_str()));
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
