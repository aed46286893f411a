// host build of the select routines (circuits_amd/csrc/ledger_select.h): cases from stdin, one record per line, every field in hex --
//   s bal kept debit tx_nonce resident expect      select_want on the two nonces, then select_step: 0, 2, 3 or 12
//   c to amount ok new                             select_credit: whether the new balance stays below 2^192, the balance it leaves
//   o d expect                                     select_offset of the distance d (32 bits, two's complement)
//   l partner_kept row partner_row expect          select_link: the offset, 0 for forced out
//   t flags token tok_s tok_r sig fee_over expect  select_static
//   g float40 selector fee over                    ledger_fee on l1_float40's amount (up to 201 bits), then ledger_fee_overflows
// -- and prints "cases=N mismatches=K".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../circuits_amd/csrc/ledger_select.h"
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
    size_t cases = 0, bad = 0;
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        std::vector<std::string> f;
        for (char* p = strtok(line, " \t\r\n"); p; p = strtok(nullptr, " \t\r\n")) f.push_back(p);
        if (f.empty()) continue;
        auto u = [&](size_t i) { return strtoull(f[i].c_str(), nullptr, 16); };
        const char op = f[0][0];
        cases++;
        bool ok = false;
        if (op == 's' && f.size() == 7) {
            const Fc bal = parse_fc(f[1].c_str());
            const Fc before = bal;
            ok = select_step(bal, (uint32_t)u(2), parse_fc(f[3].c_str()), select_want(u(4), u(5))) == u(6) && same(bal, before);
        } else if (op == 'c' && f.size() == 5) {
            Fc to = parse_fc(f[1].c_str());
            ok = select_credit(to, parse_fc(f[2].c_str())) == (u(3) != 0) && same(to, parse_fc(f[4].c_str()));
        } else if (op == 'o' && f.size() == 3) {
            ok = select_offset((int64_t)(int32_t)(uint32_t)u(1)) == u(2);
        } else if (op == 'l' && f.size() == 5) {
            ok = select_link(u(1) != 0, (uint32_t)u(2), (uint32_t)u(3)) == u(4);
        } else if (op == 't' && f.size() == 8) {
            ok = select_static((uint32_t)u(1), (uint32_t)u(2), (uint32_t)u(3), (uint32_t)u(4), (uint32_t)u(5), u(6) != 0) == u(7);
        } else if (op == 'g' && f.size() == 5) {
            const Fc fee = ledger_fee(l1_float40(u(1)), (uint32_t)u(2));
            ok = same(fee, parse_fc(f[3].c_str())) && ledger_fee_overflows(fee) == (u(4) != 0);
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
