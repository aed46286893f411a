// host build of the ledger's 256-bit routines (circuits_amd/csrc/u256.h, ledger_fee.h, l1_float40 of ledger_l1.h): records from stdin,
// one per line, every field in hex, the expectation last --
//   f float40 amount                    l1_float40
//   g float40 selector fee              ledger_fee on l1_float40's amount
//   v float40 selector over             ledger_fee_overflows on that fee (0 or 1)
//   a x y sum                           u256_add (modulo 2^256)
//   n x neg                             u256_neg
//   s x shifted                         u256_shr60
//   l a b less                          u256_less (0 or 1)
//   o r v shift result                  u256_or_shl of the 64-bit v into r
// -- and prints "cases=N mismatches=K".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../circuits_amd/csrc/ledger_fee.h"
#include "../../circuits_amd/csrc/ledger_l1.h"
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
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        std::vector<std::string> f;
        for (char* p = strtok(line, " \t\r\n"); p; p = strtok(nullptr, " \t\r\n")) f.push_back(p);
        if (f.empty()) continue;
        auto u = [&](size_t i) { return strtoull(f[i].c_str(), nullptr, 16); };
        const char op = f[0][0];
        const size_t want = op == 'o' ? 5 : (op == 'g' || op == 'v' || op == 'a' || op == 'l') ? 4 : 3;
        if (!strchr("fgvansol", op) || f.size() != want) {
            fprintf(stderr, "bad line: %s with %zu fields\n", f[0].c_str(), f.size());
            return 2;
        }
        cases++;
        const Fc expect = parse_fc(f.back());
        bool ok = false;
        if (op == 'f') {
            ok = same(l1_float40(u(1)), expect);
        } else if (op == 'g') {
            ok = same(ledger_fee(l1_float40(u(1)), (uint32_t)u(2)), expect);
        } else if (op == 'v') {
            ok = ledger_fee_overflows(ledger_fee(l1_float40(u(1)), (uint32_t)u(2))) == (u(3) != 0);
        } else if (op == 'a') {
            ok = same(u256_add(parse_fc(f[1]), parse_fc(f[2])), expect);
        } else if (op == 'n') {
            ok = same(u256_neg(parse_fc(f[1])), expect);
        } else if (op == 's') {
            ok = same(u256_shr60(parse_fc(f[1])), expect);
        } else if (op == 'l') {
            ok = u256_less(parse_fc(f[1]), parse_fc(f[2])) == (u(3) != 0);
        } else {
            Fc r = parse_fc(f[1]);
            u256_or_shl(r, u(2), (int)u(3));
            ok = same(r, expect);
        }
        if (!ok) {
            bad++;
            fprintf(stderr, "case %zu (%c) differs\n", cases, op);
        }
    }
    printf("cases=%zu mismatches=%zu\n", cases, bad);
    return bad != 0;
}
