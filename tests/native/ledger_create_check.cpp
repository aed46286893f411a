// host build of the ledger's create routines (circuits_amd/csrc/ledger_create.h): one record per line from stdin, every field in hex --
//   k key token ay sign e0            create_decode_key of the compressed key must give ay and sign, create_leaf_e0(token, sign) e0
//   i last creates next               create_next_idx(last, creates != 0)
//   r flags expect                    create_reports_old(flags)
// -- and prints "cases=N mismatches=K".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../circuits_amd/csrc/ledger_create.h"
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
static uint64_t num(const std::string& s) { return strtoull(s.c_str(), nullptr, 16); }

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
        if (op == 'k' && f.size() == 6) {
            uint32_t sign = 7;
            const Fc ay = create_decode_key(parse_fc(f[1].c_str()), &sign);
            ok = same(ay, parse_fc(f[3].c_str())) && sign == (uint32_t)num(f[4]) && same(create_leaf_e0((uint32_t)num(f[2]), sign), parse_fc(f[5].c_str()));
        } else if (op == 'i' && f.size() == 4) {
            ok = create_next_idx(num(f[1]), num(f[2]) != 0) == num(f[3]);
        } else if (op == 'r' && f.size() == 3) {
            ok = create_reports_old((uint32_t)num(f[1])) == (num(f[2]) != 0);
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
