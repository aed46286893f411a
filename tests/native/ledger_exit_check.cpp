// host build of the ledger's exit routines (circuits_amd/csrc/ledger_exit.h): the operations of exit keys from stdin, one record per line,
// every field in hex --
//   g e0_sender e0_exit                  a new exit key: exit_leaf_e0 of the sender's e0 must give e0_exit; the balance starts at zero
//   o eff3 tokenID nonce sign balance new_balance ok
//                                        the key's next operation, as k_ledger_exit_scan's lane does it: exit_leaf_rows of the leaf before
//                                        must give the four rows, exit_step the new balance (modulo 2^256) and whether it is below 2^192
//   r flags expect                       exit_reports_old(flags)
// -- and prints "cases=N mismatches=K".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../circuits_amd/csrc/ledger_exit.h"
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
    Fc e0 = fc_zero(), bal = fc_zero();
    size_t cases = 0, bad = 0;
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        std::vector<std::string> f;
        for (char* p = strtok(line, " \t\r\n"); p; p = strtok(nullptr, " \t\r\n")) f.push_back(p);
        if (f.empty()) continue;
        const char op = f[0][0];
        cases++;
        bool ok = false;
        if (op == 'g' && f.size() == 3) {
            e0 = exit_leaf_e0(parse_fc(f[1].c_str()));
            bal = fc_zero();
            ok = same(e0, parse_fc(f[2].c_str()));
        } else if (op == 'o' && f.size() == 8) {
            Fc rows[4];
            exit_leaf_rows(e0, bal, rows);
            ok = true;
            for (int q = 0; q < 4; q++) ok = ok && same(rows[q], parse_fc(f[2 + q].c_str()));
            const bool leaf = exit_step(bal, parse_fc(f[1].c_str()));
            ok = ok && same(bal, parse_fc(f[6].c_str())) && leaf == (strtoull(f[7].c_str(), nullptr, 16) != 0);
        } else if (op == 'r' && f.size() == 3) {
            ok = exit_reports_old((uint32_t)strtoull(f[1].c_str(), nullptr, 16)) == (strtoull(f[2].c_str(), nullptr, 16) != 0);
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
