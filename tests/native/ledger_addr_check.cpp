// host build of the ledger's receiver-lookup routines (circuits_amd/csrc/ledger_resolve.h): cases from stdin, one per line, every
// field in hex --
//   k token eth ay sign w0 .. w9 hash    resolve_key and resolve_hash of an account or a destination against the expected words
//   t slots                              a new, empty table of that many slots
//   i w0 .. w9 slot                      resolve_insert of the key into the current table; the slot it must take (ffffffff: full)
//   p w0 .. w9 slot                      resolve_probe of the key in the current table; the slot it must find (ffffffff: none)
// -- and prints "cases=N mismatches=K".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../circuits_amd/csrc/ledger_resolve.h"
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

int main() {
    std::vector<ResolveKey> table;
    size_t cases = 0, bad = 0;
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        std::vector<std::string> f;
        for (char* p = strtok(line, " \t\r\n"); p; p = strtok(nullptr, " \t\r\n")) f.push_back(p);
        if (f.empty()) continue;
        auto u = [&](size_t i) { return (uint32_t)strtoul(f[i].c_str(), nullptr, 16); };
        auto key_at = [&](size_t first) {
            ResolveKey k;
            for (int i = 0; i < 10; i++) k.w[i] = u(first + i);
            return k;
        };
        const char op = f[0][0];
        if (op == 't' && f.size() == 2) {
            table.assign(u(1), ResolveKey{});   // a fresh allocation of exactly `slots` keys: a probe past the end is the sanitizer's
            table.shrink_to_fit();
            continue;
        }
        cases++;
        bool ok = false;
        if (op == 'k' && f.size() == 16) {
            const ResolveKey got = resolve_key(u(1), parse_fc(f[2].c_str()), parse_fc(f[3].c_str()), u(4)), exp = key_at(5);
            ok = resolve_same(got, exp) && memcmp(got.w, exp.w, sizeof got.w) == 0 && resolve_hash(got) == u(15);
        } else if ((op == 'i' || op == 'p') && f.size() == 12 && !table.empty()) {
            const ResolveKey k = key_at(1);
            const int32_t got = op == 'i' ? resolve_insert(table.data(), (uint32_t)table.size(), k) : resolve_probe(table.data(), (uint32_t)table.size(), k);
            ok = (uint32_t)got == u(11);
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
