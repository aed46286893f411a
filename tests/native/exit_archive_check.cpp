// host build of the exit archive's routines (circuits_amd/csrc/ledger_archive.h): shapes and queries from stdin, one record per line --
//   t root nodes leaves      a new shape; the next two lines are its arrays, in arrays of exactly that size (the address sanitizer sees
//   c child[0] child[1] ...  a read past either end)
//   k key[0] key[1] ...      (hex)
//   q key n_sib              archive_walk on the shape -> "q status depth leaf src[0] .. src[min(depth, n_sib) - 1]"; the sources it must not
//                            write are checked here: a touched one ends the program with status 3
//   e limb0 limb2            (hex) the unpacking of an exit leaf's e0 -> "e tokenID sign"
// -- and prints one line per q and e record. The test compares them with a plain Python model.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../circuits_amd/csrc/ledger_archive.h"
using namespace hz;

int main() {
    int32_t root = 0;
    std::vector<int32_t> child;
    std::vector<uint64_t> keys;
    size_t nodes = 0, leaves = 0;
    std::string line;
    std::vector<char> buf(1 << 22);
    while (fgets(buf.data(), (int)buf.size(), stdin)) {
        std::vector<char*> f;
        for (char* p = strtok(buf.data(), " \t\r\n"); p; p = strtok(nullptr, " \t\r\n")) f.push_back(p);
        if (f.empty()) continue;
        const char op = f[0][0];
        if (op == 't' && f.size() == 4) {
            root = (int32_t)strtol(f[1], nullptr, 10);
            nodes = strtoull(f[2], nullptr, 10);
            leaves = strtoull(f[3], nullptr, 10);
            child.assign(0, 0);
            keys.assign(0, 0);
        } else if (op == 'c' && f.size() == 1 + 2 * nodes) {
            child.resize(2 * nodes);
            child.shrink_to_fit();
            for (size_t i = 0; i < 2 * nodes; i++) child[i] = (int32_t)strtol(f[1 + i], nullptr, 10);
        } else if (op == 'k' && f.size() == 1 + leaves) {
            keys.resize(leaves);
            keys.shrink_to_fit();
            for (size_t i = 0; i < leaves; i++) keys[i] = strtoull(f[1 + i], nullptr, 16);
        } else if (op == 'q' && f.size() == 3) {
            const uint64_t key = strtoull(f[1], nullptr, 16);
            const uint32_t n_sib = (uint32_t)strtoul(f[2], nullptr, 10);
            std::vector<uint32_t> src(n_sib, 0xFFFFFFFFu);
            src.shrink_to_fit();
            const ArchiveWalk w = archive_walk(root, child.data(), keys.data(), key, n_sib, src.data());
            const uint32_t written = w.depth < n_sib ? w.depth : n_sib;
            printf("q %u %u %u", w.status, w.depth, w.leaf);
            for (uint32_t d = 0; d < written; d++) printf(" %u", src[d]);
            printf("\n");
            for (uint32_t d = written; d < n_sib; d++)
                if (src[d] != 0xFFFFFFFFu) {
                    fprintf(stderr, "key %llx: source %u was written past depth %u\n", (unsigned long long)key, d, w.depth);
                    return 3;
                }
        } else if (op == 'e' && f.size() == 3) {
            printf("e %u %u\n", withdraw_token_id((uint32_t)strtoul(f[1], nullptr, 16)), withdraw_sign((uint32_t)strtoul(f[2], nullptr, 16)));
        } else {
            fprintf(stderr, "bad line: %s with %zu fields\n", f[0], f.size());
            return 2;
        }
    }
    return 0;
}
