// Host runner of the fr.h contract table (tests/fr_contract_common.py, tests/test_fr_contract_cpu.py): the same one-routine-per-op
// dispatch that hz_fr_raw_ops runs on the device (circuits_amd/csrc/fr_raw_ops.h), compiled for the host. It computes nothing of its
// own -- raw limbs in, the routine's raw result out -- so the judgement is left to the Python integers of the table.
//   stdin : records of  uint32 op, uint32 n, uint32 n_operands,  then uint32[n_operands][n][9]   (little-endian, binary)
//   stdout: per record  uint32[n][9]
// Exit status 2 on a malformed record (unknown op, wrong operand count, short read).
#include "../../circuits_amd/csrc/fr_raw_ops.h"
#include <stdio.h>
#include <vector>
using namespace hz;

int main() {
    uint32_t head[3];
    while (fread(head, sizeof(uint32_t), 3, stdin) == 3) {
        const int op = (int)head[0];
        const size_t n = head[1];
        if (fr_raw_operands(op) < 0 || (uint32_t)fr_raw_operands(op) != head[2] || n > (1u << 26)) {
            fprintf(stderr, "fr_contract_host: bad record (op %d, %zu elements, %u operands)\n", op, n, head[2]);
            return 2;
        }
        std::vector<uint32_t> in((size_t)head[2] * n * 9), out(n * 9);
        if (fread(in.data(), sizeof(uint32_t), in.size(), stdin) != in.size()) {
            fprintf(stderr, "fr_contract_host: short read\n");
            return 2;
        }
        fr_raw_dispatch(op, [&](auto c) {
            for (size_t i = 0; i < n; i++) {
                const auto ld = [&](int k) {
                    Fr x;
                    for (int j = 0; j < 9; j++) x.v[j] = in[((size_t)k * n + i) * 9 + j];
                    return x;
                };
                fr_raw_apply<decltype(c)::value>(ld, &out[i * 9]);
            }
        });
        if (fwrite(out.data(), sizeof(uint32_t), out.size(), stdout) != out.size()) return 2;
    }
    fflush(stdout);
    return 0;
}
