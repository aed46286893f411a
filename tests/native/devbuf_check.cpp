// host check of the growing buffers of circuits_amd/csrc/hostutil.h: an allocation that fails must leave an empty buffer behind, so that
// the next call of the same size fails again instead of finding room that is not there. 2^60 bytes fail on any machine with a plain
// error return -- "no device" without one, out of memory with one -- so the program needs no device. Exit status 0: every check held.
#include <stdio.h>
#include "../../circuits_amd/csrc/hostutil.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAILED line %d: %s\n", __LINE__, #cond);               \
            failures++;                                                    \
        }                                                                  \
    } while (0)

template <class Buf>
static void check(const char* name) {
    const size_t huge = (size_t)1 << 60;
    Buf b;
    CHECK(b.grow(0) == hipSuccess && b.p == nullptr && b.bytes == 0);
    const hipError_t first = b.grow(huge);
    CHECK(first != hipSuccess);
    CHECK(b.p == nullptr && b.bytes == 0);
    const hipError_t second = b.grow(huge);
    CHECK(second != hipSuccess);
    CHECK(b.p == nullptr && b.bytes == 0);
    CHECK(b.grow(huge / 2) != hipSuccess);   // any size up to the failed one
    printf("%s: first=%d second=%d p=%p bytes=%zu\n", name, (int)first, (int)second, b.p, b.bytes);
}

int main() {
    check<hz::DevBuf>("DevBuf");
    check<hz::PinnedBuf>("PinnedBuf");
    hz::DevBuf d;
    CHECK(d.alloc(0) == hipSuccess && d.p == nullptr && d.bytes == 0);
    CHECK(d.alloc((size_t)1 << 60) != hipSuccess && d.p == nullptr && d.bytes == 0);
    printf("failures=%d\n", failures);
    return failures ? 1 : 0;
}
