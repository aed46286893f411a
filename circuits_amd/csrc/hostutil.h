// Host-side plumbing shared by the C-ABI translation units: error text, HIP error mapping, RAII device and pinned buffers, the
// offsets of the arrays of one block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include "../../include/hermez_witness.h"

namespace hz {

hz_status set_err(hz_status st, const char* fmt, ...);

#define HZ_HIP(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return hz::set_err(HZ_ERR_HIP, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    // p == nullptr and bytes == 0 after a failure and for n == 0: `bytes` never claims room that is not there
    hipError_t alloc(size_t n) {
        release();
        if (n == 0) return hipSuccess;
        const hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess)
            bytes = n;
        else
            p = nullptr;
        return e;
    }
    // room for n bytes, half as much again when it has to allocate; the contents are not kept
    hipError_t grow(size_t n) { return n <= bytes ? hipSuccess : alloc(n + n / 2); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// DevBuf's pinned counterpart
struct PinnedBuf {
    void* p = nullptr;
    size_t bytes = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { release(); }
    hipError_t grow(size_t n) {
        if (n <= bytes) return hipSuccess;
        release();
        const hipError_t e = hipHostMalloc(&p, n + n / 2, hipHostMallocDefault);
        if (e == hipSuccess)
            bytes = n + n / 2;
        else
            p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// the arrays of one block behind each other, each at a multiple of 16 bytes: take() returns an array's offset, `end` is the block's size
struct Carve {
    size_t end = 0;
    size_t take(size_t bytes) {
        const size_t at = end;
        end = (end + bytes + 15) & ~(size_t)15;
        return at;
    }
};

// canonical 32-byte LE integer < r ?
inline bool canon_lt_p(const uint8_t* b) {
    static const uint32_t P[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
    for (int i = 7; i >= 0; i--) {
        const uint32_t w = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
        if (w < P[i]) return true;
        if (w > P[i]) return false;
    }
    return false;
}

}  // namespace hz
