// What the device-resident structures (state.hip, smt_tree.hip, ledger.hip) own besides their buffers: the stream their calls run on,
// the events that time a call, the dense Poseidon(3) constants of the level hash.
#pragma once
#include "hostutil.h"
#include "kernels.h"

namespace hz {

struct DevEvent {
    hipEvent_t e = nullptr;
    DevEvent() = default;
    DevEvent(const DevEvent&) = delete;
    DevEvent& operator=(const DevEvent&) = delete;
    ~DevEvent() { if (e) (void)hipEventDestroy(e); }
    hipError_t create() { return hipEventCreate(&e); }
    operator hipEvent_t() const { return e; }
};

// the device time between two recorded events, once the stream has been synchronised behind the second
inline hipError_t elapsed_ms(hipEvent_t a, hipEvent_t b, double& ms) {
    float f = 0;
    const hipError_t e = hipEventElapsedTime(&f, a, b);
    if (e == hipSuccess) ms = f;
    return e;
}

// a pair of events around a stretch of a stream
struct DevSpan {
    DevEvent e0, e1;
    hipError_t create() {
        const hipError_t e = e0.create();
        return e != hipSuccess ? e : e1.create();
    }
    hipError_t begin(hipStream_t s) { return hipEventRecord(e0, s); }
    hipError_t end(hipStream_t s) { return hipEventRecord(e1, s); }
    hipError_t read(double& ms) const { return elapsed_ms(e0, e1, ms); }
};

// a structure's device, its non-blocking stream and the device time of its last call: begin() .. end() on the stream, read by finish()
struct Resident {
    int32_t device = 0;
    hipStream_t s = nullptr;
    DevSpan span;
    double device_ms = 0.0;
    Resident() = default;
    Resident(const Resident&) = delete;
    Resident& operator=(const Resident&) = delete;
    ~Resident() { if (s) (void)hipStreamDestroy(s); }
    hz_status open(const char* who, int32_t dev) {
        const int32_t n_dev = hz_device_count();
        if (n_dev <= 0) return set_err(HZ_ERR_NODEVICE, "no usable gfx950 device");
        if (dev < 0 || dev >= n_dev) return set_err(HZ_ERR_ARG, "%s: device %d of %d", who, dev, n_dev);
        HZ_HIP(hipSetDevice(dev));
        device = dev;
        HZ_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        HZ_HIP(span.create());
        return HZ_OK;
    }
    hipError_t begin() { return span.begin(s); }
    hipError_t end() { return span.end(s); }
    hz_status finish() {
        HZ_HIP(hipStreamSynchronize(s));
        HZ_HIP(span.read(device_ms));
        return HZ_OK;
    }
};

// the constants of poseidon_quad.h's digest form in device memory
inline hz_status pos3_dense_create(DevBuf& b) {
    HZ_HIP(b.alloc(pos3_dense_bytes()));
    HZ_HIP(upload_pos3_dense((Fr*)b.p));
    return HZ_OK;
}

}  // namespace hz
