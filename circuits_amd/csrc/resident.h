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

// a structure's device, its non-blocking stream and the device time of its last call: begin() .. end() on the stream, read by finish()
struct Resident {
    int32_t device = 0;
    hipStream_t s = nullptr;
    DevEvent e0, e1;
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
        HZ_HIP(e0.create());
        HZ_HIP(e1.create());
        return HZ_OK;
    }
    hipError_t begin() { return hipEventRecord(e0, s); }
    hipError_t end() { return hipEventRecord(e1, s); }
    hz_status finish() {
        HZ_HIP(hipStreamSynchronize(s));
        float ms = 0;
        HZ_HIP(hipEventElapsedTime(&ms, e0, e1));
        device_ms = ms;
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
