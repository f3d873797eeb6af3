// device_mem.hpp -- host side only: device (and pinned host) memory that frees itself, and the ring-hop carry every handle type
// performs after a batch.  The handles of capi.cpp, das_fused_engine.cpp, pipeline.hip and doa.cpp own their buffers through these
// members; nothing is released by hand, so a member cannot be missing from a free list.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

#include "../../include/bfcore.h"

namespace bf {

// n elements of T in device memory (kPinned: in page-locked host memory).  Move-only; the destructor frees.  A handle that must set its
// device and synchronise before anything is freed does so before it is deleted: the members go with the handle, not earlier.
template <class T, bool kPinned = false>
class DeviceBuffer {
   public:
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_, n_ = o.n_;
            o.p_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    ~DeviceBuffer() { release(); }

    T *get() const { return p_; }
    size_t size() const { return n_; }  // elements; 0 until an allocation has succeeded

    // exactly n elements, content undefined; what the buffer held is freed first, and a failure leaves it empty
    hipError_t alloc(size_t n) {
        release();
        const hipError_t e = kPinned ? hipHostMalloc((void **)&p_, n * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&p_, n * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        else n_ = n;
        return e;
    }
    // allocate v.size() elements and copy v into them (synchronous: v may be a temporary)
    hipError_t upload(const std::vector<T> &v) {
        const hipError_t e = alloc(v.size());
        return e != hipSuccess ? e : hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    // grow-on-demand scratch: at least n elements; the content does not survive a growth.  The caller makes sure that nothing in flight
    // still reads the old allocation.
    hipError_t reserve(size_t n) { return n <= n_ ? hipSuccess : alloc(n); }

   private:
    void release() {
        if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        n_ = 0;
    }
    T *p_ = nullptr;
    size_t n_ = 0;
};
template <class T>
using PinnedBuffer = DeviceBuffer<T, true>;

// Ring-buffer carry (util.h:305-308): the last hop of a batch of n_frames frames at x becomes the hop in front of the next batch.  `hist`
// keeps the input's layout: planar [stream][mic][hop] (microphone rows of x are mic_stride samples apart, streams follow each other
// without a gap) or [stream][hop][mic] (streams of x are stream_stride samples apart).
inline hipError_t carry_last_hop(float *hist, const float *x, long n_frames, int hop, int n_mics, int n_streams, int layout,
                                 long mic_stride, long stream_stride, hipStream_t s) {
    if (layout == BF_PLANAR)
        return hipMemcpy2DAsync(hist, hop * sizeof(float), x + (n_frames - 1) * hop, (size_t)mic_stride * sizeof(float), hop * sizeof(float),
                                (size_t)n_streams * n_mics, hipMemcpyDeviceToDevice, s);
    const size_t row = (size_t)hop * n_mics * sizeof(float);
    return hipMemcpy2DAsync(hist, row, x + (n_frames - 1) * (long)hop * n_mics, (size_t)stream_stride * sizeof(float), row, (size_t)n_streams,
                            hipMemcpyDeviceToDevice, s);
}

}  // namespace bf
