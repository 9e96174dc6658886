// ajx_hostbuf.h — the buffers the host layer owns: device memory (DeviceBuf) and pinned host
// memory (PinnedBuf), move-only, freed by their destructor. reserve() only ever grows (the
// contents are not kept): it synchronizes `stream`, when one is given, before the old
// allocation is freed (work queued there may still read it), and leaves the buffer empty when
// the allocation fails. Includes the HIP runtime only: the CPU tests build it on their stand-in.
#pragma once
#include <hip/hip_runtime.h>

namespace ajx {

class OwnedBuf {
public:
    OwnedBuf(OwnedBuf&& o) noexcept : pinned_(o.pinned_), p_(o.p_), dev_(o.dev_), cap_(o.cap_) {
        o.p_ = o.dev_ = nullptr, o.cap_ = 0;
    }
    ~OwnedBuf() { drop(); }
    hipError_t reserve(size_t bytes, hipStream_t stream = nullptr) {
        if (bytes <= cap_) return hipSuccess;
        hipError_t e = stream ? hipStreamSynchronize(stream) : hipSuccess;
        if (e != hipSuccess) return e;
        drop();
        void* q = nullptr;
        e = pinned_ ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes);
        if (e != hipSuccess) return e;
        p_ = dev_ = static_cast<uint8_t*>(q);
        if (pinned_ && (e = hipHostGetDevicePointer(&q, p_, 0)) != hipSuccess) return drop(), e;
        dev_ = static_cast<uint8_t*>(q);
        cap_ = bytes;
        return hipSuccess;
    }
    size_t capacity() const { return cap_; }
    uint8_t* data() const { return p_; }
    template <class T>
    T* as() const {
        return reinterpret_cast<T*>(p_);
    }

protected:
    explicit OwnedBuf(bool pinned) : pinned_(pinned) {}
    void drop() {
        if (p_) (void)(pinned_ ? hipHostFree(p_) : hipFree(p_));
        p_ = dev_ = nullptr, cap_ = 0;
    }
    const bool pinned_;
    uint8_t *p_ = nullptr, *dev_ = nullptr;  // dev_: the address kernels use
    size_t cap_ = 0;
};

struct DeviceBuf : OwnedBuf {
    DeviceBuf() : OwnedBuf(false) {}
};
struct PinnedBuf : OwnedBuf {
    PinnedBuf() : OwnedBuf(true) {}
    uint8_t* device() const { return dev_; }  // where kernels read and write it (zero-copy)
};

}  // namespace ajx
