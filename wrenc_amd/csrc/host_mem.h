// host_mem.h -- device memory, streams and events with an owner (host code only).  The one place that allocates and frees
// device memory and that creates and destroys streams and events: what a context or a test entry holds in a DevBuf, a
// HipStream or a HipEvent is released when the holder goes, on every path.
#pragma once
#include <hip/hip_runtime_api.h>

namespace wrenc {

// `count` elements of T on the current device, or nothing.  Movable, not copyable; the destructor frees.
// (A pointer and a count, and only alloc / grow ask for sizeof(T): gpu_ctx.h holds DevBufs of types one unit only names.)
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_, n_ = o.n_;
            o.p_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    // replaces what is held by `count` elements (contents dropped).  On failure nothing is held and HIP's last error is
    // cleared, so that the next launch check (hipGetLastError) does not report the failed allocation as its own.
    hipError_t alloc(size_t count) {
        reset();
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, count * sizeof(T));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return e;
        }
        p_ = static_cast<T*>(p);
        n_ = count;
        return hipSuccess;
    }
    // at least `count` elements: what is held stays where it is enough, else alloc
    hipError_t grow(size_t count) { return p_ && n_ >= count ? hipSuccess : alloc(count); }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    T* get() const { return p_; }
    size_t count() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

// A stream or an event of the current device, or nothing.  Movable, not copyable; the destructor destroys the handle
// (whoever holds a stream synchronises it first where work may still be queued on it).
template <class H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)>
class HipHandle {
public:
    HipHandle() = default;
    HipHandle(const HipHandle&) = delete;
    HipHandle& operator=(const HipHandle&) = delete;
    HipHandle(HipHandle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    HipHandle& operator=(HipHandle&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    ~HipHandle() { reset(); }

    // replaces what is held by a new handle (flags 0: the default stream or event).  On failure nothing is held and HIP's
    // last error is cleared, as DevBuf::alloc does.
    hipError_t create(unsigned flags = 0) {
        reset();
        H h = nullptr;
        const hipError_t e = Create(&h, flags);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return e;
        }
        h_ = h;
        return hipSuccess;
    }
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }

private:
    H h_ = nullptr;
};
using HipStream = HipHandle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;
using HipEvent = HipHandle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;

} // namespace wrenc
