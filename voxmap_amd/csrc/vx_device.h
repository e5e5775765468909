// vx_device.h — move-only owners of the host code's HIP resources (vx_api.cpp).
// Host only: no .hip unit includes it.  A holder destroys what it holds with
// itself; nothing is pooled or shared.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <utility>

namespace vx {

template <class H, hipError_t (*Destroy)(H)>
class Owned {
public:
    Owned() = default;
    Owned(Owned &&o) noexcept : h_(std::exchange(o.h_, H{})) {}
    Owned &operator=(Owned &&o) noexcept { std::swap(h_, o.h_); return *this; }   // o destroys what this held
    ~Owned() { (void)reset(); }
    explicit operator bool() const { return h_ != H{}; }
    hipError_t reset() {
        H h = std::exchange(h_, H{});
        return h ? Destroy(h) : hipSuccess;
    }

protected:
    H h_{};
};

// n elements of T in device memory (hipMalloc / hipFree)
template <class T>
struct DevBuf : Owned<void *, hipFree> {
    hipError_t alloc(size_t n) {
        (void)reset();
        const hipError_t e = hipMalloc(&h_, n * sizeof(T));
        if (e != hipSuccess) h_ = nullptr;
        return e;
    }
    T *get() const { return static_cast<T *>(h_); }
};

struct Stream : Owned<hipStream_t, hipStreamDestroy> {   // non-blocking: it never waits for the null stream
    hipError_t create() { (void)reset(); return hipStreamCreateWithFlags(&h_, hipStreamNonBlocking); }
    hipStream_t get() const { return h_; }
};

struct Event : Owned<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault) { (void)reset(); return hipEventCreateWithFlags(&h_, flags); }
    hipEvent_t get() const { return h_; }
};

}  // namespace vx
