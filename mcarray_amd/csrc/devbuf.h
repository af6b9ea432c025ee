// devbuf.h -- one owning device buffer: T *p of n elements, freed with plain hipFree when it goes out of scope.  No allocator, no
// cache and no head room (that is StagePool's, stage.h).  hipFree waits for the work in flight, which the sites that grow a
// workspace between two calls on a stream rely on.  A failed allocation leaves the buffer empty and the runtime's last error
// consumed, so that the closing hipGetLastError() of a later, successful call does not report it again.
#pragma once
#include <hip/hip_runtime.h>

namespace mca {

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;                       // elements allocated

    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept { swap(o); }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~DevBuf() { reset(); }

    void reset()
    {
        if (p) (void)hipFree(p);
        p = nullptr; n = 0;
    }
    void swap(DevBuf &o) noexcept
    {
        T *tp = p; p = o.p; o.p = tp;
        const size_t tn = n; n = o.n; o.n = tn;
    }
    // exactly count elements, in place of what was held
    hipError_t alloc(size_t count)
    {
        reset();
        const hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return e; }
        n = count;
        return hipSuccess;
    }
    hipError_t alloc_zero(size_t count)
    {
        hipError_t e = alloc(count);
        if (e == hipSuccess && (e = hipMemset(p, 0, bytes())) != hipSuccess) reset();
        return e;
    }
    hipError_t upload(const T *host, size_t count)
    {
        hipError_t e = alloc(count);
        if (e == hipSuccess && (e = hipMemcpy(p, host, bytes(), hipMemcpyHostToDevice)) != hipSuccess) reset();
        return e;
    }
    // a workspace: at least count elements.  What was held is freed before the larger one is allocated
    hipError_t grow(size_t count) { return count <= n ? hipSuccess : alloc(count); }
    hipError_t zero_async(hipStream_t st) const { return p ? hipMemsetAsync(p, 0, bytes(), st) : hipSuccess; }
    size_t bytes() const { return n * sizeof(T); }
    operator T *() const { return p; }
};

}  // namespace mca
