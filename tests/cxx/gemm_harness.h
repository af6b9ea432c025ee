// gemm_harness.h -- TEST-ONLY: the exactly sized device buffer of the two translation units of libgemm_harness.so.
#pragma once
#include <hip/hip_runtime.h>

namespace gh {
// hipMalloc of exactly `bytes` (16 for an empty buffer), filled from the host; freed when the launcher returns, on every path
struct DBuf {
    void *p = nullptr;
    size_t bytes = 0;
    ~DBuf() { if (p) (void)hipFree(p); }
    hipError_t up(const void *host, size_t n)
    {
        bytes = n;
        hipError_t e = hipMalloc(&p, n ? n : 16);
        if (e == hipSuccess && n) e = hipMemcpy(p, host, n, hipMemcpyHostToDevice);
        return e;
    }
    hipError_t down(void *host) const { return bytes ? hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
};
// what every launcher does behind its launch
inline hipError_t finish()
{
    hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : hipDeviceSynchronize();
}
}  // namespace gh
