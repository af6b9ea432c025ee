// gemm_harness.hip -- TEST-ONLY library (tests/test_gpu_gemm_fold.py): csrc/kernels_gemm.hip included unchanged and compiled with the
// product's line for it, behind one launcher of k_srp_gemm_f16_fold.  One array of `rows` frames in a map of `rows_alloc` rows, so the
// caller can see that the rows behind `rows` stay as they were.
// Entry point: extern "C", host pointers and counts in, the hipError_t out as an int; it never aborts or prints.
// build: tests/cxx/gemm_harness.mk, which build() runs beside tests/cxx/Makefile (nothing of the product links this library)
#include <hip/hip_runtime.h>
#include "../../mcarray_amd/csrc/kernels_gemm.hip"

using namespace mca;

namespace {
struct DBuf {
    void *p = nullptr;
    ~DBuf() { if (p) (void)hipFree(p); }
    hipError_t up(const void *host, size_t bytes)
    {
        hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
        if (e == hipSuccess && bytes) e = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
        return e;
    }
};
}  // namespace

extern "C" {

// A:    [rows rounded up to 256][Kp] fp16 bits, planar rows (the kernel loads whole 256-row tiles)
// Bf:   [2][Kp / 64][192][32] fp16 bits, the even and the odd table (fold_table.h)
// C:    [2][rows_alloc][384] float, in / out;  part: [2][n_chunks][D] float, in / out;  nvoiced: [n_chunks] int, in / out,
//       n_chunks = (rows_alloc + 31) / 32;  scan_w: the 32 weights of a scan chunk
int gh_fold(const unsigned short *A, const unsigned short *Bf, int rows, int rows_alloc, int Kp, int D, const float *scan_w, float *C, float *part, int *nvoiced)
{
    constexpr int Dp = 384;
    if (rows < 1 || rows_alloc < rows || Kp < 64 || Kp % 64 != 0 || D < 3 || D > Dp || (D & 1) == 0 || Dp - D >= 192 || !A || !Bf || !scan_w || !C || !part || !nvoiced)
        return (int)hipErrorInvalidValue;
    const int rows_pad = (rows + 255) / 256 * 256, n_chunks = (rows_alloc + 31) / 32;
    const size_t c_bytes = (size_t)2 * rows_alloc * Dp * 4, part_bytes = (size_t)2 * n_chunks * D * 4, nv_bytes = (size_t)n_chunks * 4;
    DBuf dA, dB, dC, dP, dN;
    hipError_t e;
    if ((e = dA.up(A, (size_t)rows_pad * Kp * 2)) != hipSuccess) return (int)e;
    if ((e = dB.up(Bf, (size_t)2 * (Kp / 64) * 192 * 32 * 2)) != hipSuccess) return (int)e;
    if ((e = dC.up(C, c_bytes)) != hipSuccess) return (int)e;
    if ((e = dP.up(part, part_bytes)) != hipSuccess) return (int)e;
    if ((e = dN.up(nvoiced, nv_bytes)) != hipSuccess) return (int)e;
    GemmArgs ga{};
    ga.A = dA.p; ga.Bf = dB.p; ga.C = (float *)dC.p;
    ga.rows = rows; ga.chunk_frames = rows; ga.total_frames = rows_alloc; ga.frame0 = 0;
    ga.Kp = Kp; ga.Dp = Dp; ga.a_row_elems = Kp; ga.c_plane_elems = (long long)rows_alloc * Dp;
    ga.part = (float *)dP.p; ga.nvoiced = (int *)dN.p; ga.D = D; ga.n_chunks = n_chunks; ga.part_plane_stride = (long long)n_chunks * D;
    for (int t = 0; t < 32; ++t) ga.scan_w[t] = scan_w[t];
    const size_t smem = (size_t)FOLD_NS * (256 + 192) * 64;
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_srp_gemm_f16_fold), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_srp_gemm_f16_fold, dim3(rows_pad / 256, 2), dim3(512), smem, 0, ga);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = hipDeviceSynchronize()) != hipSuccess) return (int)e;
    if ((e = hipMemcpy(C, dC.p, c_bytes, hipMemcpyDeviceToHost)) != hipSuccess) return (int)e;
    if ((e = hipMemcpy(part, dP.p, part_bytes, hipMemcpyDeviceToHost)) != hipSuccess) return (int)e;
    return (int)hipMemcpy(nvoiced, dN.p, nv_bytes, hipMemcpyDeviceToHost);
}

}  // extern "C"
