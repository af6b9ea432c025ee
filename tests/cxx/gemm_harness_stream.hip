// gemm_harness_stream.hip -- TEST-ONLY, the second translation unit of libgemm_harness.so (tests/test_gpu_gemm_kernels.py):
// csrc/kernels_stream.hip included unchanged and compiled with the product's line for it (-fno-slp-vectorize), behind launchers of the two
// kernels that sum split-K partial maps in a stated order, k_sum_planes and k_repair_patch.  Same rules as gemm_harness.hip: host pointers
// and counts in, arguments validated -- every listed unit is checked against the maps it addresses before anything is launched --, exactly
// sized device buffers, the hipError_t out as an int, no abort and no print; in / out buffers go back whole.
#include <hip/hip_runtime.h>
#include "../../mcarray_amd/csrc/kernels_stream.hip"
#include "gemm_harness.h"

using namespace mca;

extern "C" {

// C: (planes - 1) * stride + 4 * n4 floats, in / out: plane pl at pl * stride; the first 4 * n4 floats of plane 0 take the sum
int gh_sum_planes(float *C, long long n4, int planes, long long stride)
{
    if (!C || n4 < 1 || n4 > (1 << 22) || planes < 1 || planes > 64 || stride < 4 * n4 || stride % 4 != 0 || stride > (1 << 26)) return (int)hipErrorInvalidValue;
    gh::DBuf dC;
    hipError_t e;
    if ((e = dC.up(C, (size_t)((planes - 1) * stride + 4 * n4) * 4)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_sum_planes, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, 0, (float *)dC.p, n4, planes, stride);
    if ((e = gh::finish()) != hipSuccess) return (int)e;
    return (int)dC.down(C);
}

// k_repair_patch on a fixed grid of grid_x workgroups of 128 threads.
// Cx:   [ksplit][pass_rows rounded up to 128][Dp] float (the product's room; the kernel reads repair_ksplit_eff planes at
//       repair_plane_stride of its own row count, min(n_list - list0, pass_rows / REPAIR_GROUP) * REPAIR_GROUP)
// list: [list_len] units, need: [need_len] int, in / out
// C:    (c_planes - 1) * c_plane_stride + arrays * n_frames * Dp float, in / out;  hist_C: [arrays][HIST_FRAMES][Dp] float, in / out, or NULL
int gh_repair_patch(const float *Cx, int pass_rows, int ksplit, int items, const int *list, int list_len, int n_list, int list0, int groups_per_array, int *need, int need_len,
                    float *C, int c_planes, long long c_plane_stride, int arrays, int n_frames, int Dp, float *hist_C, int hist_base, int grid_x)
{
    if (!Cx || !list || !need || !C || pass_rows < 1 || pass_rows > (1 << 20) || ksplit < 1 || ksplit > REPAIR_KSPLIT_MAX || items < 0 || list_len < 0 || n_list < 0 ||
        list0 < 0 || list0 > n_list || groups_per_array < 1 || need_len < 1 || c_planes < 1 || c_planes > 16 || arrays < 1 || arrays > 4096 || n_frames < 1 || n_frames > (1 << 20) ||
        Dp < 64 || Dp % 64 != 0 || Dp > 576 || c_plane_stride < (long long)arrays * n_frames * Dp || c_plane_stride > (1 << 26) || hist_base < 0 || grid_x < 1 || grid_x > 4096)
        return (int)hipErrorInvalidValue;
    const int n_here = n_list - list0 < pass_rows / REPAIR_GROUP ? n_list - list0 : pass_rows / REPAIR_GROUP;
    if (list0 + n_here > list_len) return (int)hipErrorInvalidValue;
    for (int g = 0; g < n_here; ++g) {
        const int e = list[list0 + g];
        if (e < 0 || e >= need_len) return (int)hipErrorInvalidValue;
        const bool hist = hist_C != nullptr && e >= hist_base;
        if ((hist ? (e - hist_base) / HIST_UNITS : e / groups_per_array) >= arrays) return (int)hipErrorInvalidValue;
    }
    gh::DBuf dX, dL, dN, dNeed, dC, dH;
    hipError_t e;
    if ((e = dX.up(Cx, (size_t)repair_cx_rows(pass_rows, ksplit) * Dp * 4)) != hipSuccess) return (int)e;
    if ((e = dL.up(list, (size_t)list_len * 4)) != hipSuccess) return (int)e;
    if ((e = dN.up(&n_list, 4)) != hipSuccess) return (int)e;
    if ((e = dNeed.up(need, (size_t)need_len * 4)) != hipSuccess) return (int)e;
    if ((e = dC.up(C, (size_t)((c_planes - 1) * c_plane_stride + (long long)arrays * n_frames * Dp) * 4)) != hipSuccess) return (int)e;
    if (hist_C && (e = dH.up(hist_C, (size_t)arrays * HIST_FRAMES * Dp * 4)) != hipSuccess) return (int)e;
    RepairPatchArgs pp{};
    pp.Cx = (const float *)dX.p; pp.pass_rows = pass_rows; pp.col_tiles = Dp == 64 ? 1 : Dp / 192; pp.ksplit = ksplit; pp.items = items;
    pp.list = (const int *)dL.p; pp.n_list = (const int *)dN.p; pp.list0 = list0; pp.groups_per_array = groups_per_array; pp.need = (int *)dNeed.p;
    pp.C = (float *)dC.p; pp.c_planes = c_planes; pp.c_plane_stride = c_plane_stride; pp.n_frames = n_frames; pp.Dp = Dp;
    pp.hist_C = hist_C ? (float *)dH.p : nullptr; pp.hist_base = hist_base;
    hipLaunchKernelGGL(k_repair_patch, dim3(grid_x), dim3(128), 0, 0, pp);
    if ((e = gh::finish()) != hipSuccess) return (int)e;
    if ((e = dC.down(C)) != hipSuccess) return (int)e;
    if ((e = dNeed.down(need)) != hipSuccess) return (int)e;
    return hist_C ? (int)dH.down(hist_C) : (int)hipSuccess;
}

}  // extern "C"
