// gemm_harness.hip -- TEST-ONLY library (tests/test_gpu_gemm_fold.py, tests/test_gpu_gemm_kernels.py): csrc/kernels_gemm.hip included
// unchanged and compiled with the product's line for it, behind one launcher per contraction kernel.  gh_fold: one array of `rows` frames
// in a map of `rows_alloc` rows, so the caller can see that the rows behind `rows` stay as they were.  The others take the product's row
// map (rows = arrays x chunk_frames written into total_frames at frame0) and its grids.  The two plane sums of csrc/kernels_stream.hip
// live in gemm_harness_stream.hip, the library's second translation unit (that file's compile line differs).
// Entry points: extern "C", host pointers and counts in, arguments validated (hipErrorInvalidValue), device buffers sized exactly (A
// rounded up to 256 rows only where the product does so, ensure_a: the 256-row kernels load whole tiles), the hipError_t out as an int;
// they never abort or print.  Output buffers come in filled by the caller and go back whole.
// build: tests/cxx/gemm_harness.mk, which build() runs beside tests/cxx/Makefile (nothing of the product links this library)
#include <hip/hip_runtime.h>
#include "../../mcarray_amd/csrc/kernels_gemm.hip"
#include "gemm_harness.h"

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

namespace {
// the product's row map: rows = arrays x chunk_frames (the last array may be short), written at frame0 of total_frames
struct RowMap { int rows, chunk_frames, total_frames, frame0; };
bool row_map_ok(const RowMap &m)
{
    return m.rows >= 1 && m.chunk_frames >= 1 && m.frame0 >= 0 && m.total_frames >= 1 && (long long)m.frame0 + m.chunk_frames <= m.total_frames && m.rows <= (1 << 20) &&
           m.total_frames <= (1 << 20);
}
int n_arrays(const RowMap &m) { return (m.rows + m.chunk_frames - 1) / m.chunk_frames; }
void fill(GemmArgs &ga, const RowMap &m, int Kp, int Dp, int planes)
{
    ga.rows = m.rows; ga.chunk_frames = m.chunk_frames; ga.total_frames = m.total_frames; ga.frame0 = m.frame0;
    ga.Kp = Kp; ga.Dp = Dp; ga.a_row_elems = planes * Kp; ga.c_plane_elems = (long long)n_arrays(m) * m.total_frames * Dp;
}
constexpr int KP_MAX = 1 << 16, KSPLIT_MAX = 64;
}  // namespace

extern "C" {

// REPAIR_GROUP, HIST_FRAMES, HIST_UNITS, REPAIR_KSPLIT_MAX, FOLD_NS (mca_internal.h), so that the tests restate none of them
void gh_constants(int *out5)
{
    out5[0] = REPAIR_GROUP; out5[1] = HIST_FRAMES; out5[2] = HIST_UNITS; out5[3] = REPAIR_KSPLIT_MAX; out5[4] = FOLD_NS;
}

// k_srp_gemm_f32 with the product's grid (row tiles, Dp / 192, ksplit), 256 threads.
// A: [rows][Kp] float;  B: [Kp][Dp] float;  C: [ksplit][arrays][total_frames][Dp] float, in / out
int gh_f32(const float *A, const float *B, int rows, int chunk_frames, int total_frames, int frame0, int Kp, int Dp, int ksplit, float *C)
{
    const RowMap m{rows, chunk_frames, total_frames, frame0};
    if (!row_map_ok(m) || Kp < G32_BK || Kp % G32_BK != 0 || Kp > KP_MAX || Dp < G32_BN || Dp % G32_BN != 0 || Dp > 3 * G32_BN || ksplit < 1 || ksplit > KSPLIT_MAX || !A || !B || !C)
        return (int)hipErrorInvalidValue;
    gh::DBuf dA, dB, dC;
    GemmArgs ga{};
    fill(ga, m, Kp, Dp, 1);
    hipError_t e;
    if ((e = dA.up(A, (size_t)rows * Kp * 4)) != hipSuccess) return (int)e;
    if ((e = dB.up(B, (size_t)Kp * Dp * 4)) != hipSuccess) return (int)e;
    if ((e = dC.up(C, (size_t)ksplit * ga.c_plane_elems * 4)) != hipSuccess) return (int)e;
    ga.A = dA.p; ga.B = dB.p; ga.C = (float *)dC.p;
    hipLaunchKernelGGL(k_srp_gemm_f32, dim3((rows + G32_BM - 1) / G32_BM, Dp / G32_BN, ksplit), dim3(256), 0, 0, ga);
    if ((e = gh::finish()) != hipSuccess) return (int)e;
    return (int)dC.down(C);
}

// k_srp_gemm_f16<planes == 2, BN> with the product's grid (row tiles, Dp / BN, ksplit), 256 threads; BN = 64 takes Dp = 64 as the product does.
// A: [rows][planes * Kp] fp16 bits (lo plane behind hi);  B: [planes][Dp][Kp] fp16 bits;  C: [ksplit][arrays][total_frames][Dp] float, in / out
int gh_f16(int planes, int BN, const unsigned short *A, const unsigned short *B, int rows, int chunk_frames, int total_frames, int frame0, int Kp, int Dp, int ksplit, float *C)
{
    const RowMap m{rows, chunk_frames, total_frames, frame0};
    const bool dp_ok = BN == 64 ? Dp == 64 : (BN == 192 && Dp >= 192 && Dp % 192 == 0 && Dp <= 576);
    if (!row_map_ok(m) || (planes != 1 && planes != 2) || !dp_ok || Kp < G16_BK || Kp % G16_BK != 0 || Kp > KP_MAX || ksplit < 1 || ksplit > KSPLIT_MAX || !A || !B || !C)
        return (int)hipErrorInvalidValue;
    gh::DBuf dA, dB, dC;
    GemmArgs ga{};
    fill(ga, m, Kp, Dp, planes);
    hipError_t e;
    if ((e = dA.up(A, (size_t)rows * planes * Kp * 2)) != hipSuccess) return (int)e;
    if ((e = dB.up(B, (size_t)planes * Dp * Kp * 2)) != hipSuccess) return (int)e;
    if ((e = dC.up(C, (size_t)ksplit * ga.c_plane_elems * 4)) != hipSuccess) return (int)e;
    ga.A = dA.p; ga.B = dB.p; ga.C = (float *)dC.p;
    const dim3 g((rows + G16_BM - 1) / G16_BM, Dp / BN, ksplit);
    if (BN == 64 && planes == 2) hipLaunchKernelGGL((k_srp_gemm_f16<true, 64>), g, dim3(256), 0, 0, ga);
    else if (BN == 64) hipLaunchKernelGGL((k_srp_gemm_f16<false, 64>), g, dim3(256), 0, 0, ga);
    else if (planes == 2) hipLaunchKernelGGL((k_srp_gemm_f16<true, 192>), g, dim3(256), 0, 0, ga);
    else hipLaunchKernelGGL((k_srp_gemm_f16<false, 192>), g, dim3(256), 0, 0, ga);
    if ((e = gh::finish()) != hipSuccess) return (int)e;
    return (int)dC.down(C);
}

// k_srp_gemm_repair<BN> on a fixed grid of grid_x workgroups; rows = pass_rows, the row count the kernel works on is the device's:
// min(rows, (n_list - list0) * REPAIR_GROUP).
// A: [rows][2 * Kp] fp16 bits;  B: [2][Dp][Kp] fp16 bits;  C: [repair_ksplit][rows rounded up to 128][Dp] float, in / out (the product's
// room, repair_cx_rows); the kernel lays its planes out at repair_plane_stride of ITS row count
int gh_repair(int BN, const unsigned short *A, const unsigned short *B, int rows, int n_list, int list0, int Kp, int Dp, int repair_ksplit, int repair_items, int grid_x, float *C)
{
    const bool dp_ok = BN == 64 ? Dp == 64 : (BN == 192 && Dp >= 192 && Dp % 192 == 0 && Dp <= 576);
    if (rows < 1 || rows > (1 << 20) || !dp_ok || Kp < G16_BK || Kp % G16_BK != 0 || Kp > KP_MAX || repair_ksplit < 1 || repair_ksplit > REPAIR_KSPLIT_MAX || repair_items < 0 ||
        list0 < 0 || n_list < 0 || n_list > (1 << 24) || list0 > (1 << 24) || grid_x < 1 || grid_x > 4096 || !A || !B || !C)
        return (int)hipErrorInvalidValue;
    gh::DBuf dA, dB, dC, dN;
    hipError_t e;
    if ((e = dA.up(A, (size_t)rows * 2 * Kp * 2)) != hipSuccess) return (int)e;
    if ((e = dB.up(B, (size_t)2 * Dp * Kp * 2)) != hipSuccess) return (int)e;
    if ((e = dC.up(C, (size_t)repair_cx_rows(rows, repair_ksplit) * Dp * 4)) != hipSuccess) return (int)e;
    if ((e = dN.up(&n_list, 4)) != hipSuccess) return (int)e;
    GemmArgs ga{};
    fill(ga, RowMap{rows, rows, rows, 0}, Kp, Dp, 2);             // (launch_repair_contraction: one array of pass_rows frames)
    ga.c_plane_elems = (long long)rows * Dp;
    ga.A = dA.p; ga.B = dB.p; ga.C = (float *)dC.p;
    ga.n_list = (const int *)dN.p; ga.list0 = list0; ga.repair_ksplit = repair_ksplit; ga.repair_items = repair_items;
    if (BN == 64) hipLaunchKernelGGL((k_srp_gemm_repair<64>), dim3(grid_x), dim3(256), 0, 0, ga);
    else hipLaunchKernelGGL((k_srp_gemm_repair<192>), dim3(grid_x), dim3(256), 0, 0, ga);
    if ((e = gh::finish()) != hipSuccess) return (int)e;
    return (int)dC.down(C);
}

// k_srp_gemm_f16_v2 (planes = 2) or k_srp_gemm_f16_v3 (planes = 1) with the product's grid (256-row tiles, ksplit), 512 threads, Dp = 384.
// A: [rows rounded up to 256][planes * Kp] fp16 bits;  Bt: [planes][Kp / 32][384][32] fp16 bits;  C: [ksplit][arrays][total_frames][384] float, in / out
// v3 only, part != NULL: part [ksplit][arrays][n_chunks][D] float and nvoiced [arrays][n_chunks] int, in / out; scan_w: 32 weights.  The epilogue
// takes every 32-row block of a tile for one scan chunk, so the row map is whole chunks then (as the product only asks for it then).
static int v23(int planes, const unsigned short *A, const unsigned short *Bt, int rows, int chunk_frames, int total_frames, int frame0, int Kp, int ksplit, float *C, float *part,
               int *nvoiced, int D, int n_chunks, const float *scan_w)
{
    constexpr int Dp = V2_BN;
    const RowMap m{rows, chunk_frames, total_frames, frame0};
    if (!row_map_ok(m) || Kp < V3_BK || Kp % V3_BK != 0 || Kp > KP_MAX || (ksplit != 1 && ksplit != 2 && ksplit != 4) || !A || !Bt || !C) return (int)hipErrorInvalidValue;
    if (part && (planes != 1 || !nvoiced || !scan_w || D < 1 || D > Dp || rows % chunk_frames != 0 || chunk_frames % 32 != 0 || frame0 % 32 != 0 || n_chunks < 1 ||
                 (long long)n_chunks * 32 < (long long)frame0 + chunk_frames))
        return (int)hipErrorInvalidValue;
    const int rows_pad = (rows + V2_BM - 1) / V2_BM * V2_BM;
    gh::DBuf dA, dB, dC, dP, dN;
    GemmArgs ga{};
    fill(ga, m, Kp, Dp, planes);
    hipError_t e;
    if ((e = dA.up(A, (size_t)rows_pad * planes * Kp * 2)) != hipSuccess) return (int)e;
    if ((e = dB.up(Bt, (size_t)planes * Kp * Dp * 2)) != hipSuccess) return (int)e;
    if ((e = dC.up(C, (size_t)ksplit * ga.c_plane_elems * 4)) != hipSuccess) return (int)e;
    ga.A = dA.p; ga.Bt = dB.p; ga.C = (float *)dC.p;
    if (part) {
        ga.D = D; ga.n_chunks = n_chunks; ga.part_plane_stride = (long long)n_arrays(m) * n_chunks * D;
        if ((e = dP.up(part, (size_t)ksplit * ga.part_plane_stride * 4)) != hipSuccess) return (int)e;
        if ((e = dN.up(nvoiced, (size_t)n_arrays(m) * n_chunks * 4)) != hipSuccess) return (int)e;
        ga.part = (float *)dP.p; ga.nvoiced = (int *)dN.p;
        for (int t = 0; t < 32; ++t) ga.scan_w[t] = scan_w[t];
    }
    const size_t smem = (size_t)(planes == 2 ? 2 : 4) * planes * (V2_BM + V2_BN) * 64;      // api.hip: two stages of hi + lo, four of one plane
    const dim3 g(rows_pad / V2_BM, ksplit);
    if (planes == 2) {
        if ((e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_srp_gemm_f16_v2), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)) != hipSuccess) return (int)e;
        hipLaunchKernelGGL(k_srp_gemm_f16_v2, g, dim3(512), smem, 0, ga);
    } else {
        if ((e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_srp_gemm_f16_v3), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)) != hipSuccess) return (int)e;
        hipLaunchKernelGGL(k_srp_gemm_f16_v3, g, dim3(512), smem, 0, ga);
    }
    if ((e = gh::finish()) != hipSuccess) return (int)e;
    if ((e = dC.down(C)) != hipSuccess) return (int)e;
    if (part && (e = dP.down(part)) != hipSuccess) return (int)e;
    return part ? (int)dN.down(nvoiced) : (int)hipSuccess;
}
int gh_v2(const unsigned short *A, const unsigned short *Bt, int rows, int chunk_frames, int total_frames, int frame0, int Kp, int ksplit, float *C)
{
    return v23(2, A, Bt, rows, chunk_frames, total_frames, frame0, Kp, ksplit, C, nullptr, nullptr, 0, 0, nullptr);
}
int gh_v3(const unsigned short *A, const unsigned short *Bt, int rows, int chunk_frames, int total_frames, int frame0, int Kp, int ksplit, float *C, float *part, int *nvoiced, int D,
          int n_chunks, const float *scan_w)
{
    return v23(1, A, Bt, rows, chunk_frames, total_frames, frame0, Kp, ksplit, C, part, nvoiced, D, n_chunks, scan_w);
}

}  // extern "C"
