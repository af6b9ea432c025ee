// bmask.h -- argument blocks and kernel declarations of the filter-bank binaural masking module
// (BinauralMaskingImpl; kernels_bmask.hip, api_bmask.hip).  Kept apart from mca_internal.h / kernels.h: nothing
// outside those two files sees the module.
#pragma once
#include <hip/hip_runtime.h>

namespace mca {

constexpr int BM_BANDS = 45;             // _nBins
constexpr int BM_FPB_1024 = 4;           // frames per pass of the 1024-sample kernels (8 waves = 4 frames x 2 channels)
constexpr int BM_SCAN_THREADS = 1024;    // workgroup of the scan over frames
constexpr int BM_FPB_2048 = 2;           // and of the 2048-sample kernels (8 waves = 2 frames x 2 channels x 2 sub-sequence pairs)

// per-context tables in device memory
struct BmaskTables {
    const float *window;      // [N] periodic Hann
    const float2 *tw;         // [N/2] exp(-j 2 pi i / N)
    const int *kb;            // [K] first band covering bin k (the second one is kb + 1), -1 if none
    const float2 *kw;         // [K] (H_kb[k], H_{kb+1}[k])
    const float2 *kp;         // [K] Parseval weights of the same two bands: c_k H^2 / N^2, c_k = 1 at DC and Nyquist, else 2
    const int *lo, *hi;       // [45] support of band b (bins with H_b > 0, inclusive), lo > hi for an empty band
    int N, logH;              // frame length, log2(N / 2)
};

struct BmaskStreamArgs {
    BmaskTables t;
    const float *pcm;
    long long stream_stride, ch_stride;
    int n_frames, ft;                        // ft: frames per run of the synthesis
    float4 *sums;                            // [streams][n_frames][45] mean(l^2), mean(r^2), mean(l r), mean(((l + r) / 2)^2)
    const float2 *gains;                     // [streams][n_frames][45] (left, right)
    const float *tail_in; float *tail_out;   // [streams][2][N/2] overlap-add carry
    float *out;                              // [streams][2][n_frames * N/2]
};

struct BmaskScanArgs {
    const float4 *sums;
    int n_frames, method;
    const float *thr;                        // [45]
    double lambda, one_minus_lambda;         // (double)0.04f, (double)(1 - 0.04f)
    float rho, inv_spatial, inv_temporal, enhance;
    double *Q;                               // [streams][45] short-time power, updated in place
    long long *frames;                       // [streams] frames seen
    float2 *gains;
    int *decisions;                          // [streams][n_frames][45], may be NULL
};

struct BmaskHookArgs {
    double *L, *R;                           // [45][W] band signals, scaled in place
    int W, method;
    const double *thr;                       // [45]
    double *Q;                               // [45]
    double lambda, one_minus_lambda, rho, spatial, temporal, enhance;
    int *decisions;                          // [45]
};

__global__ void k_bmask_analyse_1024(BmaskStreamArgs p);
__global__ void k_bmask_analyse_2048(BmaskStreamArgs p);
__global__ void k_bmask_analyse_gen(BmaskStreamArgs p);
__global__ void k_bmask_scan(BmaskScanArgs p);
__global__ void k_bmask_synth_1024(BmaskStreamArgs p);
__global__ void k_bmask_synth_2048(BmaskStreamArgs p);
__global__ void k_bmask_synth_gen(BmaskStreamArgs p);
__global__ void k_bmask_hook_analysis(const double *x, const double *h, double *analysis, int W, int n_bands);
__global__ void k_bmask_hook_residual(const double *x, double *analysis, int W);
__global__ void k_bmask_hook_param(BmaskHookArgs p);
__global__ void k_bmask_hook_synth(double *out, const double *analysis, int W, int analysis_length);

}  // namespace mca
