// module_plan.h -- a launch of the four module contexts (mask, bmask, multiband, temporal GCC) as a value, as mvdr_plan.h
// is for the MVDR path.  Host side only and pure: no HIP call, no device pointer, no context -- a plan function turns the few numbers a module fixed at
// create and a call's shape into {kernel form, grid, block, LDS, the argument fields the launch decides}; the entry point fills the arguments, asks the
// plan and launches (host_common.h).  tests/cxx/module_plan_cli.cpp prints the plans without a GPU.  None of these decisions changes an output byte --
// only speed: tests/test_module_plan.py holds them.
#pragma once
#include "../../include/mcarray_hip.h"
#include "bmask.h"
#include "fft512.h"
#include "mca_internal.h"

#include <algorithm>

namespace mca {

struct Launch { dim3 grid, block; size_t lds; };
inline dim3 grid_for(long long n, int per) { return dim3((unsigned)((n + per - 1) / per)); }
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
// frames per run of a workgroup: `hi`, halved down to `lo` while n_streams x ceil(n_frames / length) runs make fewer than `target` workgroups
inline int run_length(int n_streams, int n_frames, long long target, int lo = 16, int hi = 256)
{
    int len = hi;
    while (len > lo && (long long)n_streams * ceil_div(n_frames, len) < target) len >>= 1;
    return len;
}
// frames per workgroup of an analysis that takes them in passes: the same rule
inline int frames_per_block(int n_rows, int n_frames, int hi, int lo, long long target) { return run_length(n_rows, n_frames, target, lo, hi); }
// The LDS of the 512-point complex transform on the wave-level FFT: 16 rows of 258 words, a scratch per wave, the tables up to the window
// (k_mask_stream_2048, k_mb_analyse_512, k_bmask_*_2048, k_mvdr_analyse_512): 76 544 bytes
constexpr size_t N512_LAYOUT_BYTES = (size_t)(16 * N512_ROW + 8 * FFT_SCRATCH + TW_WIN) * sizeof(float2);

// the kernel forms by frame length (the index of each module's kernel table): the two wave-level forms, and any other power of two
enum FrameForm { FORM_A = 0, FORM_B = 1, FORM_GEN = 2 };

// ---- the masking module: k_mask_stream (N = 1024), k_mask_stream_2048, k_mask_stream_gen
// ft: frames per run (MaskArgs::ft; every run re-analyses 9 frames for the Q warm-up and the overlap-add carry); shorter runs for small batches so that two workgroups per CU
// exist.  noisy_first: the first call of a NOISY context, which takes its noise estimate from the stream's very first frame (FastBinauralMasking.cpp:193-197): one chunk.
// The any-length form is latency bound (one frame at a time behind ~20 barriers): as many workgroups per CU as LDS and wave slots allow (per_cu)
struct MaskStreamPlan { FrameForm form; int ft, nthr, per_cu; Launch l; };
inline MaskStreamPlan plan_mask_stream(int N, bool noisy_first, int n_streams, int n_frames)
{
    MaskStreamPlan p{N == FFT_N ? FORM_A : N == 2048 ? FORM_B : FORM_GEN, 0, 512, 2, {}};
    const int H = N / 2, K = H + 1;
    long long target = 512;
    if (p.form == FORM_A)            // 79 KiB: two workgroups per CU
        p.l.lds = (size_t)MK_NB * 2 * FFT_SCRATCH * sizeof(float2) + (size_t)MK_NB * 3 * 520 * sizeof(float) + TW_WIN * sizeof(float2) + (size_t)MK_NB * 48 * 8 * sizeof(float) +
                  520 * sizeof(float2) + 528;
    else if (p.form == FORM_B)       // four 512-sample sub-sequences per frame
        p.l.lds = N512_LAYOUT_BYTES + (size_t)2 * 48 * 8 * sizeof(float);
    else {
        p.l.lds = (size_t)2 * (H + 1) * sizeof(float2) + ((size_t)3 * K + 2 * H + 48 * 8) * sizeof(float);
        p.nthr = N >= 2048 ? 512 : 256;
        p.per_cu = (int)std::max<long long>(1, std::min<long long>((160 * 1024) / (long long)p.l.lds, 2048 / p.nthr));
        target = 256LL * p.per_cu;
    }
    p.ft = noisy_first ? n_frames : run_length(n_streams, n_frames, target);
    p.l.grid = dim3(ceil_div(n_frames, p.ft), n_streams); p.l.block = dim3(p.nthr);
    return p;
}

// ---- the filter-bank masking module: analyse, scan, synth; k_bmask_*_1024, _2048, _gen
// ft: frames per run of the synthesis (every run but the first re-synthesises one frame for the overlap-add carry)
struct BmaskPlan { FrameForm form; int ft, n_runs; Launch analyse, scan, synth; };
inline BmaskPlan plan_bmask(int N, int n_streams, int n_frames)
{
    BmaskPlan p{N == 1024 ? FORM_A : N == 2048 ? FORM_B : FORM_GEN, run_length(n_streams, n_frames, 512), 0, {}, {}, {}};
    p.n_runs = ceil_div(n_frames, p.ft);
    const unsigned ns = n_streams;
    if (p.form == FORM_A) {
        p.analyse = {dim3(ceil_div(n_frames, BM_FPB_1024), ns), dim3(512), (size_t)(BM_FPB_1024 * 2 * FFT_SCRATCH + TW_WIN) * sizeof(float2)};
        p.synth = {dim3(p.n_runs, ns), dim3(512), p.analyse.lds + (size_t)BM_FPB_1024 * 48 * sizeof(float2)};
    } else if (p.form == FORM_B) {
        p.analyse = {dim3(ceil_div(n_frames, BM_FPB_2048), ns), dim3(512), N512_LAYOUT_BYTES};
        p.synth = {dim3(p.n_runs, ns), dim3(512), p.analyse.lds + (size_t)BM_FPB_2048 * 48 * sizeof(float2)};
    } else {
        p.analyse = {dim3(n_frames, ns), dim3(256), (size_t)2 * (N / 2 + 1) * sizeof(float2)};
        p.synth = {dim3(p.n_runs, ns), dim3(256), p.analyse.lds + (size_t)2 * (N / 2) * sizeof(float) + 48 * sizeof(float2)};
    }
    p.scan = {dim3(ns), dim3(BM_SCAN_THREADS), 0};
    return p;
}

// ---- the multiband localiser: k_mb_analyse_1024 (wave-level FFT, 4 frames x 2 channels per pass), k_mb_analyse_512 (both channels of a frame in one
// 512-point complex transform, 8 frames per pass), k_mb_analyse (a frame per workgroup; fpb 1); k_mb_scan; k_mb_summary
struct MbAnalysePlan { FrameForm form; int fpb; Launch l; };
inline MbAnalysePlan plan_mb_analyse(int N, int n_arrays, int n_frames)
{
    const int H = N / 2, K = H + 1;
    const unsigned na = n_arrays;
    if (N == FFT_N) {
        const int fpb = frames_per_block(n_arrays, n_frames, 16, 4, 512);
        return {FORM_A, fpb, {dim3(ceil_div(n_frames, fpb), na), dim3(512), (size_t)8 * FFT_SCRATCH * 8 + (size_t)4 * 520 * (8 + 4) + (size_t)TW_WORDS * 8 + 16 * 4}};
    }
    if (N == 512) {
        const int fpb = frames_per_block(n_arrays, n_frames, 32, 8, 512);
        return {FORM_B, fpb, {dim3(ceil_div(n_frames, fpb), na), dim3(512), N512_LAYOUT_BYTES + 16 * 4}};
    }
    return {FORM_GEN, 1, {dim3(n_frames, na), dim3(256), (size_t)2 * (H + 1) * 8 + (size_t)K * 8 + (size_t)K * 4 + 8 * 4}};
}
// chunk: frames per chunk (MbScanArgs::chunk): every chunk re-reads 24 warm-up frames; its smoothed correlations stay in LDS (chunk x nbins x D floats)
struct MbScanPlan { int chunk; Launch l; };
inline MbScanPlan plan_mb_scan(int nbins, int D, int n_arrays, int n_frames)
{
    const int BD = nbins * D, chunk = (size_t)32 * (BD + D + nbins) * 4 <= 80 * 1024 ? 32 : 16;
    return {chunk, {dim3(ceil_div(n_frames, chunk), n_arrays), dim3((BD + 63) / 64 * 64), (size_t)chunk * (BD + D) * 4 + (size_t)chunk * nbins * 4}};
}
inline Launch plan_mb_summary(int n_arrays) { return {dim3(n_arrays), dim3(256), 0}; }

// ---- the temporal-GCC localiser: k_tgcc_frames (a workgroup per frame: the frame hook's workspace and both channels, the second one padded), k_tgcc_gate,
// and the frame hook k_tgcc_frame_f64.  W8: the window rounded up to 8 samples, nd: the delay pairs
inline size_t tgcc_hook_lds(int nd) { return (size_t)tgcc_frame_ws_doubles(nd) * 8; }
inline Launch plan_tgcc_frames(int W8, int nd, int n_arrays, int n_frames)
{
    return {dim3(n_frames, n_arrays), dim3(256), tgcc_hook_lds(nd) + (size_t)4 * (2 * W8 + TGCC_RPAD_FRONT + TGCC_RPAD_BACK)};
}
inline Launch plan_tgcc_gate(int n_arrays) { return {grid_for(n_arrays, 64), dim3(64), 0}; }
inline Launch plan_tgcc_hook(int nd) { return {dim3(1), dim3(256), tgcc_hook_lds(nd)}; }

}  // namespace mca
