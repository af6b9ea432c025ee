// mvdr_plan.h -- a launch of the MVDR path as a value, as stream_plan.h is for the stream path.
// Host side only and pure: the fixed shape of a context (MvdrShape) and one plan function per stage, which turns that shape, a call's shape and the
// processing parameters the decision reads into {kernel form, grid, block, LDS, the argument fields the launch decides, workspace elements}.  No HIP
// call, no device pointer, no mca_hip_mvdr_ctx: api_mvdr.hip fills the argument struct, asks the plan and hands it to launch(); tests/cxx/mvdr_plan_cli.cpp
// prints the plans without a GPU.  None of these decisions changes an output byte -- only speed and workspace size: tests/test_mvdr_plan.py holds them.
#pragma once
#include "../../include/mcarray_hip.h"
#include "fft1024c.h"
#include "fft512.h"
#include "mca_internal.h"
#include "module_plan.h"

#include <algorithm>

namespace mca {

// What mca_hip_mvdr_create fixes and every launch decision reads (mca_hip_mvdr_ctx derives from it).  The processing parameters stay
// in the context; a plan that needs one takes it as an argument.
struct MvdrShape {
    int N = 0, K = 0, H = 0, logH = 0, M = 0, tri = 0, max_streams = 0;
    int Q() const { return (M + 3) / 4; }      // row slots per lane of the quad kernels
};

typedef Launch MvdrLaunch;      // (grid_for, run_length and the 512-point layout: module_plan.h)
// frames per workgroup: `most`, halved down to `least` while n_rows x n_frames frames make fewer than 1024 workgroups
inline int mvdr_run_len(int n_rows, int n_frames, int most, int least) { return run_length(n_rows, n_frames, 1024, least, most); }

// ---- the analysis: PCM -> X and the steering tables
enum class MvdrAnalyseFamily { GEN, N1024, N512 };      // k_mvdr_analyse / _1024 / _512
struct MvdrAnalysePlan { MvdrAnalyseFamily family; int fpb; MvdrLaunch l; };      // fpb: the kernels' second argument (GEN: a frame per workgroup)
inline MvdrAnalysePlan plan_mvdr_analyse(const MvdrShape &c, int n_streams, int n_frames)
{
    if (c.N != FFT_N && c.N != 512) {
        // threads per workgroup of the block-cooperative FFT: a radix-4 pass has M * N/8 work items, two per thread
        int t = 256;
        while (t < 1024 && t * 2 <= c.M * (c.N / 8)) t <<= 1;
        return {MvdrAnalyseFamily::GEN, 1, {dim3(n_frames, n_streams), dim3(t), (size_t)c.M * (c.H + 1) * sizeof(float2)}};
    }
    // 1024-sample frames: wave-level FFT, one wave per channel, eight channels per pass; 512: two channels per wave pass (kernels_stream.hip)
    const int fpb = mvdr_run_len(n_streams, n_frames, 8, 1);
    const size_t lds = c.N == FFT_N ? (size_t)(8 * 580 + TW_WORDS) * sizeof(float2) : N512_LAYOUT_BYTES;
    return {c.N == FFT_N ? MvdrAnalyseFamily::N1024 : MvdrAnalyseFamily::N512, fpb, {dim3((n_frames + fpb - 1) / fpb, n_streams), dim3(512), lds}};
}

// ---- the solve: which kernel, and how the launch is cut
// HAND: k_mvdr_solve<Q, full>; TEMPLATE: k_mvdr_solve_t of (Q, full, S, nulls, weight, noise); RTF: k_mvdr_solve_rtf_t of (Q, full, S, noise);
// RTF_NULLS: k_mvdr_solve_rtf_nulls_t of (Q, S, noise).  Under the nulls one instantiation serves M = 4Q and M < 4Q: full is false there.
enum class MvdrSolveFamily { HAND, TEMPLATE, RTF, RTF_NULLS };
struct MvdrSolveChoice { MvdrSolveFamily family; int Q; bool full; int S; bool nulls; MvdrWeight weight; bool noise; };
// update: the caller brings weights; masked: one per cell, not per frame; pf_on: the post-filter takes the noise plane (a call without
// weights then passes ones).  An RTF call takes a weight per cell always.  A gain that rounds to 0 in fp32 is gain 0.
inline MvdrSolveChoice plan_mvdr_solve_choice(const MvdrShape &c, bool rtf, int n_sources, double null_gain, bool update, bool masked, bool pf_on)
{
    MvdrSolveChoice k{MvdrSolveFamily::TEMPLATE, c.Q(), c.M == 4 * c.Q(), n_sources, n_sources > 1 && (float)null_gain > 0.f, MvdrWeight::CELL, pf_on};
    if (rtf) k.family = k.nulls ? MvdrSolveFamily::RTF_NULLS : MvdrSolveFamily::RTF;
    else {
        k.weight = !update && !pf_on ? MvdrWeight::NONE : update && masked ? MvdrWeight::CELL : MvdrWeight::FRAME;
        if (mvdr_solve_hand_written(k.S, k.weight, k.noise)) k.family = MvdrSolveFamily::HAND;
    }
    if (k.nulls) k.full = false;
    return k;
}
// whether the build has the kernel of a choice (the rows the lookups of kernels.h instantiate), and the dynamic LDS of its workgroups
inline bool mvdr_solve_choice_row(const MvdrSolveChoice &k)
{
    const bool qs = k.Q >= 1 && k.Q <= 4 && k.S >= 1 && k.S <= MCA_MAX_SOURCES;
    switch (k.family) {
    case MvdrSolveFamily::HAND: return qs && !k.nulls && mvdr_solve_hand_written(k.S, k.weight, k.noise);
    case MvdrSolveFamily::TEMPLATE: return mvdr_solve_row(k.Q, k.full, k.S, k.nulls, k.weight, k.noise);
    case MvdrSolveFamily::RTF: return qs && !k.nulls;
    default: return qs && k.S >= 2 && k.nulls && !k.full;
    }
}
inline int mvdr_solve_lds(const MvdrSolveChoice &k) { return k.nulls ? mvdr_nulls_lds_bytes(k.Q, k.S, mvdr_solve_form(k.Q, false, k.S, true, k.weight, k.noise).S1) : 0; }
// 512 workgroups are resident (two per CU at 253 VGPRs) and all take the same time: the workgroups behind the last whole round (256
// streams x 513 bins: 4 of 2052) would hold the GPU for a round of their own.  They go in a second launch, cut along the FRAMES into
// pieces that each repeat the (cheap) covariance recursion of the frames before their own.  An unsplit launch updates the state in
// place; the pieces all read the entry state, so the last piece writes the exit state to a scratch copy (<= 128 x 64 problems) that is
// moved over behind the launch.  n_loop: the frames the launch walks (an RTF call: the chunk's).
struct MvdrSolveSplit { long long n_prob, main_prob, tail_prob; int pieces; dim3 grid, tail_grid, block; bool scratch; };
inline MvdrSolveSplit plan_mvdr_solve_split(const MvdrShape &c, int n_streams, int n_loop)
{
    MvdrSolveSplit s{};
    s.n_prob = s.main_prob = (long long)n_streams * c.K; s.pieces = 1; s.block = dim3(256);
    const long long n_wg = (s.n_prob + 63) / 64, rem_wg = n_wg % 512;
    if (n_wg > 512 && rem_wg > 0 && rem_wg <= 128)
        while (s.pieces < 8 && rem_wg * s.pieces * 2 <= 512 && n_loop / (s.pieces * 2) >= 4) s.pieces *= 2;
    if (s.pieces > 1) {
        s.main_prob = (n_wg - rem_wg) * 64; s.tail_prob = s.n_prob - s.main_prob; s.scratch = true;
        s.tail_grid = dim3((unsigned)((s.tail_prob + 63) / 64 * s.pieces));
    }
    s.grid = grid_for(s.main_prob, 64);
    return s;
}

// ---- the quad kernels beside the solve (a quad per problem, 64 problems per workgroup) and the post-filter (a thread per cell).  k_mvdr_rtf: the steering
// plane holds fc frames: all of them, or as many as the workspace cap takes, in chunks of equal length, the last one shorter at most (the cut changes no byte)
struct MvdrRtfPlan { int fc; MvdrLaunch l; };
inline MvdrRtfPlan plan_mvdr_rtf(const MvdrShape &c, int n_streams, int n_sources, int n_frames, size_t cap_cells)
{
    MvdrRtfPlan p{n_frames, {grid_for((long long)n_streams * n_sources * c.K, 64), dim3(256), 0}};
    const size_t per_frame = (size_t)n_streams * n_sources * c.K * c.M;
    if (per_frame * n_frames > cap_cells) {
        const int fmax = (int)std::max<size_t>(1, cap_cells / per_frame), chunks = (n_frames + fmax - 1) / fmax;
        p.fc = (n_frames + chunks - 1) / chunks;
    }
    return p;
}
inline MvdrLaunch plan_mvdr_estmask(const MvdrShape &c, int n_streams, int n_frames) { return {grid_for((long long)n_streams * n_frames * c.K, 64), dim3(256), 0}; }
inline MvdrLaunch plan_mvdr_postfilter(const MvdrShape &c, int n_streams, int n_sources) { return {grid_for((long long)n_streams * n_sources * c.K, 256), dim3(256), 0}; }

// ---- the synthesis: one inverse transform + overlap-add per (stream, look direction), ft frames per workgroup (MvdrSynthArgs::ft)
struct MvdrSynthPlan { int ft; MvdrLaunch l; };
inline MvdrSynthPlan plan_mvdr_synth(const MvdrShape &c, int n_streams, int n_sources, int n_frames)
{
    const int n_out = n_streams * n_sources, ft = mvdr_run_len(n_out, n_frames, 16, 2);
    return {ft, {dim3((n_frames + ft - 1) / ft, n_out), dim3(c.H >= 1024 ? 512 : 256), (size_t)(c.H + 1) * sizeof(float2) + (size_t)c.H * 4}};
}

// ---- the four scans over a band of bins: the Capon spectrum, the map, and the own tracks on either grid
// the chunks of MVDR_SPEC_CHUNK bins a band touches, the slices of partial sums (four waves per chunk), the factored phasors per
// microphone, the tiles of MVDR_MAP_TILE directions
struct MvdrBand { int chunk0, n_chunks, n_slices, nhi, nph, n_tiles; };
inline MvdrBand mvdr_band(const MvdrShape &c, int bin_lo, int bin_hi, int Dpad)
{
    const int chunk0 = bin_lo / MVDR_SPEC_CHUNK, n_chunks = bin_hi / MVDR_SPEC_CHUNK - chunk0 + 1, nhi = c.N / 64 + 1;
    return {chunk0, n_chunks, n_chunks * 4, nhi, nhi + 32, (Dpad + MVDR_MAP_TILE - 1) / MVDR_MAP_TILE};
}
struct MvdrScanPlan {
    MvdrBand b;
    int pass;                          // streams a pass takes (the spectrum and the tracks on one angle: all of them)
    size_t lds;                        // of k_mvdr_spectrum / k_mvdr_map_scan: a chunk's covariances and weights (68 KiB at 16 microphones); the track kernels' LDS is static
    size_t per_u, per_f, per_part;     // elements per stream of the workspaces U, F (map-mode tracks) and part
    int wg_tables, wg_vectors, wg_scan;      // workgroups per stream of the tables, the vectors (map-mode tracks) and the scan
    dim3 grid(int wgs, int n_streams) const { return dim3((unsigned)((long long)wgs * n_streams)); }
};
// slots: the own tracks (1: the Capon scan); tiled: a workgroup per tile of directions, and the streams in passes under the cap of
// the context's workspace (mca_hip_mvdr_set_rtf_workspace; cap_cells of 8 bytes), one stream a pass at the least -- a stream's bytes
// do not depend on its pass; vectors: U and F carry the steering vectors from one kernel to the next
inline MvdrScanPlan mvdr_scan_plan(const MvdrShape &c, int bin_lo, int bin_hi, int Dpad, int slots, bool tiled, bool vectors, int n_streams, size_t cap_cells)
{
    MvdrScanPlan p{};
    p.b = mvdr_band(c, bin_lo, bin_hi, Dpad);
    p.lds = (size_t)MVDR_SPEC_CHUNK * (c.tri * sizeof(float2) + 4);
    p.per_part = (size_t)slots * p.b.n_chunks * 4 * Dpad;
    if (vectors) { p.per_f = (size_t)slots * p.b.n_chunks * MVDR_SPEC_CHUNK; p.per_u = p.per_f * c.M; }
    p.wg_tables = slots; p.wg_vectors = slots * p.b.n_chunks; p.wg_scan = p.wg_vectors * (tiled ? p.b.n_tiles : 1);
    const size_t per = 2 * p.per_u + p.per_f + p.per_part;       // floats
    p.pass = tiled && per ? (int)std::min<size_t>(std::max<size_t>(1, cap_cells * 2 / per), (size_t)n_streams) : n_streams;
    return p;
}
inline MvdrScanPlan plan_mvdr_spectrum(const MvdrShape &c, int bin_lo, int bin_hi, int Dpad, int n_streams) { return mvdr_scan_plan(c, bin_lo, bin_hi, Dpad, 1, false, false, n_streams, 0); }
inline MvdrScanPlan plan_mvdr_tracks(const MvdrShape &c, int bin_lo, int bin_hi, int Dpad, int n_own, int n_streams) { return mvdr_scan_plan(c, bin_lo, bin_hi, Dpad, n_own, false, false, n_streams, 0); }
inline MvdrScanPlan plan_mvdr_map(const MvdrShape &c, int bin_lo, int bin_hi, int Dpad, int n_streams, size_t cap_cells) { return mvdr_scan_plan(c, bin_lo, bin_hi, Dpad, 1, true, false, n_streams, cap_cells); }
inline MvdrScanPlan plan_mvdr_tracks_map(const MvdrShape &c, int bin_lo, int bin_hi, int Dpad, int n_own, int n_streams, size_t cap_cells) { return mvdr_scan_plan(c, bin_lo, bin_hi, Dpad, n_own, true, true, n_streams, cap_cells); }

}  // namespace mca
