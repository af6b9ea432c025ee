// stream_plan.h -- a launch of the stream path as a value.
// Host side only and pure: the fixed shape of a context (StreamShape), the form of a kernel -- its family and what are template
// arguments in kernels_*.hip -- and one plan function per stage, which turns the context's shape and a call's shape into
// {form, grid, block, LDS, the argument fields the launch decides}.  No HIP call, no device pointer, no mca_hip_ctx: api.hip fills the
// argument struct, asks the plan and hands it to launch(); tests/cxx/stream_plan_cli.cpp prints the plans on a machine without a GPU.
// The predicates (*_row) say which forms the build has; the lookups beside the kernels (kernels.h) instantiate exactly those rows.
#pragma once
#include "../../include/mcarray_hip.h"
#include "fft1024c.h"
#include "fft512.h"
#include "mca_internal.h"

#include <algorithm>
#include <type_traits>
#include <utility>

namespace mca {

// What mca_hip_create fixes and every launch decision reads (mca_hip_ctx derives from it; bf_pairs is set when the beamformer's
// table is built).  The mutable state -- policy, counters, buffers -- stays in the context.
struct StreamShape {
    int M = 0, P = 0, G = 0, D = 0, Dp = 0, K = 0, N = 0, H = 0, Kp = 0, S = 1, prec = 0;
    bool ula = false, stream_ok = false, generic = false;
    bool n512 = false;             // 512-sample frames with <= 8 microphones: k_stft_phat_512 / k_beamform_512 instead of the any-length kernels
    bool n2048 = false;            // 2048-sample frames on the wave-level 1024-point transform (kernels_2048.hip): the beamformer for any M, the analysis for M <= 8 and > 2
    // ULA, one fp16 operand plane (the ADAPTIVE coarse pass, plain FP16), k_stft_phat_wave: the contraction index is the PRODUCT
    // m = k * (j - i) -- pairs of spacing g at bin k steer with exp(j 2 pi k g tau_1 / N), so all (k, g) of equal product share one
    // steering column and their PHAT sums are merged before the contraction: 1 962 instead of 3 591 complex terms per row for 8
    // microphones (build_merged_tables)
    bool merged = false, fold = false; int n_merged = 0, Kp_m = 0;      // (fold: ... folded about broadside, fold_table.h)
    int tab_planes = 1, n_cu = 256;   // planes of the steering tables (2: FP16X3 and ADAPTIVE); compute units
    int bf_pairs = 0;              // k_beamform_wave: channel pairs of the steering rows (ensure_bf_table)
    bool gate = false, no_phat = false;   // the config facts the choices read: use_power_floor, gcc_weighting NONE
    int cand = -1;                 // MCA_HIP_ADAPT_CAND: -1 / unset = by the back-off policy's reports (cand_call), 1 = wherever a lazy 4 / 8-microphone call allows (no effect on other contexts), 0 = never (whole-row repair kernels)
    bool lazy_tails = true;        // MCA_HIP_ADAPT_LAZY=0: every adaptive call repairs its own last rows for the state it hands over (round 4)
};

// Fixed launch shapes of the adaptive repair pass, whose kernels walk device-side work lists
constexpr int REPAIR_ITEMS = 768;     // work items above which the repair contraction halves its K split (repair_ksplit_eff)
constexpr int LIST_GRID = 512;        // workgroups of the list-mode analysis
constexpr int REPICK_GRID = 256;      // workgroups of k_scan_repick

// f(integral_constant<int, 0>), ..., f(integral_constant<int, N - 1>): the row walk of the kernel lookups
template <class Fn, int... I>
inline void plan_static_for(Fn &&f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class Fn>
inline void plan_static_for(Fn &&f) { plan_static_for(f, std::make_integer_sequence<int, N>{}); }

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
// frames per run: `most`, halved down to `least` while n_arrays x n_frames frames make fewer than `want` runs
inline int run_len(int n_arrays, int n_frames, int most, int least, long long want)
{
    int len = most;
    while (len > least && (long long)n_arrays * ((n_frames + len - 1) / len) < want) len >>= 1;
    return len;
}

enum class StftFamily { WAVE, WAVE16, N512, N2048, SUB2, GEN, BLOCK, FEW };   // k_stft_phat_wave / _wave16 / _512 / _2048 / _sub2 / _gen / k_stft_phat / _few
struct StftForm {
    StftFamily family = StftFamily::BLOCK;
    int mt = 0;                    // MT (0: any count); R of k_stft_phat_sub2
    bool ula = false, f32 = false;
    bool pl2 = false, power = false, nophat = false, merge = false, cand = false, fuse = false;   // k_stft_phat_wave; power: _wave16 too; merge: _2048 too
};
struct PickForm { int pl, mode; }; struct RepickForm { int pl; bool patch; };      // k_scan_pick<PL, MODE>, k_scan_repick<PL, PATCH>
enum class GemmFamily { F32, F16, V2, V3, FOLD }; struct GemmForm { GemmFamily family; bool split; int bn; };   // split, bn: k_srp_gemm_f16<SPLIT, BN>
enum class BeamformFamily { WAVE_2048, WAVE_MS, WAVE, N512, GEN, OLA };
struct BeamformForm { BeamformFamily family; int npt; bool odd; int cpw, occ; };   // k_beamform_wave_ms<NPT, ODD>, k_beamform_wave<ODD>, k_beamform_ola<CPW, OCC>

// k_stft_phat_wave<MT, ULA, OutT, PL2, POWER, NOPHAT, MERGE, CAND, FUSE>: 41 kernels
constexpr bool stft_wave_row(int MT, bool ULA, bool F32, bool PL2, bool POWER, bool NOPHAT, bool MERGE, bool CAND, bool FUSE)
{
    if (MT != 4 && MT != 8) return false;
    // the merged contraction index exists for a ULA's one fp16 plane, whitened (build_merged_tables); never in list mode, so never with CAND
    if (MERGE || FUSE) return MERGE && !F32 && ULA && !PL2 && !NOPHAT && !CAND && (!FUSE || (MT == 8 && !POWER));   // FUSE: steer.h, 8 microphones, no gate
    // list mode of a candidate-column call: two planes, no gate, with the candidate contraction of the unit behind its rows
    if (CAND) return !F32 && PL2 && !POWER && !NOPHAT;
    // fp16 rows are whitened (gcc_weighting NONE needs FP32: un-normalised spectra do not fit fp16 operands); fp32 rows have one plane
    return F32 ? !PL2 : !NOPHAT;
}
// k_stft_phat<MT, ULA, OutT>: any microphone count with and without delay groups, and the 16-microphone ULA's exact rows
constexpr bool stft_block_row(int MT, bool ULA) { return MT == 0 || (MT == 16 && ULA); }
// k_stft_phat_few<MT, ULA, OutT>: two microphones (never a ULA: delay groups start at three)
constexpr bool stft_few_row(int MT, bool ULA) { return MT == 2 && !ULA; }
// k_stft_phat_512<MT, ULA, OutT>
constexpr bool stft_512_row(int MT) { return MT == 0 || MT == 4 || MT == 8; }
// k_stft_phat_2048<MT, ULA, OutT, MERGE>: the merged index as for k_stft_phat_wave
constexpr bool stft_2048_row(int MT, bool ULA, bool F32, bool MERGE) { return (MT == 0 || MT == 4 || MT == 8) && (!MERGE || (!F32 && ULA && MT != 0)); }
// k_stft_phat_sub2<R, OutT>: 2048- / 4096-sample frames
constexpr bool stft_sub2_row(int R) { return R == 4 || R == 8; }
constexpr bool scan_pl_row(int PL) { return PL == 2 || PL == 6 || PL == 8; }
constexpr bool gemm_f16_row(int BN) { return BN == 64 || BN == 192; }
// k_beamform_wave_ms<NPT, ODD>: one pair is two microphones, never odd
constexpr bool beamform_ms_row(int NPT, bool ODD) { return NPT >= 1 && NPT <= 4 && !(NPT == 1 && ODD); }
// k_beamform_ola<CPW, OCC>: a channel per wave, four workgroups per CU up to 8 microphones; two channels per wave, two workgroups beyond
constexpr bool beamform_ola_row(int CPW, int OCC) { return (CPW == 1 && OCC == 4) || (CPW == 2 && OCC == 2); }

// the coarse (one fp16 plane) analysis of a 16-microphone uniform linear array runs on k_stft_phat_wave16
inline bool wave16_applies(const StreamShape &c) { return c.M == 16 && c.ula && !c.generic && !c.no_phat; }
// 2048-sample frames, 3 .. 8 microphones: a wave per channel on the 1024-point complex transform + split, spectra in LDS, thread = two bins (k_stft_phat_2048)
inline bool n2048_analysis(const StreamShape &c) { return c.n2048 && c.M > 2 && c.M <= 8; }
// the wave-per-run beamformer (k_beamform_wave) serves the 1024-sample path (one grid row of workgroups per source) when the caller's DOAs are grid
// bins (the localiser's own picks); everything else stays on k_beamform_ola / _512 / _gen
inline bool wave_beamformer_applies(const StreamShape &c)
{
    // several sources: up to 8 microphones k_beamform_wave_ms (forward transforms shared, the pair spectra in registers); more
    // microphones with two sources a grid row of k_beamform_wave per source, with three or four k_beamform_ola
    return !c.generic && !c.n512 && (c.S <= 2 || c.M <= 8) && c.M >= 2 && c.M <= MCA_MAX_MICS;
}
// threads per workgroup of the any-length kernels, measured per frame length (a workgroup's spectra fill half a
// CU's LDS from N = 2048 on, so more waves per workgroup are the only way to more waves per CU): analysis
// 256 / 1024 / 1024, synthesis 256 / 512 / 1024 threads for N <= 1024 / 2048 / 4096+
inline int gen_threads(const StreamShape &c, bool synthesis)
{
    if (c.N >= 4096) return 1024;
    if (c.N >= 2048) return synthesis ? 512 : 1024;
    return 256;
}

// what the caller of one analysis launch knows: it leaves the gate's frame powers; its rows take the merged contraction index (one plane of
// a merged context); every frame is to be steered at its array's predicted bin (steer.h); list mode of a candidate-column call; no PHAT
struct AnalysisFlags { bool power = false, merged = false, steer = false, cand_on = false, no_phat = false; };
struct AnalysisPlan {
    StftForm form;
    dim3 grid, block; size_t lds = 0;
    int fpb = 0, skew = 0;   // StftPhatArgs::fpb, ::skew
    bool steers = false;     // the launch is the one that also steers every frame ahead of the picks
};

// The analysis of n_arrays x n_frames frames into rows of `planes` operand planes.  list_groups > 0: list mode (the repair pass), that
// many listed groups of REPAIR_GROUP frames in the pass on a fixed grid of at most list_cap workgroups.
inline AnalysisPlan plan_analysis(const StreamShape &c, bool f32, int planes, int n_arrays, int n_frames, int list_groups, int list_cap, const AnalysisFlags &fl)
{
    AnalysisPlan p;
    const bool list = list_groups > 0;
    const int M = c.M, nf = n_frames, mt48 = M == 8 ? 8 : M == 4 ? 4 : 0;
    StftForm &f = p.form;
    f.ula = c.ula; f.f32 = f32;
    p.block = dim3(512);
    auto run_len = [&](int most, int least, long long want) { return mca::run_len(n_arrays, nf, most, least, want); };
    // one run of frames per workgroup; list mode: fixed, moderate grids -- the kernels of the repair pass walk their device-side work lists
    auto run_grid = [&]() { return list ? dim3(std::min(list_groups, list_cap), 1) : dim3((nf + p.fpb - 1) / p.fpb, n_arrays); };
    // the wave-per-run kernels: a workgroup of four runs.
    // One resident round of two workgroups per CU (the bench shapes: 8 x 4096 and 128 x 256 frames of 8 microphones): the CU issues
    // oldest-first, so the FIRST workgroup of every CU is done early (180 against 244 us on the bench shape, profiles/
    // r05_run_queue_negative.log) and the other then runs alone at 83 % of the two-wave rate.  The first half of every array's run
    // groups -- dispatched first -- takes more frames per wave (StftPhatArgs::skew).  (A device-side run queue, an XCD-aware mapping
    // and one 8-wave workgroup per CU were measured slower, HISTORY.md section 10.)
    auto wave_grid = [&](bool may_skew) {
        p.grid = dim3(((nf + p.fpb - 1) / p.fpb + 3) / 4, n_arrays);
        const int sk = (3 * p.fpb + 8) / 16;      // 16 frames per wave: 19 / 13 (measured 1 ... 4: 3 is best)
        if (may_skew && (p.grid.x & 1) == 0 && (long long)p.grid.x * p.grid.y == 2LL * c.n_cu && (long long)p.grid.x * 4 * p.fpb == nf && sk > 0 && sk < p.fpb) {
            p.skew = sk;
            p.grid = dim3(p.grid.y, p.grid.x);             // (arrays, run groups): the first half of the run groups of EVERY array is dispatched first
        }
    };
    // frames per workgroup: 16 amortise the table set-up and the half frame two neighbouring workgroups both read (17 half
    // frames of input per 16 frames; measured 4 / 8 / 16 / 32: 0.312 / 0.292 / 0.286 / 0.288 ms); small batches take fewer
    // so that a few hundred workgroups exist; list mode: REPAIR_GROUP frames per unit
    p.fpb = list ? REPAIR_GROUP : run_len(16, 1, 256);
    if (c.n512) {
        // 512-sample frames, up to 8 microphones: two frames of up to 8 channels per pass on the wave-level transform (k_stft_phat_512)
        f.family = StftFamily::N512; f.mt = mt48;
        if (!list) p.fpb = run_len(8, 2, 512);
        p.grid = run_grid();
        p.lds = ((size_t)2 * 8 * 258 + 8 * FFT_SCRATCH + TW_WIN + (size_t)p.fpb * M) * sizeof(float2) + (size_t)p.fpb * 8 * sizeof(float);
        return p;
    }
    if (!list && (c.N == 4096 || c.N == 2048) && M == 2 && c.stream_ok) {
        // two microphones at 2048- / 4096-sample frames (FreqGCC at 32 / 44.1 / 48 kHz): 512-sample sub-sequences per channel
        f.family = StftFamily::SUB2; f.mt = c.N == 4096 ? 8 : 4; f.ula = false;
        p.fpb = run_len(8, 2, 512);
        p.grid = run_grid();
        p.lds = ((size_t)16 * 258 + 8 * FFT_SCRATCH + TW_WIN) * sizeof(float2) + 4 * 8 * sizeof(float);
        return p;
    }
    if (n2048_analysis(c)) {
        f.family = StftFamily::N2048; f.mt = mt48;
        f.merge = !f32 && fl.merged && planes == 1 && !list && c.ula && (M == 8 || M == 4);      // merged contraction index: ULA, one plane
        const int fp = M == 4 ? 2 : 1, mr = M == 4 ? 4 : 8;
        if (!list) p.fpb = run_len(16, 2, 512);
        p.grid = run_grid();
        p.lds = ((size_t)fp * mr * 1026 + F1K_TWORDS + 8 * F1K_SCRATCH + (size_t)p.fpb * M) * sizeof(float2) + (size_t)p.fpb * 8 * sizeof(float);
        return p;
    }
    if (!list && c.generic) {
        f.family = StftFamily::GEN; f.ula = false;
        p.grid = dim3(nf, n_arrays); p.block = dim3(gen_threads(c, false));
        p.lds = (size_t)M * (c.H + 1) * sizeof(float2) + 16;
        return p;
    }
    p.block = dim3(256);
    // a 16-microphone uniform linear array, one fp16 operand plane (the ADAPTIVE coarse pass, plain FP16): the wave-per-run kernel
    // with its whitened spectra packed to fp16 (k_stft_phat_wave16); the exact rows of such an array stay on k_stft_phat<16>
    if (!f32 && wave16_applies(c) && planes == 1 && !list) {
        f.family = StftFamily::WAVE16; f.power = fl.power; f.ula = true;
        p.fpb = run_len(16, 1, 2048);
        wave_grid(true);
        const int fpa = p.fpb + p.skew;
        p.lds = (size_t)(F1K_TWORDS + 4 * F1K_SCRATCH + 2 * 4 * fpa * 8) * sizeof(float2) + (1024 + 4 * fpa) * sizeof(float);   // (+ the scales and DC marks of unsure frames)
        return p;
    }
    // 4 or 8 microphones: one wave per run of frames on the 1024-point transform of channel pairs (k_stft_phat_wave)
    if (M == 8 || M == 4) {
        f.family = StftFamily::WAVE; f.mt = M;
        p.fpb = list ? 1 : run_len(16, 1, 2048);      // frames per wave: two waves per SIMD want 2048 runs; a listed group of REPAIR_GROUP = 4 frames per workgroup, a frame per wave
        if (list) p.grid = run_grid(); else wave_grid(M == 8);
        const bool mg = fl.merged && !list;
        const int nrank = 2 * (M - 1) * 64 * 4 + 8, regw = mg ? std::max(F1K_SCRATCH, (c.n_merged + 63) & ~63) : F1K_SCRATCH;
        // (the merged kernel keeps its Nyquist bins in registers: with its 15.5 KiB regions two workgroups just fit the 160 KiB of a CU)
        const bool fuse = mg && M == 8 && fl.steer && !fl.power && regw >= F1K_SCRATCH + STEER_LDS_ROWS * 64;      // steering ahead of the picks (steer.h): + the waves' steps Q
        p.lds = (size_t)(F1K_TWORDS + (mg ? nrank / 4 : 0) + 4 * regw + (mg ? 0 : 4 * (p.fpb + p.skew) * (M / 2)) + (fuse ? 4 * STEER_QWORDS : 0)) * sizeof(float2);
        const bool pl2 = planes == 2;
        f.power = fl.power;
        if (!f32 && mg) { f.merge = true; f.ula = true; f.fuse = fuse; p.steers = fuse; }      // merged contraction index: ULA, one plane
        else if (!f32 && pl2 && fl.cand_on && list && !fl.power) { f.pl2 = true; f.cand = true; }
        else if (!f32) f.pl2 = pl2;
        else f.nophat = fl.no_phat;
        return p;
    }
    p.grid = run_grid(); p.block = dim3(512);
    if (M == 2 && !c.ula) {
        // 2 microphones: four frames per pass so that all eight waves transform (k_stft_phat_few)
        // (measured: 0.51 -> 0.33 ms for 131 072 two-channel frames)
        f.family = StftFamily::FEW; f.mt = 2;
        p.lds = ((size_t)8 * FFT_SCRATCH + TW_WORDS + (size_t)p.fpb * 2) * sizeof(float2) + (size_t)p.fpb * 8 * sizeof(float);
        return p;
    }
    f.family = StftFamily::BLOCK; f.mt = M == 16 && c.ula ? 16 : 0;
    p.lds = ((size_t)M * FFT_SCRATCH + TW_WORDS + (size_t)p.fpb * M) * sizeof(float2) + (size_t)p.fpb * 8 * sizeof(float);
    return p;
}

// which contraction kernel a chunk of `rows` frames runs on, and over how many workgroups its K range is split
struct GemmPlan { bool v2; int ksplit; bool fold; };      // fold: k_srp_gemm_f16_fold (256-row tiles, two K segments, one plane, a folding context)
inline int plan_kp(const StreamShape &c, int planes) { return (c.merged && planes == 1) ? c.Kp_m : c.Kp; }
inline GemmPlan plan_gemm(const StreamShape &c, int planes, long long rows)
{
    GemmPlan g;
    const int kp = plan_kp(c, planes);
    // (rows: StreamCall::planned -- a call that is worked off in pieces, the chunks of the host-pointer path, plans every piece as the
    // whole call would be planned: a row's result then does not depend on how the call was cut, same kernel, same K segments, same order)
    // 256 x 384 tiles from 16 384 rows with one operand plane (128 workgroups of k_srp_gemm_f16_v3 beat the 128 x 192 kernel
    // there: 134 vs 156 us, and leave the scan's chunk results), from 32 768 rows with the hi + lo planes (343 vs 299 us at 16 384)
    // (round 6: a contraction twice as deep -- 2048-sample frames, 16 microphones: 14 350 / 15 390 elements per plane -- gives a 256 x 384
    // workgroup of a K QUARTER the work a K half has at 7 182: two planes take the big tiles from 16 384 rows there, profiles/r06_n2048.log)
    const long long deep = kp >= 12288 ? 2 : 1;
    g.v2 = c.prec != MCA_HIP_SRP_FP32 && c.Dp == 384 && rows * (planes == 2 ? deep : 1) >= 16384LL * (planes == 2 ? 2 : 1);
    if (g.v2) {
        // 256 x 384 tiles need >= ~256 workgroups to fill the chip: one K range from 65 536 rows, two halves from 32 768, and below that four
        // quarters where the contraction is deep (round 5: 16 microphones, 15 392 terms per row -- 16 384 rows were 128 workgroups on half
        // the CUs: 0.280 -> 0.183 ms + 0.021 for k_sum_planes, which folds the four partial maps before the scan; with the 3 968 merged terms
        // of 8 microphones the fold costs what the quarters save: 75 -> 54 + 22 us, profiles/r05_gemm_ksplit4.log)
        g.ksplit = rows >= 65536 ? 1 : (rows >= 32768 || kp < 6144 ? 2 : 4);      // (6144: the merged rows of 2048-sample frames, 7 936 deep, take quarters)
    } else {
        // 128 x 192 tiles: small batches (a single stream) would leave most CUs idle and walk the whole K range
        // in a handful of workgroups (0.29 ms however few frames); split K until ~512 workgroups exist, keeping
        // at least 8 K steps per workgroup
        const long long wgs = (rows + 127) / 128 * (c.Dp == 64 ? 1 : c.Dp / 192);
        const int nk = kp / (c.prec == MCA_HIP_SRP_FP32 ? 16 : 32);
        long long ks = 512 / (wgs > 0 ? wgs : 1);
        if (ks > nk / 8) ks = nk / 8;
        if (ks > 16) ks = 16;
        if (ks < 1) ks = 1;
        g.ksplit = (int)ks;
    }
    g.fold = g.v2 && g.ksplit == 2 && planes == 1 && c.merged && c.fold;
    return g;
}
struct ContractionPlan { GemmForm form; dim3 grid, block; size_t lds; int ksplit; };
// One launch of `rows` rows.  rows_planned: what plan_gemm sees for this launch (StreamCall::planned); rows_planned_chunk: ... for the
// call's full-size chunks -- one split factor per call (the scan sums the same number of partial maps for every frame): the one that
// suits the full-size chunks; a shorter last chunk may still fall back to the 128 x 192 kernel
inline ContractionPlan plan_contraction(const StreamShape &c, int planes, long long rows, long long rows_planned, long long rows_planned_chunk)
{
    ContractionPlan p{};
    p.ksplit = plan_gemm(c, planes, rows_planned_chunk).ksplit;
    if (plan_gemm(c, planes, rows_planned).v2) {
        p.grid = dim3((unsigned)((rows + 255) / 256), p.ksplit); p.block = dim3(512);
        p.lds = (size_t)(planes == 2 ? 2 : 4) * planes * (256 + 384) * 64;   // 32-deep stages: two with hi + lo planes, four with one plane (all 160 KiB)
        // (the slices of a call all have the call's split factor, so a 256-row slice of a folding two-segment call folds like the others)
        if (planes == 2) p.form.family = GemmFamily::V2;
        else if (p.ksplit == 2 && c.merged && c.fold) { p.form.family = GemmFamily::FOLD; p.lds = (size_t)FOLD_NS * (256 + 192) * 64; }
        else p.form.family = GemmFamily::V3;
    } else {
        p.grid = dim3((unsigned)((rows + 127) / 128), c.Dp == 64 ? 1 : c.Dp / 192, p.ksplit); p.block = dim3(256);
        if (c.prec == MCA_HIP_SRP_FP32) p.form.family = GemmFamily::F32;
        else p.form = {GemmFamily::F16, planes == 2, c.Dp == 64 ? 64 : 192};
    }
    return p;
}

// the repair contraction (k_srp_gemm_repair<BN>) and the patch behind it (k_repair_patch): fixed, moderate grids over device-side lists
struct RepairContractionPlan { int bn, col_tiles; dim3 grid, block, patch_grid, patch_block; };
inline RepairContractionPlan plan_repair_contraction(const StreamShape &c, long long pass_rows, int repair_ksplit)
{
    RepairContractionPlan p{};
    p.bn = c.Dp == 64 ? 64 : 192; p.col_tiles = c.Dp == 64 ? 1 : c.Dp / 192;
    const long long max_work = (pass_rows + 127) / 128 * p.col_tiles * repair_ksplit;
    p.grid = dim3((unsigned)std::min<long long>(max_work, 768)); p.block = dim3(256);
    p.patch_grid = dim3((unsigned)std::min<long long>(pass_rows, 2048)); p.patch_block = dim3(128);
    return p;
}

inline int plan_pick_pl(const StreamShape &c) { return c.D - 2 <= 128 ? 2 : c.D - 2 <= 384 ? 6 : 8; }            // positions per lane of the peak pick
struct PickPlan { PickForm form; dim3 grid, block; size_t lds; };
inline PickPlan plan_pick(const StreamShape &c, bool adaptive, int n_arrays, int n_chunks)
{
    PickPlan p{};
    p.form = {plan_pick_pl(c), adaptive ? 1 : 0};
    p.grid = dim3(n_chunks, n_arrays); p.block = dim3(std::max(round_up(c.D, 64), 512));   // 8 waves: the per-frame pick is one wave per frame
    p.lds = (size_t)SCAN_SUB * (c.Dp + 8) * sizeof(float);
    return p;
}
struct RepickPlan { RepickForm form; dim3 grid, block; size_t lds; };
// patch: the launch also patches the steered rows: the transform's table and a scratch per wave behind the energy rows
inline RepickPlan plan_repick(const StreamShape &c, bool patch, int n_arrays, int n_chunks)
{
    RepickPlan p{};
    const int thr = std::max(round_up(c.D, 64), 512);
    p.form = {plan_pick_pl(c), patch};
    p.grid = dim3((unsigned)std::min<long long>((long long)n_chunks * n_arrays, REPICK_GRID) + (patch ? STEER_TAIL_WGS : 0)); p.block = dim3(thr);
    p.lds = (size_t)32 * (c.Dp + 8) * sizeof(float) + (patch ? (size_t)(F1K_TWORDS + thr / 64 * F1K_SCRATCH) * sizeof(float2) : 0);
    return p;
}
// Not the widest peak pick (D > 386: k_scan_pick<8, 1> has no register left for the append), and only while the launch's LDS -- energy
// rows, the transform's table, a scratch per wave, the static arrays (2 048 bytes) -- fits a CU: those calls keep the stand-alone k_steer_patch.
inline bool repick_may_patch(const StreamShape &c) { return c.D - 2 <= 384 && c.D <= 512 && plan_repick(c, true, 1, 1).lds + 2048 <= 160 * 1024; }

struct BeamformPlan {
    BeamformForm form; dim3 grid, block; size_t lds;
    int ft, skew, nb, s_pass;    // BeamformWaveArgs::ft, ::skew; BeamformArgs::ft, ::nb; k_beamform_gen: sources per launch (passes over the sources)
    const char *unsupported;     // set: no launch, MCA_HIP_ERR_UNSUPPORTED with this message
};
// table: the caller's DOAs are grid bins and the steering rows are built; out_aligned: out_pcm on 8 bytes
inline BeamformPlan plan_beamform(const StreamShape &c, bool table, bool out_aligned, int n_arrays, int n_frames)
{
    BeamformPlan p{};
    p.block = dim3(256);
    if (table && c.n2048 && out_aligned) {
        // 2048-sample frames, the localiser's own picks: one wave per run of frames, a transform per channel (k_beamform_wave_2048)
        p.form.family = BeamformFamily::WAVE_2048;
        // frames per wave: a workgroup covers 4 ft - 1 frames (one analysed twice); the smallest ft whose workgroups fit ONE resident round of
        // two per CU (255 registers: two waves per SIMD), 16 when no such ft exists (many rounds anyway)
        p.ft = 16;
        for (int ft = 2; ft <= 64; ++ft)
            if ((long long)n_arrays * c.S * ((n_frames + 4 * ft - 2) / (4 * ft - 1)) <= 2LL * c.n_cu) { p.ft = ft; break; }
        p.grid = dim3((n_frames + 4 * p.ft - 2) / (4 * p.ft - 1), n_arrays, c.S);
        p.lds = (size_t)(F1K_TWORDS + 4 * F1K_SCRATCH + 4 * 512) * sizeof(float2);
        return p;
    }
    if (table && wave_beamformer_applies(c)) {
        if (c.S >= 2 && c.M <= 8) {
            // the forward transforms of a frame shared by its sources.  Frames per run (one wave each; every run re-analyses one extra
            // frame for its overlap-add carry): long runs are cheaper per frame, short ones fill the chip -- two waves per SIMD want 2048 runs
            p.form.family = BeamformFamily::WAVE_MS;
            p.form.npt = std::min(c.bf_pairs, 4); p.form.odd = c.bf_pairs != 1 && (c.M & 1);          // two microphones: one pair (never odd)
            p.ft = run_len(n_arrays, n_frames, 16, 2, 2048);
            const int runs = (n_frames + p.ft - 1) / p.ft;
            p.lds = (size_t)(F1K_TWORDS + 4 * F1K_SCRATCH) * sizeof(float2) + (size_t)4 * c.S * FFT_H * sizeof(float);
            p.grid = dim3((runs + 3) / 4, n_arrays);
            return p;
        }
        // A workgroup covers 4 ft - 1 frames (the overlap-add carries are handed off inside it, k_beamform_wave); ft is the smallest run
        // length whose workgroups are all resident at once (two per CU: 512) -- one workgroup more than that costs a whole extra round.
        p.form.family = BeamformFamily::WAVE; p.form.odd = c.M & 1;
        p.ft = 2;
        while (p.ft < 256 && (long long)n_arrays * c.S * ((n_frames + 4 * p.ft - 2) / (4 * p.ft - 1)) > 512) ++p.ft;
        const int wgs = (n_frames + 4 * p.ft - 2) / (4 * p.ft - 1);
        p.lds = (size_t)(F1K_TWORDS + 4 * F1K_SCRATCH) * sizeof(float2) + 4 * FFT_H * sizeof(float);
        // one resident round of (nearly) two workgroups per CU: the older workgroup of every CU takes longer runs (BeamformWaveArgs::skew)
        p.grid = dim3(wgs, n_arrays, c.S);
        if (c.S == 1 && (wgs & 1) == 0 && p.ft >= 8 && (long long)wgs * n_arrays > (long long)c.n_cu * 3 / 2 && (long long)wgs * n_arrays <= 2LL * c.n_cu) {
            p.skew = (3 * p.ft + 8) / 16;
            if (p.skew >= p.ft) p.skew = 0;
            else p.grid = dim3(n_arrays, wgs, c.S);
        }
        return p;
    }
    // frames per run: every run re-analyses one extra frame for its overlap-add carry, so long runs are cheaper per
    // frame (16 -> 64 frames: 0.344 -> 0.323 ms on the bench shape); smaller batches take shorter runs so that two
    // workgroups per CU exist (multiples of the 4-frame batch)
    // (the any-length kernel walks its frames one at a time behind ~15 barriers each and is latency bound: it wants as
    // many workgroups per CU as its LDS allows, up to the 8 that fill the wave slots with 256 threads)
    long long want_wgs = 512;
    if (c.generic) {
        const size_t smem_g = (size_t)(c.M + c.S) * (c.H + 1) * sizeof(float2) + (size_t)c.S * c.H * sizeof(float);
        const long long per_cu = std::max<long long>(1, std::min<long long>((160 * 1024) / (long long)smem_g, 2048 / gen_threads(c, true)));
        want_wgs = 256 * per_cu;
    }
    p.ft = run_len(n_arrays, n_frames, 64, BF_NB, want_wgs);
    if (c.n512) {
        p.form.family = BeamformFamily::N512;
        p.lds = ((size_t)2 * 8 * 258 + 8 * FFT_SCRATCH + TW_WIN + (size_t)2 * c.S * c.M * 41) * sizeof(float2) + (size_t)2 * c.S * sizeof(double);
        p.ft = run_len(n_arrays, n_frames, 64, 4, 256 * (p.lds <= 80 * 1024 ? 2 : 1));      // (two workgroups per CU up to 80 KiB)
        p.grid = dim3((n_frames + p.ft - 1) / p.ft, n_arrays); p.block = dim3(512);
        return p;
    }
    if (c.generic) {
        // all sources in one launch while M + S spectra (and the S carries) fit the 160 KiB of a CU; else as many per launch as do --
        // 16 microphones at 2048-sample frames hold two -- each pass transforming the channels again
        p.form.family = BeamformFamily::GEN;
        auto smem_for = [&](int s_pass) {
            return (size_t)(c.M + s_pass) * (c.H + 1) * sizeof(float2) + (size_t)s_pass * c.H * sizeof(float) + (size_t)(p.ft + 1) * s_pass * sizeof(double) + 8;
        };
        p.s_pass = c.S;
        while (p.s_pass > 1 && smem_for(p.s_pass) > 160 * 1024) --p.s_pass;
        p.lds = smem_for(p.s_pass);
        if (p.lds > 160 * 1024) p.unsupported = "fft_size x n_mics exceeds the 160 KiB LDS of a CU";
        p.grid = dim3((n_frames + p.ft - 1) / p.ft, n_arrays); p.block = dim3(gen_threads(c, true));
        return p;
    }
    p.form.family = BeamformFamily::OLA;
    if (c.M <= 8) { p.form.cpw = 1; p.form.occ = 4; } else { p.form.cpw = 2; p.form.occ = 2; }
    p.nb = std::max(1, BF_NB / c.S);      // 4 beamformed slots in LDS whatever the number of sources
    p.lds = ((size_t)c.M + p.nb * c.S) * FFT_SCRATCH * sizeof(float2) + (size_t)c.S * c.M * 49 * sizeof(float2) +
            TW_WORDS * sizeof(float2) + (size_t)p.nb * c.M * (1 + c.S) * sizeof(float2) +
            (size_t)(p.ft + 1) * c.S * sizeof(double);
    if (p.lds > 160 * 1024) p.unsupported = "n_mics/n_sources combination exceeds the 160 KiB LDS of a CU";
    p.grid = dim3((n_frames + p.ft - 1) / p.ft, n_arrays); p.block = dim3(512);
    return p;
}

// the steered delay-and-sum (steer.h): the patch pass over np frames of a pass and the synthesis of its runs of ft frames, one wave each
struct SteerPlan { int ft; dim3 patch_grid, synth_grid, block; size_t lds; };
inline SteerPlan plan_steer(const StreamShape &, int n_arrays, int np)
{
    SteerPlan p{};
    p.ft = run_len(n_arrays, np, 16, 2, 1024);      // (a thousand runs: one wave each)
    const int runs = (np + p.ft - 1) / p.ft;
    p.patch_grid = dim3(std::min(STEER_PATCH_WGS, (np + 3) / 4));
    p.synth_grid = dim3((runs + 3) / 4, n_arrays); p.block = dim3(256); p.lds = (size_t)(F1K_TWORDS + 4 * F1K_SCRATCH) * sizeof(float2);
    return p;
}

}  // namespace mca
