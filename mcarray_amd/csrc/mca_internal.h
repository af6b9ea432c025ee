// mca_internal.h -- argument blocks shared by the kernels and the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>

#define MCA_MAX_SOURCES 4
#define MCA_MAX_MICS 16

namespace mca {

constexpr int MK_NB = 4;           // frames per batch of k_mask_stream (8 waves = 4 frames x 2 channels)
constexpr int MK_WARM = 8;         // frames of Q warm-up for mask chunks that do not start a stream (0.04^8 = 6.6e-12)
constexpr int BF_NB = 4;           // frames per inverse-FFT batch of k_beamform_ola
constexpr int GCC2_DOAWARM = 64;   // frames of DOA-recursion warm-up in k_gcc2_scan (0.6^64 = 6e-15)
constexpr int SCAN_WARM = 96;     // frames of IIR warm-up per scan chunk (0.8^96 = 5e-10 << fp32 epsilon)
constexpr int KG = 513;            // complex K-slots per delay group in the A / B contraction index (g * KG + k)
#ifndef MCA_SCAN_CHUNK
#define MCA_SCAN_CHUNK 32
#endif
#ifndef MCA_SCAN_SUB
#define MCA_SCAN_SUB 32
#endif
constexpr int SCAN_CHUNK = MCA_SCAN_CHUNK;    // frames per chunk of the exact chunked scan (32: 0.928 ms per bench step, 64: 0.965; must exceed REPAIR_WARM)
constexpr int SCAN_SUB = MCA_SCAN_SUB;      // frames per LDS sub-batch of k_scan_pick
#ifndef MCA_SCAN_LD
#define MCA_SCAN_LD 8
#endif
constexpr int SCAN_LD = MCA_SCAN_LD;        // map rows (x split-K planes) a thread of the scan kernels keeps in flight (16 / 32 measured slower: 0.939 / 0.955 vs 0.939 ms per step)
#ifndef MCA_REPAIR_WARM
#define MCA_REPAIR_WARM 16
#endif
constexpr int REPAIR_WARM = MCA_REPAIR_WARM;   // exact rows recomputed BEFORE a flagged frame (adaptive SRP precision): 0.8^17 = 2.3e-2 of the coarse
                                  // error (~1.6e-5 of the map's peak) remains, i.e. ~3.6e-7 of the peak -- five times below the error of the
                                  // three-product split itself and below the 1e-6 tie bar of the parity tests.  (Round 2 used 24 rows,
                                  // 0.8^25: the always-recomputed tail of every array and call is what the repair pass mostly works on
                                  // when a call has many arrays and few frames -- 128 x 256: 13.9 % of the rows with 24, 10.7 % with 16.
                                  // Round 4, ADVICE r3: the flips against FP16X3 over 40 configurations / 696 320 frames are the SAME with
                                  // 16 and with 24 rows, every differing frame a tie at the parity bar's level (profiles/r04_adaptive_check.json /
                                  // _warm24.json; the count of the shipped build is the one in include/mcarray_hip.h: 41 picks on 29 frames,
                                  // profiles/r05_adaptive_check.json); 24 rows cost +12 % / +30 % repair time at 8 x 4096 / 128 x 256.)
constexpr int REPAIR_GROUP = 4;   // frames per repair unit = frames per list-mode pass of a k_stft_phat workgroup
// Lazy tails (round 5; ADAPTIVE, ungated, the wave-per-run analysis): a call does NOT recompute its last REPAIR_WARM + 1 rows exactly for the
// state it hands over.  It keeps what the NEXT call needs to do so -- the last HIST_FRAMES frames of PCM (HIST_SAMPLES per channel), their
// coarse map rows and the energies in front of them -- and the next call lists them as repair units only when one of its first
// REPAIR_WARM frames is flagged (a few arrays per call instead of all of them: 2 560 of the 3 492 rows a 128 x 256 call recomputed).
// History units are numbered behind the call's own: hist_base + array * HIST_UNITS + u, frames 4 u .. 4 u + 3 of the history.
constexpr int HIST_FRAMES = REPAIR_WARM, HIST_UNITS = HIST_FRAMES / REPAIR_GROUP, HIST_SAMPLES = (HIST_FRAMES + 1) * 512;
static_assert(HIST_FRAMES % REPAIR_GROUP == 0, "history = whole repair units");

// cand_unit.h: the exact values of the listed rows AT THEIR CANDIDATE COLUMNS, written straight into the map.
// Which columns (wave_candidates, kernels_stream.hip): a flagged frame's pick is, on the exact map, among the positions whose coarse |En|
// reaches v - tau, v the best GUARANTEED peak of the coarse row -- a window in which the median-filtered sign chain, with every first
// difference within tau taken as of either sign, is pinned to "rising" at one end and to "falling" at the other: the exact map has a
// peak in there worth at least the window's smallest coarse energy - tau / 2, and a position below v - tau cannot reach that -- plus the
// two columns either side that feed the sign / median chain (:159-173) of such a position.  The second pick then runs on a row that is
// exact wherever it matters and coarse elsewhere.  A frame without such a window (a flat map) takes every column; the contexts that flag
// whole rows by construction (eager tails, unsure rows, several sources) keep the whole-row kernels (api.hip, cand_call).
constexpr int CAND_WORDS_MAX = 20;          // Dp <= 640 (the peak pick handles D <= 514)
struct CandArgs {
    const void *A;           // exact analysis rows of the listed units, fp16 hi + lo planes: [rows][a_row_elems], row = 4 x list position + frame
    const void *B;           // steering table, fp16 hi + lo planes: [2][Dp][Kp]
    int Kp, Dp, a_row_elems;
    const int *list; const int *n_list; int list0, pass_rows;
    unsigned *umask; int umask_words;                        // read and cleared
    int *need;                                               // the units' test-and-set words, released here
    int groups_per_array, n_frames;
    float *C; int c_planes; long long c_plane_stride;       // plane 0 takes the exact value, the others zeros (as k_repair_patch)
    float *hist_C; int hist_base;                            // lazy tails: units >= hist_base are rows of hist_C
};

// Delay-and-sum on the half spectrum (steer.h): k_stft_phat_wave<..., FUSE> steers every frame at the array's PREDICTED bin while it
// holds the separated spectra, k_steer_patch redoes the frames whose pick came out different, k_steer_synth turns the rows into audio.
constexpr int STEER_QWORDS = 8 * 7;   // float2 words of a wave's copy of the steps Q_c[1..7] of its array's predicted bin (LDS)
constexpr int STEER_LDS_ROWS = 13;     // 64-word rows of a wave's region behind the exchange scratch: 8 of Y, 3 of parked Nyquist values, 2 of the parked base
constexpr int STEER_Y_ZN = 8, STEER_Y_BASE = 11;
constexpr int STEER_MISS_NUM = 1, STEER_MISS_DEN = 3;   // the guard (api.hip, steer_policy_begin): half of the measured break-even of 0.66 (profiles/r07_miss_share_sweep.log)
constexpr int STEER_ROW = 520;   // float2 words per row of Y: A[k] = {1, 2, ..., 2, 1} Y[k] / N at bins 0..512, padded to whole 64-byte lines
struct SteerArgs {
    const float4 *rows;      // [D + 1][pairs][64 lanes] (P_a, P_b)[lam] / (M N): the base of the lane's bins lam + 64 s (k_steer_table); row 0: DOA 0 rad
    const float2 *q;         // [D + 1][M][8] P_c[64 s]: their wave-uniform steps
    const float *nyq;        // [D + 1][M] Re P_c[512] / (M N)
    const int *pred;         // [arrays] the predicted bin: the array's last pick of the previous call (-1: none yet, the initial DOA)
    float2 *Y;               // [arrays][total_frames][STEER_ROW]
};
// k_steer_patch: the frames whose pick is not the predicted bin (all = 1: every frame -- the analysis of this call did not steer) through
// the same routine at their final bins, one wave per frame, a fixed grid striding over the call's frames; counts the misses.
// An ADAPTIVE call that steered ahead has no such launch: its second pick patches (k_scan_repick<PL, true>, STEER_TAIL_WGS).
constexpr int STEER_TAIL_WGS = 256;       // k_scan_repick<PL, true>: workgroups behind the re-pick ones that stride over the miss list
constexpr int STEER_PATCH_WGS = 512;      // k_steer_patch: a fixed grid (two workgroups per CU) strides over the frames
struct SteerPatchArgs {
    const float *pcm; long long array_stride, mic_stride;
    int n_arrays, n_frames;  // n_frames: the call's (rows of Y, of doa_bin)
    int f0, f1;              // the frames of this pass
    const float *window;
    const int *doa_bin;      // [arrays][n_frames] final picks
    SteerArgs bf;
    int y_f0, y_frames;      // Y holds the frames y_f0 ... y_f0 + y_frames - 1 of every array
    int all;
    unsigned long long *miss;   // [0] running total of frames whose pick was not the predicted bin, [1] those of arrays that had a prediction (the guard's)
};
// k_steer_synth: rows of Y -> inverse transform -> overlap-add; grid (runs / 4, arrays) x 256, one wave per run of ft frames (it transforms
// the frame in front of its run once more for the carry).  The workgroup (0, a) of the call's LAST pass leaves the array's last pick as the next call's prediction.
struct SteerSynthArgs {
    const float2 *Y; int n_frames, f0, f1, ft, y_f0, y_frames;
    float *out;              // [arrays][n_frames * hop]
    const float *tail_in; float *tail_out;    // [arrays][hop] the carry into hop f0 / out of frame f1 - 1 (the stream's, or the one between two passes)
    const int *doa_bin; int *pred_out;        // pred_out: NULL unless this is the call's last pass
    unsigned long long *report; unsigned long long seq; unsigned long long *miss_total;   // last pass: the call's missed frames and its number, to page-locked memory
    int *n_miss;             // the length of the miss list (ScanPickArgs::n_miss), emptied here for the next call; NULL: the second pick did not patch
};

struct StftPhatArgs {
    const float *pcm;
    long long array_stride, mic_stride;
    int M, n_frames, frame0, fpb;
    const float *window;     // [1024] periodic Hann
    void *A;                 // [arrays][n_frames][a_row_elems]
    int Kp;                  // padded contraction depth (elements per plane)
    int a_row_elems;         // elements per A row = Kp * planes
    int a_planes;            // 1 (fp32 / fp16) or 2 (fp16 hi plane + lo plane)
    float *power;            // [arrays][total_frames] linear FFTPower per frame, or NULL (ungated)
    int total_frames;
    // any-N kernels only (kernels_generic.hip)
    int N, logH, kg, ula;    // frame length, log2(N/2), K-slots per delay group (= N/2 + 1), delay-group merging on/off
    const float2 *tw;        // [N/2] exp(-j 2 pi i / N)
    // list mode (k_stft_phat only; the repair pass of the adaptive SRP precision): workgroup b takes the REPAIR_GROUP frames of
    // list[list0 + b] = array * groups_per_array + group and writes A rows b * REPAIR_GROUP ...; b >= *n_list - list0 exits
    const int *list; const int *n_list; int list0, list_cap, groups_per_array;   // list_cap: groups of this pass at most
    // lazy tails (see HIST_FRAMES): the coarse launch keeps the call's last HIST_FRAMES frames of PCM in hist_out [arrays][M][HIST_SAMPLES];
    // the list-mode launch of the NEXT call reads the units >= hist_base from hist_in (the same layout)
    float *hist_out; const float *hist_in; int hist_base;
    const unsigned short *mrank; int n_merged;   // k_stft_phat_wave, merged index (ULA, one fp16 plane): rank of the product m = k (j - i)
                             // among the n_merged distinct ones, [(M - 1) * 512 + 1]; NULL: per-group index g * 513 + k
    int planar;              // merged rows of a context that folds about broadside (fold_table.h): row[r] = Re S[r], row[Kp_m / 2 + r] = Im S[r] instead of interleaved
    int no_phat;             // 1: gcc_weighting NONE -- the pair products of the spectra themselves (k_stft_phat_wave, fp32 rows only)
    int skew;                       // > 0 (round 5; a launch that is exactly one resident round of two workgroups per CU): grid (arrays, run groups),
                                    // and the run groups of the first half -- dispatched first: the OLDER workgroup of every CU, which the CU's
                                    // oldest-first issue favours (its waves were done at 180 us, the younger one's at 244: profiles/
                                    // r05_run_queue_negative.log) -- take fpb + skew frames per wave, the others fpb - skew, so that both finish
                                    // together (19 / 13 frames: 302 -> 281 us per 32 768 frames, profiles/r05_skew.log).  The rows do not
                                    // depend on which wave forms them: the same bits.
    unsigned char *dead;     // k_stft_phat_wave in the coarse pass of a candidate-column call, else NULL: [arrays][total_frames] 1 = every channel of the frame is
                             // exact zeros (digital silence): its row is zero in the coarse and in the exact map alike, the repair pass need not list it
    unsigned char *unsure;   // k_stft_phat_wave16 in the adaptive coarse pass, else NULL: [arrays][total_frames] 1 = a channel's DC or Nyquist bin of this
                             // frame is at the rounding level of the transform.  PHAT keeps only the SIGN of such a bin, and the exact rows of 16
                             // microphones come from another kernel (k_stft_phat<16>) that need not round it the same way: k_scan_pick repairs the
                             // frame and the six after it whatever the map says ("A limit of PHAT itself")
    // list mode of a candidate-column call: the workgroup that wrote a unit's four rows contracts them at the unit's columns (cand_unit.h)
    int cand_on; CandArgs cand;
    SteerArgs bf;            // k_stft_phat_wave<..., FUSE>
};

__device__ __forceinline__ void store_a(float *row, const StftPhatArgs &, int cidx, float2 v)
{
    reinterpret_cast<float2 *>(row)[cidx] = v;
}

typedef _Float16 half2_t __attribute__((ext_vector_type(2)));

typedef float float2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void store_a(_Float16 *row, const StftPhatArgs &p, int cidx, float2 v)
{
    // hi = fp16(v), lo = fp16(v - hi): vector conversions so that one packed convert serves both the store
    // of hi and the residual
    const float2_t vv = {v.x, v.y};
    const half2_t hi = __builtin_convertvector(vv, half2_t);
    reinterpret_cast<half2_t *>(row)[cidx] = hi;
    if (p.a_planes == 2) {
        const float2_t back = __builtin_convertvector(hi, float2_t);
        const half2_t lo = __builtin_convertvector(vv - back, half2_t);
        reinterpret_cast<half2_t *>(row + p.Kp)[cidx] = lo;
    }
}

constexpr int FOLD_NS = 4;      // LDS stages of k_srp_gemm_f16_fold (28 KiB each)

struct GemmArgs {
    const void *A;           // [rows][a_row_elems]
    const void *B;           // fp32: [Kp][Dp]; fp16: [planes][Dp][Kp] (k contiguous)
    float *C;                // [arrays][total_frames][Dp]
    int rows;                // arrays * chunk_frames
    int chunk_frames, total_frames, frame0;
    int Kp, Dp, a_row_elems;
    long long c_plane_elems;  // elements between the partial maps of a split-K launch
    const void *Bt;          // fp16 steering table tiled for the 256 x 384 kernel: [plane][Kp/32][Dp][32] (a K stage of all columns is contiguous)
    // device-side row count (repair pass): rows = min(rows, (*n_list - list0) * REPAIR_GROUP); workgroups beyond it exit
    const int *n_list; int list0;
    int repair_ksplit;       // K segments of k_srp_gemm_repair at most (shape-dependent, see REPAIR_KSPLIT_MAX)
    int repair_items;        // ... halved while the list gives more work items than this (repair_ksplit_eff; 0: never)
    // chunk-local scan result from the contraction's epilogue (256 x 384 kernel, one map, no gate, 32-row blocks = scan chunks):
    // part[arr][chunk][d] = sum_t scan_w[t] C[t][d] = the recursion E = 0.8f E + 0.2f C run from zero over the chunk's frames
    const void *Bf;          // k_srp_gemm_f16_fold: the even and the odd half-width table, [2][Kp / 64][192][32] fp16 (fold_table.h); D is set for it
    float *part; int *nvoiced; int D, n_chunks;
    long long part_plane_stride;   // a split-K launch leaves one set of results per K half (summed by k_scan_carry, half 0 first)
    float scan_w[32];
};

struct ScanPickArgs {
    const float *C;          // [c_planes][arrays][n_frames][Dp]: partial maps of a split-K contraction, summed here
    int c_planes; long long c_plane_stride;
    int n_frames, Dp, D, P, S, chunk, n_chunks;
    float mu, one_minus_mu;
    float inv_norm;          // correctly rounded 1 / (30 P): the normalisation (:155-156) divides by 30 P
    const float *state_in;   // [arrays][D]  E_prev at entry
    float *state_out;        // [arrays][D]  E_prev at exit
    float *part;             // [part_planes][arrays][n_chunks][D]  chunk-local recursion result (E from 0); 2 planes: the two K halves of the contraction
    int part_planes; long long part_plane_stride;
    int *nvoiced;            // [arrays][n_chunks]     voiced frames per chunk
    float *e_start;          // [arrays][n_chunks][D]  E at the start of every chunk
    const unsigned char *voiced;   // [arrays][n_frames] 1 = frame passed the power gate; NULL = ungated (all frames)
    const float *grid;       // [D] doaIdx2angle
    int *doa_bin; float *doa_rad; float *prob; float *energy;
    // adaptive SRP precision (fp16 coarse scan + exact repair of the frames whose pick is sensitive to the fp16 error)
    int mode;                // 0: plain; 1: coarse pass, flags the sensitive frames and plans their repair
    float tau;               // two normalised energies closer than this cannot be ordered from the coarse map
    unsigned char *flags;    // [arrays][n_frames] 1 = the frame's pick must be repeated on exact rows
    int groups_per_array;    // repair units (REPAIR_GROUP frames) per array
    int *need;               // [arrays * groups_per_array] test-and-set: the group is on the list (cleared by k_repair_patch)
    int *list;               // [arrays * groups_per_array] groups whose rows are recomputed, in order of arrival
    int *n_list;             // [1] their number (reset by k_scan_carry)
    int *chunk_from;         // [arrays][n_chunks] chunk the second pick of this chunk restarts from, >= n_chunks: no flagged frame (reset by k_scan_repick)
    int *clist; int *n_clist;     // [arrays * n_chunks], [2] (the second word counts the workgroups of k_scan_repick that are done: the last one empties both lists): the chunks that hold a flagged frame, in order of arrival (k_scan_repick walks them; reset by k_scan_carry)
    int lookback;                 // > 0 (ungated calls): no k_scan_carry -- k_scan_pick composes the start value of its chunk from the chunk-local
                                  // results of the `lookback` chunks before it (0.8^32 per chunk: the fifth chunk back is 3e-16 of it) and stores it
    unsigned long long *probe;    // host-mapped [3] or NULL: k_scan_repick leaves stats[0], stats[1] and probe_seq there (api.hip: adapt_policy_begin)
    unsigned long long probe_seq;
    int *last_vchunk;        // [arrays] chunk of the array's last frame that advanced the recursion, -1 = none (k_scan_carry)
    unsigned long long *stats;    // [4] running totals: flagged frames, listed groups, candidate columns of the flagged frames, flagged frames that took every column
    const unsigned char *dead;    // [arrays][n_frames] or NULL: frames of exact zeros (StftPhatArgs::dead): their rows are not listed
    const unsigned char *unsure;  // [arrays][n_frames] or NULL: frames the coarse analysis could not vouch for (StftPhatArgs::unsure): flagged with their six successors
    // lazy tails (see HIST_FRAMES).  lazy: the call's last frame is not flagged for the state's sake; k_scan_pick leaves the coarse rows of
    // the last HIST_FRAMES frames in hist_C_out [arrays][HIST_FRAMES][Dp] and the energies in front of them in e_hist_out [arrays][D].
    // hist_valid: the previous call did so (hist_C_in, e_hist_in): a flagged frame t < REPAIR_WARM lists the history units its rows
    // t - REPAIR_WARM .. -1 live in (numbered from hist_base), and k_scan_repick starts chunk 0 from e_hist_in over the history rows
    // (chunk_from = -1).
    int lazy, hist_valid, hist_base;
    float *hist_C_out, *e_hist_out;
    const float *hist_C_in, *e_hist_in;
    // candidate columns (round 5): per repair unit the delays its rows are needed at, one bit per column, umask_words = Dp / 32 words
    // per unit (k_scan_pick ORs a flagged frame's candidate columns into every unit it lists; cand_unit -- one workgroup per unit -- takes
    // and clears them and releases the unit's test-and-set word).  NULL: whole rows (k_srp_gemm_repair + k_repair_patch).
    unsigned *umask; int umask_words;
    // steered tail: the frames whose final pick is not the predicted bin are patched inside the second-pick launch.  k_scan_pick<PL, 1>
    // appends the misses of a chunk WITHOUT a flagged frame (its coarse picks are final; one batch per chunk: SCAN_SUB == SCAN_CHUNK) to
    // the miss list n_miss[1 ...] (entry = array * n_frames + frame, each frame at most once; n_miss[0] is its length, miss_cap its
    // room: a call's frames, and the list is empty when a call starts).  The last STEER_TAIL_WGS workgroups of k_scan_repick<PL, true>
    // stride over the list, patch and count; the workgroup that owns a chunk WITH a flagged frame patches and counts that chunk's misses
    // itself once its final picks are out.  NULL unless the call is an ADAPTIVE one whose analysis steered ahead (api.hip,
    // localise_impl); *n_miss is reset by k_steer_synth, which runs behind every reader.
    int *n_miss; int miss_cap;
    SteerPatchArgs sp;       // what steer_patch_frame reads, and pred / miss (all = 0, the whole call in Y)
};

// The repair contraction runs on however many rows the coarse pass listed (a device-side count): the K range is what
// parallelises.  It is cut into a number of segments that depends on the SHAPE of the call only (api.hip, repair_ksplit_for:
// 32 for a few arrays, 8 when the always-recomputed tails of many arrays make thousands of rows), never on how many rows were
// listed, so that an exact row's value does not depend on what was listed with it (a call worked off in chunks returns the
// same bits).  Partial maps: [ksplit][repair_plane_stride], summed in order by k_repair_patch.
constexpr int REPAIR_KSPLIT_MAX = 32;
__host__ __device__ inline long long repair_plane_stride(int n_rows, int Dp) { return (long long)((n_rows + 127) / 128 * 128) * Dp; }
__host__ __device__ inline long long repair_cx_rows(long long pass_rows, int ksplit) { return ((pass_rows + 127) / 128 * 128) * ksplit; }
// K segments the repair contraction really uses for n_rows listed rows: the call's shape gives the most (repair_ksplit_for: enough to
// fill the chip when only the tails are listed); a long list has the work items without cutting K that fine, and every halving
// halves the partial maps that are written and read back -- halved until at most items_max items (row tile, column tile, segment)
// are left.  The row count is the device's, so k_srp_gemm_repair and k_repair_patch both work it out from it.  (The exact rows' last
// bits then depend on how many rows a call lists -- as they already do on the call's shape; tie-level)
__host__ __device__ inline int repair_ksplit_eff(int ksplit, int n_rows, int Dp, int items_max)
{
    if (items_max <= 0) return ksplit;
    const int tiles = ((n_rows + 127) / 128) * (Dp == 64 ? 1 : Dp / 192);
    int k = ksplit;
    while (k > 4 && tiles * k > items_max) k >>= 1;
    return k;
}

struct RepairPatchArgs {
    const float *Cx;         // [repair_ksplit][repair_plane_stride] exact rows, split-K partial maps
    int pass_rows, col_tiles, ksplit, items;     // (ksplit, items: as GemmArgs::repair_ksplit, repair_items)
    const int *list; const int *n_list; int list0, groups_per_array;
    int *need;               // the groups' test-and-set words, released here
    float *C;                // [c_planes][arrays][n_frames][Dp]: plane 0 takes the exact row, the others zeros
    int c_planes; long long c_plane_stride;
    int n_frames, Dp;
    float *hist_C; int hist_base;   // lazy tails: the rows of the units >= hist_base go to hist_C [arrays][HIST_FRAMES][Dp] (one plane)
};

struct GateArgs {
    const float *power_lin;  // [arrays][n_frames] FFTPower of every frame
    int n_frames, fft_n, needed_samples;
    float margin_db;
    double eps;              // added to every frame's power before it is accumulated (FreqGCC: 1e-10, BinauralLocalisation.cpp:391)
    // persistent gate state per array: {accumulated power (double), samples consumed (double), floor dB (double), estimated (double 0/1)}
    double *state;           // [arrays][4]
    unsigned char *voiced;   // [arrays][n_frames]
    float *power_out;        // [arrays][n_frames] value handed to setDOA / compared with the floor (may be NULL)
    int *post0;              // [arrays] first frame of this call at which the floor estimate exists (the frame that completes it
                             // counts; 0 if it existed before the call, n_frames if it still does not); may be NULL
};

struct DoaFillArgs {
    const unsigned char *voiced;   // [arrays][n_frames]
    int n_frames, S;
    int *doa_bin; float *doa_rad; float *prob;      // [arrays][n_frames][S], filled forward over gated-out frames
    int *last_bin; float *last_rad; float *last_prob;   // [arrays][S] _currentDOA / _prob carried between calls
};

struct BeamformArgs {
    const float *pcm;
    long long array_stride, mic_stride;
    int M, Mpad, S, n_frames, ft, fs;
    int nb;                  // frames per inverse-FFT batch (<= BF_NB; fewer with several sources so that two workgroups still share a CU)
    const float *window;
    const double *mic_x;     // [M] x coordinate (Beamformer.cpp:59 steers with x only)
    const float *doa_rad;    // [arrays][n_frames][S]
    float *out;              // [arrays][S][n_frames*hop]
    const float *tail_in;    // [arrays][S][hop] overlap-add carry at entry
    float *tail_out;         // at exit
    // any-N kernel only (kernels_generic.hip)
    int N, logH;
    const float2 *tw;        // [N/2] exp(-j 2 pi i / N)
    int S_all, s0;           // ... which takes the sources s0 ... s0 + S - 1 of S_all per launch (all at once while M + S spectra fit the LDS)
};

// wave-per-run delay-and-sum on the 1024-point complex transform (kernels_wave.hip): one source, any M <= 16
struct BeamformWaveArgs {
    const float *pcm;
    long long array_stride, mic_stride;
    int M, n_pairs, n_frames, ft, S;   // S sources: blockIdx.z, each steered by its own column of doa_bin
    const float *window;     // [1024] periodic Hann
    const int *doa_bin;      // [arrays][n_frames][S] grid index of the frame's DOA, -1: the initial _currentDOA = 0
    const float2 *table;     // [D + 1][n_pairs][1024] (P_a - j P_b) / (M N) per steering angle (k_bf_table)
    float *out;              // [arrays][S][n_frames*hop]
    const float *tail_in;    // [arrays][S][hop] overlap-add carry at entry
    float *tail_out;         // at exit
    int skew;                // k_beamform_wave with the hand-off, > 0 (round 5, as StftPhatArgs::skew): grid (arrays, workgroups, sources); the first half
                             // of an array's workgroups -- dispatched first, the older workgroup of every CU -- run ft + skew frames per wave, the others ft - skew
};

struct Gcc2ScanArgs {
    const float *C;          // [c_planes][arrays][n_frames][Dp] un-smoothed GCC-PHAT R_t[d] (split-K partial maps, summed here)
    int c_planes; long long c_plane_stride;
    int n_frames, Dp, D, chunk;
    const long long *vdone_in; long long *vdone_out;   // [arrays] voiced frames processed before / after this call (0 = the stream's first)
    const int *vidx;         // [arrays][n_frames] frames that passed the gate, in order (NULL: ungated, every frame)
    const int *nv;           // [arrays] their number (NULL: n_frames)
    const unsigned char *vreset;   // [arrays][n_frames] per fired frame: 1 = both memory factors are zero at this frame (the
                             // silence rule, BinauralLocalisation.cpp:530-560); NULL (ungated): only the stream's first frame
    float mu, one_minus_mu;  // _maxCorrMemoryFactor 0.8f and 1 - 0.8f (float arithmetic)
    float doa_mem, one_minus_doa_mem;   // _maxDoaMemoryFactor 0.6f
    float step;              // _doaStep
    const float *corr_in; float *corr_out;      // [arrays][D] _prevCorrelationsReal
    const float *doa_in; float *doa_out;        // [arrays] _currentDOA
    const float *grid;       // [D]
    int *argmax; float *doa_rad; float *prob; float *corr;
};

struct Gcc2FillArgs {
    const unsigned char *voiced;   // [arrays][n_frames]
    int n_frames, D;
    int *argmax; float *doa_rad, *prob, *corr;          // outputs of the scan (corr may be NULL); gated-out frames are filled here
    const float *corr_state;       // [arrays][D] smoothed correlation at the start of the call
    int *last_idx; float *last_rad, *last_prob;          // [arrays] values of the last frame, carried to the next call
};

// k_gcc2_track (kernels_gcc2_track.hip): the particle-filter DOA tracker, one wave per array, the frames of the call in order
constexpr int GCC2_TRACK_WAVES = 2;            // arrays per workgroup
constexpr int GCC2_TRACK_MAX_PARTICLES = 1024;
struct Gcc2TrackArgs {
    const void *corr;              // [arrays][n_frames][D] smoothed rows of the frames that fired (TC)
    const void *corr_state;        // [arrays][D] the row before the call (TC)
    const int *argmax;             // [arrays][n_frames] first-max argmax of the frames that fired
    const unsigned char *voiced;   // [arrays][n_frames]; NULL: every frame fired
    const int *post0, *sil_in;     // [arrays] with `voiced`: first frame with a known floor, _silenceFramesCounter before the call
    int windows_to_decay;
    int n_arrays, n_frames, D;
    float step; const float *grid;
    int N, n_inject; unsigned long long seed; double sigma_init, sigma_step;
    long long key_a;               // >= 0: the array index that enters the key (the frame hook's 0xFFFFFFFF); < 0: the array's own
    int state0;                    // state slot of array 0 of this launch
    double *x;                     // [slots][N] particles
    double *sd;                    // [slots][2] DOA, prob
    int *si;                       // [slots][4] alive, track, upd, -
    void *doa_out, *prob_out;      // [arrays][n_frames] (TC); prob_out may be NULL
    unsigned char *fired; int *track;   // [arrays][n_frames], may be NULL
    // the frame hook (one array, one frame): the host knows the gate's decision and the counter
    int one_kind;                  // < 0: not used; 0 nothing happens, 1 the frame fired, 2 gated out with a known floor
    int one_sil, one_argmax;
    unsigned slice_bytes;          // LDS per wave
};

struct MaskParams {
    float thr[45];
    int lo[45], hi[45];       // support of band b (bins with H_b > 0), lo > hi for an empty band
    int kb[513];              // first band covering bin k (the second one is kb+1), -1 if none
    float kw0[513], kw1[513]; // H_kb[k], H_{kb+1}[k]
    float lambda, one_minus_lambda, reject, rho;
    int method, alg;
};

struct MaskArgs {
    const float *pcm;
    long long stream_stride, ch_stride;
    int n_frames, ft;
    long long frames_done;
    const float *window;
    const MaskParams *mp;
    const float *Q_in; float *Q_out; float *noise;      // [streams][45]
    const float *tail_in; float *tail_out;              // [streams][2][512]
    float *out; int *decisions;
};

// any-length variant: the per-bin band tables live in global memory (length K = N/2 + 1)
struct MaskGenArgs {
    MaskArgs a;
    int N, logH;
    const float2 *tw;         // [N/2]
    const float2 *kw;         // [K] (H_kb[k], H_{kb+1}[k])
    const int *kb;            // [K] first band covering bin k, -1 if none
};

struct MaskFrameArgs {
    const double *L, *R;      // [K] complex (CCS)
    double *outL, *outR;      // [K] complex, zeroed by the caller
    const double *H;          // [45][K] filter magnitudes
    const double *thr;        // [45]
    double *Q, *noise;        // [45] state
    int K, method, alg, first_call;
    double lambda, one_minus_lambda, reject, rho;
    int *decisions;
};

// ---- MultibandBinarualLocalisation (kernels_multiband.hip) ----
struct MbAnalyseArgs {
    const float *pcm;
    long long array_stride, ch_stride;
    int n_frames, N, logH, nbins, D;
    const float *window;
    const float2 *tw;         // [N/2]
    const float *coef;        // [nbins][K] filter magnitudes (0 outside the support)
    const int *lo, *hi;       // [nbins] support of band b (bins with H_b > 0, inclusive), lo > hi if empty
    const float2 *T;          // [K][D] exp(+j 2 pi k tau_d / N)
    float *raw;               // [arrays][n_frames][nbins * D] un-smoothed band correlations
    float *band_energy;       // [arrays][n_frames][nbins] FFTPower of the sub-band frames
    float *p_full, *p_half;   // [arrays][n_frames] FFTPower(frames, N+2) and FFTPower(frames, (N+2)/2)
};

struct MbScanArgs {
    const float *raw, *band_energy;
    int n_frames, nbins, D, chunk;
    float mem, one_minus_mem;               // _corrMemoryFactor 0.4f and 1 - 0.4f (float arithmetic)
    const float *corr_in; float *corr_out;  // [arrays][nbins * D] _prevCorrelationsReal
    int *hist_idx; float *hist_prob;        // [arrays][n_frames] argmax of _energyInDOA and its share
    int *band_idx; float *energy_in_doa; float *band_corr;   // optional outputs
};

struct MbSummaryArgs {
    const float *p_full, *p_half;
    const int *hist_idx; const float *hist_prob;
    int n_frames, K, needed_samples, use_floor;
    float margin_db;
    const float *grid;        // [D]
    double *gate;             // [arrays][4] {_powerFloor, _samplesConsumedForNoise, floor dB, _noiseEstimated}
    float *cur;               // [arrays][2] {_currentDOA[0], _prob[0]}
    float *doa_rad, *prob, *power; unsigned char *voiced;   // [arrays][n_frames]
};

// ---- MVDR-style beamformer with a per-bin spatial covariance (BASELINE configs[3]) ----
// The geometry of a context (mca_hip_mvdr_set_geometry).  xyz == 0: the steering of Beamformer.cpp:59, x only, and
// nothing else here is read.  xyz == 1: the table entry kk of microphone m has turns = kk * mvdr_projection(...), the negated
// projection of unit * r_m on e(theta, eps) = (sin theta cos eps, cos theta cos eps, sin eps), in double.
struct MvdrGeometry {
    int xyz;
    const double *u;          // [3][M]: unit * x_m, unit * y_m, unit * z_m (products formed on the host, in double)
    double ce, se;            // cos eps, sin eps of the context: the tracks and the spectrum
    // (cos eps, sin eps) per stream and look-direction slot, stride MCA_MAX_SOURCES (mca_hip_mvdr_set_elevations_*): what the steering
    // tables of the frames calls read in place of ce, se.  A slot that is unset holds the context's pair, bit for bit
    const double2 *slot_el;
};
// cd = cos((double)theta + pi/2), the x term's spelling in both modes; cy = -cos((double)theta).  A coordinate that is 0 adds no
// term at all, so an array on the x axis with eps = 0 (ce = 1) gives (unit x_m) * cd: the bytes of the x-only arm, signed zeros included
__device__ __forceinline__ double mvdr_projection(const MvdrGeometry &g, int M, int m, double cd, double cy, double ce, double se)
{
    const double ux = g.u[m], uy = g.u[M + m], uz = g.u[2 * M + m];
    double pr = ux * (cd * ce);
    if (uy != 0.0) pr += uy * (cy * ce);
    if (uz != 0.0) pr -= uz * se;
    return pr;
}
__device__ __forceinline__ double mvdr_projection(const MvdrGeometry &g, int M, int m, double cd, double cy)
{
    return mvdr_projection(g, M, m, cd, cy, g.ce, g.se);
}
// k_mvdr_elevations: the pairs of MvdrGeometry::slot_el from angles on the device (mca_hip_mvdr_set_elevations_dev)
struct MvdrElevationsArgs {
    const float *elev;        // [streams][max_sources] radians; NaN: the context's elevation
    double2 *slot_el;         // [streams][MCA_MAX_SOURCES]
    float *slot_val;          // [streams][MCA_MAX_SOURCES] what mca_hip_mvdr_get_elevations reports: NaN, or the clamped angle
    int n, max_sources;       // n = streams * max_sources
    double ce, se;            // the context's pair
};

// Angles on the circle (XYZ mode; the normative text is include/mcarray_hip.h, mca_hip_mvdr_set_geometry).  All float32, every step one
// rounded operation or an explicit fmaf, so that contraction cannot change a bit.
constexpr float MVDR_PI_F = 3.14159274f, MVDR_TWO_PI_F = 6.28318548f, MVDR_INV_TWO_PI_F = 0.159154937f;
// the shorter way round of a difference of two reduced angles (|d| <= 2 pi)
__device__ __forceinline__ float mvdr_wrap(float d)
{
    if (d > MVDR_PI_F) d = d - MVDR_TWO_PI_F;
    else if (d < -MVDR_PI_F) d = d + MVDR_TWO_PI_F;
    return d;
}
// any finite angle into [-pi_f, pi_f]
__device__ __forceinline__ float mvdr_reduce(float v)
{
    const float n = rintf(v * MVDR_INV_TWO_PI_F);
    const float r = mvdr_wrap(fmaf(-MVDR_TWO_PI_F, n, v));
    return fminf(fmaxf(r, -MVDR_PI_F), MVDR_PI_F);          // (only an angle beyond ~1e7 rad, whose float has no fraction left, gets here outside)
}

struct MvdrAnalyseArgs {
    const float *pcm;
    long long stream_stride, mic_stride;
    int n_frames, N, logH, M;
    int S;                    // look directions per frame (1 ... MCA_MAX_SOURCES)
    const float *window;
    const float2 *tw;         // [N/2]
    const float *doa_rad;     // [streams][n_frames][S]
    float2 *X;                // [streams][n_frames][K][M] one-sided spectra, microphone fastest
    // steering phasors of every (stream, frame, microphone), factored: d_m[k] = T[k >> 5] * T[nhi + (k & 31)] with
    // T[i < nhi] = exp(-j 2 pi 32 i u), T[nhi + i] = exp(-j 2 pi i u), u = fs/N/c x_m cos(DOA + pi/2) (Beamformer.cpp:59);
    // the phase is reduced in double.  N/64 + 33 sincos per microphone and frame instead of N/2 + 1.
    float2 *T;                // [streams][n_frames][S][M][nhi + 32], nhi = N/64 + 1
    const double *mic_x;      // [M]
    double unit;              // fs / N / 346.1
    MvdrGeometry geo;
};

struct MvdrSolveArgs {
    // A launch covers the problems pid0 .. pid0 + n_prob - 1 (problem = stream * K + bin), `pieces` workgroups per 64 problems:
    // piece j solves the frames [j F / pieces, (j + 1) F / pieces) after running the covariance recursion alone -- the same
    // operations in the same order, so the same bits -- over the frames before them; the last piece stores the state.
    long long pid0, n_prob;
    int pieces;
    const float2 *X;          // [streams][n_frames][K][M]
    const float2 *T;          // [streams][n_frames][S][M][nhi + 32] factored steering phasors (MvdrAnalyseArgs)
    int n_streams, n_frames, K, M;
    float alpha, one_minus_alpha, loading_over_m;
    float2 *phi;              // [streams][K][M(M+1)/2] lower triangle of the covariance, row-major (state at entry)
    float *trace;             // [streams][K] tr(Phi), carried as its own recursion
    // state at exit: problem pid goes to phi_out[(pid - out_base) tri], trace_out[pid - out_base].  The same buffers for an unsplit
    // launch (every problem is read and written by one workgroup); a launch cut into pieces writes to a scratch copy, because
    // every piece reads the entry state when it starts and nothing orders that before the last piece's stores
    float2 *phi_out; float *trace_out; long long out_base;
    float2 *Y;                // [streams][S][n_frames][K] beamformed spectra
    int S;                    // look directions per frame
    // what only some instantiations of k_mvdr_solve_t read (a kernel loads the fields it uses, no others)
    const float *update;      // WEIGHT = FRAME: [streams][n_frames]; CELL: [streams][n_frames][K]; NONE: not read
    float null_gain;          // NULLS: > 0, gain of the soft nulls at the other look directions
    float *pn;                // NOISE: [streams][S][n_frames][K] fp32, 1 / (d_s^H PhiL^-1 d_s) of every output, 0 = silent
    // k_mvdr_solve_rtf_t: [streams][S][n_loop][K][M] steering vectors (MvdrRtfArgs::D), T is not read; the launch walks n_loop frames of
    // a call of n_frames (a call whose plane exceeds the workspace cap is cut along the frames: X, update, Y and pn then point at the
    // chunk's first frame and keep n_frames as their stride)
    const float2 *D; int n_loop;
};

// k_mvdr_rtf<Q> (kernels_mvdr_rtf.hip): the target covariances Psi and the steering vectors estimated from them,
// between the analysis and the solve.  One quad per (stream, slot, bin), the layout of the solve.
struct MvdrRtfArgs {
    const float2 *X;          // [streams][n_frames][K][M]
    const float2 *T;          // [streams][n_frames][S][M][nhi + 32] (MvdrAnalyseArgs): the geometric vectors, start and fallback
    const float *update;      // [streams][n_frames][K] update mask of the noise covariance, or NULL (all 1)
    const float *tmask;       // [streams][S][n_frames][K] target masks, or NULL (all 0)
    int n_streams, n_frames, K, M;
    int n_loop;               // frames this launch walks (<= n_frames: X, T and the masks point at the chunk's first frame, stride n_frames)
    int S, slots;             // look directions of the call; slots per stream in the context (>= S)
    float alpha, one_minus_alpha;             // of the noise covariance (MvdrSolveArgs)
    float talpha, one_minus_talpha;           // of the target covariance
    float min_share;
    int iterations, ref_mic;
    const float2 *phi;        // [streams][K][tri] noise covariance at entry (read only: the solve behind this kernel advances it)
    const float *trace;       // [streams][K]
    float2 *psi;              // [streams][slots][K][tri] target covariances, read and written
    float *cpsi;              // [streams][slots][K] sum of the weights in Psi
    const float *cphi_in;     // [streams][K] sum of the weights in Phi at entry; every slot's quad reads it, so the exit value goes to
    float *cphi_out;          // a second buffer (slot 0 writes it) and the host swaps the two
    float2 *D;                // [streams][S][n_loop][K][M]
};
// k_mvdr_rtf_steering<Q>: the estimator alone on the held state of one stream and slot (mca_hip_mvdr_get_steering)
struct MvdrRtfSteerArgs {
    const float2 *phi, *psi;  // [K][tri] of the stream, of the stream and slot
    const float *cpsi, *cphi; // [K]
    const float2 *T;          // [M][nhi + 32] factored phasors of the look direction
    int K, M;
    float min_share;
    int iterations, ref_mic;
    float2 *out;              // [K][M]
    unsigned char *estimated; // [K]
};

// k_mvdr_estmask<Q> (kernels_mvdr_estmask.hip): the update mask and the target masks of a call from its own spectra,
// between the analysis and k_mvdr_rtf / the solve.  One quad per (stream, frame, bin) cell, the layout of the solve; stateless.
struct MvdrEstmaskArgs {
    const float2 *X;          // [streams][n_frames][K][M]
    const float2 *T;          // [streams][n_frames][S][M][nhi + 32] (MvdrAnalyseArgs): the geometric vectors
    int n_streams, n_frames, K, M, S;
    int bin_lo, bin_hi;       // the band, both ends included; outside it target 0 and update 1
    int n_protected;          // P (>= 1): the look directions s < P close the update mask where they win
    float coherence_lo, coherence_span;       // v = clamp((c_w - lo) / span), span = hi - lo formed in double
    float *update;            // [streams][n_frames][K]
    float *target;            // [streams][S][n_frames][K], or NULL: not stored
};

// ---- the instantiations of the MVDR solve (mvdr_solve.h) ----
// k_mvdr_solve_t<Q, FULL, S, S1, PF, NULLS, REUSE, WEIGHT, NOISE>: Q row slots per lane, FULL: M == 4 Q, S look directions per frame,
// NULLS: soft nulls at the other directions (4.3), WEIGHT: the covariance update weight of a frame (4.5, 4.7), NOISE: the noise plane
// of the post-filter beside Y (4.6).  A call fixes these six; mvdr_solve_form() adds the three that only say how the kernel is built.
enum class MvdrWeight { NONE, FRAME, CELL };   // no weight (all 1) / update[streams][n_frames] / update_mask[streams][n_frames][K]
struct MvdrSolveForm {
    int S1;        // look directions per pass of the factorisation's column loop (S1 < S: several passes, each repeats the factorisation)
    bool PF;       // the next frame's spectra are loaded a frame ahead
    bool REUSE;    // a frame with weight 0 behind a solved one runs the substitutions against the held factor only
};
// Every choice is by what leaves the kernel without scratch under __launch_bounds__(256, 2) (tools/check_spills.py holds the build to it).
constexpr MvdrSolveForm mvdr_solve_form(int Q, bool FULL, int S, bool NULLS, MvdrWeight WEIGHT, bool NOISE)
{
    const bool big = Q == 4 && S >= 3;             // 13 ... 16 microphones with three or four directions: the rows a register or two short
    MvdrSolveForm f{S, true, false};
    // four directions on four row slots do not fit in one pass: two passes of two, the second repeating the factorisation
    if (Q == 4 && S == 4) f.S1 = 2;
    // the load a frame ahead costs 2 Q registers.  Given up by the two-pass nulls kernel; by the two NOISE rows that spill 12 bytes
    // per lane with the store of the noise plane (M = 13 ... 15, three and four directions, per-frame weights: 250 VGPRs without it;
    // one direction per pass is clean too, but repeats the factorisation per direction); and by every CELL row of that size, where
    // the cell's 64-bit address would otherwise cost scratch
    if (NULLS && Q == 4 && S == 4) f.PF = false;
    if (WEIGHT == MvdrWeight::FRAME && NOISE && !NULLS && !FULL && big) f.PF = false;
    if (WEIGHT == MvdrWeight::CELL && big) f.PF = false;
    // REUSE keeps the inverse pivots (Q registers) and a second column body.  Per-frame weights only: without weights no frame is
    // frozen, and with a weight per quad the rows of three and four row slots spill up to 158 registers and a mixed wave would run
    // both column bodies.  Off where it spills: four row slots with several directions, and the nulls of three row slots with four
    if (WEIGHT == MvdrWeight::FRAME) f.REUSE = NULLS ? !(Q == 4 || (Q == 3 && S == 4)) : !(Q == 4 && S >= 2);
    return f;
}
// The single-look call without weights keeps the hand-written k_mvdr_solve<Q, FULL> (kernels_mvdr.hip; DESIGN.md 4.2 on the
// measurement that decided it); every other call takes an instantiation of the template.
constexpr bool mvdr_solve_hand_written(int S, MvdrWeight WEIGHT, bool NOISE) { return S == 1 && WEIGHT == MvdrWeight::NONE && !NOISE; }
// the (Q, FULL, S, NULLS) a build instantiates per (WEIGHT, NOISE): one instantiation serves M = 4Q and M < 4Q under the nulls (the
// branch-free M = 4Q form costs that kernel registers, it saves none); the noise plane comes with weights (a call without them
// passes ones)
constexpr bool mvdr_solve_row(int Q, bool FULL, int S, bool NULLS, MvdrWeight WEIGHT, bool NOISE)
{
    return Q >= 1 && Q <= 4 && S >= 1 && S <= MCA_MAX_SOURCES && (!NULLS || (S >= 2 && !FULL)) && !(NOISE && WEIGHT == MvdrWeight::NONE) &&
           !mvdr_solve_hand_written(S, WEIGHT, NOISE);
}
// dynamic LDS of a NULLS workgroup: the parked u [Q][S][256] float2 and, with several passes, num / den [S][256]
inline int mvdr_nulls_lds_bytes(int Q, int S, int S1) { return 256 * (8 * Q * S + (S1 < S ? 12 * S : 0)); }


// the decision-directed Wiener post-filter on the beamformed spectra (kernels_mvdr_postfilter.hip): one thread per
// (stream, slot, bin), bins fastest; Y is rewritten in place, A is read and written once
struct MvdrPostfilterArgs {
    float2 *Y;                // [streams][S][n_frames][K] output of the solve, replaced by Z = G Y
    const float *pn;          // [streams][S][n_frames][K] 1 / (d^H PhiL^-1 d), 0 = silent (MvdrSolveArgs::pn)
    float *A;                 // [streams][slots][K] |Z|^2 of the frame before
    int n_streams, S, slots, n_frames, K;
    float smoothing, one_minus_smoothing, gain_floor, noise_scale;
};

// k_mvdr_spectrum<Q> / k_mvdr_spectrum_pick (kernels_mvdr_spectrum.hip): the Capon spatial spectrum of the covariance a
// context holds, P[i] = sum_k w[k] / (d(theta_i,k)^H PhiL[k]^-1 d(theta_i,k)).  A workgroup takes one stream and one chunk of
// MVDR_SPEC_CHUNK consecutive bins (chunk c = bins 64 c ... 64 c + 63, cut to the band); its four waves leave one partial sum per
// angle each, and the pick kernel adds the partial sums of a stream in (chunk, wave) order and selects the peaks.
constexpr int MVDR_SPEC_CHUNK = 64;
constexpr int MVDR_SPEC_MAX_ANGLES = 361;
struct MvdrSpectrumArgs {
    const float2 *phi;        // [streams][K][M(M+1)/2] (read only)
    const float *trace;       // [streams][K] (read only)
    // factored steering phasors of the grid, angle fastest: d_m(theta_i, k) = T[(m nph + (k >> 5)) Dpad + i] * T[(m nph + nhi + (k & 31)) Dpad + i]
    // (the factors of MvdrAnalyseArgs::T); the angles D ... Dpad - 1 repeat angle D - 1
    const float2 *T;
    float *part;              // [streams][n_chunks][4][Dpad] partial sums
    int K, M, D, Dpad, nph, nhi;
    int bin_lo, bin_hi, chunk0, n_chunks;
    int power;                // 1: w[k] = 1 (MCA_HIP_MVDR_SPECTRUM_POWER), 0: w[k] = M / tr[k]
    float loading;
};
struct MvdrSpectrumPickArgs {
    const float *part;        // [streams][n_slices][Dpad]
    const float *grid;        // [D] (float) theta_i
    int n_slices, D, Dpad, n_peaks;
    int circular;             // XYZ mode: the grid is periodic, the neighbours of i are (i - 1) mod D and (i + 1) mod D
    float *spectrum;          // [streams][D] or NULL
    float *peak_doa, *peak_val;   // [streams][n_peaks] or NULL
};

// k_mvdr_map_scan<Q> / k_mvdr_map_pick (kernels_mvdr_map.hip): the same quantity on a grid of azimuths x elevations,
// the directions as one flat list d = j n_az + i.  A workgroup takes one (stream, chunk of 64 bins, tile of MVDR_MAP_TILE directions):
// two directions per lane, the one register shape of the scan that k_mvdr_spectrum<Q> runs at two workgroups per CU.  The partial sums
// have the layout of MvdrSpectrumArgs::part, and the pick kernel adds them in the same (chunk, wave) order.
constexpr int MVDR_MAP_TILE = 128;
constexpr int MVDR_MAP_MAX_DIRS = 2048;
struct MvdrMapScanArgs {
    MvdrSpectrumArgs s;       // phi, trace and part of the first stream of the pass; T, D, Dpad of the flat list of directions
    int n_tiles;              // ceil(Dpad / MVDR_MAP_TILE)
    int n_streams;            // streams of the pass; blockIdx.x = (chunk n_tiles + tile) n_streams + stream, the stream fastest
};
struct MvdrMapPickArgs {
    const float *part;        // [streams][n_slices][Dpad]
    const float *az, *el;     // [n_az] (float) theta_i, [n_el] (float) eps_j
    int n_slices, n_az, n_el, Dpad, n_peaks;
    float ctx_el;             // (float) eps of the context: the elevation of every slot of a stream without a local maximum
    float *map;               // [streams][n_el][n_az] or NULL
    float *peak_az, *peak_el, *peak_val;   // [streams][n_peaks] or NULL
};

// ---- tracks of the look directions, updated on the device between chunks (kernels_mvdr_track.hip) ----
// per stream and slot, stride MCA_MAX_SOURCES whatever max_sources is (mca_hip_mvdr_set_max_sources moves nothing)
constexpr int MVDR_TRACK_MAX_CAND = 8;       // candidates an association call carries
struct MvdrTrackState {
    float *theta;             // [streams][MCA_MAX_SOURCES]
    int *alive, *miss, *gen;  // [streams][MCA_MAX_SOURCES]
};
// k_mvdr_track_tables: the factored phasors of theta of every own slot, with the operations of the analysis (MvdrAnalyseArgs::T)
struct MvdrTrackTablesArgs {
    const float *theta;       // [streams][MCA_MAX_SOURCES]
    float2 *T0;               // [streams][n_own][M][nhi + 32]
    const double *mic_x;      // [M]
    double unit;              // fs / N / 346.1
    int N, M, n_own;
    MvdrGeometry geo;
};
// k_mvdr_track_spectrum<Q>: T_s[i] = sum over the used bins of |d(theta_i,k)^H u_k|^2 / M, u the normalised estimated steering vector of
// own slot s.  A workgroup takes one (stream, own slot, chunk of MVDR_SPEC_CHUNK bins), the cut of k_mvdr_spectrum<Q>
struct MvdrTrackSpectrumArgs {
    const float2 *phi;        // [streams][K][tri] (read only)
    const float *trace;       // [streams][K]
    const float2 *psi;        // [streams][slots][K][tri]
    const float *cpsi;        // [streams][slots][K]
    const float *cphi;        // [streams][K]
    const float2 *T0;         // [streams][n_own][M][nph] (MvdrTrackTablesArgs)
    const float2 *T;          // the grid's phasors (MvdrSpectrumArgs::T)
    const int *alive;         // [streams][MCA_MAX_SOURCES]: a dead slot uses no bin
    float *part;              // [streams][n_own][n_chunks][4][Dpad] partial sums
    unsigned char *used;      // [streams][n_own][K] or NULL; the bins of an alive slot's chunks are written, the caller clears the rest
    int K, M, D, Dpad, nph, nhi;
    int bin_lo, bin_hi, chunk0, n_chunks;
    int n_own, slots;
    float min_share;
    int iterations, ref_mic;
};
// k_mvdr_track_pick: one workgroup per stream.  With part: the own spectra summed in (chunk, wave) order and their window argmax; then
// one lane runs the association (include/mcarray_hip.h) and the workgroup clears Psi and cpsi of the slots born
struct MvdrTrackPickArgs {
    MvdrTrackState st;
    const float *part;        // [streams][n_own][n_slices][Dpad], or NULL: own_doa is given
    const float *grid;        // [D]
    int n_slices, D, Dpad;
    float *own_spectrum;      // [streams][n_own][D] or NULL
    const float *own_doa;     // [streams][n_own] (part == NULL; may be NULL when n_own == 0)
    const float *cand_doa, *cand_val;   // [streams][n_cand]
    int n_cand, n_tracks, n_own, hold;
    float max_step, min_sep;
    float2 *psi;              // [streams][slots][K][tri], or NULL on a context without RTF
    float *cpsi;              // [streams][slots][K]
    int slots, K, tri;
    int circular;             // XYZ mode: angles live on the circle (mvdr_reduce, mvdr_wrap)
};
struct MvdrTrackFillArgs {
    MvdrTrackState st;
    float *doa_rad;           // [streams][n_frames][n_tracks]
    int n_streams, n_frames, n_tracks;
};
struct MvdrTrackSeedArgs {
    MvdrTrackState st;
    const float *doa;         // [streams][n_tracks], NaN: leave the slot
    int n_streams, n_tracks;
    int circular;             // XYZ mode: the seed is reduced to [-pi, pi]
};

// ---- tracks in azimuth and elevation, fed by the Capon map (kernels_mvdr_trk2.hip) ----
constexpr float MVDR_HALF_PI_F = 1.57079637f;            // (float) pi/2: the elevations of the tracks are clamped to +- this
struct MvdrTrk2State {
    float *theta, *eps;       // [streams][MCA_MAX_SOURCES]
    int *alive, *miss, *gen;  // [streams][MCA_MAX_SOURCES]
};
// k_mvdr_trk2_tables: MvdrTrackTablesArgs in XYZ geometry with the pair of eps_s in the place of the context's
struct MvdrTrk2TablesArgs {
    const float *theta, *eps; // [streams][MCA_MAX_SOURCES]
    const int *alive;
    float2 *T0;               // [streams][n_own][M][nhi + 32]
    int N, M, n_own;
    MvdrGeometry geo;
};
// k_mvdr_trk2_vectors<Q> and k_mvdr_trk2_scan: s as k_mvdr_track_spectrum<Q> takes it, with T, D and Dpad those of the map's flat list
// of directions; U and F carry the vectors from the one kernel to the other
struct MvdrTrk2ScanArgs {
    MvdrTrackSpectrumArgs s;
    float2 *U;                // [streams][n_own][n_chunks][64][M] u of the bin, zero where it is not used
    int *F;                   // [streams][n_own][n_chunks][64] used
    const float *az, *el;     // [n_az], [n_el]: the map's grid
    const float *theta, *eps; // [streams][MCA_MAX_SOURCES]: the centre of a slot's search window
    float max_step, max_step_el;
    int n_az, n_tiles;        // n_tiles = ceil(Dpad / MVDR_MAP_TILE)
    int n_streams;            // of the pass; blockIdx.x = ((chunk n_tiles + tile) n_own + slot) n_streams + stream, the stream fastest
    int skip;                 // the caller takes no map: a tile without a cell of the window is not scanned
};
// k_mvdr_trk2_pick: one workgroup per stream.  With part: the window argmax of every own slot; then the association in two angles
struct MvdrTrk2PickArgs {
    MvdrTrk2State st;
    const float *part;        // [streams][n_own][n_slices][Dpad], or NULL: own_az / own_el are given
    const float *az, *el;     // [n_az], [n_el]
    int n_az, n_el, n_slices, Dpad;
    float *own_map;           // [streams][n_own][n_el][n_az] or NULL
    const float *own_az, *own_el;             // [streams][n_own] (part == NULL; may be NULL when n_own == 0)
    const float *cand_az, *cand_el, *cand_val;   // [streams][n_cand]
    int n_cand, n_tracks, n_own, hold;
    float max_step, min_sep, max_step_el, min_sep_el;
    float2 *psi;              // [streams][slots][K][tri]
    float *cpsi;              // [streams][slots][K]
    int slots, K, tri;
};
struct MvdrTrk2FillArgs {
    MvdrTrk2State st;
    float *doa_rad;           // [streams][n_frames][n_tracks]
    int n_streams, n_frames, n_tracks;
    double2 *slot_el;         // [streams][MCA_MAX_SOURCES] (MvdrGeometry::slot_el)
    float *slot_val;          // [streams][MCA_MAX_SOURCES]
    double ce, se;            // the context's pair: a stream without an alive slot
};
struct MvdrTrk2SeedArgs {
    MvdrTrk2State st;
    const float *az, *el;     // [streams][n_tracks]; a slot with a value that is not finite is left
    int n_streams, n_tracks;
};

struct MvdrSynthArgs {
    const float2 *Y;          // [streams][S][n_frames][K]
    int n_frames, N, logH, ft;
    int S, tail_slots;        // outputs per stream in this call; tail slots per stream in the context (>= S)
    const float2 *tw;
    const float *tail_in; float *tail_out;   // [streams][tail_slots][N/2] overlap-add carry
    float *out;               // [streams][S][n_frames * N/2]
};

// ---- TemporalGCCBinauralLocalisation (kernels_tgcc.hip) ----
constexpr int TGCC_MAX_ND = 32;          // delay pairs the kernels support (4 nd - 1 <= 127 lags)
constexpr int TGCC_RPAD_FRONT = 64;      // zeros in front of channel 1 (lags down to -2 nd)
constexpr int TGCC_RPAD_BACK = 80;       // and behind its W rounded up to 8 (the last tile reads up to 2 nd + 13 past it)
constexpr int TGCC_RES = 6;              // per frame: DOA (deg), log-likelihood, pick, logPower, energy of W, of the floor's last part
constexpr int TGCC_STATE = 8;            // per array: _currentDOA, _prob, _powerFloor, samples consumed, _noiseEstimated, 3 spare
// doubles of LDS scratch in front of the staged channels: body sums [8][16], wave partials [4][16], totals [16],
// divisors [32], index [32], channel statistics [8], |c| [nd][2nd+1]; even, so that the channels behind it start 16-byte aligned
inline __host__ __device__ int tgcc_frame_ws_doubles(int nd) { return (8 * 16 + 4 * 16 + 16 + 2 * TGCC_MAX_ND + 8 + nd * (2 * nd + 1) + 1) & ~1; }

struct TgccFrameArgs {
    const float *pcm;
    long long array_stride, ch_stride;
    int n_frames, W, hop, nd, rem;  // rem = needed % W: the length of the floor estimation's last, partial frame
    double *res;                    // [arrays][n_frames][TGCC_RES]
    double *index;                  // [arrays][n_frames][nd] normalised index (may be NULL)
};

struct TgccGateArgs {
    const double *res;
    double *state;                  // [arrays][TGCC_STATE]
    int n_arrays, n_frames, W, needed, use_floor;
    float *doa_deg, *prob, *power;  // [arrays][n_frames], may be NULL
    unsigned char *voiced; int *delay_idx;
    double *out_f64;                // frame hook: [n_frames][5] {voiced, doa, prob, power, pick} (may be NULL)
};

}  // namespace mca
