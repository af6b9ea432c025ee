// api.hip -- the extern "C" layer of libmcarray_hip.so (see include/mcarray_hip.h).
// Host side only: validates arguments (every shape a kernel or its grid assumes is checked here
// before a launch), builds the tables the reference builds in its constructors, owns the
// per-context state and workspace, and enqueues the kernels.  No compute happens on the host
// and there is no CPU fallback: without a gfx950 device mca_hip_create fails.
#include "../../include/mcarray_hip.h"
#include "fft1024c.h"
#include "fold_table.h"
#include "host_common.h"
#include "kernels.h"
#include "knobs.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

using namespace mca;

namespace {

struct TimedEvent { int id; hipEvent_t a, b; };

}  // namespace

struct mca_hip_graph;

// ---- switches --------------------------------------------------------------------------------------------------------------
// Read ONCE, by mca_hip_create, into the context: nothing on a call path reads the environment.  The product switches are fields of
// mca_hip_config (adaptive_fallback, adaptive_min_rows, adaptive_max_sources, scan_carry) with an environment override for tests and
// tools that reach a context only through a wrapper.
// The back-off policy reads the report of an adaptive call at a FIXED lag: the eligible call FB_LAG calls after the one that enqueued
// it (and blocks on the page-locked word if it has not arrived: at a lag of two the work of the call in between is still queued
// behind it, so the device does not idle).  What a call does therefore depends on the sequence of calls and their content only, not
// on when a report happens to land: two runs of one stream return the same bits.
constexpr int FB_LAG = 2, FB_RING = 64, FB_WAIT_MS = 4000;
struct Knobs {
    bool fb_enabled = true;            // MCA_HIP_ADAPT_FALLBACK=0 / cfg.adaptive_fallback = OFF
    long long adapt_min_rows = 4096;   // MCA_HIP_ADAPT_MIN_ROWS / cfg.adaptive_min_rows
    int adapt_max_sources = 1;         // MCA_HIP_ADAPT_MAX_SOURCES / cfg.adaptive_max_sources
    double tau_scale = 1.0;            // MCA_HIP_ADAPT_TAU_SCALE (tools/adaptive_check.py: 1e9 turns the repair off to measure the coarse error)
    long long ws_max_bytes = 4LL << 30;   // MCA_HIP_WS_MAX_MB: A-operand workspace budget per slice of frames (tests force the sliced path)
    bool force_generic = false;        // MCA_HIP_FORCE_GENERIC: the any-length kernels at N = 1024 too (parity test of both)
    bool no_n2048 = false;             // MCA_HIP_NO_N2048: the any-length kernels at 2048-sample frames (parity of both paths)
    bool scan_carry = false;           // MCA_HIP_SCAN_CARRY / cfg.scan_carry
};      // (MCA_HIP_ADAPT_CAND and MCA_HIP_ADAPT_LAZY: StreamShape::cand, ::lazy_tails)

// Per-call workspace (everything a stream call allocates besides the per-array state, which lives in the context).  A call
// can be worked off in pieces over a sub-range of its arrays -- the chunks of the host-pointer path -- with the per-array
// state addressed at the call record's a0 (StreamCall).  Every buffer grows on its own need (grow_ws, the one place that reallocates)
// and its n is its capacity.  Buffers only: what a contraction left in d_C travels in the call record (MapResult).
struct Workspace {
    DevBuf<unsigned char> d_A;                        // A operand: [rows][a_row_elems], in bytes (the element is the precision's)
    DevBuf<unsigned char> d_Ax;                       // ADAPTIVE: the two-plane A rows (repair pass, FP16X3 calls)
    DevBuf<float> d_C;                                // correlation map
    DevBuf<float> d_Cx;                               // ADAPTIVE: partial maps of the repair contraction
    // exact chunked scan + power gate
    DevBuf<float> d_part, d_estart; DevBuf<int> d_nv;
    DevBuf<float> d_power, d_power_out; DevBuf<unsigned char> d_voiced;
    // ADAPTIVE: flags, repair list
    DevBuf<unsigned char> d_flags; DevBuf<int> d_list, d_need; DevBuf<unsigned> d_umask;
    DevBuf<int> d_chunk_from;                         // [2][chunks]: the first flagged frame per chunk, then the list of the chunks that hold one (at n / 2)
    DevBuf<unsigned char> d_unsure;                   // 16 microphones: frames whose DC / Nyquist bin the coarse analysis could not vouch for (StftPhatArgs::unsure)
    DevBuf<int> d_nlist, d_last_vchunk;
};

// FreqGCCBinauralLocalisation::processParametrisation (mca_hip_gcc2_process_frame): the scalars of BinauralLocalisation.cpp:320-404
// and :530-560, host side.  All of them are doubles (the ints, the bool and the float memory factors exactly) so that the blob part
// they make (mca_hip_state_save, version 3) is 8 doubles in this order.
struct G2FrameState {
    double power_floor = 0, samples = 0, noise_estimated = 0;   // _powerFloor, _samplesConsumedForNoise, _noiseEstimated
    double silence = 0;                                         // _silenceFramesCounter
    double corr_mem = 0, doa_mem = 0;                           // _corrMemoryFactor, _doaMemoryFactor (floats, :323-324)
    double doa = 0, prob = -1;                                  // _currentDOA, _prob (:339-340)
};

struct mca_hip_ctx : StreamShape {      // (the fixed shape every launch plan reads: stream_plan.h)
    mca_hip_config cfg{};
    std::vector<double> xyz;
    int logH = 0;
    std::string stream_why;       // why the stream API is unavailable for this configuration
    float step = 0.f;
    std::vector<float> delays, grid;
    std::vector<int2> pairs;
    // device tables
    DevBuf<float> d_window, d_grid, d_delays;
    DevBuf<float2> d_tw;          // [N/2] exp(-j 2 pi i / N), any-N kernels
    DevBuf<double> d_micx;
    DevBuf<int2> d_pairs;
    DevBuf<unsigned char> d_B, d_Bt;      // (in bytes: float or fp16 by the precision, like the merged and folded tables below)
    // the merged contraction index (StreamShape::merged, build_merged_tables)
    DevBuf<unsigned char> d_Bm, d_Btm; DevBuf<unsigned short> d_mrank;
    // ... folded about broadside (fold_table.h): the merged rows are planar ([R | I]), d_Bm / d_Btm hold the folded values at full width in
    // planar K order, and d_Bfold the even and the odd half-width tables of k_srp_gemm_f16_fold: [2][Kp_m / 64][192][32]
    DevBuf<unsigned char> d_Bfold;
    DevBuf<float2> d_bftab;                     // k_beamform_wave: steering rows per grid angle, [D + 1][bf_pairs][1024] (built on first use)
    // Delay-and-sum on the half spectrum (steer.h; steer_applies): the per-channel steering table, the predicted bin per array (the last pick of
    // the previous call; -1 on a new stream), the running miss total, the rows of Y (grown on demand) and two carries between frame passes
    DevBuf<float4> d_steer_rows; DevBuf<float2> d_steer_q; DevBuf<float> d_steer_nyq; DevBuf<int> d_steer_pred; DevBuf<unsigned long long> d_steer_miss;
    DevBuf<float2> d_steer_Y; DevBuf<float> d_steer_tail;
    DevBuf<int> d_steer_mlist;                              // the miss list of the patching second pick (ScanPickArgs::n_miss): [0] its length, then an entry per row of Y
    bool steer_mlist_dirty = false;                         // misses were listed by a call whose synthesis (which empties the list) has not been enqueued
    unsigned long long steer_frames_total = 0, steer_fused_calls = 0;
    // the guard of that path (steer_policy_begin): a call steers ahead of its picks unless the report of the call FB_LAG calls before it -- its
    // frames whose pick was not the predicted bin, through page-locked memory, consumed at that fixed lag like the AUTO policy's -- had more
    // than STEER_MISS_NUM / STEER_MISS_DEN of its frames missing
    unsigned long long *h_steer = nullptr;              // [FB_RING][2] per call (seq - 1) % FB_RING: missed frames, sequence number
    unsigned long long steer_seq = 0, steer_seq_seen = 0, steer_call_frames[FB_RING] = {};
    bool steer_spec = true, steer_lost = false;
    // stream state (double buffered: kernels read [cur], write [cur^1])
    DevBuf<float> d_E[2];
    DevBuf<float> d_tail[2];
    int e_cur = 0, tail_cur = 0;
    Workspace ws;
    hipStream_t io_stream[3] = {}; hipEvent_t io_ev[8] = {};   // host-pointer entry points with page-locked buffers: copy in / run / copy out
    DevBuf<double> d_gate_state;
    DevBuf<int> d_last_bin; DevBuf<float> d_last_rad, d_last_prob;
    int last_arrays = 0, last_frames = 0;   // the shape of the last stream call that succeeded (mca_hip_copy_gate)
    DevBuf<float> d_doa[2];                 // 2-mic path: smoothed _currentDOA per array
    int doa_cur = 0;
    long long gcc2_frames_done = 0;         // (kept in the state header for blob compatibility; the counters below are what runs)
    DevBuf<long long> d_vdone[2];           // 2-mic path: frames that fired so far, per array (double-buffered with d_doa)
    DevBuf<int> d_g2_vidx, d_g2_nv; DevBuf<float> d_g2_rad, d_g2_prob;   // gated 2-mic path: workspaces of [rows], d_g2_nv [max_arrays]
    DevBuf<unsigned char> d_g2_reset;       // [rows] per fired frame: the memory factors are zero (silence rule)
    DevBuf<int> d_g2_post0;                 // [max_arrays] first frame of the call at which the floor estimate exists
    DevBuf<int> d_silence;                  // [max_arrays] _silenceFramesCounter (BinauralLocalisation.cpp:326), stream state
    // the DOA tracker (mca_hip_gcc2_tracker_attach; kernels_gcc2_track.hip): slots 0 .. max_arrays - 1 belong to the stream state,
    // slot max_arrays to the frame hook
    bool tracked = false;
    mca_hip_gcc2_tracker_config trk{};      // as resolved by attach (no zeros left)
    DevBuf<double> d_trk_x, d_trk_sd; DevBuf<int> d_trk_si;   // [slots][N] particles, [slots][2] DOA / prob, [slots][4] alive / track / upd
    DevBuf<int> d_trk_sil;                  // [max_arrays] the silence counters before the call (k_gcc2_compact overwrites d_silence)
    DevBuf<float> d_trk_corr; DevBuf<int> d_trk_idx;   // workspaces: the rows / argmaxes of a call whose caller did not ask for them
    DevBuf<double> d_trk_res;               // [4] what the frame hook's launch returns: DOA, prob, fired (the first byte of [2]), track (an int in [3])
    // workspace
    unsigned long long ws_gen = 0;          // bumped by grow_ws, and by nothing else, whenever a workspace buffer is reallocated: recorded graphs hold the old pointers
    std::vector<mca_hip_graph *> graphs;   // live graphs of this context (orphaned by mca_hip_destroy)
    // adaptive SRP precision: fp16 coarse scan (one plane) + exact repair (hi + lo planes)
    DevBuf<unsigned long long> d_rstats;
    // lazy tails (mca_internal.h, HIST_FRAMES): what the last lazy adaptive call left for the next one, double buffered like d_E
    DevBuf<float> d_hist_pcm[2];                   // [max_arrays][M][HIST_SAMPLES]
    DevBuf<float> d_hist_C[2];                     // [max_arrays][HIST_FRAMES][Dp] coarse rows (patched where a repair pass recomputed them)
    DevBuf<float> d_ehist[2];                      // [max_arrays][D] the energies in front of them
    int hist_cur = 0, hist_n = 0;                  // the buffers that hold the pending history, the arrays it covers
    bool hist_pending = false;                     // the state in d_E is coarse: exact = settle_history, or the next lazy call's own repair pass
    unsigned long long adapt_frames_total = 0;
    float tau_en = 0.f;            // normalised energies closer than this cannot be ordered from the coarse map
    // ADAPTIVE backs off to plain FP16X3 (the arithmetic its repair pass reproduces) while most rows need the repair -- noise
    // only, silence: every pick is a near tie and coarse + repair of everything costs twice the direct exact pass.  The last
    // kernel of an adaptive call leaves its running totals in page-locked memory; the next calls read them when they have arrived
    // (no synchronisation) and suspend the mode for fb_backoff eligible calls, then probe again with one adaptive call.
    Knobs kn;
    bool adapt_suspended = false;                       // policy state between calls (a recording looks past it: StreamCall::recording)
    int fb_left = 0, fb_backoff = 8, fb_state = 0;      // (adapt_policy_begin)
    bool cand_heavy = false;                            // the last report had more than a fifth of the rows recomputed: whole-row repair kernels (adapt_policy_begin)
    unsigned long long fb_probe_seq = 0;
    unsigned long long *h_probe = nullptr;              // [FB_RING][4] one slot per adaptive call (seq - 1) % FB_RING: flagged frames, listed repair units, sequence number of the call
    unsigned long long fb_calls = 0, fb_seq_seen = 0, fb_groups_prev = 0, fb_frames_prev = 0, fb_flagged_prev = 0;
    unsigned long long fb_frames_ring[FB_RING] = {};    // adapt_frames_total after adaptive call number i + 1
    unsigned long long fb_m = 0;                        // eligible stream calls seen by adapt_policy_begin
    unsigned long long fb_launch_m[FB_RING] = {};       // ... and the one during which adaptive call number i + 1 was enqueued
    bool fb_lost = false;                               // a report did not arrive within FB_WAIT_MS: the policy stops consuming reports (until mca_hip_reset)
    int a_elem = 4;                // bytes per element of the A operand (its row layout is the call's: RowLayout)
    // frame API (double)
    DevBuf<double> d_fr;          // workspace: the frame's spectra [M][ccs_len]
    DevBuf<double> d_E64[2]; int e64_cur = 0;
    DevBuf<double> d_res;         // [S] doa, [S] prob, power
    DevBuf<int> d_bins;
    DevBuf<double> d_out64;       // workspace: the beamformed spectrum [ccs_len]
    // FreqGCC frame hook (double): its own smoothed correlation, apart from the stream state d_E and the steering frame state d_E64
    DevBuf<double> d_g2f_corr[2]; int g2f_cur = 0;                 // _prevCorrelationsReal [D], double buffered like d_E64
    DevBuf<double> d_g2f_res;                                      // [4] argmax, prob, DOA (k_frame_gcc2), linear power (k_frame_power)
    G2FrameState g2f;
    std::vector<double> h_stage;
    StagePool stage;              // device staging of the host-pointer entry points
    // timing
    unsigned timing = 0;                 // bit k: launches of kernel id k are bracketed with events
    bool timing_open = false;
    std::vector<TimedEvent> events;
    std::vector<hipEvent_t> pool;
    int t_launches[MCA_HIP_K_COUNT] = {};
    double t_ms[MCA_HIP_K_COUNT] = {};
    std::string err;
};

namespace {

// ---- the call record ------------------------------------------------------------------------------
// What holds for ONE stream call, or one piece of it, and for nothing after it: built on the entry point's stack and handed down by
// reference.  The context keeps what outlives a call (state, policy, counters, buffers).
struct MapResult {                 // what run_correlation_map left in Workspace::d_C: partial maps of a split-K contraction, the elements
    int c_planes = 1; long long c_plane = 0;       // between them,
    bool partial_done = false; int part_planes = 1;   // whether it also left the scan's chunk-local results (d_part, d_nv), one set per K half
};
enum class Caller { DEVICE, HOST, RECORDING };   // a device-pointer entry point / a host-pointer one (the eager form on its pageable and its page-locked path: the same bits) / graph_record
struct StreamCall {
    Caller caller = Caller::DEVICE;
    int a0 = 0;                    // the first array of the piece being enqueued: per-array state is addressed from it
    long long rows_planned = 0;       // > 0: the rows the contraction is planned for -- the whole call's while it is worked off in pieces (plan_gemm)
    int arrays_planned = 0;           // ... and its arrays (repair_ksplit_for)
    // what the call decided on its way down: it leaves the repair of its last rows to the next call (the coarse analysis keeps the PCM);
    // its analysis may steer ahead of the picks (Y holds the whole call) / did (AnalysisPlan::steers); the second pick patches the missed frames
    bool lazy = false, steer = false, steer_fused = false, steer_patched = false;
    MapResult map;
    bool recording() const { return caller == Caller::RECORDING; }   // the mode's own kernels whatever the back-off does; no policy, no counters, no event pairs
    bool may_lazy() const { return caller == Caller::DEVICE; }       // device-pointer calls outside recordings may leave their tails to the next call
    long long planned(long long rows) const { return rows_planned > 0 ? rows_planned : rows; }
    int planned_arrays(int n_arrays) const { return arrays_planned > 0 ? arrays_planned : n_arrays; }
};
// The row layout of the A operand in one phase of a call: 1 plane (fp32, fp16, the ADAPTIVE coarse pass) or 2 (fp16 hi + lo: FP16X3, the
// repair pass, ADAPTIVE calls that run as FP16X3 -- mca_hip_ctx::tab_planes), the contraction depth per plane and the elements per row
struct RowLayout { int planes, kp, row_elems; };

mca_hip_ctx *const NO_CTX = nullptr;             // a failing create (and the calls that have no context): the text goes to the creation error
// the staging-pool slots of the host-pointer calls (process_frames_host_impl keeps its own); the numbers stay
enum Gcc2StageSlot { SG_PCM = 0, SG_ARGMAX = 1, SG_DOA = 2, SG_PROB = 3, SG_CORR = 4, SG_TRACK = 5, SG_FIRED = 6, SG_PROB_IN = 5, SG_PROB_OUT = 6 };

// ---- the reference's helper chain, host side (exact float/double sequence of
//      src/mcarray/microhponeArrayHelpers.cpp:38-120; [BUILD-DEFINES] double sin) ----
double speed_of_sound() { return 346.1; }                                           // :38-43
float doa_idx2angle(int idx, float step) { float pr = (float)idx * step; return (float)((double)pr - M_PI_2); }   // :117-120
float doa_to_delay_far_field(float doa, float microDist)                            // :46-67
{
    return (float)(((double)microDist * std::sin((double)doa)) / speed_of_sound());
}
float doa_to_delay_samples(float doa, float microDist, int fs) { return doa_to_delay_far_field(doa, microDist) * (float)fs; }   // :69-72
double distance(const std::vector<double> &xyz, int i, int j)                        // ArrayDescription.cpp:57-64
{
    return std::sqrt(std::pow(xyz[3 * j] - xyz[3 * i], 2) + std::pow(xyz[3 * j + 1] - xyz[3 * i + 1], 2) +
                     std::pow(xyz[3 * j + 2] - xyz[3 * i + 2], 2));
}

// A workspace of at least n elements -- the one place that reallocates a buffer a call hands to kernels, and so the one place that
// bumps ws_gen: whatever a recorded graph may have baked in is gone with the buffer (also when the allocation then fails).
template <typename T>
int grow_ws(mca_hip_ctx *c, DevBuf<T> &b, size_t n, const char *what)
{
    if (n <= b.n) return MCA_HIP_OK;
    ++c->ws_gen;
    const hipError_t e = b.alloc(n);
    return e == hipSuccess ? MCA_HIP_OK : hip_fail(c, e, what);
}

// ... whose first `fill` elements start out as the byte `v` (the self-cleaning words of the adaptive path, the zero padding of the A
// rows): filled on the null stream and waited for, since the caller's stream need not wait for the null stream by itself.  A buffer
// that could not be filled is dropped, so that a retry starts from nothing.
template <typename T>
int grow_ws_filled(mca_hip_ctx *c, DevBuf<T> &b, size_t n, size_t fill, int v, const char *what)
{
    if (n <= b.n) return MCA_HIP_OK;
    const int rc = grow_ws(c, b, n, what);
    if (rc) return rc;
    hipError_t e = hipMemset(b.p, v, fill * sizeof(T));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) return MCA_HIP_OK;
    b.reset();
    return hip_fail(c, e, what);
}

void free_ctx(mca_hip_ctx *c)
{
    if (!c) return;
    if (c->h_probe) (void)hipHostFree(c->h_probe);
    if (c->h_steer) (void)hipHostFree(c->h_steer);
    for (auto &e : c->io_ev) if (e) (void)hipEventDestroy(e);
    for (auto &q : c->io_stream) if (q) (void)hipStreamDestroy(q);
    for (auto &e : c->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto &e : c->pool) (void)hipEventDestroy(e);
    delete c;                                                  // every device buffer goes with its member
}

// (the environment is read through knobs.h, by mca_hip_create only)
Knobs read_knobs(const mca_hip_config &cfg, StreamShape &shape)
{
    Knobs k;
    auto geti = [](const char *v, long long dflt) { return v ? std::atoll(v) : dflt; };
    k.fb_enabled = cfg.adaptive_fallback != MCA_HIP_ADAPT_FALLBACK_OFF;
    if (const char *v = env_str("MCA_HIP_ADAPT_FALLBACK")) k.fb_enabled = std::atoi(v) != 0;
    // (4096 rows -- round 2: 8192; with the merged index the coarse contraction of 4096 rows takes 26 us against 81 + 12 us of the
    // three-product one: the literal BASELINE configs[2] call, 1 array x 4096 frames, is inside)
    k.adapt_min_rows = geti(env_str("MCA_HIP_ADAPT_MIN_ROWS"), cfg.adaptive_min_rows > 0 ? cfg.adaptive_min_rows : 4096);
    k.adapt_max_sources = (int)geti(env_str("MCA_HIP_ADAPT_MAX_SOURCES"), cfg.adaptive_max_sources > 0 ? cfg.adaptive_max_sources : 1);
    if (const char *v = env_str("MCA_HIP_ADAPT_TAU_SCALE")) k.tau_scale = std::atof(v);
    if (const char *v = env_str("MCA_HIP_WS_MAX_MB")) k.ws_max_bytes = (long long)std::atoll(v) << 20;
    k.force_generic = env_str("MCA_HIP_FORCE_GENERIC") != nullptr;
    k.scan_carry = cfg.scan_carry != 0 || env_str("MCA_HIP_SCAN_CARRY") != nullptr;
    if (const char *v = env_str("MCA_HIP_ADAPT_LAZY")) shape.lazy_tails = std::atoi(v) != 0;
    if (const char *v = env_str("MCA_HIP_ADAPT_CAND")) shape.cand = std::atoi(v) != 0 ? 1 : 0;
    k.no_n2048 = env_str("MCA_HIP_NO_N2048") != nullptr;
    return k;
}

// _currentDOA = 0, _prob = -1 (BeamformingSeparationAndLocalisation.cpp:51-52); no frame has fired yet -> bin -1
int init_last_state(mca_hip_ctx *c, hipStream_t st)
{
    const size_t n = (size_t)c->cfg.max_arrays * MCA_MAX_SOURCES;
    std::vector<int> b(n, -1); std::vector<float> pr(n, -1.f);
    HIP_TRY(c, hipMemcpyAsync(c->d_last_bin, b.data(), n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, c->d_last_rad.zero_async(st));
    HIP_TRY(c, hipMemcpyAsync(c->d_last_prob, pr.data(), n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, c->d_gate_state.zero_async(st));
    HIP_TRY(c, hipStreamSynchronize(st));       // (the host vectors above go out of scope; mca_hip_reset returns with nothing queued)
    return MCA_HIP_OK;
}

// steering table B of the SRP contraction = precomputeTauMatrix (SteeringBeamforming.cpp:87-88)
// for the first pair of every delay group, laid out for the MFMA kernels.
// a table of `bytes` bytes built on the host, into a buffer sized in bytes
int upload_bytes(mca_hip_ctx *c, DevBuf<unsigned char> &b, const void *host, size_t bytes, const char *what)
{
    const hipError_t e = b.upload(static_cast<const unsigned char *>(host), bytes);
    return e == hipSuccess ? MCA_HIP_OK : hip_fail(c, e, what);
}

// (built into locals and moved into the context behind the last upload, like build_merged_tables: a failure leaves no half of a table set)
int build_steering_table(mca_hip_ctx *c)
{
    const int K = c->K, D = c->D, Dp = c->Dp, Kp = c->Kp;
    DevBuf<unsigned char> dB, dBt;
    int rc;
    std::vector<int> first_pair(c->G);
    if (c->ula) { for (int g = 0; g < c->G; ++g) first_pair[g] = g; /* pair (0, g+1) has index g */ }
    else for (int g = 0; g < c->G; ++g) first_pair[g] = g;
    const double N = 2.0 * (K - 1);
    if (c->prec == MCA_HIP_SRP_FP32) {
        std::vector<float> B((size_t)Kp * Dp, 0.f);
        for (int g = 0; g < c->G; ++g)
            for (int k = 0; k < K; ++k)
                for (int d = 0; d < D; ++d) {
                    double ph = 2.0 * M_PI * (double)k * (double)c->delays[(size_t)first_pair[g] * D + d] / N;
                    size_t r = ((size_t)g * K + k) * 2;
                    B[r * Dp + d] = (float)std::cos(ph);
                    B[(r + 1) * Dp + d] = (float)(-std::sin(ph));
                }
        if ((rc = upload_bytes(c, dB, B.data(), B.size() * sizeof(float), "the steering table"))) return rc;
    } else {
        const int planes = c->tab_planes;
        std::vector<_Float16> B((size_t)planes * Dp * Kp, (_Float16)0.f);
        for (int g = 0; g < c->G; ++g)
            for (int d = 0; d < D; ++d)
                for (int k = 0; k < K; ++k) {
                    double ph = 2.0 * M_PI * (double)k * (double)c->delays[(size_t)first_pair[g] * D + d] / N;
                    float v[2] = {(float)std::cos(ph), (float)(-std::sin(ph))};
                    for (int q = 0; q < 2; ++q) {
                        size_t kk = ((size_t)g * K + k) * 2 + q;
                        _Float16 hi = (_Float16)v[q];
                        B[(size_t)d * Kp + kk] = hi;
                        if (planes == 2) B[((size_t)Dp + d) * Kp + kk] = (_Float16)(v[q] - (float)hi);
                    }
                }
        if ((rc = upload_bytes(c, dB, B.data(), B.size() * sizeof(_Float16), "the steering table"))) return rc;
        if (Dp == 384) {
            // the same table tiled for the 256 x 384 kernel: one 32-deep K stage of all 384 columns is 24 KiB
            // contiguous, so every LDS-DMA instruction of that kernel moves one contiguous KiB
            const int ns32 = Kp / 32;
            std::vector<_Float16> Bt(B.size());
            for (int pl = 0; pl < planes; ++pl)
                for (int sl = 0; sl < ns32; ++sl)
                    for (int d = 0; d < Dp; ++d)
                        std::memcpy(&Bt[(((size_t)pl * ns32 + sl) * Dp + d) * 32], &B[((size_t)pl * Dp + d) * Kp + (size_t)sl * 32], 32 * sizeof(_Float16));
            if ((rc = upload_bytes(c, dBt, Bt.data(), Bt.size() * sizeof(_Float16), "the tiled steering table"))) return rc;
        }
    }
    c->d_B.swap(dB); c->d_Bt.swap(dBt);
    return MCA_HIP_OK;
}

// the layout of rows of `planes` planes: the merged index with one plane on a merged context
RowLayout row_layout(const mca_hip_ctx *c, int planes)
{
    const int kp = plan_kp(*c, planes);
    return {planes, kp, kp * planes};
}

// Merged contraction index of the one-plane fp16 path on a uniform linear array (see mca_hip_ctx::merged).  The pairs of
// spacing g have the delay table tau_g(d); on a ULA tau_g = g tau_1 up to the rounding of the reference's float chain
// (doaToDelayFarFieldSamples, SteeringBeamforming.cpp:73), so exp(j 2 pi k tau_g / N) = exp(j 2 pi (k g) tau_1 / N) to ~1e-5
// rad -- a twentieth of the fp16 rounding of the operands this path carries anyway; checked here, else no merging.  The exact
// paths (FP32, FP16X3, the repair pass) keep the per-group index and the reference's own tables.
int build_merged_tables(mca_hip_ctx *c)
{
    // (round 6: also at 2048-sample frames, k_stft_phat_2048<..., MERGE>)
    if (!c->ula || (c->generic && !c->n2048) || c->n512 || (c->M != 4 && c->M != 8) || c->Dp % 64 != 0) return MCA_HIP_OK;
    if (c->prec != MCA_HIP_SRP_ADAPTIVE && c->prec != MCA_HIP_SRP_FP16) return MCA_HIP_OK;
    const int K = c->K, D = c->D, Dp = c->Dp, G = c->G;
    const double N = 2.0 * (K - 1);
    for (int g = 1; g < G; ++g)
        for (int d = 0; d < D; ++d)
            if (std::fabs((double)c->delays[(size_t)g * D + d] - (g + 1) * (double)c->delays[d]) > 1e-4) return MCA_HIP_OK;   // (pair (0, g + 1) has index g)
    std::vector<unsigned short> rank;
    std::vector<int> ms;
    merged_products(G, K, rank, ms);
    const int n_merged = (int)ms.size();
    const int Kp = round_up(2 * ((n_merged + 63) & ~63), 32);       // (whole wave rows: the analysis kernel stores its LDS region as it stands, zeros behind n_merged)
    const bool fold = fold_applies(true, c->N, FFT_N, D, Dp, c->delays.data());
    DevBuf<unsigned char> dBm, dBtm, dBfold; DevBuf<unsigned short> dmrank;
    int rc;
    if (fold) {
        // mirror fold (fold_table.h): planar rows, the folded values at full width for the kernels that keep it, the two half-width tables
        FoldTables ft;
        build_fold_tables(c->delays.data(), D, Dp, ms.data(), n_merged, Kp, c->N, ft);
        ft.even.insert(ft.even.end(), ft.odd.begin(), ft.odd.end());      // [even | odd]
        if ((rc = upload_bytes(c, dBm, ft.full.data(), ft.full.size() * 2, "the folded steering table")) ||
            (rc = upload_bytes(c, dBtm, ft.full_tiled.data(), ft.full_tiled.size() * 2, "the tiled folded steering table")) ||
            (rc = upload_bytes(c, dBfold, ft.even.data(), ft.even.size() * 2, "the half-width steering tables"))) return rc;
    } else {
    std::vector<_Float16> B((size_t)Dp * Kp, (_Float16)0.f);
    for (int d = 0; d < D; ++d)
        for (int r = 0; r < n_merged; ++r) {
            const double ph = 2.0 * M_PI * (double)ms[(size_t)r] * (double)c->delays[d] / N;
            B[(size_t)d * Kp + 2 * r] = (_Float16)(float)std::cos(ph);
            B[(size_t)d * Kp + 2 * r + 1] = (_Float16)(float)(-std::sin(ph));
        }
    if ((rc = upload_bytes(c, dBm, B.data(), B.size() * sizeof(_Float16), "the merged steering table"))) return rc;
    if (Dp == 384) {
        const int ns32 = Kp / 32;
        std::vector<_Float16> Bt(B.size());
        for (int sl = 0; sl < ns32; ++sl)
            for (int d = 0; d < Dp; ++d)
                std::memcpy(&Bt[((size_t)sl * Dp + d) * 32], &B[(size_t)d * Kp + (size_t)sl * 32], 32 * sizeof(_Float16));
        if ((rc = upload_bytes(c, dBtm, Bt.data(), Bt.size() * sizeof(_Float16), "the tiled merged steering table"))) return rc;
    }
    }
    rank.resize((rank.size() + 3) / 4 * 4, 0xffff);
    const hipError_t e = dmrank.upload(rank.data(), rank.size());
    if (e != hipSuccess) return hip_fail(c, e, "the ranks of the merged index");
    // the last upload has succeeded: only now does the context change
    c->d_Bm.swap(dBm); c->d_Btm.swap(dBtm); c->d_Bfold.swap(dBfold); c->d_mrank.swap(dmrank);
    c->n_merged = n_merged; c->Kp_m = Kp; c->fold = fold;
    c->merged = true;
    return MCA_HIP_OK;
}

void time_begin(mca_hip_ctx *c, const StreamCall &call, int id, hipStream_t st)
{
    c->timing_open = !call.recording() && ((c->timing >> id) & 1u);      // (event pairs belong to eager calls)
    if (!c->timing_open) return;
    TimedEvent ev; ev.id = id;
    auto get = [&]() { hipEvent_t e; if (!c->pool.empty()) { e = c->pool.back(); c->pool.pop_back(); } else (void)hipEventCreate(&e); return e; };
    ev.a = get(); ev.b = get();
    (void)hipEventRecord(ev.a, st);
    c->events.push_back(ev);
}
void time_end(mca_hip_ctx *c, hipStream_t st)
{
    if (!c->timing_open) return;
    c->timing_open = false;
    (void)hipEventRecord(c->events.back().b, st);
}

// the A buffer of rows of this layout: an ADAPTIVE context keeps its two-plane rows (repair pass, FP16X3 calls) apart from the
// one-plane rows of the coarse pass, so that a buffer only ever sees one row layout (its Kp padding columns stay zero)
DevBuf<unsigned char> &a_buf(mca_hip_ctx *c, const RowLayout &lay) { return (c->prec == MCA_HIP_SRP_ADAPTIVE && lay.planes == 2) ? c->ws.d_Ax : c->ws.d_A; }

int ensure_a(mca_hip_ctx *c, const RowLayout &lay, long long rows)
{
    // rows rounded up to the 256-row tile of the split-K MFMA kernel, which loads whole tiles unclamped
    const size_t need_a = (size_t)((rows + 255) / 256 * 256) * lay.row_elems * c->a_elem;
    return grow_ws_filled(c, a_buf(c, lay), need_a, need_a, 0, "the A operand");          // the Kp padding columns stay zero forever
}

int ensure_workspace(mca_hip_ctx *c, const RowLayout &lay, long long rows_chunk, long long rows_plan, long long rows_total)      // (rows_plan: StreamCall::planned)
{
    int rc_a = ensure_a(c, lay, rows_chunk);
    if (rc_a) return rc_a;
    const int planes = std::max(2, plan_gemm(*c, lay.planes, rows_plan).ksplit);
    return grow_ws(c, c->ws.d_C, (size_t)rows_total * c->Dp * planes, "the correlation map");   // room for the partial maps of a split-K contraction
}

int ensure_scan_workspace(mca_hip_ctx *c, int n_arrays, int n_frames, int n_chunks)
{
    Workspace &w = c->ws;
    const size_t need = (size_t)n_arrays * n_chunks, nf = (size_t)n_arrays * n_frames;
    int rc;
    if ((rc = grow_ws(c, w.d_part, need * c->D * 2, "the scan's chunk results")) ||      // (two sets when a split-K contraction leaves them)
        (rc = grow_ws(c, w.d_estart, need * c->D, "the scan's chunk starts")) || (rc = grow_ws(c, w.d_nv, need, "the scan's voiced counts"))) return rc;
    if (c->cfg.use_power_floor &&
        ((rc = grow_ws(c, w.d_power, nf, "the gate's frame powers")) || (rc = grow_ws(c, w.d_power_out, nf, "the gate's frame powers (dB)")) ||
         (rc = grow_ws(c, w.d_voiced, nf, "the gate's flags")))) return rc;
    return MCA_HIP_OK;
}

// A-operand workspace budget per slice of frames (MCA_HIP_WS_MAX_MB lets the tests force the sliced path)
long long ws_max_bytes(const mca_hip_ctx *c) { return c->kn.ws_max_bytes; }

long long chunk_frames_for(const mca_hip_ctx *c, const RowLayout &lay, int n_arrays, int n_frames)
{
    long long row_bytes = (long long)lay.row_elems * c->a_elem;
    long long rows_cap = ws_max_bytes(c) / row_bytes;
    long long fc = rows_cap / n_arrays;
    if (fc >= n_frames) return n_frames;
    fc = fc / 8 * 8;
    if (fc < 8) fc = 8;
    return fc < n_frames ? fc : n_frames;
}

// ---- adaptive SRP precision (MCA_HIP_SRP_ADAPTIVE) ------------------------------------------------------------
// Does a call of this shape run coarse + repair?  The repair pass needs the list mode of k_stft_phat (1024-sample frames,
// more than two microphones) and has a fixed cost of a few small launches, so small batches -- which are latency bound
// whatever the precision -- run as plain FP16X3, which is what the repair pass reproduces.  (Gated streams do take the
// adaptive path: the planning wave lists the last 25 VOICED rows behind a flagged frame)
bool adaptive_shape(const mca_hip_ctx *c, int n_arrays, int n_frames, long long rows_planned = 0)
{
    const long long rows = rows_planned > 0 ? rows_planned : (long long)n_arrays * n_frames;     // (see plan_gemm)
    // (more than one source: the S-th pick is a weak peak more often than not -- a second source, or noise when fewer than S
    // are active -- and a third to all of the frames are flagged: 8 x 4096 frames with S = 2 / 3 / 4 real sources spend 0.89 / 1.60 /
    // 1.76 ms in the repair pass, more than the 0.3 ms the coarse contraction saves; MCA_HIP_ADAPT_MAX_SOURCES lifts the limit)
    return c->prec == MCA_HIP_SRP_ADAPTIVE && ((!c->generic && !c->n512 && c->N == FFT_N) || ((c->n2048 || c->n512) && c->M <= 8)) && c->M > 2 && c->S <= c->kn.adapt_max_sources &&
           rows >= c->kn.adapt_min_rows && n_frames >= 2 * SCAN_CHUNK;
}
bool adaptive_applies(const mca_hip_ctx *c, const StreamCall &call, int n_arrays, int n_frames)      // (a recording looks past the suspension)
{ return adaptive_shape(c, n_arrays, n_frames, call.rows_planned) && (call.recording() || !c->adapt_suspended); }
// lazy tails: contexts whose adaptive calls may leave the repair of their last rows to the next call -- no power gate (the rows a frame
// depends on are then simply the 16 before it), the wave-per-run analysis (4 / 8 microphones at 1024 samples: it keeps the PCM and reads it back)
bool lazy_context(const mca_hip_ctx *c)
{
    return c->prec == MCA_HIP_SRP_ADAPTIVE && c->lazy_tails && !c->cfg.use_power_floor && (c->M == 8 || c->M == 4) && !c->generic && !c->n512 &&
           c->cfg.gcc_weighting == MCA_HIP_GCC_PHAT && c->stream_ok;
}

// Candidate columns (cand_unit.h) for this call?  Lazy calls (no frame is repeated for the state's sake; lazy_context: 4 / 8 microphones) of
// contexts whose coarse analysis marks no unsure rows, one source (wave_candidates bounds the first pick) -- a unit that wants every column
// costs the contraction the whole steering table.  Only under the AUTO back-off policy, and not while it is probing or the last report
// was heavy (noise only: 45 % of the frames flagged, ten columns each -- 4.3 ms per call against 2.0 for the whole-row kernels): a context
// pinned to the mode (adaptive_fallback OFF: bit-reproducible runs) keeps the whole-row kernels whatever the content.
// MCA_HIP_ADAPT_CAND=1 / 0 overrides the policy (always where the shape allows / never).  16 microphones keep whole rows for every flagged
// frame: a second work list that sent the frames not bound to whole rows to candidate columns measured slower
// (profiles/r06_m16_two_lists_negative.log; the code is tools/probes/r06_m16_two_work_lists_negative.patch).
static bool cand_call(const mca_hip_ctx *c, bool lazy)
{
    if (c->cand == 0 || !lazy || wave16_applies(*c) || c->S != 1 || c->Dp / 32 > CAND_WORDS_MAX) return false;
    if (c->cand == 1) return true;                                 // MCA_HIP_ADAPT_CAND=1: whatever the content (tests, sweeps, pinned contexts that want it)
    return c->kn.fb_enabled && c->h_probe && c->fb_state == 0 && !c->cand_heavy;
}

// Called once at the top of an eager stream call (not per piece of a call, not while a graph is recorded): consumes the reports of
// the adaptive calls that were enqueued FB_LAG eligible calls ago (or earlier) and decides whether this call runs coarse + repair or
// plain FP16X3.
//   NORMAL     adaptive; a report of more than 30 % of the rows recomputed (or of the frames flagged) since the last one suspends the mode for fb_backoff
//              eligible calls (8, doubling up to 256 while the probes keep reporting that)
//   SUSPENDED  plain FP16X3, counting down; then ONE adaptive call probes
//   WAITING    plain FP16X3 until the probe's report is consumed (FB_LAG calls after the probe): heavy again -> SUSPENDED, else NORMAL
// Round 6: every adaptive call has its own report slot and a report is consumed by the call FB_LAG calls after its
// own, which WAITS for it if need be -- before, a call took "whatever has arrived by now" and the switch (and with it the choice between
// candidate columns and whole rows, cand_call) could move by a call from run to run.  A report that does not arrive within FB_WAIT_MS (a
// stream held up by something only this thread would release) ends the policy for the stream: the mode stays what it is.
void adapt_policy_begin(mca_hip_ctx *c, const StreamCall &call, int n_arrays, int n_frames)
{
    if (!c->kn.fb_enabled || call.recording() || !c->h_probe || !adaptive_shape(c, n_arrays, n_frames)) return;
    bool fresh = false, heavy = false;
    const unsigned long long m = c->fb_m++;
    unsigned long long seq = c->fb_seq_seen;                                   // the last report due at this call
    while (seq < c->fb_calls && c->fb_launch_m[seq % FB_RING] + FB_LAG <= m) ++seq;      // (call number seq + 1 lives at index seq % FB_RING)
    if (seq > c->fb_seq_seen && !c->fb_lost && c->fb_calls - seq < FB_RING - 8) {
        const unsigned long long *slot = c->h_probe + 4 * ((seq - 1) % FB_RING);
        const auto t0 = std::chrono::steady_clock::now();
        while (__atomic_load_n(&slot[2], __ATOMIC_ACQUIRE) != seq) {
            if (std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() > FB_WAIT_MS) { c->fb_lost = true; break; }
            std::this_thread::yield();
        }
        if (!c->fb_lost) {
        const unsigned long long groups = __atomic_load_n(&slot[1], __ATOMIC_RELAXED), frames = c->fb_frames_ring[(seq - 1) % FB_RING];
        const unsigned long long flagged = __atomic_load_n(&slot[0], __ATOMIC_RELAXED);
        const bool fwd = groups >= c->fb_groups_prev && frames > c->fb_frames_prev && flagged >= c->fb_flagged_prev;      // (the totals restart with mca_hip_reset_timing)
        const unsigned long long dg = fwd ? groups - c->fb_groups_prev : 0, df = fwd ? frames - c->fb_frames_prev : 0, dfl = fwd ? flagged - c->fb_flagged_prev : 0;
        c->fb_seq_seen = seq; c->fb_groups_prev = groups; c->fb_frames_prev = frames; c->fb_flagged_prev = flagged;
        fresh = df > 0;
        // (... or 30 % of the frames flagged: digital silence lists no rows -- they are zero in both maps -- but every frame is planned and picked twice)
        heavy = fresh && (dg * REPAIR_GROUP * 100 > df * 30 || dfl * 100 > df * 30);
        // candidate columns pay while the list is short (one workgroup per unit); a call that recomputes most rows is a dense contraction again
        if (fresh) c->cand_heavy = dg * REPAIR_GROUP * 100 > df * 20;
        }
    } else if (seq > c->fb_seq_seen) {
        c->fb_seq_seen = seq;                                                  // (more calls in flight than slots, or the policy has ended: dropped)
    }
    auto suspend = [&]() {
        c->fb_state = 1; c->adapt_suspended = true;
        c->fb_left = c->fb_backoff - 1;                                                   // (this call is the first of them)
        c->fb_backoff = std::min(c->fb_backoff * 2, 256);
    };
    switch (c->fb_state) {
    case 0:
        if (heavy) suspend(); else if (fresh) c->fb_backoff = 8;
        break;
    case 1:
        if (--c->fb_left < 0) { c->fb_state = 2; c->adapt_suspended = false; c->fb_probe_seq = c->fb_calls + 1; }   // this call probes
        break;
    default:
        c->adapt_suspended = true;
        if (fresh && seq >= c->fb_probe_seq) {
            if (heavy) suspend(); else { c->fb_state = 0; c->adapt_suspended = false; c->fb_backoff = 8; }
        }
        break;
    }
}

// K segments of the repair contraction AT MOST: by the shape of the (whole) call (a long list lowers the number on the device,
// repair_ksplit_eff).  The tails of every array -- REPAIR_WARM + 1 rows
// rounded up to repair units -- are always recomputed: a few arrays leave a few hundred rows, where 32 segments fill the chip;
// 128 arrays leave thousands, where 32 partial maps per row cost more (k_repair_patch reads them all) than they buy.
int repair_ksplit_for(const mca_hip_ctx *c, int n_arrays)      // (n_arrays: StreamCall::planned_arrays)
{
    // lazy tails: no array lists its last rows as a matter of course -- the list is as long as the content makes it, and the device-side
    // rule (repair_ksplit_eff) halves the segments when it is long
    if (lazy_context(c)) return REPAIR_KSPLIT_MAX;
    const long long tail_rows = (long long)n_arrays * (REPAIR_WARM + 1 + REPAIR_GROUP);
    return tail_rows <= 1024 ? 32 : (tail_rows <= 2560 ? 16 : 8);
}

// rows of one repair pass (the two-plane A rows of all listed groups may not fit the workspace budget at once)
long long repair_pass_rows(const mca_hip_ctx *c, int n_arrays, int n_frames)
{
    const long long gpa = (n_frames + REPAIR_GROUP - 1) / REPAIR_GROUP + HIST_UNITS;     // (+ the history units of the lazy tails)
    const long long all = (long long)n_arrays * gpa * REPAIR_GROUP;
    long long cap = ws_max_bytes(c) / ((long long)2 * c->Kp * 2) / 128 * 128;
    // (the repair contraction always leaves REPAIR_KSPLIT partial maps: Cx is sized for the worst case, all rows listed --
    // 1.6 GB next to the 1.9 GB of two-plane A rows on the bench shape; one pass in the common case, so no empty launches)
    if (cap < 128) cap = 128;
    return std::min((all + 127) / 128 * 128, cap);
}

int ensure_adapt_workspace(mca_hip_ctx *c, int n_arrays, int n_frames, int n_chunks)
{
    Workspace &w = c->ws;
    const size_t nf = (size_t)n_arrays * n_frames, nc = (size_t)n_arrays * n_chunks;
    const size_t ng = (size_t)n_arrays * ((n_frames + REPAIR_GROUP - 1) / REPAIR_GROUP + HIST_UNITS);     // (+ the history units of the lazy tails)
    int rc;
    if ((rc = grow_ws(c, w.d_flags, nf, "the flags of the coarse picks")) || (rc = grow_ws(c, w.d_unsure, nf, "the unsure frames")) ||
        // + the list of the chunks that hold a flagged frame; 0x7f: "no flagged frame", kept so by k_scan_repick
        (rc = grow_ws_filled(c, w.d_chunk_from, 2 * nc, nc, 0x7f, "the flagged chunks")) ||
        (rc = grow_ws(c, w.d_list, ng, "the repair list")) ||
        (rc = grow_ws_filled(c, w.d_need, ng, ng, 0, "the repair units' marks")) ||                         // test-and-set words; released by k_repair_patch / k_scan_repick
        (rc = grow_ws_filled(c, w.d_umask, ng * (c->Dp / 32), ng * (c->Dp / 32), 0, "the candidate columns")) ||   // per unit; cleared by k_scan_repick
        (rc = grow_ws(c, w.d_last_vchunk, (size_t)n_arrays, "the last voiced chunks")) ||
        (rc = grow_ws_filled(c, w.d_nlist, 4, 4, 0, "the list counters"))) return rc;                      // listed repair units | listed chunks, workgroups of k_scan_repick done | unused
    const long long rows = repair_pass_rows(c, n_arrays, n_frames);
    if ((rc = ensure_a(c, row_layout(c, 2), rows))) return rc;
    return grow_ws(c, w.d_Cx, (size_t)repair_cx_rows(rows, REPAIR_KSPLIT_MAX) * c->Dp, "the repair contraction's partial maps");
}

// The correctly rounded float reciprocal of d (a small positive integer): the candidate nearest 1/d in exact arithmetic
// (r d is exact in a double: 24 + <= 24 bits).  The scan kernels divide by d with it (normalised_energy).
static float exact_reciprocal(float d)
{
    const float r0 = (float)(1.0 / (double)d);
    float best = r0;
    double err = std::fabs(1.0 - (double)r0 * (double)d);
    const float cand[2] = {std::nextafterf(r0, 0.f), std::nextafterf(r0, 1.f)};
    for (float r : cand) {
        const double e = std::fabs(1.0 - (double)r * (double)d);
        if (e < err) { err = e; best = r; }
    }
    return best;
}

// the fields of StftPhatArgs that are the context's, the same for every launch
void stft_common(const mca_hip_ctx *c, StftPhatArgs &sa)
{
    sa.M = c->M; sa.window = c->d_window; sa.Kp = c->Kp;
    sa.N = c->N; sa.logH = c->logH; sa.kg = c->K; sa.ula = c->ula ? 1 : 0; sa.tw = c->d_tw;
}
// The launcher of the stream path, on the attribute rule of host_common.h (lds_limit): a plan's kernel (the lookups of kernels.h; nullptr: a form the build lacks -- plan and predicate disagree, which
// tests/test_stream_plan.py rules out), grid, block, dynamic LDS and the kernel's one argument struct; every launch is checked.
int launch(mca_hip_ctx *c, const void *kernel, dim3 grid, dim3 block, size_t lds, void *args, hipStream_t st, const char *form)
{
    if (!kernel) return fail(c, MCA_HIP_ERR_UNSUPPORTED, std::string("the build has no kernel of the form ") + form);
    void *argv[1] = {args};
    if (const int rc = lds_limit(c, kernel, lds)) return rc;
    HIP_TRY(c, hipLaunchKernel(kernel, grid, block, argv, lds, st));
    HIP_TRY(c, hipGetLastError());
    return MCA_HIP_OK;
}

// one analysis launch: the plan's fields into the arguments, the kernel of the plan's form (named in the launcher's message) on the plan's grid
int launch_analysis(mca_hip_ctx *c, StftPhatArgs &sa, const AnalysisPlan &p, hipStream_t st)
{
    static const void *(*const lookup[])(const StftForm &) = {stft_wave_kernel, stft_wave16_kernel, stft_512_kernel, stft_2048_kernel, stft_sub2_kernel, stft_gen_kernel,
                                                              stft_block_kernel, stft_few_kernel};      // (in the order of StftFamily)
    const StftForm &f = p.form;
    char name[160];
    std::snprintf(name, sizeof name, "analysis family %d: MT %d, ULA %d, fp32 %d, PL2 %d, POWER %d, NOPHAT %d, MERGE %d, CAND %d, FUSE %d", (int)f.family, f.mt, f.ula, f.f32, f.pl2,
                  f.power, f.nophat, f.merge, f.cand, f.fuse);
    sa.fpb = p.fpb; sa.skew = p.skew;
    return launch(c, lookup[(int)f.family](f), p.grid, p.block, p.lds, &sa, st, name);
}

int check_stream_args(mca_hip_ctx *c, const float *pcm, long long array_stride, long long mic_stride, int n_arrays, int n_frames)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!c->stream_ok) return fail(c, MCA_HIP_ERR_UNSUPPORTED, c->stream_why);
    if (!pcm) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "pcm_dev is NULL");
    if (n_arrays < 1 || n_arrays > c->cfg.max_arrays) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_arrays outside [1, max_arrays]");
    if (n_frames < 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_frames < 1");
    const long long need = (long long)(n_frames + 1) * c->H;
    if (mic_stride < need) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "mic_stride shorter than (n_frames+1)*hop samples");
    if (n_arrays > 1 && array_stride < (long long)(c->M - 1) * mic_stride + need) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "array_stride too short");
    if ((mic_stride & 1) || (array_stride & 1) || (reinterpret_cast<uintptr_t>(pcm) & 7))
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "pcm_dev must be 8-byte aligned with even strides (float2 loads)");
    return MCA_HIP_OK;
}

}  // namespace

extern "C" {

static int settle_history(mca_hip_ctx *c, hipStream_t st);    // lazy tails: exact state from the kept history (defined with localise_impl)

const char *mca_hip_version(void) { return "mcarray-hip 0.1.0 (gfx950)"; }

const char *mca_hip_last_error(const mca_hip_ctx *ctx) { return last_error(ctx); }

// the tables, the state and the switches of a new context; on an error the caller (mca_hip_create) frees what was built
static int init_ctx(mca_hip_ctx *c, const mca_hip_config *cfg, const hipDeviceProp_t &prop)
{
    c->cfg = *cfg;
    c->kn = read_knobs(*cfg, *c);
    c->gate = cfg->use_power_floor != 0; c->no_phat = cfg->gcc_weighting == MCA_HIP_GCC_NONE;
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c->M = cfg->n_mics; c->S = cfg->n_sources; c->N = cfg->fft_size; c->K = c->N / 2 + 1; c->prec = cfg->srp_precision;
    c->xyz.assign(cfg->mic_xyz, cfg->mic_xyz + 3 * c->M);
    c->cfg.mic_xyz = nullptr;
    c->step = (float)(cfg->doa_step_deg * M_PI / 180.0);                    // SteeringBeamforming.cpp:39
    c->D = (int)(std::round(M_PI / (double)c->step) + 1);                   // :40
    if (c->D < 3 || c->D > 512) return fail(c, MCA_HIP_ERR_UNSUPPORTED, "number of steering angles must be in [3,512]");
    c->P = c->M * (c->M - 1) / 2;
    // column padding of the correlation map = tile width of the contraction kernels: 192, or 64 for the fp16 kernels on
    // grids of up to 64 angles (the reference's own 37, the 2-microphone module's 61)
    c->Dp = (c->D <= 64 && c->prec != MCA_HIP_SRP_FP32) ? 64 : round_up(c->D, 192);
    c->H = c->N / 2;
    // stream API: the tuned 1024-sample kernels, or the any-power-of-two kernels (kernels_generic.hip)
    // whose channel spectra of one frame must fit the 160 KiB LDS of a CU
    c->generic = c->N != FFT_N || c->kn.force_generic;
    c->stream_ok = true;
    if (c->generic) {
        while ((1 << c->logH) < c->H) ++c->logH;
        if ((1 << c->logH) != c->H || c->N < 64) { c->stream_ok = false; c->stream_why = "the stream API needs a power-of-two fft_size >= 64 (the frame API takes any even size)"; }
        else if ((size_t)(c->M + 1) * (c->H + 1) * 8 + (size_t)c->H * 4 + 17 * 8 + 16 > 160 * 1024) {      // (the beamformer takes the sources in passes if need be)
            c->stream_ok = false; c->stream_why = "fft_size x n_mics exceeds the 160 KiB LDS of a CU in the stream API (use the frame API)";
        }
    }
    if (c->stream_ok && c->cfg.gcc_weighting == MCA_HIP_GCC_NONE && (c->generic || (c->M != 4 && c->M != 8))) {
        c->stream_ok = false;
        c->stream_why = "gcc_weighting NONE: the stream API serves it at fft_size 1024 with 4 or 8 microphones (the frame API takes any shape)";
    }
    c->n512 = c->N == 512 && c->M <= 8 && c->stream_ok;
    c->n2048 = c->N == 2048 && c->stream_ok && !c->kn.no_n2048;

    // generateLookupTable (SteeringBeamforming.cpp:58-94): pairs i<j lexicographic, float delays
    c->delays.resize((size_t)c->P * c->D);
    std::vector<float> fdist(c->P);
    {
        int p = 0;
        for (int i = 0; i < c->M; ++i)
            for (int j = i + 1; j < c->M; ++j, ++p) {
                double dist = distance(c->xyz, i, j);                         // :67
                fdist[p] = (float)dist;                                       // `float microDist` parameter
                for (int d = 0; d < c->D; ++d)                                // :71-73
                    c->delays[(size_t)p * c->D + d] = doa_to_delay_samples(doa_idx2angle(d, c->step), (float)dist, cfg->sample_rate);
                c->pairs.push_back(make_int2(i, j));
            }
    }
    c->grid.resize(c->D);
    for (int d = 0; d < c->D; ++d) c->grid[d] = doa_idx2angle(d, c->step);
    // delay-group merging: legal iff all pairs with equal (j - i) have bit-identical float distances
    // (then their D delays are bit-identical too) -- true for uniform linear arrays.
    c->ula = c->M > 2;
    {
        int p = 0;
        for (int i = 0; i < c->M && c->ula; ++i)
            for (int j = i + 1; j < c->M; ++j, ++p)
                if (std::memcmp(&fdist[p], &fdist[j - i - 1], sizeof(float)) != 0) { c->ula = false; break; }
    }
    c->G = c->ula ? c->M - 1 : c->P;
    c->Kp = round_up(c->G * c->K * 2, 32);     // K == KG == 513 on the tuned path
    c->tab_planes = (c->prec == MCA_HIP_SRP_FP16X3 || c->prec == MCA_HIP_SRP_ADAPTIVE) ? 2 : 1;
    c->a_elem = c->prec == MCA_HIP_SRP_FP32 ? 4 : 2;              // (planes of the A rows: tab_planes, but 1 for the ADAPTIVE coarse pass -- row_layout, per call)
    {
        // Error model of the coarse (one fp16 product) map, for the sensitivity test of k_scan_pick: every operand carries
        // a relative rounding error of rms ~2-3e-4 (11-bit significand), so a term a*b of the contraction is off by
        // ~4e-4 rms and C[d] by sigma_C = 4e-4 sqrt(sum_k a_k^2 b_k^2) <= 4e-4 sqrt(K/2 sum_g n_g^2) (n_g = pairs per delay
        // group, |PHAT sum of a group| <= n_g; b = cos / sin).  For a static source the error repeats from frame to frame,
        // so the 0.8 recursion does not average it: sigma_E = sigma_C.  A difference of two energies is decided at
        // 8 sigma plus head room: tau = 8 sqrt(2) 1.25 sigma_C, in units of the normalised energy En = (E + 15 P) / (30 P).
        // Calibration (tools/adaptive_check.py, 60 random configurations, 1e9 map values): the largest |E_fp16 - E_fp16x3|
        // seen is 0.42 tau (16-microphone ULA, static source), typically 0.2 tau.
        double sum_n2 = 0;
        if (c->ula) for (int g = 0; g < c->G; ++g) sum_n2 += (double)(c->M - 1 - g) * (c->M - 1 - g);
        else sum_n2 = c->P;
        const double sigma_c = 5.0e-4 * std::sqrt(0.5 * c->K * sum_n2);
        c->tau_en = (float)(c->kn.tau_scale * 8.0 * std::sqrt(2.0) * sigma_c / (30.0 * c->P));
    }

    std::vector<double> micx(c->M);
    for (int m = 0; m < c->M; ++m) micx[m] = c->xyz[3 * m];
    std::vector<float> win(c->N);
    for (int n = 0; n < c->N; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / c->N));   // periodic Hann
    std::vector<float2> twv(c->N / 2);
    for (int i = 0; i < c->N / 2; ++i) twv[i] = make_float2((float)std::cos(2.0 * M_PI * i / c->N), (float)(-std::sin(2.0 * M_PI * i / c->N)));
    const size_t na = (size_t)cfg->max_arrays;
    hipError_t e;
    if ((e = c->d_window.upload(win.data(), win.size())) || (e = c->d_tw.upload(twv.data(), twv.size())) || (e = c->d_grid.upload(c->grid.data(), c->grid.size())) ||
        (e = c->d_delays.upload(c->delays.data(), c->delays.size())) || (e = c->d_micx.upload(micx.data(), micx.size())) ||
        (e = c->d_pairs.upload(c->pairs.data(), c->pairs.size())) ||
        // the state: every array at exactly its state size (state_parts hands the buffers' own sizes to the blob code)
        (e = c->d_gate_state.alloc_zero(na * 4)) || (e = c->d_last_bin.alloc_zero(na * MCA_MAX_SOURCES)) ||
        (e = c->d_last_rad.alloc_zero(na * MCA_MAX_SOURCES)) || (e = c->d_last_prob.alloc_zero(na * MCA_MAX_SOURCES)) ||
        (e = c->d_silence.alloc_zero(na)) || (e = c->d_g2_post0.alloc_zero(na)) ||
        (e = c->d_rstats.alloc_zero(4)) ||
        (e = c->d_res.alloc_zero(2 * MCA_MAX_SOURCES + 1)) || (e = c->d_bins.alloc_zero(MCA_MAX_SOURCES)) ||
        (e = c->d_g2f_res.alloc_zero(4))) return hip_fail(c, e, "device memory for the tables and the state of the context");
    for (int i = 0; i < 2; ++i)
        if ((e = c->d_E[i].alloc_zero(na * c->D)) || (e = c->d_tail[i].alloc_zero(na * c->S * c->H)) || (e = c->d_doa[i].alloc_zero(na)) ||
            (e = c->d_vdone[i].alloc_zero(na)) || (e = c->d_E64[i].alloc_zero(c->D)) || (e = c->d_g2f_corr[i].alloc_zero(c->D)) ||
            (lazy_context(c) && ((e = c->d_hist_pcm[i].alloc_zero(na * c->M * HIST_SAMPLES)) || (e = c->d_hist_C[i].alloc_zero(na * HIST_FRAMES * c->Dp)) ||
                                 (e = c->d_ehist[i].alloc_zero(na * c->D))))) return hip_fail(c, e, "device memory for the double-buffered state of the context");
    if (c->prec == MCA_HIP_SRP_ADAPTIVE && c->kn.fb_enabled) {
        if (hipHostMalloc((void **)&c->h_probe, FB_RING * 32, hipHostMallocDefault) == hipSuccess) std::memset(c->h_probe, 0, FB_RING * 32);
        else { c->h_probe = nullptr; (void)hipGetLastError(); }                    // (no page-locked memory: the mode never backs off)
    }
    int rc;
    if (c->stream_ok && ((rc = build_steering_table(c)) || (rc = build_merged_tables(c)))) return rc;
    return init_last_state(c, nullptr);
}

int mca_hip_create(const mca_hip_config *cfg, mca_hip_ctx **out)
{
    if (!cfg || !out) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "cfg/out is NULL");
    *out = nullptr;
    // Callers built against an earlier header pass its size: round 2 ended before gcc_weighting (PHAT), round 3 behind it -- that
    // struct was 60 bytes of fields padded to 64, and the padding is not read -- and the fields appended since default to zero.
    constexpr int size_r2 = (int)offsetof(mca_hip_config, gcc_weighting), size_r3 = (size_r2 + 4 + 7) / 8 * 8;
    static_assert(size_r3 <= (int)offsetof(mca_hip_config, adaptive_min_rows), "round-3 struct size");
    if (cfg->struct_size != (int)sizeof(mca_hip_config) && cfg->struct_size != size_r2 && cfg->struct_size != size_r3)
        return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "struct_size mismatch");
    mca_hip_config cfg_full{};
    std::memcpy(&cfg_full, cfg, cfg->struct_size == size_r3 ? (size_t)offsetof(mca_hip_config, adaptive_fallback) : (size_t)cfg->struct_size);
    cfg_full.struct_size = (int)sizeof(mca_hip_config);
    cfg = &cfg_full;
    if (cfg->gcc_weighting != MCA_HIP_GCC_PHAT && cfg->gcc_weighting != MCA_HIP_GCC_NONE)
        return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "gcc_weighting must be MCA_HIP_GCC_PHAT or MCA_HIP_GCC_NONE");
    if (cfg->gcc_weighting == MCA_HIP_GCC_NONE && cfg->srp_precision != MCA_HIP_SRP_FP32)
        return fail(NO_CTX, MCA_HIP_ERR_UNSUPPORTED, "gcc_weighting NONE needs srp_precision MCA_HIP_SRP_FP32 (un-normalised spectra do not fit fp16 operands)");
    if (cfg->n_mics < 2 || cfg->n_mics > MCA_MAX_MICS) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "n_mics must be in [2,16]");
    if (!cfg->mic_xyz) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "mic_xyz is NULL");
    if (cfg->n_sources < 1 || cfg->n_sources > MCA_MAX_SOURCES) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "n_sources must be in [1,4]");
    if (cfg->fft_size < 16 || (cfg->fft_size & 1) || cfg->fft_size > 8192) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "fft_size must be even, 16..8192");
    if (cfg->sample_rate <= 0) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "sample_rate <= 0");
    if (!(cfg->doa_step_deg > 0) || cfg->doa_step_deg > 45) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "doa_step_deg must be in (0,45]");
    if (cfg->srp_precision < 0 || cfg->srp_precision > 3) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "bad srp_precision");
    if (cfg->max_arrays < 1) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "max_arrays < 1");
    if (cfg->adaptive_fallback != MCA_HIP_ADAPT_FALLBACK_AUTO && cfg->adaptive_fallback != MCA_HIP_ADAPT_FALLBACK_OFF)
        return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "adaptive_fallback must be MCA_HIP_ADAPT_FALLBACK_AUTO or _OFF");
    if (cfg->adaptive_min_rows < 0 || cfg->adaptive_max_sources < 0) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "adaptive_min_rows / adaptive_max_sources < 0");

    if (const int rc = check_device(NO_CTX, cfg->device)) return rc;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return fail(NO_CTX, MCA_HIP_ERR_HIP, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(NO_CTX, MCA_HIP_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");

    mca_hip_ctx *c = new mca_hip_ctx();
    const int rc = init_ctx(c, cfg, prop);
    if (rc) return create_failed(c, rc, free_ctx);
    *out = c;
    return MCA_HIP_OK;
}

static void graph_drop_recordings(mca_hip_graph *g);
static void graph_orphan(mca_hip_graph *g);

void mca_hip_destroy(mca_hip_ctx *ctx)
{
    destroy_ctx(ctx, [](mca_hip_ctx *c) {
        // graphs that outlive their context: their recordings point into this context's buffers, so they go now; the handle
        // stays valid for mca_hip_graph_destroy and fails cleanly in mca_hip_graph_launch
        for (mca_hip_graph *g : c->graphs) graph_orphan(g);
        c->graphs.clear();
        free_ctx(c);
    });
}

int mca_hip_num_steps(const mca_hip_ctx *c) { return c ? c->D : MCA_HIP_ERR_INVALID_ARGUMENT; }
int mca_hip_num_pairs(const mca_hip_ctx *c) { return c ? c->P : MCA_HIP_ERR_INVALID_ARGUMENT; }
int mca_hip_num_groups(const mca_hip_ctx *c) { return c ? c->G : MCA_HIP_ERR_INVALID_ARGUMENT; }

int mca_hip_get_pair_delays(const mca_hip_ctx *c, float *out)
{
    if (!c || !out) return MCA_HIP_ERR_INVALID_ARGUMENT;
    std::memcpy(out, c->delays.data(), c->delays.size() * sizeof(float));
    return MCA_HIP_OK;
}

int mca_hip_get_doa_grid(const mca_hip_ctx *c, float *out)
{
    if (!c || !out) return MCA_HIP_ERR_INVALID_ARGUMENT;
    std::memcpy(out, c->grid.data(), c->grid.size() * sizeof(float));
    return MCA_HIP_OK;
}

// the DOA tracker as mca_hip_gcc2_tracker_attach leaves it: no track anywhere, _currentDOA = 0, _prob = -1
// (x, sd, si: the context's own, or the buffers mca_hip_gcc2_tracker_attach is about to hand over)
static int trk_init_state(mca_hip_ctx *c, const DevBuf<double> &x, const DevBuf<double> &sd_dev, const DevBuf<int> &si, hipStream_t st)
{
    const size_t slots = (size_t)c->cfg.max_arrays + 1;
    std::vector<double> sd(slots * 2);
    for (size_t i = 0; i < slots; ++i) { sd[i * 2] = 0.0; sd[i * 2 + 1] = -1.0; }
    HIP_TRY(c, x.zero_async(st));
    HIP_TRY(c, si.zero_async(st));
    HIP_TRY(c, hipMemcpyAsync(sd_dev, sd.data(), sd_dev.bytes(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return MCA_HIP_OK;
}
static int trk_init_state(mca_hip_ctx *c, hipStream_t st) { return trk_init_state(c, c->d_trk_x, c->d_trk_sd, c->d_trk_si, st); }

int mca_hip_reset(mca_hip_ctx *c, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(c, c->d_E[i].zero_async(st));
        HIP_TRY(c, c->d_tail[i].zero_async(st));
        HIP_TRY(c, c->d_E64[i].zero_async(st));
        HIP_TRY(c, c->d_g2f_corr[i].zero_async(st));
        HIP_TRY(c, c->d_doa[i].zero_async(st));
        HIP_TRY(c, c->d_vdone[i].zero_async(st));
    }
    HIP_TRY(c, c->d_silence.zero_async(st));
    c->adapt_suspended = false; c->fb_state = 0; c->fb_left = 0; c->fb_backoff = 8; c->cand_heavy = false;     // new streams: the adaptive mode starts afresh
    c->fb_lost = false; c->fb_seq_seen = c->fb_calls;                                                          // (reports still in flight belong to the old streams)
    c->hist_pending = false;                                                              // ... and no call owes the next one its last rows
    // the self-cleaning words of the adaptive path (a call that failed half way may have left some set)
    Workspace &w = c->ws;
    HIP_TRY(c, w.d_need.zero_async(st));
    HIP_TRY(c, w.d_umask.zero_async(st));
    if (w.d_chunk_from) HIP_TRY(c, hipMemsetAsync(w.d_chunk_from, 0x7f, w.d_chunk_from.bytes() / 2, st));
    HIP_TRY(c, w.d_nlist.zero_async(st));
    if (c->d_steer_pred) HIP_TRY(c, hipMemsetAsync(c->d_steer_pred, 0xff, c->d_steer_pred.bytes(), st));      // no pick yet: bin -1, the initial DOA
    if (c->d_steer_mlist) { HIP_TRY(c, hipMemsetAsync(c->d_steer_mlist, 0, 4, st)); c->steer_mlist_dirty = false; }   // (a call that failed half way may have left misses listed)
    c->steer_spec = true; c->steer_lost = false; c->steer_seq_seen = c->steer_seq;              // (reports still in flight belong to the old streams)
    c->gcc2_frames_done = 0;
    c->g2f = G2FrameState();                                                              // the frame hook as a newly built module
    if (c->tracked) { const int rc = trk_init_state(c, st); if (rc) return rc; }          // every track forgotten: track numbers start at 1 again
    return init_last_state(c, st);
}

extern "C++" {
namespace {

struct StateHeader {
    unsigned magic; int version, M, D, S, H, max_arrays, use_floor;
    unsigned delays_hash;            // FNV-1a of the float delay tables: geometry + sample rate + grid
    long long gcc2_frames_done;
};
constexpr unsigned STATE_MAGIC = 0x4d434153u;   // "MCAS"
constexpr int STATE_VERSION = 3;                // 2: + _silenceFramesCounter per array; 3: + the FreqGCC frame hook (frame_part_bytes)
constexpr int STATE_VERSION_TRACKED = 4;        // 3 + the DOA tracker's part (tracker_part_bytes), written by contexts with a tracker only

unsigned delays_hash(const mca_hip_ctx *c)
{
    unsigned h = 2166136261u;
    const unsigned char *p = reinterpret_cast<const unsigned char *>(c->delays.data());
    for (size_t i = 0; i < c->delays.size() * sizeof(float); ++i) { h ^= p[i]; h *= 16777619u; }
    return h;
}

// the device buffers that make up the state, in blob order (current halves of the double buffers)
struct StatePart { void *ptr; size_t bytes; };
std::vector<StatePart> state_parts(mca_hip_ctx *c)
{
    // (every one of them is allocated at exactly its state size, init_ctx: the buffer's own size is the part's)
    auto part = [](const auto &b) { return StatePart{b.p, b.bytes()}; };
    return {
        part(c->d_E[c->e_cur]), part(c->d_tail[c->tail_cur]), part(c->d_gate_state),
        part(c->d_last_bin), part(c->d_last_rad), part(c->d_last_prob),
        part(c->d_doa[c->doa_cur]), part(c->d_E64[c->e64_cur]), part(c->d_vdone[c->doa_cur]),
        part(c->d_silence),
        part(c->d_g2f_corr[c->g2f_cur]),     // version 3: the frame hook's correlation, then its scalars (host side)
    };
}

// the part a version-3 blob ends with: the frame hook's double correlation [D], then G2FrameState as 8 doubles
size_t frame_part_bytes(const mca_hip_ctx *c) { return (size_t)c->D * 8 + sizeof(G2FrameState); }
static_assert(sizeof(G2FrameState) == 8 * sizeof(double), "G2FrameState is the 8 doubles of the blob");

// the part a version-4 blob ends with: the tracker's configuration, then for the max_arrays arrays and the frame hook
// alive / track / upd / 0 as int[4], DOA / prob as double[2], the particles double[N] (three arrays, in this order)
struct TrackerBlobHead { int n_particles, n_inject; unsigned long long seed; double sigma_init, sigma_step; };
static_assert(sizeof(TrackerBlobHead) == 32, "TrackerBlobHead is 32 bytes of the blob");
std::vector<StatePart> tracker_parts(const mca_hip_ctx *c)
{
    return {{c->d_trk_si.p, c->d_trk_si.bytes()}, {c->d_trk_sd.p, c->d_trk_sd.bytes()}, {c->d_trk_x.p, c->d_trk_x.bytes()}};
}
size_t tracker_part_bytes(const mca_hip_ctx *c)
{
    if (!c->tracked) return 0;
    size_t n = sizeof(TrackerBlobHead);
    for (const StatePart &p : tracker_parts(c)) n += p.bytes;
    return n;
}

}  // namespace
}  // extern "C++"

long long mca_hip_state_size(const mca_hip_ctx *c)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    long long n = sizeof(StateHeader) + (long long)sizeof(G2FrameState);
    for (const StatePart &p : state_parts(const_cast<mca_hip_ctx *>(c))) n += (long long)p.bytes;
    return n + (long long)tracker_part_bytes(c);
}

int mca_hip_state_save(mca_hip_ctx *c, void *blob, long long blob_bytes)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!blob || blob_bytes < mca_hip_state_size(c)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "state blob is NULL or smaller than mca_hip_state_size()");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (c->hist_pending) {                        // lazy tails: the blob holds the exact state, as the eager form's would
        HIP_TRY(c, hipDeviceSynchronize());
        const int rc = settle_history(c, nullptr);
        if (rc) return rc;
    }
    HIP_TRY(c, hipDeviceSynchronize());
    StateHeader h{STATE_MAGIC, c->tracked ? STATE_VERSION_TRACKED : STATE_VERSION, c->M, c->D, c->S, c->H, c->cfg.max_arrays, c->cfg.use_power_floor, delays_hash(c), c->gcc2_frames_done};
    unsigned char *out = static_cast<unsigned char *>(blob);
    std::memcpy(out, &h, sizeof(h)); out += sizeof(h);
    for (const StatePart &p : state_parts(c)) { HIP_TRY(c, hipMemcpy(out, p.ptr, p.bytes, hipMemcpyDeviceToHost)); out += p.bytes; }
    std::memcpy(out, &c->g2f, sizeof(G2FrameState)); out += sizeof(G2FrameState);
    if (c->tracked) {
        const TrackerBlobHead th{c->trk.n_particles, c->trk.n_inject, c->trk.seed, c->trk.sigma_init, c->trk.sigma_step};
        std::memcpy(out, &th, sizeof(th)); out += sizeof(th);
        for (const StatePart &p : tracker_parts(c)) { HIP_TRY(c, hipMemcpy(out, p.ptr, p.bytes, hipMemcpyDeviceToHost)); out += p.bytes; }
    }
    return MCA_HIP_OK;
}

int mca_hip_state_load(mca_hip_ctx *c, const void *blob, long long blob_bytes)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!blob || blob_bytes < (long long)sizeof(StateHeader)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "state blob is NULL or truncated");
    StateHeader h;
    std::memcpy(&h, blob, sizeof(h));
    // version 1 blobs end before the _silenceFramesCounter part (the change of version 2): they load with the counters at zero;
    // version 1 and 2 blobs end before the frame hook's part (the change of version 3): they load with a fresh frame hook
    // version 4 = version 3 + the DOA tracker's part: only a context with the same tracker loads it; older blobs load into a
    // context with a tracker and leave every track unstarted
    if (h.magic != STATE_MAGIC || h.version < 1 || h.version > STATE_VERSION_TRACKED) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "not a state blob of this library version");
    if (h.M != c->M || h.D != c->D || h.S != c->S || h.H != c->H || h.max_arrays != c->cfg.max_arrays || h.use_floor != c->cfg.use_power_floor ||
        h.delays_hash != delays_hash(c))
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "state blob was saved by a context with a different configuration");
    if (h.version == STATE_VERSION_TRACKED && !c->tracked)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "state blob was saved by a context with a DOA tracker (mca_hip_gcc2_tracker_attach first)");
    if (h.version == STATE_VERSION_TRACKED) {      // the tracker's configuration first: nothing is loaded from a blob that does not fit
        long long at = sizeof(StateHeader) + sizeof(G2FrameState);
        for (const StatePart &p : state_parts(c)) at += (long long)p.bytes;
        TrackerBlobHead th;
        if (blob_bytes < at + (long long)sizeof(th)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "state blob is truncated");
        std::memcpy(&th, static_cast<const unsigned char *>(blob) + at, sizeof(th));
        if (th.n_particles != c->trk.n_particles || th.n_inject != c->trk.n_inject || th.seed != c->trk.seed ||
            th.sigma_init != c->trk.sigma_init || th.sigma_step != c->trk.sigma_step)
            return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "state blob was saved by a context with a different DOA tracker configuration");
    }
    const long long short_by = (h.version == 1 ? (long long)c->cfg.max_arrays * 4 : 0) +         // bytes of the parts an older blob lacks
                               (h.version < 3 ? (long long)frame_part_bytes(c) : 0) +
                               (h.version < STATE_VERSION_TRACKED ? (long long)tracker_part_bytes(c) : 0);
    if (blob_bytes < mca_hip_state_size(c) - short_by) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "state blob is truncated");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipDeviceSynchronize());
    const unsigned char *in = static_cast<const unsigned char *>(blob) + sizeof(h);
    for (const StatePart &p : state_parts(c)) {
        if (h.version == 1 && p.ptr == c->d_silence.p) { HIP_TRY(c, hipMemset(p.ptr, 0, p.bytes)); continue; }
        if (h.version < 3 && p.ptr == c->d_g2f_corr[c->g2f_cur].p) { HIP_TRY(c, hipMemset(p.ptr, 0, p.bytes)); continue; }
        HIP_TRY(c, hipMemcpy(p.ptr, in, p.bytes, hipMemcpyHostToDevice)); in += p.bytes;
    }
    if (h.version >= 3) { std::memcpy(&c->g2f, in, sizeof(G2FrameState)); in += sizeof(G2FrameState); }
    else c->g2f = G2FrameState();
    if (c->tracked) {
        if (h.version == STATE_VERSION_TRACKED) {
            in += sizeof(TrackerBlobHead);          // (checked above)
            for (const StatePart &p : tracker_parts(c)) { HIP_TRY(c, hipMemcpy(p.ptr, in, p.bytes, hipMemcpyHostToDevice)); in += p.bytes; }
        } else {
            const int rc = trk_init_state(c, nullptr);
            if (rc) return rc;
        }
    }
    c->gcc2_frames_done = h.gcc2_frames_done;
    c->hist_pending = false;                      // (a blob holds the exact state)
    return MCA_HIP_OK;
}

// the workspace of a call of n_arrays x n_frames
static int steer_reserve(mca_hip_ctx *c, int n_arrays, int n_frames);
static int reserve_impl(mca_hip_ctx *c, int n_arrays, int n_frames)
{
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int n_chunks = (n_frames + SCAN_CHUNK - 1) / SCAN_CHUNK;
    int rc;
    if (c->prec == MCA_HIP_SRP_ADAPTIVE && adaptive_shape(c, n_arrays, n_frames)) {
        // by the SHAPE of the call, whatever the back-off is doing at the moment: a graph recording always runs coarse + repair
        // (graph_record clears adapt_suspended), and reserving for plain FP16X3 only would make it allocate inside the capture
        // (ADVICE r3).  While the mode is suspended the eager calls run as FP16X3: their two-plane rows are reserved as well.
        const RowLayout coarse = row_layout(c, 1);
        if ((rc = ensure_adapt_workspace(c, n_arrays, n_frames, n_chunks))) return rc;
        const long long fc1 = chunk_frames_for(c, coarse, n_arrays, n_frames);
        if ((rc = ensure_workspace(c, coarse, (long long)n_arrays * fc1, (long long)n_arrays * fc1, (long long)n_arrays * n_frames))) return rc;
        if (!c->adapt_suspended) return ensure_scan_workspace(c, n_arrays, n_frames, n_chunks);
    }
    const RowLayout lay = row_layout(c, c->tab_planes);      // the context's own rows: two planes for FP16X3 and for ADAPTIVE calls that run as FP16X3
    long long fc = chunk_frames_for(c, lay, n_arrays, n_frames);
    rc = ensure_workspace(c, lay, (long long)n_arrays * fc, (long long)n_arrays * fc, (long long)n_arrays * n_frames);
    if (rc) return rc;
    return ensure_scan_workspace(c, n_arrays, n_frames, n_chunks);
}

int mca_hip_reserve(mca_hip_ctx *c, int n_arrays, int n_frames)
{
    if (!c || n_arrays < 1 || n_frames < 1) return MCA_HIP_ERR_INVALID_ARGUMENT;
    const int rc = reserve_impl(c, n_arrays, n_frames);
    return rc ? rc : steer_reserve(c, n_arrays, n_frames);      // (the rows of Y of a context that steers on the half spectrum)
}

// STFT + PHAT + steering contraction for every frame, on rows of the layout `lay`: fills c->ws.d_C [arrays][n_frames][Dp], call.map says how
static int run_correlation_map(mca_hip_ctx *c, StreamCall &call, const RowLayout &lay, const float *pcm, long long array_stride, long long mic_stride,
                               int n_arrays, int n_frames, hipStream_t st)
{
    int rc;
    const long long fc = chunk_frames_for(c, lay, n_arrays, n_frames);
    auto plan = [&](long long rows) { return plan_gemm(*c, lay.planes, call.planned(rows)); };
    if ((rc = ensure_workspace(c, lay, (long long)n_arrays * fc, call.planned((long long)n_arrays * fc), (long long)n_arrays * n_frames))) return rc;
    if ((rc = ensure_scan_workspace(c, n_arrays, n_frames, (n_frames + SCAN_CHUNK - 1) / SCAN_CHUNK))) return rc;
    // The 256 x 384 contraction leaves the chunk-local results of the scan over frames (k_scan_partial's job) when every
    // 32-row block of every launch is one scan chunk of one map: no gate, one map, whole chunks, that kernel for every slice.
    bool fused_partial = SCAN_CHUNK == 32 && lay.planes == 1 && !c->cfg.use_power_floor && n_frames % SCAN_CHUNK == 0 && fc % SCAN_CHUNK == 0 &&
                         plan((long long)n_arrays * fc).ksplit <= 2;
    for (int f0 = 0; fused_partial && f0 < n_frames; f0 += (int)fc)
        fused_partial = plan((long long)n_arrays * std::min<long long>(fc, n_frames - f0)).v2;
    MapResult &map = call.map;
    map.partial_done = fused_partial;
    map.part_planes = fused_partial ? plan((long long)n_arrays * fc).ksplit : 1;
    for (int f0 = 0; f0 < n_frames; f0 += (int)fc) {
        const int nf = (int)std::min<long long>(fc, n_frames - f0);
        StftPhatArgs sa{};
        sa.pcm = pcm; sa.array_stride = array_stride; sa.mic_stride = mic_stride;
        stft_common(c, sa);
        sa.n_frames = nf; sa.frame0 = f0;
        sa.power = c->cfg.use_power_floor ? c->ws.d_power : nullptr; sa.total_frames = n_frames;
        sa.A = a_buf(c, lay); sa.a_row_elems = lay.row_elems; sa.a_planes = lay.planes;
        if (c->merged && lay.planes == 1) { sa.mrank = c->d_mrank; sa.n_merged = c->n_merged; sa.planar = c->fold ? 1 : 0; }
        sa.no_phat = c->cfg.gcc_weighting == MCA_HIP_GCC_NONE ? 1 : 0;
        if (c->prec == MCA_HIP_SRP_ADAPTIVE && lay.planes == 1 && wave16_applies(*c)) sa.unsure = c->ws.d_unsure;   // (adaptive coarse pass)
        if (call.lazy && cand_call(c, true)) sa.dead = c->ws.d_unsure;                                                 // (... of a candidate-column call: frames of exact zeros)
        if (call.lazy) sa.hist_out = c->d_hist_pcm[c->hist_cur ^ 1];         // lazy tails: the call's last frames of PCM stay behind
        if (call.steer && sa.mrank && !sa.power) {                            // the merged 8-microphone kernel also steers every frame at the array's predicted bin
            sa.bf.rows = c->d_steer_rows; sa.bf.q = c->d_steer_q; sa.bf.nyq = c->d_steer_nyq; sa.bf.pred = c->d_steer_pred + call.a0; sa.bf.Y = c->d_steer_Y;
        }
        AnalysisFlags fl;
        fl.power = sa.power != nullptr; fl.merged = sa.mrank != nullptr; fl.steer = sa.bf.rows != nullptr; fl.no_phat = sa.no_phat != 0;
        const AnalysisPlan ap = plan_analysis(*c, c->prec == MCA_HIP_SRP_FP32, lay.planes, n_arrays, nf, 0, 0, fl);
        time_begin(c, call, MCA_HIP_K_STFT_PHAT, st);
        rc = launch_analysis(c, sa, ap, st);
        if (ap.steers) call.steer_fused = true;
        time_end(c, st);
        if (rc) return rc;

        GemmArgs ga{};
        const bool mg = c->merged && lay.planes == 1;
        ga.A = a_buf(c, lay); ga.B = mg ? c->d_Bm : c->d_B; ga.C = c->ws.d_C; ga.Bt = mg ? c->d_Btm : c->d_Bt;
        ga.rows = n_arrays * nf; ga.chunk_frames = nf; ga.total_frames = n_frames; ga.frame0 = f0;
        ga.Kp = lay.kp; ga.Dp = c->Dp; ga.a_row_elems = lay.row_elems;
        ga.c_plane_elems = (long long)n_arrays * n_frames * c->Dp;
        ga.Bf = mg ? c->d_Bfold : nullptr; ga.D = c->D;
        if (fused_partial) {
            ga.part = c->ws.d_part; ga.nvoiced = c->ws.d_nv; ga.D = c->D; ga.n_chunks = n_frames / SCAN_CHUNK;
            ga.part_plane_stride = (long long)n_arrays * ga.n_chunks * c->D;
            ga.scan_w[31] = 1 - 0.8f;                                              // as pa.one_minus_mu / pa.mu below
            for (int t = 30; t >= 0; --t) ga.scan_w[t] = ga.scan_w[t + 1] * 0.8f;
        }
        const ContractionPlan gp = plan_contraction(*c, lay.planes, ga.rows, call.planned(ga.rows), call.planned((long long)n_arrays * fc));
        map.c_planes = gp.ksplit; map.c_plane = ga.c_plane_elems;
        const void *const one[] = {reinterpret_cast<const void *>(&k_srp_gemm_f32), nullptr, reinterpret_cast<const void *>(&k_srp_gemm_f16_v2),
                                   reinterpret_cast<const void *>(&k_srp_gemm_f16_v3), reinterpret_cast<const void *>(&k_srp_gemm_f16_fold)};      // (in the order of GemmFamily)
        const void *gk = gp.form.family == GemmFamily::F16 ? srp_gemm_f16_kernel(gp.form.split, gp.form.bn) : one[(int)gp.form.family];
        time_begin(c, call, MCA_HIP_K_SRP_GEMM, st);
        rc = launch(c, gk, gp.grid, gp.block, gp.lds, &ga, st, "k_srp_gemm_f16");
        time_end(c, st);
        if (rc) return rc;
    }
    if (map.c_planes > 2) {      // deep split-K of a small batch: fold the partial maps once, the scans read one map
        const long long n4 = map.c_plane / 4;       // Dp is a multiple of 64
        time_begin(c, call, MCA_HIP_K_FOLD, st);
        hipLaunchKernelGGL(k_sum_planes, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, c->ws.d_C, n4, map.c_planes, map.c_plane);
        time_end(c, st);
        HIP_TRY(c, hipGetLastError());
        map.c_planes = 1;
    }

    return MCA_HIP_OK;
}

// _energyMemoryFactor and its float complement (SteeringBeamforming.h:70, .cpp:134,139: float arithmetic) -- one place for every launch
constexpr float ENERGY_MU = 0.8f, ENERGY_ONE_MINUS_MU = 1 - 0.8f;

// One pass of the whole-row repair behind the list-mode analysis: the exact rows of the listed units [list0, list0 + pass_rows /
// REPAIR_GROUP) in w.d_Ax -> three-product contraction in K segments (w.d_Cx) -> summed into the map by k_repair_patch (pp: where the
// rows go; list0, pass_rows, col_tiles, ksplit and items are filled in here).  Shared by localise_impl and settle_history.
// x2: the two-plane layout of the exact rows; ksplit_arrays: the arrays the K split is planned for (repair_ksplit_for)
static int launch_repair_contraction(mca_hip_ctx *c, Workspace &w, const RowLayout &x2, long long list0, long long pass_rows, int ksplit_arrays, RepairPatchArgs pp, hipStream_t st)
{
    GemmArgs ga{};
    ga.A = w.d_Ax; ga.B = c->d_B; ga.C = w.d_Cx; ga.Bt = c->d_Bt;
    ga.rows = (int)pass_rows; ga.chunk_frames = (int)pass_rows; ga.total_frames = (int)pass_rows; ga.frame0 = 0;
    ga.Kp = c->Kp; ga.Dp = c->Dp; ga.a_row_elems = x2.row_elems; ga.c_plane_elems = pass_rows * c->Dp;
    ga.n_list = w.d_nlist; ga.list0 = (int)list0;
    ga.repair_ksplit = repair_ksplit_for(c, ksplit_arrays); ga.repair_items = REPAIR_ITEMS;
    const RepairContractionPlan rp = plan_repair_contraction(*c, pass_rows, ga.repair_ksplit);
    int rc;
    if ((rc = launch(c, srp_gemm_repair_kernel(rp.bn), rp.grid, rp.block, 0, &ga, st, "k_srp_gemm_repair"))) return rc;
    pp.Cx = w.d_Cx; pp.pass_rows = (int)pass_rows; pp.col_tiles = rp.col_tiles; pp.ksplit = ga.repair_ksplit; pp.items = ga.repair_items;
    pp.list = w.d_list; pp.n_list = w.d_nlist; pp.list0 = (int)list0; pp.need = w.d_need; pp.Dp = c->Dp;
    return launch(c, reinterpret_cast<const void *>(&k_repair_patch), rp.patch_grid, rp.patch_block, 0, &pp, st, "k_repair_patch");
}

// Lazy tails (mca_internal.h, HIST_FRAMES): the repair of a call's last rows is left to the call that needs them.  Settling the debt --
// for every consumer of the state that is not the next lazy call itself (an FP16X3 call of the same context, another array count,
// state_save, a recorded graph): the previous call's last HIST_FRAMES rows of EVERY array are recomputed exactly from the kept PCM (the
// repair pass's own kernels on a list of all history units) and the state becomes what the eager form would have left.
static int settle_history(mca_hip_ctx *c, hipStream_t st)
{
    if (!c->hist_pending) return MCA_HIP_OK;
    const int n = c->hist_n, units = n * HIST_UNITS, rows = units * REPAIR_GROUP, cur = c->hist_cur;
    Workspace &w = c->ws;
    if (!w.d_list || !w.d_need || !w.d_nlist || !w.d_Ax || !w.d_Cx) return fail(c, MCA_HIP_ERR_HIP, "lazy tails: the adaptive workspace is gone");
    // The workspace was sized by the lazy call that left the debt (ensure_adapt_workspace: repair_pass_rows of its shape, capped by the
    // budget, MCA_HIP_WS_MAX_MB); the history's rows go through it in passes of at most that many rows, as localise_impl's do (ADVICE r5:
    // one pass of all of them wrote past d_Ax / d_Cx when the budget was small and the arrays many).
    const int ksplit = repair_ksplit_for(c, n);
    long long pass_rows = std::min<long long>((rows + 127) / 128 * 128, repair_pass_rows(c, n, HIST_FRAMES));
    const long long fit_a = (long long)(w.d_Ax.n / ((size_t)2 * c->Kp * 2)) / 128 * 128, fit_c = (long long)(w.d_Cx.bytes() / ((size_t)ksplit * c->Dp * 4)) / 128 * 128;
    pass_rows = std::min(pass_rows, std::min(fit_a, fit_c));
    if (pass_rows < 128) return fail(c, MCA_HIP_ERR_HIP, "lazy tails: the adaptive workspace is smaller than one repair pass");
    const int pass_groups = (int)(pass_rows / REPAIR_GROUP);
    const RowLayout x2 = row_layout(c, 2);
    hipLaunchKernelGGL(k_hist_list, dim3((units + 255) / 256), dim3(256), 0, st, w.d_list, w.d_nlist, w.d_need, units);
    int rc = MCA_HIP_OK;
    for (long long g0 = 0; g0 < units && !rc; g0 += pass_groups) {
        StftPhatArgs sa{};
        sa.pcm = c->d_hist_pcm[cur]; sa.array_stride = (long long)c->M * HIST_SAMPLES; sa.mic_stride = HIST_SAMPLES;
        stft_common(c, sa);
        sa.n_frames = HIST_FRAMES; sa.frame0 = 0; sa.total_frames = HIST_FRAMES;
        sa.A = w.d_Ax; sa.a_row_elems = x2.row_elems; sa.a_planes = 2;
        sa.list = w.d_list; sa.n_list = w.d_nlist; sa.list0 = (int)g0; sa.list_cap = pass_groups; sa.groups_per_array = HIST_UNITS;
        sa.hist_in = c->d_hist_pcm[cur]; sa.hist_base = 0;
        rc = launch_analysis(c, sa, plan_analysis(*c, false, 2, n, HIST_FRAMES, pass_groups, 512, AnalysisFlags{}), st);
        if (rc) break;
        RepairPatchArgs pp{};
        pp.groups_per_array = HIST_UNITS;
        pp.C = w.d_C; pp.c_planes = 1; pp.c_plane_stride = 0; pp.n_frames = HIST_FRAMES;
        pp.hist_C = c->d_hist_C[cur]; pp.hist_base = 0;
        rc = launch_repair_contraction(c, w, x2, g0, pass_rows, n, pp, st);
    }
    if (!rc) {
        hipLaunchKernelGGL(k_hist_settle, dim3(n), dim3(std::max(round_up(c->D, 64), 64)), 0, st, c->d_ehist[cur], c->d_hist_C[cur], c->d_E[c->e_cur], w.d_nlist, c->D, c->Dp,
                           ENERGY_MU, ENERGY_ONE_MINUS_MU);
        if (hipGetLastError() != hipSuccess) rc = fail(c, MCA_HIP_ERR_HIP, "lazy tails: a launch of the settling pass failed");
    }
    if (!rc) c->hist_pending = false;          // (only now: a settling pass that failed leaves the debt standing and is tried again by the next consumer -- ADVICE r5)
    return rc;
}

// the localisation stage of the arrays [call.a0, call.a0 + n_arrays) of a call; all pointers already point at the piece's first array
static int localise_impl(mca_hip_ctx *c, StreamCall &call, const float *pcm, long long array_stride, long long mic_stride,
                         int n_arrays, int n_frames, int *doa_bin, float *doa_rad, float *prob, float *energy, hipStream_t st)
{
    int rc;
    const size_t a0 = (size_t)call.a0;
    const bool adaptive = adaptive_applies(c, call, n_arrays, n_frames);
    // Lazy tails: this call leaves the exact repair of its last rows to the next one (lazy), and repairs the previous call's last rows
    // itself where one of its own first frames needs them (hist_valid).  Any other consumer of the state settles the debt first.
    const bool lazy = adaptive && call.may_lazy() && lazy_context(c) && call.a0 == 0 && n_frames >= 2 * SCAN_CHUNK && SCAN_CHUNK == 32;
    const bool hist_valid = lazy && c->hist_pending && c->hist_n == n_arrays;
    if (c->hist_pending && !hist_valid) {
        if (call.recording()) return fail(c, MCA_HIP_ERR_HIP, "lazy tails: a recording found an unsettled state (mca_hip_graph_launch settles it first)");
        if ((rc = settle_history(c, st))) return rc;
    }
    call.lazy = lazy;
    // the coarse pass of an adaptive call on one fp16 plane; every other call on the context's own rows (ADAPTIVE: as FP16X3)
    const RowLayout lay = row_layout(c, adaptive ? 1 : c->tab_planes), x2 = row_layout(c, 2);
    const int n_chunks = (n_frames + SCAN_CHUNK - 1) / SCAN_CHUNK;
    if (adaptive && (rc = ensure_adapt_workspace(c, n_arrays, n_frames, n_chunks))) return rc;
    if ((rc = run_correlation_map(c, call, lay, pcm, array_stride, mic_stride, n_arrays, n_frames, st))) return rc;
    const MapResult &map = call.map;

    const bool gate = c->cfg.use_power_floor != 0;
    time_begin(c, call, MCA_HIP_K_SCAN_PICK, st);
    if (gate) {
        GateArgs gg{};
        gg.power_lin = c->ws.d_power; gg.n_frames = n_frames; gg.fft_n = c->N;
        gg.needed_samples = (int)(3.0 * c->cfg.sample_rate);              // _durationToEstimatePowerFloor (SoundLocalisationImpl.h:77)
        gg.margin_db = 3.f;                                                // _noiseMarginDB (BeamformingSeparationAndLocalistaion.h:52)
        gg.state = c->d_gate_state + a0 * 4; gg.voiced = c->ws.d_voiced; gg.power_out = c->ws.d_power_out;
        hipLaunchKernelGGL(k_gate, dim3(n_arrays), dim3(256), 0, st, gg);
    }
    ScanPickArgs pa{};
    pa.C = c->ws.d_C; pa.c_planes = map.c_planes; pa.c_plane_stride = map.c_plane; pa.n_frames = n_frames; pa.Dp = c->Dp; pa.D = c->D; pa.P = c->P; pa.S = c->S;
    pa.chunk = SCAN_CHUNK; pa.n_chunks = n_chunks;
    pa.mu = ENERGY_MU; pa.one_minus_mu = ENERGY_ONE_MINUS_MU;                 // SteeringBeamforming.h:70, .cpp:134,139 (float arithmetic)
    pa.inv_norm = exact_reciprocal(30.f * (float)c->P);
    pa.state_in = c->d_E[c->e_cur] + a0 * c->D; pa.state_out = c->d_E[c->e_cur ^ 1] + a0 * c->D;
    pa.part_planes = map.partial_done ? map.part_planes : 1; pa.part_plane_stride = (long long)n_arrays * n_chunks * c->D;
    pa.part = c->ws.d_part; pa.nvoiced = c->ws.d_nv; pa.e_start = c->ws.d_estart; pa.voiced = gate ? c->ws.d_voiced : nullptr;
    pa.grid = c->d_grid; pa.doa_bin = doa_bin; pa.doa_rad = doa_rad; pa.prob = prob; pa.energy = energy;
    const int gpa = (n_frames + REPAIR_GROUP - 1) / REPAIR_GROUP;
    if (adaptive) {
        pa.mode = 1; pa.tau = c->tau_en; pa.flags = c->ws.d_flags; pa.groups_per_array = gpa;
        pa.need = c->ws.d_need; pa.list = c->ws.d_list; pa.n_list = c->ws.d_nlist; pa.chunk_from = c->ws.d_chunk_from; pa.last_vchunk = c->ws.d_last_vchunk; pa.stats = c->d_rstats;
        pa.unsure = wave16_applies(*c) ? c->ws.d_unsure : nullptr;
        pa.hist_base = n_arrays * gpa;
        if (lazy) { pa.lazy = 1; pa.hist_C_out = c->d_hist_C[c->hist_cur ^ 1]; pa.e_hist_out = c->d_ehist[c->hist_cur ^ 1]; }
        if (hist_valid) { pa.hist_valid = 1; pa.hist_C_in = c->d_hist_C[c->hist_cur]; pa.e_hist_in = c->d_ehist[c->hist_cur]; }
        if (cand_call(c, lazy)) { pa.umask = c->ws.d_umask; pa.umask_words = c->Dp / 32; pa.dead = c->ws.d_unsure; }   // (dead: the unsure bytes, unused by these contexts)
        pa.clist = c->ws.d_chunk_from + c->ws.d_chunk_from.n / 2; pa.n_clist = c->ws.d_nlist + 1;   // (+ 2: see ScanPickArgs)
        // steered tail: the analysis of this call steered every frame at its array's predicted bin, so the frames that miss it are patched inside
        // the second pick's launch (k_scan_repick<PL, true>) and steer_separate launches no k_steer_patch.  One batch of k_scan_pick per chunk
        // is what makes "no flagged frame in the batch" mean "the chunk's coarse picks are final".
        // (repick_may_patch: not the widest peak pick, and only while the patching launch's LDS fits a CU -- those calls keep the stand-alone k_steer_patch)
        if (call.steer && call.steer_fused && c->d_steer_mlist && SCAN_SUB == SCAN_CHUNK && c->S == 1 && !gate && (size_t)n_arrays * n_frames < c->d_steer_mlist.n &&
            repick_may_patch(*c)) {
            // the list is empty unless a call that listed misses never reached its synthesis (which empties it): an error in between
            if (c->steer_mlist_dirty) HIP_TRY(c, hipMemsetAsync(c->d_steer_mlist, 0, sizeof(int), st));
            c->steer_mlist_dirty = true;
            pa.n_miss = c->d_steer_mlist; pa.miss_cap = (int)((size_t)n_arrays * n_frames);
            SteerPatchArgs &sp = pa.sp;
            sp.pcm = pcm; sp.array_stride = array_stride; sp.mic_stride = mic_stride; sp.n_arrays = n_arrays; sp.n_frames = n_frames; sp.f0 = 0; sp.f1 = n_frames;
            sp.window = c->d_window; sp.doa_bin = doa_bin; sp.all = 0; sp.miss = c->d_steer_miss;
            sp.bf.rows = c->d_steer_rows; sp.bf.q = c->d_steer_q; sp.bf.nyq = c->d_steer_nyq; sp.bf.pred = c->d_steer_pred + a0; sp.bf.Y = c->d_steer_Y;
            sp.y_f0 = 0; sp.y_frames = n_frames;
            call.steer_patched = true;
        }
        if (c->h_probe && !call.recording()) {
            c->fb_frames_ring[c->fb_calls % FB_RING] = c->adapt_frames_total + (unsigned long long)n_arrays * n_frames;
            c->fb_launch_m[c->fb_calls % FB_RING] = c->fb_m > 0 ? c->fb_m - 1 : 0;       // (the eligible call this piece belongs to)
            pa.probe = c->h_probe + 4 * (c->fb_calls % FB_RING); pa.probe_seq = ++c->fb_calls;
        }
    }
    const int nthr = round_up(c->D, 64);
    dim3 g3(pa.n_chunks, n_arrays);
    if (!map.partial_done) hipLaunchKernelGGL(k_scan_partial, g3, dim3(round_up(c->Dp / 4, 64)), 0, st, pa);   // a thread per four delays
    // ungated calls: k_scan_pick composes its chunk's start value itself (the chunks further back than four have decayed below the
    // last bit); with the gate a chunk may hold no advancing frame at all and the composition runs over all of them, in order
    // The look-back drops g^4 E_{c-4} (g = 0.8^32: 3.9e-13 of E), which is below the last bit only while the map is bounded: under PHAT
    // |C| <= P whatever the level.  With gcc_weighting NONE the map scales with the amplitude squared, and after a loud passage that
    // falls to digital silence the exact recursion still carries the old peak for ~180 frames when the look-back has zeroed it
    // (ADVICE r3): NONE always runs the serial carry pass.
    pa.lookback = (!gate && !c->kn.scan_carry && c->cfg.gcc_weighting == MCA_HIP_GCC_PHAT) ? 4 : 0;
    if (!pa.lookback) hipLaunchKernelGGL(k_scan_carry, dim3(n_arrays, nthr / 64), dim3(64), 0, st, pa);   // one wave per 64 delays
    const PickPlan kp = plan_pick(*c, adaptive, n_arrays, pa.n_chunks);
    if ((rc = launch(c, scan_pick_kernel(kp.form), kp.grid, kp.block, kp.lds, &pa, st, "k_scan_pick"))) return rc;
    DoaFillArgs fa{};
    fa.voiced = c->ws.d_voiced; fa.n_frames = n_frames; fa.S = c->S;
    fa.doa_bin = doa_bin; fa.doa_rad = doa_rad; fa.prob = prob;
    fa.last_bin = c->d_last_bin + a0 * c->S; fa.last_rad = c->d_last_rad + a0 * c->S; fa.last_prob = c->d_last_prob + a0 * c->S;
    if (gate && !adaptive) hipLaunchKernelGGL(k_doa_fill, dim3(n_arrays), dim3(1024), 0, st, fa);   // (ADAPTIVE: after the second pick)
    time_end(c, st);
    HIP_TRY(c, hipGetLastError());
    if (adaptive) {
        // exact repair: list the row groups the flagged frames depend on, recompute them with the hi + lo operand planes and
        // the three-product contraction, patch them into the map, pick the flagged chunks again (k_scan_repick).
        // Every launch is sized for the worst case (all rows) and exits at the device-side count.
        time_begin(c, call, MCA_HIP_K_REPAIR, st);
        const long long pass_rows = repair_pass_rows(c, n_arrays, n_frames);
        const int pass_groups = (int)(pass_rows / REPAIR_GROUP);
        const long long all_groups = (long long)n_arrays * (gpa + (hist_valid ? HIST_UNITS : 0));     // (the list cannot be longer)
        for (long long g0 = 0; g0 < all_groups; g0 += pass_groups) {      // (the exact rows: two planes, x2)
            StftPhatArgs sa{};
            sa.pcm = pcm; sa.array_stride = array_stride; sa.mic_stride = mic_stride;
            stft_common(c, sa);
            sa.n_frames = n_frames; sa.frame0 = 0; sa.total_frames = n_frames;
            sa.A = c->ws.d_Ax; sa.a_row_elems = x2.row_elems; sa.a_planes = 2;
            sa.list = c->ws.d_list; sa.n_list = c->ws.d_nlist; sa.list0 = (int)g0; sa.list_cap = pass_groups; sa.groups_per_array = gpa;
            if (hist_valid) { sa.hist_in = c->d_hist_pcm[c->hist_cur]; sa.hist_base = n_arrays * gpa; }
            CandArgs ca{};
            if (pa.umask) {
                // candidate columns: the exact values where the flagged frames need them, straight into the map (no partial maps, no patch) --
                // by the workgroup that writes a unit's rows, inside the list-mode launch (4 / 8 microphones: k_stft_phat_wave)
                ca.A = c->ws.d_Ax; ca.B = c->d_B; ca.Kp = c->Kp; ca.Dp = c->Dp; ca.a_row_elems = x2.row_elems;
                ca.list = c->ws.d_list; ca.n_list = c->ws.d_nlist; ca.list0 = (int)g0; ca.pass_rows = (int)pass_rows;
                ca.umask = c->ws.d_umask; ca.umask_words = pa.umask_words; ca.need = c->ws.d_need; ca.groups_per_array = gpa; ca.n_frames = n_frames;
                ca.C = c->ws.d_C; ca.c_planes = map.c_planes; ca.c_plane_stride = map.c_plane;
                if (hist_valid) { ca.hist_C = c->d_hist_C[c->hist_cur]; ca.hist_base = n_arrays * gpa; }
                sa.cand_on = 1; sa.cand = ca;       // (pa.umask: cand_call, which requires a lazy call, so lazy_context, so M is 4 or 8 -- the list-mode launch contracts)
            }
            AnalysisFlags fl;
            fl.cand_on = sa.cand_on != 0;
            if ((rc = launch_analysis(c, sa, plan_analysis(*c, false, 2, n_arrays, n_frames, pass_groups, LIST_GRID, fl), st))) return rc;
            if (sa.cand_on) continue;
            RepairPatchArgs pp{};
            pp.groups_per_array = gpa;
            pp.C = c->ws.d_C; pp.c_planes = map.c_planes; pp.c_plane_stride = map.c_plane; pp.n_frames = n_frames;
            if (hist_valid) { pp.hist_C = c->d_hist_C[c->hist_cur]; pp.hist_base = n_arrays * gpa; }
            if ((rc = launch_repair_contraction(c, c->ws, x2, g0, pass_rows, call.planned_arrays(n_arrays), pp, st))) return rc;
        }
        const RepickPlan rk = plan_repick(*c, pa.n_miss != nullptr, n_arrays, pa.n_chunks);      // (n_miss: the launch also patches the steered rows)
        if ((rc = launch(c, scan_repick_kernel(rk.form), rk.grid, rk.block, rk.lds, &pa, st, "k_scan_repick"))) return rc;
        if (gate) hipLaunchKernelGGL(k_doa_fill, dim3(n_arrays), dim3(1024), 0, st, fa);   // gated-out frames repeat the last FINAL pick
        time_end(c, st);
        HIP_TRY(c, hipGetLastError());
        if (!call.recording()) c->adapt_frames_total += (unsigned long long)n_arrays * n_frames;      // (a recording processes no frame: mca_hip_graph_launch counts the replays)
    }
    if (lazy) { c->hist_cur ^= 1; c->hist_n = n_arrays; c->hist_pending = true; }
    else c->hist_pending = false;                // (settled above, or consumed by an eager adaptive call: its own last frame was repaired)
    return MCA_HIP_OK;
}

int mca_hip_get_repair_stats(mca_hip_ctx *c, unsigned long long *frames, unsigned long long *flagged_frames,
                             unsigned long long *recomputed_frames)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipDeviceSynchronize());
    unsigned long long st[2] = {0, 0};
    HIP_TRY(c, hipMemcpy(st, c->d_rstats, sizeof(st), hipMemcpyDeviceToHost));
    if (frames) *frames = c->adapt_frames_total;
    if (flagged_frames) *flagged_frames = st[0];
    if (recomputed_frames) *recomputed_frames = st[1] * REPAIR_GROUP;
    return MCA_HIP_OK;
}

int mca_hip_get_steer_stats(mca_hip_ctx *c, unsigned long long *frames, unsigned long long *missed_frames, unsigned long long *fused_calls)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipDeviceSynchronize());
    unsigned long long m = 0;
    if (c->d_steer_miss) HIP_TRY(c, hipMemcpy(&m, c->d_steer_miss, sizeof(m), hipMemcpyDeviceToHost));
    if (frames) *frames = c->steer_frames_total;
    if (missed_frames) *missed_frames = m;
    if (fused_calls) *fused_calls = c->steer_fused_calls;
    return MCA_HIP_OK;
}

int mca_hip_get_repair_columns(mca_hip_ctx *c, unsigned long long *candidate_columns, unsigned long long *whole_row_frames)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipDeviceSynchronize());
    unsigned long long st[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpy(st, c->d_rstats, sizeof(st), hipMemcpyDeviceToHost));
    if (candidate_columns) *candidate_columns = st[2];
    if (whole_row_frames) *whole_row_frames = st[3];
    return MCA_HIP_OK;
}

// steering rows of every grid angle (+ the initial DOA): allocated and built once, outside any capture.  Built into a local and handed
// to the context when the table kernel has run: d_bftab set means the table is there
static int ensure_bf_table(mca_hip_ctx *c)
{
    if (c->d_bftab || (!c->n2048 && !wave_beamformer_applies(*c))) return MCA_HIP_OK;
    // 2048-sample frames: a row per (angle, CHANNEL), [D + 1][M][1032] (k_beamform_wave_2048); else per channel pair, [D + 1][np][1024]
    const int np = c->n2048 ? c->M : (c->M + 1) / 2;
    DevBuf<float2> tab;
    const hipError_t e = tab.alloc((size_t)(c->D + 1) * np * (c->n2048 ? 1032 : 1024));
    if (e != hipSuccess) return hip_fail(c, e, "the beamformer's steering rows");
    const double unit = (double)c->cfg.sample_rate / (double)(c->n2048 ? c->N : FFT_N) / 346.1;     // Beamformer.cpp:59 without 2 pi
    if (c->n2048) hipLaunchKernelGGL(k_bf_table_2048, dim3(c->D + 1, c->M), dim3(256), 0, nullptr, tab.p, c->d_grid, c->d_micx, c->M, unit);
    else hipLaunchKernelGGL(k_bf_table, dim3(c->D + 1, np), dim3(256), 0, nullptr, tab.p, c->d_grid, c->d_micx, c->M, np, unit);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipDeviceSynchronize());
    c->d_bftab.swap(tab); c->bf_pairs = np;
    return MCA_HIP_OK;
}

// Delay-and-sum on the half spectrum of the separated channels (steer.h): device-pointer calls of the one-source, ungated 8-microphone ULA at
// 1024-sample frames whose coarse rows are the merged one-plane ones (ADAPTIVE, FP16).  Such a context ALWAYS takes this path for
// mca_hip_process_frames_dev -- whether a call's analysis steered ahead of the picks or not, its audio comes from the same routine.
static bool steer_applies(const mca_hip_ctx *c)
{
    return !c->generic && !c->n512 && !c->n2048 && c->N == FFT_N && c->M == 8 && c->ula && c->S == 1 && !c->cfg.use_power_floor && c->merged &&
           (c->prec == MCA_HIP_SRP_ADAPTIVE || c->prec == MCA_HIP_SRP_FP16) && c->cfg.gcc_weighting != MCA_HIP_GCC_NONE;
}

// frames of Y per pass: the whole call while its rows fit the workspace budget (MCA_HIP_WS_MAX_MB)
static int steer_pass_frames(const mca_hip_ctx *c, int n_arrays, int n_frames)
{
    const long long cap = ws_max_bytes(c) / ((long long)n_arrays * STEER_ROW * (long long)sizeof(float2));
    return (int)std::max<long long>(1, std::min<long long>(n_frames, cap));
}

// The guard for content that moves.  Call number s consumes the report of call s - FB_LAG (waiting for it if need be: the call in between is
// still queued behind it), so which call switches depends on the calls and their content only -- reproducible run to run, like the AUTO
// policy (adapt_policy_begin).  Without page-locked memory, or once a report stayed away for FB_WAIT_MS, every call steers ahead.
static void steer_policy_begin(mca_hip_ctx *c)
{
    const unsigned long long s = c->steer_seq + 1;                              // this call
    if (!c->h_steer || c->steer_lost || s <= FB_LAG) return;
    const unsigned long long r = s - FB_LAG;
    if (r <= c->steer_seq_seen) return;
    const unsigned long long *slot = c->h_steer + 2 * ((r - 1) % FB_RING);
    const auto t0 = std::chrono::steady_clock::now();
    while (__atomic_load_n(&slot[1], __ATOMIC_ACQUIRE) != r) {
        if (std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() > FB_WAIT_MS) { c->steer_lost = true; c->steer_spec = true; return; }
        std::this_thread::yield();
    }
    c->steer_seq_seen = r;
    c->steer_spec = __atomic_load_n(&slot[0], __ATOMIC_RELAXED) * STEER_MISS_DEN <= c->steer_call_frames[(r - 1) % FB_RING] * STEER_MISS_NUM;
}

// The table and the state of the steered path, once and outside any capture: built into locals and handed to the context when the table
// kernel has run -- d_steer_rows set means all of it is there, and a failure on the way leaves the context as it was.
static int steer_build(mca_hip_ctx *c)
{
    const size_t na = (size_t)c->cfg.max_arrays;
    DevBuf<float4> rows; DevBuf<float2> q; DevBuf<float> nyq, tail; DevBuf<int> pred; DevBuf<unsigned long long> miss;
    hipError_t e;
    if ((e = rows.alloc((size_t)(c->D + 1) * 4 * 64)) || (e = q.alloc((size_t)(c->D + 1) * c->M * 8)) || (e = nyq.alloc((size_t)(c->D + 1) * c->M)) ||
        (e = pred.alloc(na)) ||
        (e = miss.alloc(3)) ||           // running total; the guard's (arrays that had a prediction); the guard's at the end of the previous call
        (e = tail.alloc(2 * na * FFT_H)) ||
        (e = hipMemset(pred.p, 0xff, pred.bytes())) || (e = hipMemset(miss.p, 0, miss.bytes()))) return hip_fail(c, e, "the table and the state of the steered delay-and-sum");
    const double unit = (double)c->cfg.sample_rate / (double)FFT_N / 346.1;     // Beamformer.cpp:59 without 2 pi
    hipLaunchKernelGGL(k_steer_table, dim3(c->D + 1, 4), dim3(64), 0, nullptr, rows.p, q.p, nyq.p, c->d_grid, c->d_micx, c->M, unit);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipDeviceSynchronize());
    if (!c->h_steer) {
        if (hipHostMalloc((void **)&c->h_steer, FB_RING * 16, hipHostMallocDefault) == hipSuccess) std::memset(c->h_steer, 0, FB_RING * 16);
        else { c->h_steer = nullptr; (void)hipGetLastError(); }
    }
    c->d_steer_rows.swap(rows); c->d_steer_q.swap(q); c->d_steer_nyq.swap(nyq); c->d_steer_pred.swap(pred); c->d_steer_miss.swap(miss); c->d_steer_tail.swap(tail);
    return MCA_HIP_OK;
}

// ... and the rows of Y for this call, with the miss list that has an entry per row.  Workspaces: each grows on its own (grow_ws), a list
// that could not be emptied is dropped
static int steer_prepare(mca_hip_ctx *c, int n_arrays, int n_frames)
{
    int rc;
    if (!c->d_steer_rows && (rc = steer_build(c))) return rc;
    const size_t rows = (size_t)n_arrays * steer_pass_frames(c, n_arrays, n_frames);
    const bool relist = rows + 1 > c->d_steer_mlist.n;                      // an entry per row of Y at most, behind the list's length
    if (rows * STEER_ROW > c->d_steer_Y.n || relist) {
        HIP_TRY(c, hipDeviceSynchronize());
        if ((rc = grow_ws(c, c->d_steer_Y, rows * STEER_ROW, "the rows of the steered spectra")) ||
            (rc = grow_ws_filled(c, c->d_steer_mlist, rows + 1, 1, 0, "the miss list of the steered path"))) return rc;
        if (relist) c->steer_mlist_dirty = false;
    }
    return MCA_HIP_OK;
}

static int steer_reserve(mca_hip_ctx *c, int n_arrays, int n_frames) { return steer_applies(c) ? steer_prepare(c, n_arrays, n_frames) : MCA_HIP_OK; }

// the separation stage of such a call: patch pass (the frames whose pick is not the predicted bin; every frame if the analysis did not steer)
// and synthesis, in passes of frames when Y does not hold the whole call
static int steer_separate(mca_hip_ctx *c, const StreamCall &call, const float *pcm, long long array_stride, long long mic_stride, int n_arrays, int n_frames,
                          const int *doa_bin, float *out_pcm, hipStream_t st)
{
    const size_t a0 = (size_t)call.a0;
    const int pf = steer_pass_frames(c, n_arrays, n_frames);
    const bool fused = call.steer_fused && pf == n_frames;
    const bool patched = fused && call.steer_patched;         // the second pick of the localiser patched the missed frames and counted them (localise_impl)
    float *tails[2] = {c->d_steer_tail, c->d_steer_tail + (size_t)c->cfg.max_arrays * FFT_H};
    time_begin(c, call, MCA_HIP_K_BEAMFORM, st);
    int pass = 0, rc = MCA_HIP_OK;
    for (int f0 = 0; f0 < n_frames && !rc; f0 += pf, ++pass) {
        const int f1 = std::min(n_frames, f0 + pf), np = f1 - f0;
        const bool last = f1 == n_frames;
        SteerPatchArgs pa{};
        pa.pcm = pcm; pa.array_stride = array_stride; pa.mic_stride = mic_stride; pa.n_arrays = n_arrays; pa.n_frames = n_frames; pa.f0 = f0; pa.f1 = f1;
        pa.window = c->d_window; pa.doa_bin = doa_bin; pa.all = fused ? 0 : 1; pa.miss = c->d_steer_miss;
        pa.bf.rows = c->d_steer_rows; pa.bf.q = c->d_steer_q; pa.bf.nyq = c->d_steer_nyq; pa.bf.pred = c->d_steer_pred + a0; pa.bf.Y = c->d_steer_Y;
        pa.y_f0 = f0; pa.y_frames = fused ? n_frames : np;
        const SteerPlan sp = plan_steer(*c, n_arrays, np);
        if (!patched && (rc = launch(c, reinterpret_cast<const void *>(&k_steer_patch), sp.patch_grid, sp.block, sp.lds, &pa, st, "k_steer_patch"))) break;
        SteerSynthArgs sy{};
        sy.Y = c->d_steer_Y; sy.n_frames = n_frames; sy.f0 = f0; sy.f1 = f1; sy.y_f0 = pa.y_f0; sy.y_frames = pa.y_frames;
        sy.ft = sp.ft;
        sy.out = out_pcm;
        sy.tail_in = pass == 0 ? c->d_tail[c->tail_cur] + a0 * FFT_H : tails[(pass - 1) & 1];
        sy.tail_out = last ? c->d_tail[c->tail_cur ^ 1] + a0 * FFT_H : tails[pass & 1];
        sy.doa_bin = doa_bin; sy.pred_out = last ? c->d_steer_pred + a0 : nullptr;
        if (last && c->h_steer) { sy.report = c->h_steer + 2 * (c->steer_seq % FB_RING); sy.seq = c->steer_seq + 1; sy.miss_total = c->d_steer_miss; }
        if (patched) sy.n_miss = c->d_steer_mlist;
        rc = launch(c, reinterpret_cast<const void *>(&k_steer_synth), sp.synth_grid, sp.block, sp.lds, &sy, st, "k_steer_synth");
    }
    time_end(c, st);
    if (rc) return rc;
    c->steer_call_frames[c->steer_seq % FB_RING] = (unsigned long long)n_arrays * n_frames; ++c->steer_seq;
    c->steer_frames_total += (unsigned long long)n_arrays * n_frames;
    if (fused) ++c->steer_fused_calls;
    if (patched) c->steer_mlist_dirty = false;                 // (the synthesis above empties the miss list)
    return MCA_HIP_OK;
}

static int separate_impl(mca_hip_ctx *c, const StreamCall &call, const float *pcm, long long array_stride, long long mic_stride,
                         int n_arrays, int n_frames, const float *doa_rad, float *out_pcm, hipStream_t st, const int *doa_bin = nullptr)
{
    const size_t a0 = (size_t)call.a0;
    const BeamformPlan bp = plan_beamform(*c, doa_bin && c->d_bftab, (reinterpret_cast<uintptr_t>(out_pcm) & 7) == 0, n_arrays, n_frames);
    if (bp.unsupported) return fail(c, MCA_HIP_ERR_UNSUPPORTED, bp.unsupported);
    const BeamformFamily family = bp.form.family;
    int rc = MCA_HIP_OK;
    if (family == BeamformFamily::WAVE_2048 || family == BeamformFamily::WAVE_MS || family == BeamformFamily::WAVE) {
        // the localiser's own picks against the table of steering rows: a transform per channel (k_beamform_wave_2048), per channel pair with
        // the forward transforms of a frame shared by its sources (k_beamform_wave_ms) or a grid row per source (k_beamform_wave)
        BeamformWaveArgs wa{};
        wa.pcm = pcm; wa.array_stride = array_stride; wa.mic_stride = mic_stride;
        wa.M = c->M; wa.n_pairs = family == BeamformFamily::WAVE_2048 ? c->M : c->bf_pairs; wa.n_frames = n_frames; wa.S = c->S;
        wa.ft = bp.ft; wa.skew = bp.skew;
        wa.window = c->d_window; wa.doa_bin = doa_bin; wa.table = c->d_bftab; wa.out = out_pcm;
        wa.tail_in = c->d_tail[c->tail_cur] + a0 * c->S * c->H; wa.tail_out = c->d_tail[c->tail_cur ^ 1] + a0 * c->S * c->H;
        const void *k = family == BeamformFamily::WAVE_2048 ? reinterpret_cast<const void *>(&k_beamform_wave_2048)
                        : family == BeamformFamily::WAVE_MS ? beamform_wave_ms_kernel(bp.form) : beamform_wave_kernel(bp.form);
        time_begin(c, call, MCA_HIP_K_BEAMFORM, st);
        rc = launch(c, k, bp.grid, bp.block, bp.lds, &wa, st, "k_beamform_wave");
        time_end(c, st);
        return rc;
    }
    BeamformArgs ba{};
    ba.pcm = pcm; ba.array_stride = array_stride; ba.mic_stride = mic_stride;
    ba.M = c->M; ba.Mpad = c->M; ba.S = c->S; ba.n_frames = n_frames; ba.fs = c->cfg.sample_rate;
    ba.ft = bp.ft; ba.nb = bp.nb;
    ba.window = c->d_window; ba.mic_x = c->d_micx; ba.doa_rad = doa_rad; ba.out = out_pcm;
    ba.tail_in = c->d_tail[c->tail_cur] + a0 * c->S * c->H; ba.tail_out = c->d_tail[c->tail_cur ^ 1] + a0 * c->S * c->H;
    ba.N = c->N; ba.logH = c->logH; ba.tw = c->d_tw;
    time_begin(c, call, MCA_HIP_K_BEAMFORM, st);
    if (family == BeamformFamily::GEN) {
        ba.S_all = c->S;
        for (int s0 = 0; s0 < c->S && !rc; s0 += bp.s_pass) {      // (the sources in passes, each transforming the channels again: plan_beamform)
            ba.s0 = s0; ba.S = std::min(bp.s_pass, c->S - s0);
            rc = launch(c, reinterpret_cast<const void *>(&k_beamform_gen), bp.grid, bp.block, bp.lds, &ba, st, "k_beamform_gen");
        }
    } else {
        const void *k = family == BeamformFamily::N512 ? reinterpret_cast<const void *>(&k_beamform_512) : beamform_ola_kernel(bp.form);
        rc = launch(c, k, bp.grid, bp.block, bp.lds, &ba, st, "k_beamform_ola");
    }
    time_end(c, st);
    return rc;
}

// The stream calls behind the public entry points, which build the record; graph_record and the host-pointer entry points come with
// records of their own.  A recording enqueues into a capture: nothing runs, so no state index moves (mca_hip_graph_launch does it, per replay).
static int localise_call(mca_hip_ctx *c, StreamCall &call, const float *pcm, long long array_stride, long long mic_stride,
                         int n_arrays, int n_frames, int *doa_bin, float *doa_rad, float *prob, float *energy, hipStream_t st)
{
    int rc = check_stream_args(c, pcm, array_stride, mic_stride, n_arrays, n_frames);
    if (rc) return rc;
    if (!doa_bin) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "doa_bin_dev is NULL");
    adapt_policy_begin(c, call, n_arrays, n_frames);
    if ((rc = localise_impl(c, call, pcm, array_stride, mic_stride, n_arrays, n_frames, doa_bin, doa_rad, prob, energy, st))) return rc;
    if (!call.recording()) { c->last_arrays = n_arrays; c->last_frames = n_frames; c->e_cur ^= 1; }
    return MCA_HIP_OK;
}

// doa_bin: the grid bins behind doa_rad when they are the localiser's own picks (NULL: arbitrary angles)
static int separate_call(mca_hip_ctx *c, const StreamCall &call, const float *pcm, long long array_stride, long long mic_stride,
                         int n_arrays, int n_frames, const float *doa_rad, float *out_pcm, hipStream_t st, const int *doa_bin)
{
    int rc = check_stream_args(c, pcm, array_stride, mic_stride, n_arrays, n_frames);
    if (rc) return rc;
    if (!doa_rad || !out_pcm) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "doa_rad_dev/out_pcm_dev is NULL");
    if ((rc = separate_impl(c, call, pcm, array_stride, mic_stride, n_arrays, n_frames, doa_rad, out_pcm, st, doa_bin))) return rc;
    if (!call.recording()) c->tail_cur ^= 1;
    return MCA_HIP_OK;
}

int mca_hip_process_frames_dev(mca_hip_ctx *c, const float *pcm, long long array_stride, long long mic_stride,
                               int n_arrays, int n_frames, int *doa_bin, float *doa_rad, float *prob,
                               float *energy, float *out_pcm, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!doa_rad) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "doa_rad_dev is NULL (the separation stage steers with it)");
    int rc = check_stream_args(c, pcm, array_stride, mic_stride, n_arrays, n_frames);
    if (rc) return rc;
    if (!doa_bin) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "doa_bin_dev is NULL");
    if (!out_pcm) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "doa_rad_dev/out_pcm_dev is NULL");
    if ((rc = ensure_bf_table(c))) return rc;
    StreamCall call; hipStream_t st = (hipStream_t)stream;     // (a device-pointer call: the host-pointer entry points and the recordings run the two stages)
    const bool steer = steer_applies(c);
    if (steer && (rc = steer_prepare(c, n_arrays, n_frames))) return rc;
    if (steer) steer_policy_begin(c);
    call.steer = steer && c->steer_spec && steer_pass_frames(c, n_arrays, n_frames) == n_frames;
    adapt_policy_begin(c, call, n_arrays, n_frames);
    rc = localise_impl(c, call, pcm, array_stride, mic_stride, n_arrays, n_frames, doa_bin, doa_rad, prob, energy, st);
    if (!rc && steer) rc = steer_separate(c, call, pcm, array_stride, mic_stride, n_arrays, n_frames, doa_bin, out_pcm, st);
    else if (!rc) rc = separate_impl(c, call, pcm, array_stride, mic_stride, n_arrays, n_frames, doa_rad, out_pcm, st, doa_bin);
    if (rc) return rc;
    c->last_arrays = n_arrays; c->last_frames = n_frames;
    c->e_cur ^= 1; c->tail_cur ^= 1;
    return MCA_HIP_OK;
}

int mca_hip_localise_frames_dev(mca_hip_ctx *c, const float *pcm, long long array_stride, long long mic_stride,
                                int n_arrays, int n_frames, int *doa_bin, float *doa_rad, float *prob,
                                float *energy, void *stream)
{
    StreamCall call;
    return localise_call(c, call, pcm, array_stride, mic_stride, n_arrays, n_frames, doa_bin, doa_rad, prob, energy, (hipStream_t)stream);
}

int mca_hip_separate_frames_dev(mca_hip_ctx *c, const float *pcm, long long array_stride, long long mic_stride,
                                int n_arrays, int n_frames, const float *doa_rad, float *out_pcm, void *stream)
{
    return separate_call(c, StreamCall(), pcm, array_stride, mic_stride, n_arrays, n_frames, doa_rad, out_pcm, (hipStream_t)stream, nullptr);
}

int mca_hip_separate_frames_bins_dev(mca_hip_ctx *c, const float *pcm, long long array_stride, long long mic_stride,
                                     int n_arrays, int n_frames, const int *doa_bin, const float *doa_rad, float *out_pcm, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!doa_bin) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "doa_bin_dev is NULL");
    int rc = ensure_bf_table(c);
    if (rc) return rc;
    return separate_call(c, StreamCall(), pcm, array_stride, mic_stride, n_arrays, n_frames, doa_rad, out_pcm, (hipStream_t)stream, doa_bin);
}

// ---- real-time mode: the stream call as a HIP graph ------------------------------------------
struct mca_hip_graph {
    mca_hip_ctx *c = nullptr;
    const float *pcm = nullptr; long long array_stride = 0, mic_stride = 0;
    int n_arrays = 0, n_frames = 0;
    int *doa_bin = nullptr; float *doa_rad = nullptr, *prob = nullptr, *energy = nullptr, *out_pcm = nullptr;
    hipStream_t cap = nullptr;                 // recording stream
    hipGraph_t graph[4] = {};                  // one per (e_cur, tail_cur): the state buffers a call reads / writes
    hipGraphExec_t exec[4] = {};
    unsigned long long ws_gen = 0;             // c->ws_gen the recordings were made under
};

static void graph_orphan(mca_hip_graph *g);
// a recording bakes in the workspace pointers (d_A, d_C, scan / gate buffers): drop every recording of the graph
static void graph_drop_recordings(mca_hip_graph *g)
{
    for (int i = 0; i < 4; ++i) {
        if (g->exec[i]) (void)hipGraphExecDestroy(g->exec[i]);
        if (g->graph[i]) (void)hipGraphDestroy(g->graph[i]);
        g->exec[i] = nullptr; g->graph[i] = nullptr;
    }
}

static void graph_orphan(mca_hip_graph *g) { graph_drop_recordings(g); g->c = nullptr; }

int mca_hip_graph_create(mca_hip_ctx *c, const float *pcm, long long array_stride, long long mic_stride, int n_arrays,
                         int n_frames, int *doa_bin, float *doa_rad, float *prob, float *energy, float *out_pcm,
                         mca_hip_graph **out)
{
    if (!out) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    int rc = check_stream_args(c, pcm, array_stride, mic_stride, n_arrays, n_frames);
    if (rc) return rc;
    // doa_bin_dev NULL: the separation stage alone, steered by the caller's angles in doa_rad_dev (mca_hip_separate_frames_dev: the
    // delay-and-sum stream of mcabeamf.cpp:77-122, BASELINE configs[1])
    if (!doa_bin && !out_pcm) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "doa_bin_dev and out_pcm_dev are both NULL: nothing to record");
    if (out_pcm && !doa_rad) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "doa_rad_dev is NULL (the separation stage steers with it)");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (doa_bin && (rc = reserve_impl(c, n_arrays, n_frames))) return rc;   // recording must not allocate
    if (out_pcm && (rc = ensure_bf_table(c))) return rc;
    mca_hip_graph *g = new mca_hip_graph();
    g->c = c; g->pcm = pcm; g->array_stride = array_stride; g->mic_stride = mic_stride; g->n_arrays = n_arrays; g->n_frames = n_frames;
    g->doa_bin = doa_bin; g->doa_rad = doa_rad; g->prob = prob; g->energy = energy; g->out_pcm = out_pcm;
    if (hipStreamCreateWithFlags(&g->cap, hipStreamNonBlocking) != hipSuccess) { delete g; return fail(c, MCA_HIP_ERR_HIP, "hipStreamCreateWithFlags failed"); }
    g->ws_gen = c->ws_gen;
    c->graphs.push_back(g);
    *out = g;
    return MCA_HIP_OK;
}

static int graph_record(mca_hip_graph *g, int idx)
{
    mca_hip_ctx *c = g->c;
    StreamCall call;               // a recording: the mode's own kernels whatever the eager calls do at the moment, no event pairs, no state moved
    call.caller = Caller::RECORDING;
    HIP_TRY(c, hipStreamBeginCapture(g->cap, hipStreamCaptureModeRelaxed));
    int rc = MCA_HIP_OK;
    if (g->doa_bin)
        rc = localise_call(c, call, g->pcm, g->array_stride, g->mic_stride, g->n_arrays, g->n_frames, g->doa_bin, g->doa_rad, g->prob, g->energy, g->cap);
    if (!rc && g->out_pcm)
        rc = separate_call(c, call, g->pcm, g->array_stride, g->mic_stride, g->n_arrays, g->n_frames, g->doa_rad, g->out_pcm, g->cap, g->doa_bin);
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(g->cap, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return fail(c, MCA_HIP_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    g->graph[idx] = graph;
    HIP_TRY(c, hipGraphInstantiate(&g->exec[idx], graph, nullptr, nullptr, 0));
    return MCA_HIP_OK;
}

int mca_hip_graph_launch(mca_hip_graph *g, void *stream)
{
    if (!g) return MCA_HIP_ERR_INVALID_ARGUMENT;
    mca_hip_ctx *c = g->c;
    if (!c) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "mca_hip_graph_launch: the context of this graph has been destroyed");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (g->doa_bin && c->hist_pending) {          // lazy tails: a recording takes the state as exact
        const int rc = settle_history(c, (hipStream_t)stream);
        if (rc) return rc;
    }
    if (g->ws_gen != c->ws_gen) {
        // an eager call with more arrays / frames reallocated the workspace since the recording: the recorded kernels
        // would run on freed memory.  Make sure the workspace (still) fits this graph's shape, then record afresh.
        HIP_TRY(c, hipDeviceSynchronize());      // launches of the old recordings may still be in flight
        graph_drop_recordings(g);
        const int rc = g->doa_bin ? reserve_impl(c, g->n_arrays, g->n_frames) : MCA_HIP_OK;
        if (rc) return rc;
        g->ws_gen = c->ws_gen;
    }
    const int idx = c->e_cur | (c->tail_cur << 1);
    if (!g->exec[idx]) {
        const int rc = graph_record(g, idx);
        if (rc) return rc;
    }
    HIP_TRY(c, hipGraphLaunch(g->exec[idx], (hipStream_t)stream));
    if (g->doa_bin && adaptive_shape(c, g->n_arrays, g->n_frames)) c->adapt_frames_total += (unsigned long long)g->n_arrays * g->n_frames;   // (a recording counts nothing)
    if (g->doa_bin) c->e_cur ^= 1;              // as the eager calls do
    if (g->out_pcm) c->tail_cur ^= 1;
    if (g->doa_bin) {
        c->last_arrays = g->n_arrays; c->last_frames = g->n_frames;
    }
    return MCA_HIP_OK;
}

void mca_hip_graph_destroy(mca_hip_graph *g)
{
    if (!g) return;
    if (g->c) {
        (void)hipSetDevice(g->c->cfg.device);
        (void)hipDeviceSynchronize();
        auto &v = g->c->graphs;
        for (size_t i = 0; i < v.size(); ++i) if (v[i] == g) { v.erase(v.begin() + i); break; }
    }
    graph_drop_recordings(g);
    if (g->cap) (void)hipStreamDestroy(g->cap);
    delete g;
}

// 16-bit PCM: upload the shorts (half the PCIe bytes), widen on the GPU
__global__ void k_i16_to_f32(const short *src, float *dst, long long n4)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) {
        const short4 v = reinterpret_cast<const short4 *>(src)[i];
        reinterpret_cast<float4 *>(dst)[i] = make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
    }
}

extern "C++" {
namespace {

// is p page-locked host memory (hipHostMalloc / hipHostRegister, e.g. through mca_hip_host_alloc / _register)?
bool is_pinned(const void *p)
{
    if (!p) return false;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}

// The host-pointer stream call.  Pageable buffers: one synchronous copy in, the kernels, synchronous copies out (the
// driver stages pageable memory through its own bounce buffers at about half the PCIe rate).  Page-locked input: the
// arrays go up in up to four chunks on a copy stream, each chunk's kernels start when its samples have arrived, and its
// results leave on a third stream while the next chunk computes -- input, kernels and output of a call overlap, and the
// rate is that of the PCIe link.  Same kernels on the same per-array state either way: the outputs are bit-identical.
template <typename SampleT>
int process_frames_host_impl(mca_hip_ctx *c, const SampleT *pcm, int n_arrays, int n_frames, int *doa_bin, float *doa_rad, float *prob,
                             float *energy, float *out_pcm)
{
    constexpr bool I16 = sizeof(SampleT) == 2;
    if (!c || !pcm || !doa_bin) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_arrays < 1 || n_frames < 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_arrays/n_frames < 1");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const long long ms = (long long)(n_frames + 1) * c->H, as = ms * c->M;
    const size_t n_pcm = (size_t)as * n_arrays, fs_ = (size_t)n_frames * c->S, fd_ = (size_t)n_frames * c->D, fo_ = (size_t)c->S * n_frames * c->H;
    const size_t n_fs = n_arrays * fs_, n_en = energy ? n_arrays * fd_ : 0, n_out = out_pcm ? n_arrays * fo_ : 0;
    float *d_pcm = (float *)c->stage.get(0, n_pcm * 4), *d_rad = (float *)c->stage.get(2, n_fs * 4), *d_prob = (float *)c->stage.get(3, n_fs * 4);
    float *d_en = (float *)c->stage.get(4, n_en * 4), *d_out = (float *)c->stage.get(5, n_out * 4);
    int *d_bin = (int *)c->stage.get(1, n_fs * 4);
    short *d_i16 = I16 ? (short *)c->stage.get(6, n_pcm * 2) : nullptr;
    if (!d_pcm || !d_bin || !d_rad || !d_prob || (energy && !d_en) || (out_pcm && !d_out) || (I16 && !d_i16))
        return fail(c, MCA_HIP_ERR_OUT_OF_MEMORY, "device staging buffers for the host-pointer call");
    int rc = check_stream_args(c, d_pcm, as, ms, n_arrays, n_frames);
    if (!rc && out_pcm) rc = ensure_bf_table(c);
    if (rc) return rc;
    StreamCall call;                                             // the eager form on either path: the pageable and the page-locked one return the same bits
    call.caller = Caller::HOST;

    if (!is_pinned(pcm)) {
        if (I16) {
            HIP_TRY(c, hipMemcpy(d_i16, pcm, n_pcm * 2, hipMemcpyHostToDevice));
            const long long n4 = (long long)(n_pcm / 4);                    // (F+1)*hop is a multiple of 32
            hipLaunchKernelGGL(k_i16_to_f32, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, nullptr, d_i16, d_pcm, n4);
        } else {
            HIP_TRY(c, hipMemcpy(d_pcm, pcm, n_pcm * 4, hipMemcpyHostToDevice));
        }
        rc = localise_call(c, call, d_pcm, as, ms, n_arrays, n_frames, d_bin, d_rad, d_prob, d_en, nullptr);
        if (!rc && out_pcm) rc = separate_call(c, call, d_pcm, as, ms, n_arrays, n_frames, d_rad, d_out, nullptr, d_bin);
        if (rc) return rc;
        HIP_TRY(c, hipDeviceSynchronize());
        HIP_TRY(c, hipMemcpy(doa_bin, d_bin, n_fs * 4, hipMemcpyDeviceToHost));
        if (doa_rad) HIP_TRY(c, hipMemcpy(doa_rad, d_rad, n_fs * 4, hipMemcpyDeviceToHost));
        if (prob) HIP_TRY(c, hipMemcpy(prob, d_prob, n_fs * 4, hipMemcpyDeviceToHost));
        if (energy) HIP_TRY(c, hipMemcpy(energy, d_en, n_en * 4, hipMemcpyDeviceToHost));
        if (out_pcm) HIP_TRY(c, hipMemcpy(out_pcm, d_out, n_out * 4, hipMemcpyDeviceToHost));
        return MCA_HIP_OK;
    }

    // page-locked input: chunks of arrays through three streams
    for (int i = 0; i < 3; ++i)
        if (!c->io_stream[i]) HIP_TRY(c, hipStreamCreateWithFlags(&c->io_stream[i], hipStreamNonBlocking));
    constexpr int MAXC = 4;
    for (int i = 0; i < 2 * MAXC; ++i)
        if (!c->io_ev[i]) HIP_TRY(c, hipEventCreateWithFlags(&c->io_ev[i], hipEventDisableTiming));
    hipStream_t s_in = c->io_stream[0], s_run = c->io_stream[1], s_out = c->io_stream[2];
    // the three internal streams are non-blocking: nothing orders them after earlier work on the null stream or on a caller's
    // stream (a *_dev call or a graph launch that still writes d_E / d_tail, the memsets of mca_hip_reset).  This entry point
    // is synchronous anyway, so it starts from an idle device.
    HIP_TRY(c, hipDeviceSynchronize());
    // on every exit -- also the early ones of HIP_TRY -- the streams are drained
    struct Guard { hipStream_t s[3]; ~Guard() { for (hipStream_t q : s) (void)hipStreamSynchronize(q); } } guard{{s_in, s_run, s_out}};
    // (with the power gate the call stays one chunk: mca_hip_copy_gate reads the flags of the whole call from one workspace)
    const int nchunk = c->cfg.use_power_floor ? 1 : std::min(n_arrays, MAXC);
    const bool out_pinned[5] = {is_pinned(doa_bin), is_pinned(doa_rad), is_pinned(prob), is_pinned(energy), is_pinned(out_pcm)};
    int a0 = 0;
    for (int k = 0; k < nchunk; ++k) {                       // all uploads are queued first: the link never waits for a kernel
        const int na = n_arrays / nchunk + (k < n_arrays % nchunk ? 1 : 0);
        if (I16) HIP_TRY(c, hipMemcpyAsync(d_i16 + (size_t)a0 * as, pcm + (size_t)a0 * as, (size_t)na * as * 2, hipMemcpyHostToDevice, s_in));
        else HIP_TRY(c, hipMemcpyAsync(d_pcm + (size_t)a0 * as, pcm + (size_t)a0 * as, (size_t)na * as * 4, hipMemcpyHostToDevice, s_in));
        HIP_TRY(c, hipEventRecord(c->io_ev[k], s_in));
        a0 += na;
    }
    a0 = 0;
    adapt_policy_begin(c, call, n_arrays, n_frames);
    call.rows_planned = (long long)n_arrays * n_frames;         // every chunk is planned as the whole call (bit-identical results)
    call.arrays_planned = n_arrays;
    for (int k = 0; k < nchunk && !rc; ++k) {
        const int na = n_arrays / nchunk + (k < n_arrays % nchunk ? 1 : 0);
        HIP_TRY(c, hipStreamWaitEvent(s_run, c->io_ev[k], 0));
        if (I16) {
            const long long n4 = (long long)na * as / 4;
            hipLaunchKernelGGL(k_i16_to_f32, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s_run, d_i16 + (size_t)a0 * as, d_pcm + (size_t)a0 * as, n4);
        }
        StreamCall piece = call;
        piece.a0 = a0;                                        // the chunk's arrays on the one workspace, per-array state at its offset
        rc = localise_impl(c, piece, d_pcm + (size_t)a0 * as, as, ms, na, n_frames, d_bin + a0 * fs_, d_rad + a0 * fs_, d_prob + a0 * fs_,
                           energy ? d_en + a0 * fd_ : nullptr, s_run);
        if (!rc && out_pcm) rc = separate_impl(c, piece, d_pcm + (size_t)a0 * as, as, ms, na, n_frames, d_rad + a0 * fs_, d_out + a0 * fo_, s_run, d_bin + a0 * fs_);
        if (rc) break;
        HIP_TRY(c, hipEventRecord(c->io_ev[MAXC + k], s_run));
        HIP_TRY(c, hipStreamWaitEvent(s_out, c->io_ev[MAXC + k], 0));
        if (out_pinned[0]) HIP_TRY(c, hipMemcpyAsync(doa_bin + a0 * fs_, d_bin + a0 * fs_, na * fs_ * 4, hipMemcpyDeviceToHost, s_out));
        if (doa_rad && out_pinned[1]) HIP_TRY(c, hipMemcpyAsync(doa_rad + a0 * fs_, d_rad + a0 * fs_, na * fs_ * 4, hipMemcpyDeviceToHost, s_out));
        if (prob && out_pinned[2]) HIP_TRY(c, hipMemcpyAsync(prob + a0 * fs_, d_prob + a0 * fs_, na * fs_ * 4, hipMemcpyDeviceToHost, s_out));
        if (energy && out_pinned[3]) HIP_TRY(c, hipMemcpyAsync(energy + a0 * fd_, d_en + a0 * fd_, na * fd_ * 4, hipMemcpyDeviceToHost, s_out));
        if (out_pcm && out_pinned[4]) HIP_TRY(c, hipMemcpyAsync(out_pcm + a0 * fo_, d_out + a0 * fo_, na * fo_ * 4, hipMemcpyDeviceToHost, s_out));
        a0 += na;
    }
    (void)hipStreamSynchronize(s_in); (void)hipStreamSynchronize(s_run); (void)hipStreamSynchronize(s_out);
    if (rc) return rc;
    c->last_arrays = n_arrays; c->last_frames = n_frames;
    c->e_cur ^= 1;
    if (out_pcm) c->tail_cur ^= 1;
    // pageable result buffers: plain copies now that everything has finished
    if (!out_pinned[0]) HIP_TRY(c, hipMemcpy(doa_bin, d_bin, n_fs * 4, hipMemcpyDeviceToHost));
    if (doa_rad && !out_pinned[1]) HIP_TRY(c, hipMemcpy(doa_rad, d_rad, n_fs * 4, hipMemcpyDeviceToHost));
    if (prob && !out_pinned[2]) HIP_TRY(c, hipMemcpy(prob, d_prob, n_fs * 4, hipMemcpyDeviceToHost));
    if (energy && !out_pinned[3]) HIP_TRY(c, hipMemcpy(energy, d_en, n_en * 4, hipMemcpyDeviceToHost));
    if (out_pcm && !out_pinned[4]) HIP_TRY(c, hipMemcpy(out_pcm, d_out, n_out * 4, hipMemcpyDeviceToHost));
    return MCA_HIP_OK;
}

}  // namespace
}  // extern "C++"

int mca_hip_process_frames_host(mca_hip_ctx *c, const float *pcm, int n_arrays, int n_frames, int *doa_bin,
                                float *doa_rad, float *prob, float *energy, float *out_pcm)
{
    return process_frames_host_impl<float>(c, pcm, n_arrays, n_frames, doa_bin, doa_rad, prob, energy, out_pcm);
}

int mca_hip_process_frames_host_i16(mca_hip_ctx *c, const short *pcm, int n_arrays, int n_frames, int *doa_bin,
                                    float *doa_rad, float *prob, float *energy, float *out_pcm)
{
    return process_frames_host_impl<short>(c, pcm, n_arrays, n_frames, doa_bin, doa_rad, prob, energy, out_pcm);
}

// page-locked host memory for the host-pointer entry points (thin wrappers, so that a caller need not link HIP)
void *mca_hip_host_alloc(long long bytes)
{
    void *p = nullptr;
    if (bytes <= 0 || hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void mca_hip_host_free(void *p) { if (p) (void)hipHostFree(p); }
int mca_hip_host_register(void *p, long long bytes)
{
    if (!p || bytes <= 0) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (hipHostRegister(p, (size_t)bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return fail(NO_CTX, MCA_HIP_ERR_HIP, "hipHostRegister failed"); }
    return MCA_HIP_OK;
}
int mca_hip_host_unregister(void *p)
{
    if (!p) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (hipHostUnregister(p) != hipSuccess) { (void)hipGetLastError(); return fail(NO_CTX, MCA_HIP_ERR_HIP, "hipHostUnregister failed"); }
    return MCA_HIP_OK;
}

// what the tracked call (mca_hip_gcc2_tracked_frames_dev) adds to the stream call: the tracker's outputs
struct Gcc2TrackOut { float *doa_rad, *prob; unsigned char *fired; int *track; };

// the launch of k_gcc2_track: SLOTS = particles per lane (8 up to 512 particles, 16 up to 1024)
extern "C++" template <typename TC>
static void launch_gcc2_track(mca_hip_ctx *c, Gcc2TrackArgs &ta, hipStream_t st)
{
    ta.grid = c->d_grid; ta.step = c->step; ta.D = c->D;
    ta.N = c->trk.n_particles; ta.n_inject = c->trk.n_inject; ta.seed = c->trk.seed;
    const int slots = ta.N <= 512 ? 8 : 16, Dl = (ta.D + 1) & ~1;
    ta.slice_bytes = (unsigned)(((size_t)slots * 64 * 16 + (size_t)Dl * (sizeof(TC) + 4) + 15) / 16 * 16);
    ta.sigma_init = c->trk.sigma_init; ta.sigma_step = c->trk.sigma_step;
    ta.x = c->d_trk_x; ta.sd = c->d_trk_sd; ta.si = c->d_trk_si;
    const dim3 g((ta.n_arrays + GCC2_TRACK_WAVES - 1) / GCC2_TRACK_WAVES), b(64 * GCC2_TRACK_WAVES);
    const size_t smem = (size_t)ta.slice_bytes * GCC2_TRACK_WAVES;      // at most 2 x 17.9 KB
    if (slots == 8) hipLaunchKernelGGL((k_gcc2_track<TC, 8>), g, b, smem, st, ta);
    else hipLaunchKernelGGL((k_gcc2_track<TC, 16>), g, b, smem, st, ta);
}

// mca_hip_gcc2_frames_dev, and with `trk` the tracked call: the same kernels up to the smoothed rows and their argmaxes, then
// k_gcc2_track instead of the outputs of the scan's DOA recursion
static int gcc2_frames_impl(mca_hip_ctx *c, const float *pcm, long long array_stride, long long mic_stride,
                            int n_arrays, int n_frames, int *argmax, float *doa_rad, float *prob, float *corr, void *stream,
                            const Gcc2TrackOut *trk)
{
    int rc = check_stream_args(c, pcm, array_stride, mic_stride, n_arrays, n_frames);
    if (rc) return rc;
    if (c->M != 2) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "the 2-microphone GCC path needs a context with n_mics == 2");
    if (c->Dp > 192) return fail(c, MCA_HIP_ERR_UNSUPPORTED, "the 2-microphone GCC path supports up to 192 steering delays");
    if (!argmax && !trk) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "argmax_dev is NULL");
    hipStream_t st = (hipStream_t)stream;
    if (trk) {
        if (!trk->doa_rad) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "doa_rad_dev is NULL");
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            return fail(c, MCA_HIP_ERR_UNSUPPORTED, "the tracked call cannot be recorded into a HIP graph");
        // the rows and argmaxes of the call, where the caller does not take them
        const size_t rows = (size_t)n_arrays * n_frames;
        if (!corr && (rc = grow_ws(c, c->d_trk_corr, rows * c->D, "the tracked call's correlation rows"))) return rc;
        if (!argmax && (rc = grow_ws(c, c->d_trk_idx, rows, "the tracked call's argmaxes"))) return rc;
        if (!argmax) argmax = c->d_trk_idx;
    }
    StreamCall call;
    const RowLayout lay = row_layout(c, c->tab_planes);              // the context's own rows (ADAPTIVE: the 2-microphone path always runs the exact split)
    // the tracked call plans its contraction as one K range whatever the batch (plan_gemm): the rows of an array, and so its track,
    // then do not depend on how many arrays run beside it.  (The K range of two microphones is short: the split buys little.)
    if (trk) call.rows_planned = 1LL << 40;
    if ((rc = run_correlation_map(c, call, lay, pcm, array_stride, mic_stride, n_arrays, n_frames, st))) return rc;
    Gcc2ScanArgs ga{};
    ga.C = c->ws.d_C; ga.c_planes = call.map.c_planes; ga.c_plane_stride = call.map.c_plane; ga.n_frames = n_frames; ga.Dp = c->Dp; ga.D = c->D;
    // frames per chunk: every chunk re-reads 160 warm-up frames (recursion + DOA smoothing), so long chunks are cheaper;
    // shorter ones for small batches so that a few hundred workgroups exist
    ga.chunk = 128;
    while (ga.chunk > 32 && (long long)n_arrays * ((n_frames + ga.chunk - 1) / ga.chunk) < 512) ga.chunk >>= 1;
    ga.vdone_in = c->d_vdone[c->doa_cur]; ga.vdone_out = c->d_vdone[c->doa_cur ^ 1];
    ga.mu = 0.8f; ga.one_minus_mu = 1 - 0.8f;                      // _maxCorrMemoryFactor (BinauralLocalisation.h:198)
    ga.doa_mem = 0.6f; ga.one_minus_doa_mem = 1 - 0.6f;            // _maxDoaMemoryFactor (:199)
    ga.step = c->step;
    ga.corr_in = c->d_E[c->e_cur]; ga.corr_out = c->d_E[c->e_cur ^ 1];
    ga.doa_in = c->d_doa[c->doa_cur]; ga.doa_out = c->d_doa[c->doa_cur ^ 1];
    ga.grid = c->d_grid; ga.argmax = argmax; ga.doa_rad = doa_rad; ga.prob = prob; ga.corr = corr;
    if (trk && !ga.corr) ga.corr = c->d_trk_corr;
    const bool gate = c->cfg.use_power_floor != 0;
    time_begin(c, call, MCA_HIP_K_GCC2_SCAN, st);
    if (gate) {
        // setPowerFloor + the gate of processParametrisation (BinauralLocalisation.cpp:387-404, :425-434): 3 s of floor
        // estimation (power + 1e-10 per frame), then voiced = FFTLogPower > floor + 6 dB; the recursions below only see
        // the frames that fired, gated-out frames repeat the previous outputs
        const size_t rows = (size_t)n_arrays * n_frames;
        if ((rc = grow_ws(c, c->d_g2_vidx, rows, "the fired frames")) || (rc = grow_ws(c, c->d_g2_nv, (size_t)c->cfg.max_arrays, "the fired frames' counts")) ||
            (rc = grow_ws(c, c->d_g2_rad, rows, "the gated call's DOAs")) || (rc = grow_ws(c, c->d_g2_prob, rows, "the gated call's probabilities")) ||
            (rc = grow_ws(c, c->d_g2_reset, rows, "the silence rule's marks"))) return rc;
        GateArgs gg{};
        gg.power_lin = c->ws.d_power; gg.n_frames = n_frames; gg.fft_n = c->N;
        gg.needed_samples = (int)(3.0 * c->cfg.sample_rate);              // _durationToEstimatePowerFloor (SoundLocalisationImpl.h:77)
        gg.margin_db = 6.f;                                                // _noiseMarginDB (BinauralLocalisation.h:197)
        gg.eps = 1e-10;                                                    // BinauralLocalisation.cpp:391
        gg.state = c->d_gate_state; gg.voiced = c->ws.d_voiced; gg.power_out = c->ws.d_power_out; gg.post0 = c->d_g2_post0;
        hipLaunchKernelGGL(k_gate, dim3(n_arrays), dim3(256), 0, st, gg);
        // the silence rule (:530-560): windowsToDecay = 3 * fs / (analysisLength / 2 - 1), int arithmetic, analysisLength = N + 2
        const int windows_to_decay = 3 * c->cfg.sample_rate / c->H;
        if (trk) HIP_TRY(c, hipMemcpyAsync(c->d_trk_sil, c->d_silence, (size_t)n_arrays * 4, hipMemcpyDeviceToDevice, st));   // the counters before the call
        hipLaunchKernelGGL(k_gcc2_compact, dim3(n_arrays), dim3(256), 0, st, c->ws.d_voiced, n_frames, c->d_g2_vidx, c->d_g2_nv,
                           c->d_g2_post0, c->d_silence, windows_to_decay, c->d_g2_reset);
        ga.vidx = c->d_g2_vidx; ga.nv = c->d_g2_nv; ga.vreset = c->d_g2_reset;
        if (!ga.doa_rad) ga.doa_rad = c->d_g2_rad;                         // the hold-over needs them whatever the caller asked for
        if (!ga.prob) ga.prob = c->d_g2_prob;
    }
    const int nslot = GCC2_DOAWARM + ga.chunk;
    const size_t smem = (size_t)nslot * ((c->D + 3) / 4 * 4 + 4) * sizeof(float) + ((size_t)nslot * 5 + 1) * sizeof(float);
    dim3 g((n_frames + ga.chunk - 1) / ga.chunk, n_arrays);
    if ((rc = launch_kernel(c, k_gcc2_scan, g, dim3(std::max(256, round_up(c->D, 64))), smem, st, ga))) return rc;   // >= 4 waves: the per-frame argmax / min / sum is one wave per frame
    if (gate) {
        Gcc2FillArgs fa{};
        fa.voiced = c->ws.d_voiced; fa.n_frames = n_frames; fa.D = c->D;
        fa.argmax = argmax; fa.doa_rad = ga.doa_rad; fa.prob = ga.prob; fa.corr = corr; fa.corr_state = ga.corr_in;
        fa.last_idx = c->d_last_bin; fa.last_rad = c->d_last_rad; fa.last_prob = c->d_last_prob;
        hipLaunchKernelGGL(k_gcc2_fill, dim3(n_arrays), dim3(1024), 0, st, fa);
    }
    if (trk) {
        Gcc2TrackArgs ta{};
        ta.corr = ga.corr; ta.corr_state = ga.corr_in; ta.argmax = argmax;
        if (gate) { ta.voiced = c->ws.d_voiced; ta.post0 = c->d_g2_post0; ta.sil_in = c->d_trk_sil; }
        ta.windows_to_decay = 3 * c->cfg.sample_rate / c->H;
        ta.n_arrays = n_arrays; ta.n_frames = n_frames;
        ta.key_a = -1; ta.state0 = 0; ta.one_kind = -1;
        ta.doa_out = trk->doa_rad; ta.prob_out = trk->prob; ta.fired = trk->fired; ta.track = trk->track;
        launch_gcc2_track<float>(c, ta, st);
    }
    time_end(c, st);
    HIP_TRY(c, hipGetLastError());
    c->e_cur ^= 1; c->doa_cur ^= 1;
    c->last_arrays = n_arrays; c->last_frames = n_frames;
    return MCA_HIP_OK;
}

int mca_hip_gcc2_frames_dev(mca_hip_ctx *c, const float *pcm, long long array_stride, long long mic_stride,
                            int n_arrays, int n_frames, int *argmax, float *doa_rad, float *prob, float *corr, void *stream)
{
    if (c && c->tracked)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "this context has a DOA tracker attached: call mca_hip_gcc2_tracked_frames_dev / _host");
    return gcc2_frames_impl(c, pcm, array_stride, mic_stride, n_arrays, n_frames, argmax, doa_rad, prob, corr, stream, nullptr);
}

int mca_hip_gcc2_tracked_frames_dev(mca_hip_ctx *c, const float *pcm, long long array_stride, long long mic_stride, int n_arrays,
                                    int n_frames, int *argmax, float *doa_rad, float *prob, unsigned char *fired, int *track,
                                    float *corr, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!c->tracked) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "no DOA tracker attached (mca_hip_gcc2_tracker_attach)");
    const Gcc2TrackOut out{doa_rad, prob, fired, track};
    return gcc2_frames_impl(c, pcm, array_stride, mic_stride, n_arrays, n_frames, argmax, nullptr, nullptr, corr, stream, &out);
}

int mca_hip_gcc2_tracked_frames_host(mca_hip_ctx *c, const float *pcm, int n_arrays, int n_frames, int *argmax, float *doa_rad,
                                     float *prob, unsigned char *fired, int *track, float *corr)
{
    if (!c || !pcm || !doa_rad) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_arrays < 1 || n_frames < 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_arrays/n_frames < 1");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const long long ms = (long long)(n_frames + 1) * c->H, as = ms * c->M;
    const size_t n_pcm = (size_t)as * n_arrays, n_f = (size_t)n_arrays * n_frames;
    // (the _dev call gets a buffer for every optional output but the rows, whatever the caller takes back)
    StageBuf b[] = {{SG_PCM, pcm, n_pcm * 4, STAGE_IN}, {SG_DOA, doa_rad, n_f * 4, STAGE_OUT}, {SG_ARGMAX, argmax, n_f * 4, STAGE_OUT | STAGE_ALWAYS},
                    {SG_PROB, prob, n_f * 4, STAGE_OUT | STAGE_ALWAYS}, {SG_FIRED, fired, n_f, STAGE_OUT | STAGE_ALWAYS}, {SG_TRACK, track, n_f * 4, STAGE_OUT | STAGE_ALWAYS},
                    {SG_CORR, corr, n_f * c->D * 4, STAGE_OUT}};
    return staged(c, b, [&] {
        return mca_hip_gcc2_tracked_frames_dev(c, (float *)b[0].dev, as, ms, n_arrays, n_frames, (int *)b[2].dev, (float *)b[1].dev, (float *)b[3].dev, (unsigned char *)b[4].dev,
                                               (int *)b[5].dev, (float *)b[6].dev, nullptr);
    });
}

int mca_hip_gcc2_tracker_attach(mca_hip_ctx *c, const mca_hip_gcc2_tracker_config *cfg)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!cfg || cfg->struct_size != (int)sizeof(mca_hip_gcc2_tracker_config))
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "tracker config is NULL or struct_size != sizeof(mca_hip_gcc2_tracker_config)");
    if (c->M != 2) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "the DOA tracker needs a context with n_mics == 2");
    if (c->tracked) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "a DOA tracker is already attached to this context");
    mca_hip_gcc2_tracker_config t = *cfg;
    if (t.n_particles == 0) t.n_particles = 500;                                   // BinauralLocalisation.cpp:463
    if (t.n_particles < 16 || t.n_particles > GCC2_TRACK_MAX_PARTICLES) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_particles must be 0 (500) or in [16, 1024]");
    if (t.n_inject == 0) t.n_inject = t.n_particles / 20;
    else if (t.n_inject == -1) t.n_inject = 0;
    else if (t.n_inject < 0 || t.n_inject >= t.n_particles) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_inject must be -1 (none), 0 (n_particles / 20) or in [1, n_particles)");
    if (!(t.sigma_init >= 0.0) || !(t.sigma_step >= 0.0) || std::isinf(t.sigma_init) || std::isinf(t.sigma_step))
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "sigma_init / sigma_step must be finite and >= 0 (0 = the grid step)");
    if (t.sigma_init == 0.0) t.sigma_init = (double)c->step;
    if (t.sigma_step == 0.0) t.sigma_step = (double)c->step;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    // built into locals (the state arrays at exactly their blob sizes, tracker_parts) and handed over behind the last step: a failure
    // leaves the context without a tracker, as it was
    const size_t slots = (size_t)c->cfg.max_arrays + 1;
    DevBuf<double> x, sd, res; DevBuf<int> si, sil;
    if (x.alloc(slots * t.n_particles) != hipSuccess || sd.alloc(slots * 2) != hipSuccess || si.alloc(slots * 4) != hipSuccess ||
        sil.alloc(slots) != hipSuccess || res.alloc(4) != hipSuccess)
        return fail(c, MCA_HIP_ERR_OUT_OF_MEMORY, "device memory for the DOA tracker's state");
    const int rc = trk_init_state(c, x, sd, si, nullptr);
    if (rc) return rc;
    c->d_trk_x.swap(x); c->d_trk_sd.swap(sd); c->d_trk_si.swap(si); c->d_trk_sil.swap(sil); c->d_trk_res.swap(res);
    c->trk = t;
    c->tracked = true;
    return MCA_HIP_OK;
}

int mca_hip_gcc2_tracker_get_particles(mca_hip_ctx *c, int array_index, double *particles, int *alive, int *track)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!c->tracked) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "no DOA tracker attached (mca_hip_gcc2_tracker_attach)");
    if (array_index < -1 || array_index >= c->cfg.max_arrays) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "array_index outside [-1, max_arrays) (-1: the frame hook)");
    const size_t slot = array_index < 0 ? (size_t)c->cfg.max_arrays : (size_t)array_index;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipDeviceSynchronize());
    if (particles) HIP_TRY(c, hipMemcpy(particles, c->d_trk_x + slot * c->trk.n_particles, (size_t)c->trk.n_particles * 8, hipMemcpyDeviceToHost));
    int si[4];
    HIP_TRY(c, hipMemcpy(si, c->d_trk_si + slot * 4, sizeof(si), hipMemcpyDeviceToHost));
    if (alive) *alive = si[0];
    if (track) *track = si[1];
    return MCA_HIP_OK;
}

int mca_hip_gcc2_frames_host(mca_hip_ctx *c, const float *pcm, int n_arrays, int n_frames, int *argmax,
                             float *doa_rad, float *prob, float *corr)
{
    if (!c || !pcm || !argmax) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_arrays < 1 || n_frames < 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_arrays/n_frames < 1");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const long long ms = (long long)(n_frames + 1) * c->H, as = ms * c->M;
    const size_t n_pcm = (size_t)as * n_arrays, n_f = (size_t)n_arrays * n_frames;
    // (the _dev call gets a buffer for doa_rad and prob whatever the caller takes back)
    StageBuf b[] = {{SG_PCM, pcm, n_pcm * 4, STAGE_IN}, {SG_ARGMAX, argmax, n_f * 4, STAGE_OUT}, {SG_DOA, doa_rad, n_f * 4, STAGE_OUT | STAGE_ALWAYS},
                    {SG_PROB, prob, n_f * 4, STAGE_OUT | STAGE_ALWAYS}, {SG_CORR, corr, n_f * c->D * 4, STAGE_OUT}};
    return staged(c, b, [&] {
        return mca_hip_gcc2_frames_dev(c, (float *)b[0].dev, as, ms, n_arrays, n_frames, (int *)b[1].dev, (float *)b[2].dev, (float *)b[3].dev, (float *)b[4].dev, nullptr);
    });
}

int mca_hip_copy_gate(mca_hip_ctx *c, unsigned char *voiced, float *power)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!c->cfg.use_power_floor) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "the context was created with use_power_floor = 0");
    if (c->last_frames == 0) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "no stream call has run yet");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipDeviceSynchronize());
    // (a gated call is never worked off in pieces, process_frames_host_impl: the one workspace holds the flags of all its arrays from 0)
    const size_t n = (size_t)c->last_arrays * c->last_frames;
    if (voiced) HIP_TRY(c, hipMemcpy(voiced, c->ws.d_voiced, n, hipMemcpyDeviceToHost));
    if (power) HIP_TRY(c, hipMemcpy(power, c->ws.d_power_out, n * 4, hipMemcpyDeviceToHost));
    return MCA_HIP_OK;
}

// ---- frame API ---------------------------------------------------------------------------
static int upload_frames(mca_hip_ctx *c, const double *const *frames, int ccs_len)
{
    if (!frames) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "frames is NULL");
    if (ccs_len != c->N + 2) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "ccs_len != fft_size + 2");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t n = (size_t)c->M * ccs_len;
    const int rc = grow_ws(c, c->d_fr, n, "the frame's spectra");
    if (rc) return rc;
    // SignalVector = one separate allocation per channel (mcadefs.h:86-88): gather, then one copy
    c->h_stage.resize(n);
    for (int m = 0; m < c->M; ++m) {
        if (!frames[m]) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "frames[c] is NULL");
        std::memcpy(c->h_stage.data() + (size_t)m * ccs_len, frames[m], (size_t)ccs_len * 8);
    }
    HIP_TRY(c, hipMemcpy(c->d_fr, c->h_stage.data(), n * 8, hipMemcpyHostToDevice));
    return MCA_HIP_OK;
}

int mca_hip_steering_process_frame(mca_hip_ctx *c, const double *const *frames, int ccs_len, double *DOA,
                                   double *prob, int *doa_bin, int n_sources)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (n_sources < 1 || n_sources > MCA_MAX_SOURCES) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_sources must be in [1,4]");
    if (!DOA || !prob) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "DOA/prob is NULL");
    int rc = upload_frames(c, frames, ccs_len);
    if (rc) return rc;
    const float memf = 0.8f;                                                  // SteeringBeamforming.h:70
    const double mu = (double)memf, omu = (double)(1 - memf);
    double *Ein = c->d_E64[c->e64_cur], *Eout = c->d_E64[c->e64_cur ^ 1];
    hipLaunchKernelGGL(k_frame_srp<double>, dim3(c->D), dim3(256), 0, 0, reinterpret_cast<const C2<double> *>(c->d_fr.p), c->K, c->D,
                       c->P, c->d_pairs, c->d_delays, Ein, Eout, mu, omu, c->cfg.gcc_weighting == MCA_HIP_GCC_NONE ? 1 : 0);
    hipLaunchKernelGGL(k_frame_pick<double>, dim3(1), dim3(512), 0, 0, Eout, c->D, c->P, n_sources, c->d_grid, c->d_res,
                       c->d_res + MCA_MAX_SOURCES, c->d_bins);
    HIP_TRY(c, hipGetLastError());
    c->e64_cur ^= 1;
    double res[2 * MCA_MAX_SOURCES]; int bins[MCA_MAX_SOURCES];
    HIP_TRY(c, hipMemcpy(res, c->d_res, sizeof(res), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(bins, c->d_bins, sizeof(bins), hipMemcpyDeviceToHost));
    for (int s = 0; s < n_sources; ++s) {
        DOA[s] = res[s]; prob[s] = res[MCA_MAX_SOURCES + s];
        if (doa_bin) doa_bin[s] = bins[s];
    }
    return MCA_HIP_OK;
}

int mca_hip_beamformer_process_frame(mca_hip_ctx *c, const double *const *frames, int ccs_len, double *out, double DOA)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!out) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "out is NULL");
    int rc = upload_frames(c, frames, ccs_len);
    if (rc) return rc;
    if ((rc = grow_ws(c, c->d_out64, (size_t)ccs_len, "the beamformed spectrum"))) return rc;
    hipLaunchKernelGGL(k_frame_beamform<double>, dim3((c->K + 255) / 256), dim3(256), 0, 0,
                       reinterpret_cast<const C2<double> *>(c->d_fr.p), c->M, c->K, c->cfg.sample_rate, c->d_micx, DOA,
                       reinterpret_cast<C2<double> *>(c->d_out64.p));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpy(out, c->d_out64, (size_t)ccs_len * 8, hipMemcpyDeviceToHost));
    return MCA_HIP_OK;
}

int mca_hip_fft_log_power(mca_hip_ctx *c, const double *const *frames, int ccs_len, double *power_db)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!power_db) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "power_db is NULL");
    int rc = upload_frames(c, frames, ccs_len);
    if (rc) return rc;
    double *dp = c->d_res + 2 * MCA_MAX_SOURCES;
    hipLaunchKernelGGL(k_frame_power<double>, dim3(1), dim3(256), 0, 0, reinterpret_cast<const C2<double> *>(c->d_fr.p), c->M, c->K, dp);
    HIP_TRY(c, hipGetLastError());
    double lin = 0;
    HIP_TRY(c, hipMemcpy(&lin, dp, 8, hipMemcpyDeviceToHost));
    *power_db = 10.0 * std::log10(lin);
    return MCA_HIP_OK;
}

int mca_hip_get_energy(mca_hip_ctx *c, double *out)
{
    if (!c || !out) return MCA_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipMemcpy(out, c->d_E64[c->e64_cur], (size_t)c->D * 8, hipMemcpyDeviceToHost));
    return MCA_HIP_OK;
}

// ---- FreqGCC: setProbability at caller-given angles and the frame hook ---------------------------------------------------
static int gcc2_prob_args(mca_hip_ctx *c, const void *doas, const void *probs, int n)
{
    if (c->M != 2) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "setProbability of the 2-microphone GCC path needs a context with n_mics == 2");
    if (n < 0) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n < 0");
    if (n > 0 && (!doas || !probs)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "doas/probs is NULL");
    return MCA_HIP_OK;
}

// host angles in, host probabilities out, one correlation row (synchronises: the row may still be written by a *_dev call)
extern "C++" template <typename TC>
static int gcc2_prob_host(mca_hip_ctx *c, const TC *row, const double *doas, double *probs, int n)
{
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipDeviceSynchronize());
    double *d_in = (double *)c->stage.get(SG_PROB_IN, (size_t)n * 8), *d_out = (double *)c->stage.get(SG_PROB_OUT, (size_t)n * 8);
    if (!d_in || !d_out) return fail(c, MCA_HIP_ERR_OUT_OF_MEMORY, "device staging buffers for the host-pointer call");
    HIP_TRY(c, hipMemcpy(d_in, doas, (size_t)n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL((k_gcc2_prob<TC, double>), dim3((n + 255) / 256, 1), dim3(256), 0, 0, row, 0LL, c->D, c->step, c->d_grid, d_in, d_out, n);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpy(probs, d_out, (size_t)n * 8, hipMemcpyDeviceToHost));
    return MCA_HIP_OK;
}

int mca_hip_gcc2_set_probability(mca_hip_ctx *c, int array_index, const double *doas, double *probs, int n)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    int rc = gcc2_prob_args(c, doas, probs, n);
    if (rc) return rc;
    if (array_index < 0 || array_index >= c->cfg.max_arrays) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "array_index outside [0, max_arrays)");
    if (n == 0) return MCA_HIP_OK;
    return gcc2_prob_host<float>(c, c->d_E[c->e_cur] + (size_t)array_index * c->D, doas, probs, n);
}

int mca_hip_gcc2_set_probability_dev(mca_hip_ctx *c, int n_arrays, const float *doas_dev, float *probs_dev, int n, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    int rc = gcc2_prob_args(c, doas_dev, probs_dev, n);
    if (rc) return rc;
    if (n_arrays < 0 || n_arrays > c->cfg.max_arrays) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_arrays outside [0, max_arrays]");
    if (n == 0 || n_arrays == 0) return MCA_HIP_OK;
    // d_E[e_cur] is the row the last ENQUEUED gcc2_frames_dev call writes: stream order does the rest
    hipLaunchKernelGGL((k_gcc2_prob<float, float>), dim3((n + 255) / 256, n_arrays), dim3(256), 0, (hipStream_t)stream, c->d_E[c->e_cur],
                       (long long)c->D, c->D, c->step, c->d_grid, doas_dev, probs_dev, n);
    HIP_TRY(c, hipGetLastError());
    return MCA_HIP_OK;
}

int mca_hip_gcc2_frame_set_probability(mca_hip_ctx *c, const double *doas, double *probs, int n)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    int rc = gcc2_prob_args(c, doas, probs, n);
    if (rc) return rc;
    if (n == 0) return MCA_HIP_OK;
    return gcc2_prob_host<double>(c, c->d_g2f_corr[c->g2f_cur], doas, probs, n);
}

// FreqGCCBinauralLocalisation::processParametrisation (BinauralLocalisation.cpp:406-567), deterministic branch, one frame.  The
// correlation, its smoothing, argmax, setProbability of the previous DOA and the DOA recursion are enqueued whatever the gate
// decides (one round trip per frame); a gated-out frame leaves the state's half of the double buffer current, so it changes nothing.
int mca_hip_gcc2_process_frame(mca_hip_ctx *c, const double *const *frames, int ccs_len, int *voiced, double *doa_rad,
                               double *prob, double *power, int *argmax, double *corr)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (c->M != 2) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "the FreqGCC frame hook needs a context with n_mics == 2");
    if (!voiced || !doa_rad || !prob || !power) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "voiced/doa_rad/prob/power is NULL");
    int rc = upload_frames(c, frames, ccs_len);
    if (rc) return rc;
    G2FrameState &g = c->g2f;
    const float corr_mem = (float)g.corr_mem, doa_mem = (float)g.doa_mem;
    const C2<double> *X = reinterpret_cast<const C2<double> *>(c->d_fr.p);
    double *Ein = c->d_g2f_corr[c->g2f_cur], *Eout = c->d_g2f_corr[c->g2f_cur ^ 1];
    hipLaunchKernelGGL(k_frame_power<double>, dim3(1), dim3(256), 0, 0, X, 2, c->K, c->d_g2f_res + 3);
    // GCC-PHAT at the D delays of the pair (0, 1), corr = (1 - mu) R + mu prev (:438-448)
    hipLaunchKernelGGL(k_frame_srp<double>, dim3(c->D), dim3(256), 0, 0, X, c->K, c->D, 1, c->d_pairs, c->d_delays, Ein, Eout,
                       (double)corr_mem, (double)(1 - corr_mem), c->cfg.gcc_weighting == MCA_HIP_GCC_NONE ? 1 : 0);
    hipLaunchKernelGGL(k_frame_gcc2<double>, dim3(1), dim3(64), 0, 0, Eout, c->D, c->step, c->d_grid, g.doa, (double)doa_mem,
                       (double)(1 - doa_mem), c->d_g2f_res);
    HIP_TRY(c, hipGetLastError());
    double res[4];
    HIP_TRY(c, hipMemcpy(res, c->d_g2f_res, sizeof(res), hipMemcpyDeviceToHost));
    // the gate (:425-434): setPowerFloor while the floor is estimated -- with or without usePowerFloor -- and `power` is the floor
    // meanwhile (:387-404); FFTLogPower afterwards
    double pw;
    if (g.noise_estimated == 0) {
        const int needed = (int)(3.0 * c->cfg.sample_rate);                    // _durationToEstimatePowerFloor (SoundLocalisationImpl.h:77)
        g.power_floor += res[3] * (ccs_len - 2) + 1e-10;                       // :390-391
        g.samples += ccs_len - 2;                                              // :392
        if (g.samples >= needed) {
            g.noise_estimated = 1;
            if (g.samples > 0) g.power_floor /= g.samples;
            g.power_floor = 10 * std::log10(g.power_floor) + (double)6.0f;      // _noiseMarginDB (BinauralLocalisation.h:197)
        }
        pw = g.power_floor;
    } else {
        pw = 10.0 * std::log10(res[3]);
    }
    const bool fire = pw > g.power_floor || !c->cfg.use_power_floor;          // :434
    int fired = fire ? 1 : 0;
    if (c->tracked) {
        // the DOA tracker on the hook's own state (slot max_arrays, key index 0xFFFFFFFF): one frame of the table in DESIGN.md.
        // The gate's decision and the counter are the host's, so they go in by value; DOA / prob / fired / track come back.
        Gcc2TrackArgs ta{};
        ta.corr = Eout; ta.corr_state = Ein;
        ta.windows_to_decay = 3 * c->cfg.sample_rate / (ccs_len / 2 - 1);
        ta.n_arrays = 1; ta.n_frames = 1;
        ta.key_a = 0xFFFFFFFFll; ta.state0 = c->cfg.max_arrays;
        ta.one_kind = fire ? 1 : (g.noise_estimated != 0 ? 2 : 0); ta.one_sil = (int)g.silence; ta.one_argmax = (int)res[0];
        ta.doa_out = c->d_trk_res; ta.prob_out = c->d_trk_res + 1;
        ta.fired = reinterpret_cast<unsigned char *>(c->d_trk_res + 2); ta.track = reinterpret_cast<int *>(c->d_trk_res + 3);
        launch_gcc2_track<double>(c, ta, nullptr);
        HIP_TRY(c, hipGetLastError());
        double out[4];
        HIP_TRY(c, hipMemcpy(out, c->d_trk_res, sizeof(out), hipMemcpyDeviceToHost));
        unsigned char f8; std::memcpy(&f8, &out[2], 1);
        fired = f8;
        res[1] = out[1]; res[2] = out[0];                                      // _prob (:454) and _currentDOA = updateFilter() (:473)
        if (!fire) { g.doa = out[0]; g.prob = out[1]; }                        // a coasting track moves the DOA (:545)
    }
    if (fire) {
        g.prob = res[1];                                                       // :454
        g.doa = res[2];                                                        // :502-504
        g.corr_mem = 0.8f; g.doa_mem = 0.6f; g.silence = 0;                    // :523-525
        c->g2f_cur ^= 1;
    } else if (g.noise_estimated != 0) {                                       // the silence rule (:530-560)
        const int windows_to_decay = 3 * c->cfg.sample_rate / (ccs_len / 2 - 1);
        if (g.silence < windows_to_decay) { g.corr_mem = 0.8f; g.doa_mem = 0.6f; }
        else { g.corr_mem = 0; g.doa_mem = 0; }
        g.silence += 1;
    }
    *voiced = fired;
    *doa_rad = g.doa; *prob = g.prob; *power = pw;
    if (argmax) *argmax = fire ? (int)res[0] : -1;
    if (corr) HIP_TRY(c, hipMemcpy(corr, c->d_g2f_corr[c->g2f_cur], (size_t)c->D * 8, hipMemcpyDeviceToHost));
    return MCA_HIP_OK;
}

// ---- timing ------------------------------------------------------------------------------
int mca_hip_set_timing(mca_hip_ctx *c, int enable)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    c->timing = enable != 0 ? ~0u : 0u;
    return MCA_HIP_OK;
}

int mca_hip_set_timing_mask(mca_hip_ctx *c, unsigned kernel_mask)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    c->timing = kernel_mask;
    return MCA_HIP_OK;
}

static int drain_events(mca_hip_ctx *c)
{
    for (auto &e : c->events) {
        HIP_TRY(c, hipEventSynchronize(e.b));
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, e.a, e.b));
        c->t_ms[e.id] += ms; c->t_launches[e.id] += 1;
        c->pool.push_back(e.a); c->pool.push_back(e.b);
    }
    c->events.clear();
    return MCA_HIP_OK;
}

int mca_hip_get_timing(mca_hip_ctx *c, int kernel_id, int *launches, double *total_ms)
{
    if (!c || kernel_id < 0 || kernel_id >= MCA_HIP_K_COUNT) return MCA_HIP_ERR_INVALID_ARGUMENT;
    int rc = drain_events(c);
    if (rc) return rc;
    if (launches) *launches = c->t_launches[kernel_id];
    if (total_ms) *total_ms = c->t_ms[kernel_id];
    return MCA_HIP_OK;
}

int mca_hip_reset_timing(mca_hip_ctx *c)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    int rc = drain_events(c);
    for (int i = 0; i < MCA_HIP_K_COUNT; ++i) { c->t_ms[i] = 0; c->t_launches[i] = 0; }
    if (c->d_rstats) { HIP_TRY(c, hipDeviceSynchronize()); HIP_TRY(c, hipMemset(c->d_rstats, 0, 32)); }
    c->adapt_frames_total = 0;
    c->fb_groups_prev = 0; c->fb_frames_prev = 0; c->fb_flagged_prev = 0; c->fb_seq_seen = c->fb_calls;   // (the reports in flight belong to the old totals)
    // ... including a probe's, if the back-off is waiting for one: that report will never count as fresh, so the wait ends here
    // and the mode resumes (the context stayed on FP16X3 until mca_hip_reset)
    if (c->fb_state == 2) { c->fb_state = 0; c->adapt_suspended = false; }
    return rc;
}

}  // extern "C"
