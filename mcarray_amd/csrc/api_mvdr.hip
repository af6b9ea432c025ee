// api_mvdr.hip -- C ABI of the MVDR-style beamformer with a per-bin spatial covariance (include/mcarray_hip.h,
// mca_hip_mvdr_*; BASELINE.json configs[3]; SURVEY A.9 -- no reference counterpart, conventions of Beamformer.cpp:59).
// Host side only: owns the per-stream state and the workspaces, checks a call, fills the argument structs and enqueues the kernels of
// kernels_mvdr*.hip and mvdr_solve.h.  Every launch is a plan (mvdr_plan.h: kernel form, grid, block, LDS, workspace sizes) handed to the one launch(); the
// kernels are looked up beside their code (kernels.h); a host-pointer call lists its buffers for the one staging helper (staged).  No CPU fallback.
#include "../../include/mcarray_hip.h"
#include "host_common.h"
#include "kernels.h"
#include "mvdr_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace mca;

// the timing slots: kernel_id of mca_hip_mvdr_get_timing (include/mcarray_hip.h)
enum MvdrTimer { T_ANALYSE, T_SOLVE, T_SYNTH, T_SPECTRUM, T_POSTFILTER, T_RTF, T_ESTMASK, T_TRACKS, T_MAP, T_TRACKS_MAP, T_COUNT, T_NONE = -1 };
static_assert(T_ANALYSE == 0 && T_SOLVE == 1 && T_SYNTH == 2 && T_SPECTRUM == 3 && T_POSTFILTER == 4 && T_RTF == 5 && T_ESTMASK == 6 && T_TRACKS == 7 &&
              T_MAP == 8 && T_TRACKS_MAP == 9 && T_COUNT == 10, "the public numbering of kernel_id");

struct mca_hip_mvdr_ctx : MvdrShape {
    mca_hip_mvdr_config cfg{};
    // Device memory: every d_* member owns its buffer (devbuf.h).  A state array is allocated at exactly its state size, so its n
    // is that size (init_state, mvdr_parts); a workspace only grows, and its n is a capacity that no state size is read from.
    DevBuf<float> d_window;
    DevBuf<float2> d_tw;
    DevBuf<double> d_micx;
    // the geometry of the steering vectors (mca_hip_mvdr_set_geometry): a processing parameter like null_gain
    int geo_mode = MCA_HIP_MVDR_GEOMETRY_LINEAR_X;
    double geo_elevation = 0.0;
    std::vector<double> geo_u;    // [3][M]: unit * x_m, unit * y_m, unit * z_m, unit = fs / N / 346.1
    DevBuf<double> d_geo_u;       // the same on the device (MvdrGeometry::u)
    // an elevation per look-direction slot (mca_hip_mvdr_set_elevations_*): a processing parameter, kept across reset, no part of the blobs
    DevBuf<double2> d_slot_el;    // [max_streams][MCA_MAX_SOURCES] (cos eps, sin eps) (MvdrGeometry::slot_el); an unset slot: the context's pair
    DevBuf<float> d_slot_val;     // [max_streams][MCA_MAX_SOURCES] the angle as mca_hip_mvdr_get_elevations reports it; NaN: unset
    DevBuf<float2> d_phi;         // [max_streams][K][tri]
    DevBuf<float> d_trace;        // [max_streams][K]
    DevBuf<float2> d_phi_tail; DevBuf<float> d_trace_tail;   // exit state of the pieced tail launch (<= 128 workgroups x 64 problems), copied back behind it
    int max_sources = 1;          // look directions per frame a call may carry (mca_hip_mvdr_set_max_sources)
    double null_gain = 0.0;       // soft nulls at the other look directions of a call with n_sources >= 2 (mca_hip_mvdr_set_null_gain);
                                  // a processing parameter, not stream state: no part of the state blobs
    bool rtf_nulls = false;       // the RTF-bodied calls honour null_gain, at the vectors of the steering plane (mca_hip_mvdr_set_rtf_nulls);
                                  // a processing parameter like null_gain
    DevBuf<float> d_tail[2]; int tail_cur = 0;   // [max_streams][max_sources][H]; a single-look call uses slot 0
    // the Wiener post-filter (mca_hip_mvdr_set_postfilter): the three values are processing parameters like null_gain; A is stream state
    bool pf_on = false;
    bool pf_ever = false;         // enabled at some time: timing slot 4 exists (a context that never enabled it refuses kernel_id 4 as it always did)
    double pf_smoothing = 0.98, pf_gain_floor = 0.1, pf_noise_scale = 1.0;
    DevBuf<float> d_pf_A;         // [max_streams][max_sources][K] |Z|^2 of the frame before; allocated while enabled
    DevBuf<float> d_pf_pn;        // workspace [rows x look directions][K]: the residual noise power of every output of the call; while enabled
    DevBuf<float> d_pf_ones;      // workspace [rows]: update weights of a call that brings none, all 1
    // steering vectors estimated from a target covariance (mca_hip_mvdr_set_rtf): the four values are processing parameters like
    // null_gain; Psi, cpsi and cphi are stream state, allocated while enabled
    bool rtf_on = false;
    bool rtf_ever = false;        // enabled at some time: timing slot 5 exists
    double rtf_alpha = 0.0, rtf_min_share = 0.05;   // (rtf_alpha: the context's alpha until set)
    int rtf_iterations = 2, rtf_ref = 0;
    DevBuf<float2> d_psi;         // [max_streams][max_sources][K][tri]
    DevBuf<float> d_cpsi;         // [max_streams][max_sources][K]
    DevBuf<float> d_cphi;         // [max_streams][K]
    DevBuf<float> d_cphi_next;    // exit value of the streams of a call, copied over d_cphi behind k_mvdr_rtf (MvdrRtfArgs::cphi_out)
    DevBuf<float2> d_D;           // workspace: the steering plane [rows x look directions][K][M] of a chunk of frames
    size_t plane_cap_cells = (size_t)1 << 27;            // its cap (1 GiB; mca_hip_mvdr_set_rtf_workspace): a call above it is cut along the frames
    DevBuf<float> d_rtf_ones;     // workspace [rows][K]: update mask of an RTF call that brings none, all 1
    // the mask estimator (mca_hip_mvdr_set_mask_estimator): processing parameters like null_gain, and no state at all
    bool em_on = false;
    bool em_ever = false;         // enabled at some time: timing slot 6 exists
    int em_bin_lo = 0, em_bin_hi = 0, em_protected = 0;   // (em_bin_hi: N/2 until set)
    double em_lo = 0.0, em_hi = 0.05;
    DevBuf<float> d_em_update;    // workspace [rows][K]: the update mask of an auto call that hands none back; while enabled
    DevBuf<float> d_em_target;    // workspace [rows x look directions][K]: its target masks
    // workspace
    DevBuf<float2> d_X;           // [rows][K][M]
    DevBuf<float2> d_Y, d_T;      // rows x look directions: [..][K], and the factored steering phasors [..][M][N/64 + 33]
    // the Capon spectrum of the held covariance (mca_hip_mvdr_spectrum_*): a processing parameter like null_gain, no part of the state blobs
    bool spec_set = false;
    mca_hip_mvdr_spectrum_config spec{};
    int spec_dpad = 0;                              // n_angles rounded up to whole waves
    std::vector<float> spec_grid;                   // [D] (float) theta_i
    DevBuf<float> d_spec_grid;
    DevBuf<float2> d_spec_T;                        // [M][N/64 + 33][Dpad] factored steering phasors of the grid (MvdrSpectrumArgs::T)
    DevBuf<float> d_spec_part;                      // workspace: partial sums [streams][chunks][4][Dpad]
    // the azimuth x elevation Capon map (mca_hip_mvdr_map_*): a processing parameter like the spectrum's configuration
    bool map_set = false;
    bool map_ever = false;        // configured at some time: timing slot 8 exists
    mca_hip_mvdr_map_config map{};
    int map_dpad = 0;                               // n_az n_el rounded up to whole waves
    std::vector<float> map_az, map_el;              // [n_az] (float) theta_i, [n_el] (float) eps_j
    DevBuf<float> d_map_az, d_map_el;
    DevBuf<float2> d_map_T;                         // [M][N/64 + 33][Dpad] over the flat list of directions j n_az + i (MvdrSpectrumArgs::T)
    DevBuf<float> d_map_part;                       // workspace: partial sums [streams of a pass][chunks][4][Dpad]
    // tracks of the look directions (mca_hip_mvdr_tracks_*): the configuration is a processing parameter like null_gain; theta, alive,
    // miss and gen are per-stream state that no state blob carries
    bool trk_on = false;
    bool trk_ever = false;        // configured at some time: timing slot 7 exists
    mca_hip_mvdr_tracks_config trk{};
    DevBuf<float> d_trk_theta; DevBuf<int> d_trk_int;   // [max_streams][MCA_MAX_SOURCES]; alive, miss, gen one behind the other
    DevBuf<float> d_trk_peak;                       // [2][max_streams][MCA_MAX_SOURCES]: the Capon peaks of an update (angles, values)
    DevBuf<float2> d_trk_T0;                        // [max_streams][MCA_MAX_SOURCES][M][N/64 + 33] phasors of the own tracks
    DevBuf<float> d_trk_part;                       // workspace: partial sums [streams][n_own][chunks][4][Dpad]
    // the tracks' map mode (mca_hip_mvdr_tracks_set_map, kernels_mvdr_trk2.hip): a second angle per slot, the candidates from the Capon map
    bool trk_map_on = false;
    bool trk_map_ever = false;    // enabled at some time: timing slot 9 exists
    mca_hip_mvdr_tracks_map_config trkm{};
    DevBuf<float> d_trk_eps;                        // [max_streams][MCA_MAX_SOURCES], beside d_trk_theta
    DevBuf<float> d_trk2_peak;                      // [3][max_streams][MCA_MAX_SOURCES]: the map's peaks of an update (az, el, values)
    DevBuf<float2> d_trk2_U;                        // workspace: u [streams of a pass][n_own][chunks][64][M]
    DevBuf<int> d_trk2_F;                           // workspace: used [streams of a pass][n_own][chunks][64]
    DevBuf<float> d_trk2_part;                      // workspace: partial sums [streams of a pass][n_own][chunks][4][Dpad]
    StagePool stage;
    bool timing = false;
    struct Ev { int id; hipEvent_t a, b; };
    std::vector<Ev> events;
    int t_launches[T_COUNT] = {};
    double t_ms[T_COUNT] = {};
    std::string err;
};

namespace {

mca_hip_mvdr_ctx *const NO_CTX = nullptr;        // a failing create: the text goes to the module's creation error

void free_mvdr(mca_hip_mvdr_ctx *c)
{
    if (!c) return;
    for (auto &e : c->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    delete c;                                                  // every device buffer goes with its member
}

// elements of a per-source array [max_streams][slots][row] (slots = 1: of a per-stream array [max_streams][row])
inline size_t slot_elems(const mca_hip_mvdr_ctx *c, int slots, size_t row) { return (size_t)c->cfg.max_streams * slots * row; }

// a workspace of at least n elements; wait: the device is waited for before it grows (a call in flight may read the former one)
template <typename T>
int grow_ws(mca_hip_mvdr_ctx *c, DevBuf<T> &b, size_t n, const char *what, bool wait = false)
{
    if (wait && n > b.n) HIP_TRY(c, hipDeviceSynchronize());
    const hipError_t e = b.grow(n);
    return e == hipSuccess ? MCA_HIP_OK : hip_fail(c, e, what);
}

// weights of 1 for a call that brings none: at least n of them
hipError_t ensure_ones(DevBuf<float> &b, size_t n)
{
    if (n <= b.n) return hipSuccess;
    const std::vector<float> ones(n, 1.f);
    return b.upload(ones.data(), n);
}

// the array [max_streams][old_slots][row] laid out anew for new_slots: the slots both layouts have keep their content, the
// others start at zero.  Synchronous; `fresh` is empty on failure
template <typename T>
hipError_t reslot(const mca_hip_mvdr_ctx *c, const DevBuf<T> &old, int old_slots, int new_slots, size_t row, DevBuf<T> &fresh)
{
    const size_t rb = row * sizeof(T);
    hipError_t e = fresh.alloc_zero(slot_elems(c, new_slots, row));
    if (e == hipSuccess) e = hipMemcpy2D(fresh.p, new_slots * rb, old.p, old_slots * rb, std::min(old_slots, new_slots) * rb, (size_t)c->cfg.max_streams, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) fresh.reset();
    return e;
}

// a slot the call leaves out restarts from nothing: the slots n_sources ... max_sources - 1 of the first n_streams streams of
// buf [max_streams][max_sources][row_elems] are cleared on the stream.  The kernels touch only the slots below n_sources
template <typename T>
hipError_t clear_unused_slots(const mca_hip_mvdr_ctx *c, T *buf, size_t row_elems, int n_sources, int n_streams, hipStream_t st)
{
    if (n_sources >= c->max_sources) return hipSuccess;
    const size_t rb = row_elems * sizeof(T);
    return hipMemset2DAsync(buf + n_sources * row_elems, c->max_sources * rb, 0, (c->max_sources - n_sources) * rb, (size_t)n_streams, st);
}

MvdrGeometry geometry_args(const mca_hip_mvdr_ctx *c)
{
    return MvdrGeometry{c->geo_mode == MCA_HIP_MVDR_GEOMETRY_XYZ ? 1 : 0, c->d_geo_u, std::cos(c->geo_elevation), std::sin(c->geo_elevation), c->d_slot_el};
}

// every look-direction slot back to unset: the context's pair, NaN as its angle.  Synchronous; the caller has waited for the device
hipError_t reset_elevations(mca_hip_mvdr_ctx *c)
{
    const size_t n = (size_t)c->cfg.max_streams * MCA_MAX_SOURCES;
    const std::vector<double2> pairs(n, make_double2(std::cos(c->geo_elevation), std::sin(c->geo_elevation)));
    const std::vector<float> vals(n, std::nanf(""));
    hipError_t e = hipMemcpy(c->d_slot_el, pairs.data(), n * sizeof(double2), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->d_slot_val, vals.data(), n * sizeof(float), hipMemcpyHostToDevice);
    return e;
}

// the tracks end, and their map mode with them: configured anew
void tracks_off(mca_hip_mvdr_ctx *c)
{
    if (c->trk_on) { c->trk_on = false; c->trk.enable = 0; }
    c->trk_map_on = false;
}

// turns per unit of kk of microphone m towards theta: what the steering tables of the kernels form (mvdr_projection), on the host
// the XYZ arm: the projection on e(theta, eps) with ce = cos eps, se = sin eps
double host_projection_xyz(const mca_hip_mvdr_ctx *c, int m, double theta, double ce, double se)
{
    const int M = c->M;
    const double cd = std::cos(theta + M_PI / 2), cy = -std::cos(theta);
    double pr = c->geo_u[m] * (cd * ce);
    if (c->geo_u[M + m] != 0.0) pr += c->geo_u[M + m] * (cy * ce);
    if (c->geo_u[2 * M + m] != 0.0) pr -= c->geo_u[2 * M + m] * se;
    return pr;
}
double host_projection(const mca_hip_mvdr_ctx *c, int m, double theta)
{
    if (c->geo_mode != MCA_HIP_MVDR_GEOMETRY_XYZ) return c->geo_u[m] * std::cos(theta + M_PI / 2);   // (unit x_m) cd, Beamformer.cpp:59
    return host_projection_xyz(c, m, theta, std::cos(c->geo_elevation), std::sin(c->geo_elevation));
}

// the factored phasors of one (direction, microphone) with projection u: exp(-j 2 pi 32 i u), i <= N/64, and exp(-j 2 pi i u), i < 32
// (MvdrAnalyseArgs::T), written with stride `stride`
void host_phasors(double u, int nhi, int nph, float2 *T, size_t stride)
{
    for (int e = 0; e < nph; ++e) {
        double t = (e < nhi ? 32.0 * e : (double)(e - nhi)) * u;
        t -= std::floor(t);
        T[(size_t)e * stride] = make_float2((float)std::cos(2.0 * M_PI * t), (float)(-std::sin(2.0 * M_PI * t)));
    }
}

// every state array from nothing (those of a feature that is off are empty, and cleared as such)
int init_state(mca_hip_mvdr_ctx *c, hipStream_t st)
{
    HIP_TRY(c, c->d_phi.zero_async(st));
    HIP_TRY(c, c->d_trace.zero_async(st));
    for (int i = 0; i < 2; ++i) HIP_TRY(c, c->d_tail[i].zero_async(st));
    HIP_TRY(c, c->d_pf_A.zero_async(st));
    HIP_TRY(c, c->d_psi.zero_async(st));
    HIP_TRY(c, c->d_cpsi.zero_async(st));
    HIP_TRY(c, c->d_cphi.zero_async(st));
    HIP_TRY(c, c->d_trk_theta.zero_async(st));
    HIP_TRY(c, c->d_trk_int.zero_async(st));
    HIP_TRY(c, c->d_trk_eps.zero_async(st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return MCA_HIP_OK;
}

// the workspaces of a call of `rows` (stream, frame) pairs; plane_rows: those of a chunk of an RTF call
int ensure_ws(mca_hip_mvdr_ctx *c, size_t rows, int n_sources, bool want_ones, bool rtf, size_t plane_rows = 0)
{
    int rc;
    if (rtf) {
        if ((rc = grow_ws(c, c->d_D, plane_rows * n_sources * c->K * c->M, "steering plane of the RTF call"))) return rc;
        // the solve behind k_mvdr_rtf takes a weight per cell: a call without an update mask passes ones, whose bytes are those of no weights
        if (want_ones)
            if (const hipError_t e = ensure_ones(c->d_rtf_ones, rows * c->K)) return hip_fail(c, e, "update mask of ones of the RTF call");
        want_ones = false;
    }
    // a call without update weights still takes the gated kernels (they emit the noise plane): weights of 1, whose bytes are
    // those of the unweighted kernels
    if (c->pf_on && want_ones)
        if (const hipError_t e = ensure_ones(c->d_pf_ones, rows)) return hip_fail(c, e, "update weights of ones of the post-filter");
    if ((rc = grow_ws(c, c->d_X, rows * c->K * c->M, "spectra of the call"))) return rc;
    const size_t yrows = rows * n_sources;
    if ((rc = grow_ws(c, c->d_Y, yrows * c->K, "beamformed spectra of the call"))) return rc;
    if ((rc = grow_ws(c, c->d_T, yrows * c->M * (c->N / 64 + 33), "steering tables of the call"))) return rc;
    if (c->pf_on && (rc = grow_ws(c, c->d_pf_pn, yrows * c->K, "noise plane of the post-filter"))) return rc;
    return MCA_HIP_OK;
}

// the masks of an auto call that the caller does not take back: workspace that grows with the call's shape, as d_T does
int ensure_estmask_ws(mca_hip_mvdr_ctx *c, size_t rows, int n_sources, bool want_update, bool want_target)
{
    int rc;
    if (want_update && (rc = grow_ws(c, c->d_em_update, rows * c->K, "estimated update mask"))) return rc;
    if (want_target && (rc = grow_ws(c, c->d_em_target, rows * n_sources * c->K, "estimated target masks"))) return rc;
    return MCA_HIP_OK;
}

void t_begin(mca_hip_mvdr_ctx *c, MvdrTimer id, hipStream_t st)
{
    if (!c->timing) return;
    mca_hip_mvdr_ctx::Ev ev; ev.id = id;
    (void)hipEventCreate(&ev.a); (void)hipEventCreate(&ev.b);
    (void)hipEventRecord(ev.a, st);
    c->events.push_back(ev);
}
void t_end(mca_hip_mvdr_ctx *c, hipStream_t st)
{
    if (!c->timing) return;
    (void)hipEventRecord(c->events.back().b, st);
}

// The launcher of the MVDR path, on the attribute rule of host_common.h (lds_limit): a kernel (the lookups of kernels.h, or kptr), a plan's grid, block and dynamic LDS, and the kernel's argument struct (arg2:
// the second argument of the two kernels that take one).  slot: the timing slot whose events bracket the
// launch; T_NONE inside a stage of several launches, which keeps one pair around all of them (t_begin / t_end).  Launch errors surface at the call's hipGetLastError.
int launch(mca_hip_mvdr_ctx *c, const void *kernel, dim3 grid, dim3 block, int lds, void *args, MvdrTimer slot, hipStream_t st, void *arg2 = nullptr)
{
    if (const int rc = lds_limit(c, kernel, (size_t)lds)) return rc;      // (outside the events, and before any is recorded)
    void *kargs[2] = {args, arg2};
    if (slot != T_NONE) t_begin(c, slot, st);
    (void)hipLaunchKernel(kernel, grid, block, kargs, (size_t)lds, st);
    if (slot != T_NONE) t_end(c, st);
    return MCA_HIP_OK;
}
template <class... A> const void *kptr(void (*k)(A...)) { return reinterpret_cast<const void *>(k); }

// The solve kernel of a choice (mvdr_plan.h) and the dynamic LDS of its workgroups, from each family's lookup beside its code (kernels.h); nullptr: not in the build
const void *mvdr_solve_kernel(const MvdrSolveChoice &k, int &lds)
{
    const int Q = k.Q, n_sources = k.S;
    typedef const void *(*Of)(int, bool, int, bool, int *);
    static const Of of[3][2] = {{mvdr_solve_kernel_of<MvdrWeight::NONE, false>, nullptr}, {mvdr_solve_kernel_of<MvdrWeight::FRAME, false>, mvdr_solve_kernel_of<MvdrWeight::FRAME, true>},
                                {mvdr_solve_kernel_of<MvdrWeight::CELL, false>, mvdr_solve_kernel_of<MvdrWeight::CELL, true>}};      // [weight][noise]
    lds = 0;
    switch (k.family) {
    case MvdrSolveFamily::HAND: return mvdr_solve_hand_kernel(Q, k.full);
    case MvdrSolveFamily::RTF: return k.noise ? mvdr_solve_rtf_kernel_of<true>(Q, k.full, n_sources) : mvdr_solve_rtf_kernel_of<false>(Q, k.full, n_sources);
    case MvdrSolveFamily::RTF_NULLS: return k.noise ? mvdr_solve_rtf_nulls_kernel_of<true>(Q, n_sources, &lds) : mvdr_solve_rtf_nulls_kernel_of<false>(Q, n_sources, &lds);
    default: return of[(int)k.weight][k.noise] ? of[(int)k.weight][k.noise](Q, k.full, n_sources, k.nulls, &lds) : nullptr;
    }
}

// the staging-pool slots of the host-pointer calls (stage.h).  The pool's buffers are reused across calls by number: the numbers stay
enum MvdrStageSlot {
    SG_PCM = 0,           // the frames calls: the samples
    SG_DOA = 1,           // the frames calls: the look directions
    SG_OUT_PCM = 2,       // the frames calls: the audio
    SG_OUT_SPEC = 3,      // the frames calls: the beamformed spectra
    SG_SCAN = 4,          // spectrum: the spectrum; map: the map; tracks update: own_spectrum; map-mode update: own_map
    SG_AUX1 = 5,          // spectrum: peak_doa; map: peak_az; both tracks updates: own_used; map-mode seed: az
    SG_AUX2 = 6,          // spectrum: peak_val; map: peak_el; tracks seed and fill: doa; map-mode seed: el
    SG_WEIGHTS = 7,       // the frames calls: the update weights per frame; map: peak_val
    SG_UPDATE_MASK = 8,   // the frames calls: the update mask per cell, taken or (auto call) handed back
    SG_TARGET_MASK = 9,   // the frames calls: the target masks, taken or (auto call) handed back
};
static_assert(SG_TARGET_MASK + 1 == StagePool::N, "a slot per buffer of the pool");
// (a host-pointer call lists its buffers for staged, host_common.h: host NULL means nothing staged)

}  // namespace

extern "C" {

const char *mca_hip_mvdr_last_error(const mca_hip_mvdr_ctx *ctx) { return last_error(ctx); }

int mca_hip_mvdr_create(const mca_hip_mvdr_config *cfg, mca_hip_mvdr_ctx **out)
{
    if (!cfg || !out) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "cfg/out is NULL");
    *out = nullptr;
    if (cfg->struct_size != (int)sizeof(mca_hip_mvdr_config)) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "struct_size mismatch");
    if (cfg->fft_size < 64 || (cfg->fft_size & (cfg->fft_size - 1)) || cfg->fft_size > 8192)
        return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "fft_size must be a power of two in [64,8192]");
    if (cfg->sample_rate <= 0) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "sample_rate <= 0");
    if (cfg->n_mics < 2 || cfg->n_mics > 16) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "n_mics must be in [2,16]");
    if (!cfg->mic_xyz) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "mic_xyz is NULL");
    if (!(cfg->alpha >= 0.0 && cfg->alpha < 1.0)) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "alpha must be in [0,1)");
    if (!(cfg->loading > 0.0)) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "loading must be > 0 (the first M-1 covariances of a stream are rank deficient)");
    if (cfg->max_streams < 1) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "max_streams < 1");
    if ((size_t)cfg->n_mics * (cfg->fft_size / 2 + 1) * 8 > 160 * 1024)
        return fail(NO_CTX, MCA_HIP_ERR_UNSUPPORTED, "n_mics spectra of N/2+1 bins exceed the 160 KiB LDS of a CU");
    if (const int rc = check_device(NO_CTX, cfg->device)) return rc;

    mca_hip_mvdr_ctx *c = new mca_hip_mvdr_ctx();
    c->cfg = *cfg; c->cfg.mic_xyz = nullptr;
    c->rtf_alpha = cfg->alpha;
    c->N = cfg->fft_size; c->H = c->N / 2; c->K = c->H + 1; c->M = cfg->n_mics; c->tri = c->M * (c->M + 1) / 2; c->max_streams = cfg->max_streams;
    c->em_bin_hi = c->N / 2;
    while ((1 << c->logH) < c->H) ++c->logH;
    std::vector<float> win(c->N);
    for (int n = 0; n < c->N; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / c->N));
    std::vector<float2> tw(c->N / 2);
    for (int i = 0; i < c->N / 2; ++i) tw[i] = make_float2((float)std::cos(2.0 * M_PI * i / c->N), (float)(-std::sin(2.0 * M_PI * i / c->N)));
    std::vector<double> mx(c->M);
    for (int m = 0; m < c->M; ++m) mx[m] = cfg->mic_xyz[3 * m];                                                // Beamformer.cpp:59: x only
    c->geo_u.resize((size_t)3 * c->M);                                                                          // all three for XYZ mode
    const double unit = (double)cfg->sample_rate / (double)c->N / 346.1;
    for (int m = 0; m < c->M; ++m)
        for (int j = 0; j < 3; ++j) c->geo_u[(size_t)j * c->M + m] = unit * cfg->mic_xyz[3 * m + j];

    const size_t nk = slot_elems(c, 1, c->K);
    hipError_t e = c->d_window.upload(win.data(), win.size());
    if (e == hipSuccess) e = c->d_tw.upload(tw.data(), tw.size());
    if (e == hipSuccess) e = c->d_micx.upload(mx.data(), mx.size());
    if (e == hipSuccess) e = c->d_geo_u.upload(c->geo_u.data(), c->geo_u.size());
    if (e == hipSuccess) e = c->d_slot_el.alloc((size_t)cfg->max_streams * MCA_MAX_SOURCES);
    if (e == hipSuccess) e = c->d_slot_val.alloc((size_t)cfg->max_streams * MCA_MAX_SOURCES);
    if (e == hipSuccess) e = reset_elevations(c);
    if (e == hipSuccess) e = c->d_phi.alloc(nk * c->tri);
    if (e == hipSuccess) e = c->d_trace.alloc(nk);
    if (e == hipSuccess) e = c->d_phi_tail.alloc((size_t)128 * 64 * c->tri);
    if (e == hipSuccess) e = c->d_trace_tail.alloc((size_t)128 * 64);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = c->d_tail[i].alloc(slot_elems(c, c->max_sources, c->H));
    const int rc = e != hipSuccess ? hip_fail(c, e, "tables and state of the context") : init_state(c, nullptr);
    if (rc) return create_failed(c, rc, free_mvdr);
    *out = c;
    return MCA_HIP_OK;
}

void mca_hip_mvdr_destroy(mca_hip_mvdr_ctx *c) { destroy_ctx(c, free_mvdr); }

int mca_hip_mvdr_reset(mca_hip_mvdr_ctx *c, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return init_state(c, (hipStream_t)stream);
}

int mca_hip_mvdr_set_max_sources(mca_hip_mvdr_ctx *c, int max_sources)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (max_sources < 1 || max_sources > MCA_MAX_SOURCES) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "max_sources must be in [1,4]");
    if (max_sources == c->max_sources) return MCA_HIP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipDeviceSynchronize());
    // every array [max_streams][max_sources][...] is built anew by the slot rule (reslot) and swapped in once all of them stand:
    // a failure leaves the context as it was.  The tail that is not current starts at zero
    const int old = c->max_sources;
    DevBuf<float> nt[2], ncpsi, na;
    DevBuf<float2> npsi;
    hipError_t e = reslot(c, c->d_tail[c->tail_cur], old, max_sources, c->H, nt[0]);
    if (e == hipSuccess) e = nt[1].alloc_zero(slot_elems(c, max_sources, c->H));
    if (e != hipSuccess) return hip_fail(c, e, "overlap-add tails of the new sources");
    if (c->rtf_on) {
        e = reslot(c, c->d_psi, old, max_sources, (size_t)c->K * c->tri, npsi);
        if (e == hipSuccess) e = reslot(c, c->d_cpsi, old, max_sources, c->K, ncpsi);
        if (e != hipSuccess) return hip_fail(c, e, "target covariances of the new sources");
    }
    if (c->pf_on && (e = reslot(c, c->d_pf_A, old, max_sources, c->K, na)) != hipSuccess) return hip_fail(c, e, "post-filter state of the new sources");
    c->d_tail[0].swap(nt[0]); c->d_tail[1].swap(nt[1]); c->tail_cur = 0;
    c->d_psi.swap(npsi); c->d_cpsi.swap(ncpsi); c->d_pf_A.swap(na);    // (empty for empty where the feature is off)
    c->max_sources = max_sources;
    if (c->trk_on && max_sources < c->trk.n_tracks) tracks_off(c);                                  // fewer slots than tracks
    return MCA_HIP_OK;
}

int mca_hip_mvdr_set_null_gain(mca_hip_mvdr_ctx *c, double null_gain)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    // the cap: the denominator of the nulled output cancels by up to 1 + null_gain, and fp32 eps (1 + 1000) stays an order of
    // magnitude under the module's 5e-4 parity bar
    if (!std::isfinite(null_gain) || null_gain < 0.0 || null_gain > 1000.0)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "null_gain must be finite and in [0,1000]");
    c->null_gain = null_gain;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_get_null_gain(const mca_hip_mvdr_ctx *c, double *null_gain)
{
    if (!c || !null_gain) return MCA_HIP_ERR_INVALID_ARGUMENT;
    *null_gain = c->null_gain;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_set_rtf_nulls(mca_hip_mvdr_ctx *c, int enable)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (enable != 0 && enable != 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "enable must be 0 or 1");
    c->rtf_nulls = enable == 1;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_get_rtf_nulls(const mca_hip_mvdr_ctx *c, int *enable)
{
    if (!c || !enable) return MCA_HIP_ERR_INVALID_ARGUMENT;
    *enable = c->rtf_nulls ? 1 : 0;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_set_geometry(mca_hip_mvdr_ctx *c, const mca_hip_mvdr_geometry_config *cfg)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!cfg) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (cfg->struct_size != (int)sizeof(mca_hip_mvdr_geometry_config)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "struct_size mismatch");
    if (cfg->mode != MCA_HIP_MVDR_GEOMETRY_LINEAR_X && cfg->mode != MCA_HIP_MVDR_GEOMETRY_XYZ)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "mode must be 0 (linear, x only) or 1 (xyz)");
    if (!std::isfinite(cfg->elevation_rad) || std::fabs(cfg->elevation_rad) > M_PI / 2)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "elevation_rad must be finite and in [-pi/2, pi/2]");
    // LINEAR_X ignores the elevation: it is kept as 0 there, so that setting it is no change
    const double el = cfg->mode == MCA_HIP_MVDR_GEOMETRY_XYZ ? cfg->elevation_rad : 0.0;
    if (cfg->mode == c->geo_mode && el == c->geo_elevation) return MCA_HIP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipDeviceSynchronize());                       // no call in flight reads the tables of the former geometry
    c->geo_mode = cfg->mode; c->geo_elevation = el;
    if (const hipError_t e = reset_elevations(c)) return hip_fail(c, e, "elevations of the look-direction slots");   // unset: the new pair
    c->spec_set = false;                                       // its phasor table and grid are stale (freed by the next configure)
    c->map_set = false;                                        // and so are the map's
    tracks_off(c);                                             // the angles change meaning: configured anew
    return MCA_HIP_OK;
}

int mca_hip_mvdr_get_geometry(const mca_hip_mvdr_ctx *c, mca_hip_mvdr_geometry_config *cfg)
{
    if (!c || !cfg) return MCA_HIP_ERR_INVALID_ARGUMENT;
    cfg->struct_size = (int)sizeof(mca_hip_mvdr_geometry_config);
    cfg->mode = c->geo_mode; cfg->elevation_rad = c->geo_elevation;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_set_postfilter(mca_hip_mvdr_ctx *c, const mca_hip_mvdr_postfilter_config *cfg)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!cfg) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (cfg->struct_size != (int)sizeof(mca_hip_mvdr_postfilter_config)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "struct_size mismatch");
    if (!std::isfinite(cfg->smoothing) || cfg->smoothing < 0.0 || cfg->smoothing >= 1.0)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "smoothing must be finite and in [0,1)");
    if (!std::isfinite(cfg->gain_floor) || cfg->gain_floor < 0.0 || cfg->gain_floor > 1.0)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "gain_floor must be finite and in [0,1]");
    if (!std::isfinite(cfg->noise_scale) || !(cfg->noise_scale > 0.0) || cfg->noise_scale > 100.0)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "noise_scale must be finite and in (0,100]");
    const bool on = cfg->enable != 0;
    if (on != c->pf_on) {
        HIP_TRY(c, hipSetDevice(c->cfg.device));
        HIP_TRY(c, hipDeviceSynchronize());                   // no call in flight reads what is freed here
        if (on) {
            // A starts from zero; the noise plane and the ones come with the first call (ensure_ws)
            DevBuf<float> na;
            if (const hipError_t e = na.alloc_zero(slot_elems(c, c->max_sources, c->K))) return hip_fail(c, e, "post-filter state");
            c->d_pf_A.swap(na);
        } else {
            c->d_pf_A.reset(); c->d_pf_pn.reset(); c->d_pf_ones.reset();
        }
        c->pf_on = on;
        if (on) c->pf_ever = true;
    }
    c->pf_smoothing = cfg->smoothing; c->pf_gain_floor = cfg->gain_floor; c->pf_noise_scale = cfg->noise_scale;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_get_postfilter(const mca_hip_mvdr_ctx *c, mca_hip_mvdr_postfilter_config *cfg)
{
    if (!c || !cfg) return MCA_HIP_ERR_INVALID_ARGUMENT;
    cfg->struct_size = (int)sizeof(mca_hip_mvdr_postfilter_config);
    cfg->enable = c->pf_on ? 1 : 0;
    cfg->smoothing = c->pf_smoothing; cfg->gain_floor = c->pf_gain_floor; cfg->noise_scale = c->pf_noise_scale;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_set_rtf(mca_hip_mvdr_ctx *c, const mca_hip_mvdr_rtf_config *cfg)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!cfg) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (cfg->struct_size != (int)sizeof(mca_hip_mvdr_rtf_config)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "struct_size mismatch");
    if (!std::isfinite(cfg->target_alpha) || cfg->target_alpha < 0.0 || cfg->target_alpha >= 1.0)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "target_alpha must be finite and in [0,1)");
    if (cfg->iterations < 1 || cfg->iterations > 4) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "iterations must be in [1,4]");
    if (cfg->ref_mic < 0 || cfg->ref_mic >= c->M) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "ref_mic must be in [0, n_mics)");
    if (!std::isfinite(cfg->min_share) || cfg->min_share < 0.0 || cfg->min_share >= 1.0)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "min_share must be finite and in [0,1)");
    const bool on = cfg->enable != 0;
    if (on != c->rtf_on) {
        HIP_TRY(c, hipSetDevice(c->cfg.device));
        HIP_TRY(c, hipDeviceSynchronize());                   // no call in flight reads what is freed here
        if (on) {
            // Psi = 0, cpsi = 0; cphi = 1 where the covariance holds something (its weights were not counted: taken as complete)
            DevBuf<float2> npsi;
            DevBuf<float> ncpsi, ncphi, nnext;
            std::vector<float> tr(c->d_trace.n);
            hipError_t e = npsi.alloc_zero(slot_elems(c, c->max_sources, (size_t)c->K * c->tri));
            if (e == hipSuccess) e = ncpsi.alloc_zero(slot_elems(c, c->max_sources, c->K));
            if (e == hipSuccess) e = nnext.alloc(tr.size());
            if (e == hipSuccess) e = hipMemcpy(tr.data(), c->d_trace, c->d_trace.bytes(), hipMemcpyDeviceToHost);
            for (auto &v : tr) v = v > 1e-30f ? 1.f : 0.f;
            if (e == hipSuccess) e = ncphi.upload(tr.data(), tr.size());
            if (e != hipSuccess) return hip_fail(c, e, "RTF state");
            c->d_psi.swap(npsi); c->d_cpsi.swap(ncpsi); c->d_cphi.swap(ncphi); c->d_cphi_next.swap(nnext);
        } else {
            c->d_psi.reset(); c->d_cpsi.reset(); c->d_cphi.reset(); c->d_cphi_next.reset(); c->d_D.reset(); c->d_rtf_ones.reset();
            tracks_off(c);                                               // own tracks read Psi and a birth clears it: configured anew
        }
        c->rtf_on = on;
        if (on) c->rtf_ever = true;
    }
    c->rtf_alpha = cfg->target_alpha; c->rtf_iterations = cfg->iterations; c->rtf_ref = cfg->ref_mic; c->rtf_min_share = cfg->min_share;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_set_rtf_workspace(mca_hip_mvdr_ctx *c, long long max_bytes)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (max_bytes < 8) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "max_bytes must be at least 8");
    c->plane_cap_cells = (size_t)(max_bytes / 8);          // (a plane already held stays until a call needs a larger one)
    return MCA_HIP_OK;
}

int mca_hip_mvdr_get_rtf(const mca_hip_mvdr_ctx *c, mca_hip_mvdr_rtf_config *cfg)
{
    if (!c || !cfg) return MCA_HIP_ERR_INVALID_ARGUMENT;
    cfg->struct_size = (int)sizeof(mca_hip_mvdr_rtf_config);
    cfg->enable = c->rtf_on ? 1 : 0;
    cfg->target_alpha = c->rtf_alpha; cfg->iterations = c->rtf_iterations; cfg->ref_mic = c->rtf_ref; cfg->min_share = c->rtf_min_share;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_set_mask_estimator(mca_hip_mvdr_ctx *c, const mca_hip_mvdr_estmask_config *cfg)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!cfg) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (cfg->struct_size != (int)sizeof(mca_hip_mvdr_estmask_config)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "struct_size mismatch");
    if (cfg->bin_lo < 0 || cfg->bin_lo > cfg->bin_hi || cfg->bin_hi > c->N / 2)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "the band must satisfy 0 <= bin_lo <= bin_hi <= N/2");
    if (!std::isfinite(cfg->coherence_lo) || !std::isfinite(cfg->coherence_hi) || cfg->coherence_lo < 0.0 || cfg->coherence_hi > 1.0 ||
        !(cfg->coherence_hi - cfg->coherence_lo >= 1e-3))
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "the thresholds must be finite with 0 <= coherence_lo, coherence_hi <= 1 and coherence_hi - coherence_lo >= 1e-3");
    if (cfg->n_protected < 0 || cfg->n_protected > MCA_MAX_SOURCES) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_protected must be in [0,4]");
    const bool on = cfg->enable != 0;
    if (on != c->em_on) {
        if (!on) {
            HIP_TRY(c, hipSetDevice(c->cfg.device));
            HIP_TRY(c, hipDeviceSynchronize());               // no call in flight reads what is freed here
            c->d_em_update.reset(); c->d_em_target.reset();
        }
        c->em_on = on;                                         // (the workspace comes with the first auto call: ensure_estmask_ws)
        if (on) c->em_ever = true;
    }
    c->em_bin_lo = cfg->bin_lo; c->em_bin_hi = cfg->bin_hi; c->em_lo = cfg->coherence_lo; c->em_hi = cfg->coherence_hi; c->em_protected = cfg->n_protected;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_get_mask_estimator(const mca_hip_mvdr_ctx *c, mca_hip_mvdr_estmask_config *cfg)
{
    if (!c || !cfg) return MCA_HIP_ERR_INVALID_ARGUMENT;
    cfg->struct_size = (int)sizeof(mca_hip_mvdr_estmask_config);
    cfg->enable = c->em_on ? 1 : 0;
    cfg->bin_lo = c->em_bin_lo; cfg->bin_hi = c->em_bin_hi; cfg->coherence_lo = c->em_lo; cfg->coherence_hi = c->em_hi; cfg->n_protected = c->em_protected;
    return MCA_HIP_OK;
}

namespace {

// A call with n_sources look directions per frame, every pointer of the same side (device for mvdr_frames_dev and the launches,
// host for mvdr_frames_host).  doa [streams][F][n_sources], out_pcm [streams][n_sources][F hop], out_spec [streams][n_sources][F][K]
// update: covariance update weights [streams][F], or [streams][F][K] (masked), or NULL (all 1)
// rtf: the call of mca_hip_mvdr_sources_frames_rtf_*, tmask [streams][n_sources][F][K] or NULL (all 0), update its update mask
// est: the call of mca_hip_mvdr_sources_frames_auto_* (masked, rtf on a context with RTF enabled; update and tmask NULL): both masks
// come from k_mvdr_estmask, into em_update / em_target where the caller takes them back, else into the workspace
struct MvdrCall {
    int n_streams = 0, n_frames = 0, n_sources = 0;
    const float *doa = nullptr, *update = nullptr;
    bool masked = false;
    const float *tmask = nullptr;
    bool rtf = false, est = false;
    float *em_update = nullptr, *em_target = nullptr, *out_pcm = nullptr, *out_spec = nullptr;
    // the plain call of make_call with update weights per frame; with an update mask per cell; as the RTF call; as the auto call on a context with or without RTF
    MvdrCall weighted(const float *w) const { MvdrCall q = *this; q.update = w; return q; }
    MvdrCall with_mask(const float *um) const { MvdrCall q = weighted(um); q.masked = true; return q; }
    MvdrCall with_rtf(const float *um, const float *tm) const { MvdrCall q = with_mask(um); q.tmask = tm; q.rtf = true; return q; }
    MvdrCall estimating(bool rtf_on, float *um_out, float *tm_out) const { MvdrCall q = with_mask(nullptr); q.rtf = rtf_on; q.est = true; q.em_update = um_out; q.em_target = tm_out; return q; }
};

// the analysis (timing slot 0): PCM -> X, and the steering tables T of doa [streams][F][n_sources]
int launch_analyse(mca_hip_mvdr_ctx *c, const float *pcm, long long stream_stride, long long mic_stride, const MvdrCall &q, hipStream_t st)
{
    MvdrAnalyseArgs aa{};
    aa.pcm = pcm; aa.stream_stride = stream_stride; aa.mic_stride = mic_stride; aa.n_frames = q.n_frames;
    aa.N = c->N; aa.logH = c->logH; aa.M = c->M; aa.S = q.n_sources; aa.window = c->d_window; aa.tw = c->d_tw; aa.doa_rad = q.doa;
    aa.X = c->d_X; aa.T = c->d_T; aa.mic_x = c->d_micx; aa.geo = geometry_args(c);
    aa.unit = (double)c->cfg.sample_rate / (double)c->N / 346.1;                      // Beamformer.cpp:59 without 2 pi
    MvdrAnalysePlan p = plan_mvdr_analyse(*c, q.n_streams, q.n_frames);
    const void *const kernels[] = {kptr(k_mvdr_analyse), kptr(k_mvdr_analyse_1024), kptr(k_mvdr_analyse_512)};      // (in the order of MvdrAnalyseFamily)
    return launch(c, kernels[(int)p.family], p.l.grid, p.l.block, p.l.lds, &aa, T_ANALYSE, st, &p.fpb);
}

// the solve (timing slot 1): X, T -> Y, the covariance and, for the post-filter, the noise plane
// rtf: the frames f0 ... f0 + n_loop - 1 of the call (the steering plane holds those), else the whole call
int launch_solve(mca_hip_mvdr_ctx *c, const MvdrCall &q, float2 *Y, hipStream_t st, int f0 = 0, int n_loop = 0)
{
    const int n_streams = q.n_streams, n_frames = q.n_frames, n_sources = q.n_sources;
    const float *update = q.update;
    const bool rtf = q.rtf;
    if (!rtf) n_loop = n_frames;
    MvdrSolveArgs sa{};
    sa.X = c->d_X; sa.T = c->d_T; sa.n_frames = n_frames; sa.K = c->K; sa.M = c->M; sa.null_gain = (float)c->null_gain;
    sa.alpha = (float)c->cfg.alpha; sa.one_minus_alpha = (float)(1.0 - c->cfg.alpha); sa.loading_over_m = (float)(c->cfg.loading / c->M);
    sa.phi = c->d_phi; sa.trace = c->d_trace; sa.Y = Y; sa.n_streams = n_streams; sa.S = n_sources;
    // the kernels that store the noise plane take weights: a call without them passes ones, whose bytes are those of no weights
    sa.update = update ? update : c->pf_on ? c->d_pf_ones.p : nullptr; sa.pn = c->pf_on ? c->d_pf_pn.p : nullptr;
    const MvdrSolveChoice choice = plan_mvdr_solve_choice(*c, rtf, n_sources, c->null_gain, update != nullptr, q.masked, c->pf_on);
    if (rtf) {
        // the right-hand sides come from the steering plane; a weight per cell always (ones for a call without an update mask).  Nulls at the
        // vectors of the plane (mvdr_frames_dev lets a gain through only under mca_hip_mvdr_set_rtf_nulls); else the RTF kernels
        sa.D = c->d_D; sa.n_loop = n_loop;
        sa.update = (update ? update : c->d_rtf_ones.p) + (size_t)f0 * c->K;
        sa.X += (size_t)f0 * c->K * c->M; sa.Y += (size_t)f0 * c->K;
        if (sa.pn) sa.pn += (size_t)f0 * c->K;
    }
    int lds = 0;                                                // the lookup's; the plan's (mvdr_solve_lds) is what the CPU table pins: one value
    const void *const kernel = mvdr_solve_kernel(choice, lds);
    if (!kernel || lds != mvdr_solve_lds(choice)) return fail(c, MCA_HIP_ERR_UNSUPPORTED, "no MVDR solve kernel for this call in the build");
    const MvdrSolveSplit sp = plan_mvdr_solve_split(*c, n_streams, n_loop);
    auto piece = [&](long long pid0, long long n_prob, int pieces, dim3 grid) {
        sa.pid0 = pid0; sa.n_prob = n_prob; sa.pieces = pieces;
        if (pieces > 1) { sa.phi_out = c->d_phi_tail; sa.trace_out = c->d_trace_tail; sa.out_base = pid0; }      // the scratch copy (MvdrSolveSplit)
        else { sa.phi_out = c->d_phi; sa.trace_out = c->d_trace; sa.out_base = 0; }
        return launch(c, kernel, grid, sp.block, lds, &sa, T_NONE, st);
    };
    t_begin(c, T_SOLVE, st);
    piece(0, sp.main_prob, 1, sp.grid);
    if (sp.scratch) {
        piece(sp.main_prob, sp.tail_prob, sp.pieces, sp.tail_grid);
        HIP_TRY(c, hipMemcpyAsync(c->d_phi + sp.main_prob * c->tri, c->d_phi_tail, (size_t)sp.tail_prob * c->tri * sizeof(float2), hipMemcpyDeviceToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(c->d_trace + sp.main_prob, c->d_trace_tail, (size_t)sp.tail_prob * 4, hipMemcpyDeviceToDevice, st));
    }
    t_end(c, st);
    return MCA_HIP_OK;
}

// the target covariances and the steering plane (timing slot 5): X, T, the masks -> D, Psi, cpsi, cphi; between the analysis and the solve
int launch_rtf(mca_hip_mvdr_ctx *c, const MvdrCall &q, hipStream_t st, int f0, int n_loop)
{
    const int n_streams = q.n_streams, n_frames = q.n_frames, n_sources = q.n_sources;
    const float *update = q.update, *tmask = q.tmask;
    // a slot the call leaves out restarts from nothing learned; the kernel touches only the slots below n_sources
    if (f0 == 0) {
        HIP_TRY(c, clear_unused_slots(c, c->d_psi.p, (size_t)c->K * c->tri, n_sources, n_streams, st));
        HIP_TRY(c, clear_unused_slots(c, c->d_cpsi.p, c->K, n_sources, n_streams, st));
    }
    MvdrRtfArgs ra{};
    const size_t nph = (size_t)c->N / 64 + 33;
    ra.X = c->d_X + (size_t)f0 * c->K * c->M; ra.T = c->d_T + (size_t)f0 * n_sources * c->M * nph;
    ra.update = update ? update + (size_t)f0 * c->K : nullptr; ra.tmask = tmask ? tmask + (size_t)f0 * c->K : nullptr; ra.n_loop = n_loop;
    ra.n_streams = n_streams; ra.n_frames = n_frames; ra.K = c->K; ra.M = c->M; ra.S = n_sources; ra.slots = c->max_sources;
    ra.alpha = (float)c->cfg.alpha; ra.one_minus_alpha = (float)(1.0 - c->cfg.alpha);
    ra.talpha = (float)c->rtf_alpha; ra.one_minus_talpha = (float)(1.0 - c->rtf_alpha);
    ra.min_share = (float)c->rtf_min_share; ra.iterations = c->rtf_iterations; ra.ref_mic = c->rtf_ref;
    ra.phi = c->d_phi; ra.trace = c->d_trace; ra.psi = c->d_psi; ra.cpsi = c->d_cpsi; ra.cphi_in = c->d_cphi; ra.cphi_out = c->d_cphi_next; ra.D = c->d_D;
    const MvdrLaunch l = plan_mvdr_rtf(*c, n_streams, n_sources, n_frames, c->plane_cap_cells).l;
    launch(c, mvdr_rtf_kernel(c->Q(), false), l.grid, l.block, l.lds, &ra, T_RTF, st);
    HIP_TRY(c, hipMemcpyAsync(c->d_cphi, c->d_cphi_next, (size_t)n_streams * c->K * 4, hipMemcpyDeviceToDevice, st));
    return MCA_HIP_OK;
}

// the mask estimator (timing slot 6): X, T -> the update mask and the target masks of the whole call; between the analysis and
// k_mvdr_rtf / the solve, into em_update and em_target.  em_target may be NULL (a call without RTF whose caller takes no target masks back)
int launch_estmask(mca_hip_mvdr_ctx *c, const MvdrCall &q, hipStream_t st)
{
    const int n_streams = q.n_streams, n_frames = q.n_frames, n_sources = q.n_sources;
    MvdrEstmaskArgs ea{};
    ea.X = c->d_X; ea.T = c->d_T; ea.n_streams = n_streams; ea.n_frames = n_frames; ea.K = c->K; ea.M = c->M; ea.S = n_sources;
    ea.bin_lo = c->em_bin_lo; ea.bin_hi = c->em_bin_hi;
    ea.n_protected = c->em_protected == 0 || c->em_protected > n_sources ? n_sources : c->em_protected;
    ea.coherence_lo = (float)c->em_lo; ea.coherence_span = (float)(c->em_hi - c->em_lo);
    ea.update = q.em_update; ea.target = q.em_target;
    const MvdrLaunch l = plan_mvdr_estmask(*c, n_streams, n_frames);
    return launch(c, mvdr_estmask_kernel(c->Q()), l.grid, l.block, l.lds, &ea, T_ESTMASK, st);
}

// the post-filter (timing slot 4): Z = G Y in place, between the solve and the synthesis
int launch_postfilter(mca_hip_mvdr_ctx *c, const MvdrCall &q, float2 *Y, hipStream_t st)
{
    const int n_streams = q.n_streams, n_frames = q.n_frames, n_sources = q.n_sources;
    // A slot the call leaves out restarts from silence, whether the call has out_pcm or not; the kernel touches only the slots below n_sources
    HIP_TRY(c, clear_unused_slots(c, c->d_pf_A.p, c->K, n_sources, n_streams, st));
    MvdrPostfilterArgs fa{};
    fa.Y = Y; fa.pn = c->d_pf_pn; fa.A = c->d_pf_A;
    fa.n_streams = n_streams; fa.S = n_sources; fa.slots = c->max_sources; fa.n_frames = n_frames; fa.K = c->K;
    fa.smoothing = (float)c->pf_smoothing; fa.one_minus_smoothing = (float)(1.0 - c->pf_smoothing);
    fa.gain_floor = (float)c->pf_gain_floor; fa.noise_scale = (float)c->pf_noise_scale;
    const MvdrLaunch l = plan_mvdr_postfilter(*c, n_streams, n_sources);
    return launch(c, kptr(k_mvdr_postfilter), l.grid, l.block, l.lds, &fa, T_POSTFILTER, st);
}

// the synthesis (timing slot 2): Y -> out_pcm [streams][n_sources][F hop], and the overlap-add tails
int launch_synth(mca_hip_mvdr_ctx *c, const MvdrCall &q, const float2 *Y, hipStream_t st)
{
    const int n_streams = q.n_streams, n_frames = q.n_frames, n_sources = q.n_sources;
    MvdrSynthArgs ya{};
    const MvdrSynthPlan p = plan_mvdr_synth(*c, n_streams, n_sources, n_frames);
    ya.Y = Y; ya.n_frames = n_frames; ya.N = c->N; ya.logH = c->logH; ya.tw = c->d_tw; ya.S = n_sources; ya.tail_slots = c->max_sources; ya.ft = p.ft;
    ya.tail_in = c->d_tail[c->tail_cur]; ya.tail_out = c->d_tail[c->tail_cur ^ 1]; ya.out = q.out_pcm;
    // a slot the call leaves out restarts from silence.  The kernel writes only the slots below n_sources, so the clear goes
    // first: if it fails, nothing has touched the tails yet and tail_cur still names the valid ones
    HIP_TRY(c, clear_unused_slots(c, ya.tail_out, c->H, n_sources, n_streams, st));
    if (const int rc = launch(c, kptr(k_mvdr_synth), p.l.grid, p.l.block, p.l.lds, &ya, T_SYNTH, st)) return rc;
    c->tail_cur ^= 1;
    return MCA_HIP_OK;
}

// the call on device pointers: pcm with its strides, the launches on `stream`
int mvdr_frames_dev(mca_hip_mvdr_ctx *c, const float *pcm, long long stream_stride, long long mic_stride, const MvdrCall &call, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    MvdrCall q = call;                                          // (an auto call: update and tmask become the estimated masks below)
    const int n_streams = q.n_streams, n_frames = q.n_frames, n_sources = q.n_sources;
    if (q.est && !c->em_on) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "the mask estimator is not enabled on this context (mca_hip_mvdr_set_mask_estimator)");
    if (q.rtf && !c->rtf_on) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "RTF is not enabled on this context (mca_hip_mvdr_set_rtf)");
    if (q.rtf && c->null_gain != 0.0 && !c->rtf_nulls)
        return fail(c, MCA_HIP_ERR_UNSUPPORTED, "nulls at estimated steering vectors are not built: set the null gain to 0, or enable them (mca_hip_mvdr_set_rtf_nulls)");
    if (n_sources < 1 || n_sources > c->max_sources)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_sources outside [1, max_sources] (mca_hip_mvdr_set_max_sources; " + std::to_string(c->max_sources) + " here)");
    if (!pcm || !q.doa) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "pcm_dev / doa_rad_dev is NULL");
    if (!q.out_pcm && !q.out_spec) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "out_pcm_dev and out_spec_dev are both NULL");
    if (n_streams < 1 || n_streams > c->cfg.max_streams) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_streams outside [1, max_streams]");
    if (n_frames < 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_frames < 1");
    const long long need = (long long)(n_frames + 1) * c->H;
    if (mic_stride < need) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "mic_stride shorter than (n_frames+1)*hop samples");
    if (n_streams > 1 && stream_stride < (long long)(c->M - 1) * mic_stride + need) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "stream_stride too short");
    if ((mic_stride & 1) || (stream_stride & 1) || (reinterpret_cast<uintptr_t>(pcm) & 7))
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "pcm_dev must be 8-byte aligned with even strides (float2 loads)");
    if (q.out_spec && (reinterpret_cast<uintptr_t>(q.out_spec) & 7)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "out_spec_dev must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    // the steering plane of an RTF call holds fc frames: all of them, or as many as the workspace cap takes
    const int fc = q.rtf ? plan_mvdr_rtf(*c, n_streams, n_sources, n_frames, c->plane_cap_cells).fc : n_frames;
    int rc = ensure_ws(c, (size_t)n_streams * n_frames, n_sources, !q.update && !q.est, q.rtf, (size_t)n_streams * fc);
    if (rc) return rc;
    if (q.est && (rc = ensure_estmask_ws(c, (size_t)n_streams * n_frames, n_sources, !q.em_update, q.rtf && !q.em_target))) return rc;
    // the beamformed spectra go straight to the caller's buffer when one is given
    float2 *Y = q.out_spec ? reinterpret_cast<float2 *>(q.out_spec) : c->d_Y.p;
    if ((rc = launch_analyse(c, pcm, stream_stride, mic_stride, q, st))) return rc;
    if (q.est) {
        // the masks of the whole call, once, ahead of the chunk loop as the analysis is
        if (!q.em_update) q.em_update = c->d_em_update;
        if (!q.em_target && q.rtf) q.em_target = c->d_em_target;
        if ((rc = launch_estmask(c, q, st))) return rc;
        q.update = q.em_update; q.tmask = q.em_target;
    }
    if (q.rtf) {
        for (int f0 = 0; f0 < n_frames; f0 += fc) {
            const int n = std::min(fc, n_frames - f0);
            if ((rc = launch_rtf(c, q, st, f0, n))) return rc;
            if ((rc = launch_solve(c, q, Y, st, f0, n))) return rc;
        }
    } else if ((rc = launch_solve(c, q, Y, st))) return rc;
    if (c->pf_on && (rc = launch_postfilter(c, q, Y, st))) return rc;
    if (q.out_pcm && (rc = launch_synth(c, q, Y, st))) return rc;
    HIP_TRY(c, hipGetLastError());
    return MCA_HIP_OK;
}

// the host-pointer form: pcm packed [streams][M][(F + 1) hop]; 1 or K (masked) floats of update weights per (stream, frame)
int mvdr_frames_host(mca_hip_mvdr_ctx *c, const float *pcm, const MvdrCall &q)
{
    if (!c || !pcm || !q.doa) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    const int n_streams = q.n_streams, n_frames = q.n_frames, n_sources = q.n_sources;
    if (n_streams < 1 || n_frames < 1 || n_sources < 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_streams/n_frames/n_sources < 1");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const long long ms = (long long)(n_frames + 1) * c->H, ss = ms * c->M;
    const size_t nf = (size_t)n_streams * n_frames * n_sources;
    const size_t nu = (size_t)n_streams * n_frames * (q.masked ? (size_t)c->K : 1), tb = nf * c->K * 4;      // (target masks: [streams][n_sources][F][K])
    // (the target mask goes first; the masks an auto call hands back are staged where the other calls stage the masks they take)
    StageBuf b[] = {{SG_TARGET_MASK, q.tmask, tb, STAGE_IN}, {SG_PCM, pcm, (size_t)ss * n_streams * 4, STAGE_IN}, {SG_DOA, q.doa, nf * 4, STAGE_IN},
                    {q.masked ? SG_UPDATE_MASK : SG_WEIGHTS, q.update, nu * 4, STAGE_IN}, {SG_UPDATE_MASK, q.em_update, nu * 4, STAGE_OUT},
                    {SG_TARGET_MASK, q.em_target, tb, STAGE_OUT}, {SG_OUT_PCM, q.out_pcm, nf * c->H * 4, STAGE_OUT}, {SG_OUT_SPEC, q.out_spec, nf * c->K * 8, STAGE_OUT}};
    return staged(c, b, [&] {
        MvdrCall d = q;                                         // the same call on the staged copies
        d.tmask = (float *)b[0].dev; d.doa = (float *)b[2].dev; d.update = (float *)b[3].dev; d.em_update = (float *)b[4].dev; d.em_target = (float *)b[5].dev;
        d.out_pcm = (float *)b[6].dev; d.out_spec = (float *)b[7].dev;
        return mvdr_frames_dev(c, (float *)b[1].dev, ss, ms, d, nullptr);
    });
}

// the call every mca_hip_mvdr_*frames* entry point starts from
extern "C++" MvdrCall make_call(int n_streams, int n_frames, int n_sources, const float *doa, float *out_pcm, float *out_spec)
{
    MvdrCall q;
    q.n_streams = n_streams; q.n_frames = n_frames; q.n_sources = n_sources; q.doa = doa; q.out_pcm = out_pcm; q.out_spec = out_spec;
    return q;
}

}  // namespace

int mca_hip_mvdr_sources_frames_weighted_dev(mca_hip_mvdr_ctx *c, const float *pcm, long long stream_stride, long long mic_stride, int n_streams,
                                             int n_frames, int n_sources, const float *doa_rad, const float *update, float *out_pcm,
                                             float *out_spec, void *stream)
{
    return mvdr_frames_dev(c, pcm, stream_stride, mic_stride, make_call(n_streams, n_frames, n_sources, doa_rad, out_pcm, out_spec).weighted(update), stream);
}

// update_mask [streams][F][K] or NULL (all 1)
int mca_hip_mvdr_sources_frames_masked_dev(mca_hip_mvdr_ctx *c, const float *pcm, long long stream_stride, long long mic_stride, int n_streams,
                                           int n_frames, int n_sources, const float *doa_rad, const float *update_mask, float *out_pcm,
                                           float *out_spec, void *stream)
{
    return mvdr_frames_dev(c, pcm, stream_stride, mic_stride, make_call(n_streams, n_frames, n_sources, doa_rad, out_pcm, out_spec).with_mask(update_mask), stream);
}

// update_mask [streams][F][K] or NULL (all 1), target_mask [streams][n_sources][F][K] or NULL (all 0)
int mca_hip_mvdr_sources_frames_rtf_dev(mca_hip_mvdr_ctx *c, const float *pcm, long long stream_stride, long long mic_stride, int n_streams,
                                        int n_frames, int n_sources, const float *doa_rad, const float *update_mask, const float *target_mask,
                                        float *out_pcm, float *out_spec, void *stream)
{
    return mvdr_frames_dev(c, pcm, stream_stride, mic_stride, make_call(n_streams, n_frames, n_sources, doa_rad, out_pcm, out_spec).with_rtf(update_mask, target_mask), stream);
}

int mca_hip_mvdr_sources_frames_rtf_host(mca_hip_mvdr_ctx *c, const float *pcm, int n_streams, int n_frames, int n_sources, const float *doa_rad,
                                         const float *update_mask, const float *target_mask, float *out_pcm, float *out_spec)
{
    if (c && !c->rtf_on) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "RTF is not enabled on this context (mca_hip_mvdr_set_rtf)");
    return mvdr_frames_host(c, pcm, make_call(n_streams, n_frames, n_sources, doa_rad, out_pcm, out_spec).with_rtf(update_mask, target_mask));
}

// update_mask_out [streams][F][K] and target_mask_out [streams][n_sources][F][K]: either may be NULL
int mca_hip_mvdr_sources_frames_auto_dev(mca_hip_mvdr_ctx *c, const float *pcm, long long stream_stride, long long mic_stride, int n_streams,
                                         int n_frames, int n_sources, const float *doa_rad, float *update_mask_out, float *target_mask_out,
                                         float *out_pcm, float *out_spec, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(update_mask_out) | reinterpret_cast<uintptr_t>(target_mask_out)) & 3)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "update_mask_out_dev / target_mask_out_dev must be 4-byte aligned");
    return mvdr_frames_dev(c, pcm, stream_stride, mic_stride, make_call(n_streams, n_frames, n_sources, doa_rad, out_pcm, out_spec).estimating(c->rtf_on, update_mask_out, target_mask_out), stream);
}

int mca_hip_mvdr_sources_frames_auto_host(mca_hip_mvdr_ctx *c, const float *pcm, int n_streams, int n_frames, int n_sources, const float *doa_rad,
                                          float *update_mask_out, float *target_mask_out, float *out_pcm, float *out_spec)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!c->em_on) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "the mask estimator is not enabled on this context (mca_hip_mvdr_set_mask_estimator)");
    return mvdr_frames_host(c, pcm, make_call(n_streams, n_frames, n_sources, doa_rad, out_pcm, out_spec).estimating(c->rtf_on, update_mask_out, target_mask_out));
}

int mca_hip_mvdr_sources_frames_dev(mca_hip_mvdr_ctx *c, const float *pcm, long long stream_stride, long long mic_stride, int n_streams,
                                    int n_frames, int n_sources, const float *doa_rad, float *out_pcm, float *out_spec, void *stream)
{
    return mca_hip_mvdr_sources_frames_weighted_dev(c, pcm, stream_stride, mic_stride, n_streams, n_frames, n_sources, doa_rad, nullptr, out_pcm, out_spec, stream);
}

int mca_hip_mvdr_frames_dev(mca_hip_mvdr_ctx *c, const float *pcm, long long stream_stride, long long mic_stride, int n_streams,
                            int n_frames, const float *doa_rad, float *out_pcm, float *out_spec, void *stream)
{
    return mca_hip_mvdr_sources_frames_weighted_dev(c, pcm, stream_stride, mic_stride, n_streams, n_frames, 1, doa_rad, nullptr, out_pcm, out_spec, stream);
}

int mca_hip_mvdr_sources_frames_weighted_host(mca_hip_mvdr_ctx *c, const float *pcm, int n_streams, int n_frames, int n_sources, const float *doa_rad,
                                              const float *update, float *out_pcm, float *out_spec)
{
    return mvdr_frames_host(c, pcm, make_call(n_streams, n_frames, n_sources, doa_rad, out_pcm, out_spec).weighted(update));
}

int mca_hip_mvdr_sources_frames_masked_host(mca_hip_mvdr_ctx *c, const float *pcm, int n_streams, int n_frames, int n_sources, const float *doa_rad,
                                            const float *update_mask, float *out_pcm, float *out_spec)
{
    return mvdr_frames_host(c, pcm, make_call(n_streams, n_frames, n_sources, doa_rad, out_pcm, out_spec).with_mask(update_mask));
}

int mca_hip_mvdr_sources_frames_host(mca_hip_mvdr_ctx *c, const float *pcm, int n_streams, int n_frames, int n_sources, const float *doa_rad,
                                     float *out_pcm, float *out_spec)
{
    return mca_hip_mvdr_sources_frames_weighted_host(c, pcm, n_streams, n_frames, n_sources, doa_rad, nullptr, out_pcm, out_spec);
}

int mca_hip_mvdr_frames_host(mca_hip_mvdr_ctx *c, const float *pcm, int n_streams, int n_frames, const float *doa_rad,
                             float *out_pcm, float *out_spec)
{
    return mca_hip_mvdr_sources_frames_weighted_host(c, pcm, n_streams, n_frames, 1, doa_rad, nullptr, out_pcm, out_spec);
}

int mca_hip_mvdr_spectrum_configure(mca_hip_mvdr_ctx *c, const mca_hip_mvdr_spectrum_config *cfg)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!cfg) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (cfg->struct_size != (int)sizeof(mca_hip_mvdr_spectrum_config)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "struct_size mismatch");
    if (cfg->n_angles < 2 || cfg->n_angles > MVDR_SPEC_MAX_ANGLES) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_angles must be in [2,361]");
    const bool xyz = c->geo_mode == MCA_HIP_MVDR_GEOMETRY_XYZ;
    if (xyz && cfg->n_angles < 3) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_angles must be in [3,361] on the periodic grid of XYZ geometry");
    if (cfg->bin_lo < 0 || cfg->bin_lo > cfg->bin_hi || cfg->bin_hi > c->N / 2)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "the band must satisfy 0 <= bin_lo <= bin_hi <= N/2");
    if (cfg->weighting != MCA_HIP_MVDR_SPECTRUM_POWER && cfg->weighting != MCA_HIP_MVDR_SPECTRUM_NORMALISED)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "weighting must be 0 (power) or 1 (normalised)");
    if (cfg->n_peaks < 1 || cfg->n_peaks > MCA_MAX_SOURCES) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_peaks must be in [1,4]");
    if (c->spec_set && cfg->n_angles == c->spec.n_angles) { c->spec = *cfg; return MCA_HIP_OK; }    // the grid and its phasors stay
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    // grid and steering phasors of the new angle count, in double: theta_i = -pi/2 + i pi/(D-1), u = fs/(N c) x_m cos(theta + pi/2)
    // (Beamformer.cpp:59), factors exp(-j 2 pi 32 i u), i <= N/64, and exp(-j 2 pi i u), i < 32, as in MvdrAnalyseArgs::T
    const int D = cfg->n_angles, Dpad = (D + 63) & ~63, nhi = c->N / 64 + 1, nph = nhi + 32, M = c->M;
    // XYZ geometry: the periodic grid theta_i = -pi + i 2 pi / D and the projection on e(theta, eps) (host_projection)
    std::vector<float> grid(D);
    std::vector<float2> T((size_t)M * nph * Dpad);
    for (int i = 0; i < Dpad; ++i) {
        const double ii = (double)(i < D ? i : D - 1);                                          // the surplus lanes repeat the last angle
        const double th = xyz ? -M_PI + ii * (2.0 * M_PI) / (double)D : -M_PI / 2 + ii * M_PI / (double)(D - 1);
        if (i < D) grid[i] = (float)th;
        for (int m = 0; m < M; ++m) {
            host_phasors(host_projection(c, m, th), nhi, nph, &T[(size_t)m * nph * Dpad + i], Dpad);
        }
    }
    // the former tables and spec_set stay when the new ones fail; else they go, behind the wait, with ng and nT
    DevBuf<float> ng;
    DevBuf<float2> nT;
    hipError_t e = ng.upload(grid.data(), grid.size());
    if (e == hipSuccess) e = nT.upload(T.data(), T.size());
    if (e == hipSuccess) e = hipDeviceSynchronize();            // no spectrum call in flight reads the former tables
    if (e != hipSuccess) return hip_fail(c, e, "steering tables of the spectrum");
    c->d_spec_grid.swap(ng); c->d_spec_T.swap(nT); c->spec_grid.swap(grid); c->spec_dpad = Dpad; c->spec = *cfg; c->spec_set = true;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_spectrum_get_grid(const mca_hip_mvdr_ctx *c, float *doa_rad)
{
    if (!c || !doa_rad || !c->spec_set) return MCA_HIP_ERR_INVALID_ARGUMENT;
    std::memcpy(doa_rad, c->spec_grid.data(), c->spec_grid.size() * 4);
    return MCA_HIP_OK;
}

extern "C++" {
namespace {
// the part of the arguments every scan shares (MvdrSpectrumArgs, MvdrTrackSpectrumArgs): the state of the streams from first_stream on, the
// grid's phasors and sizes, the band and its chunks
template <class Args>
void scan_args(const mca_hip_mvdr_ctx *c, Args &sa, const MvdrBand &b, const float2 *T, int D, int Dpad, int bin_lo, int bin_hi, int first_stream = 0)
{
    sa.phi = c->d_phi + (size_t)first_stream * c->K * c->tri; sa.trace = c->d_trace + (size_t)first_stream * c->K; sa.T = T;
    sa.K = c->K; sa.M = c->M; sa.D = D; sa.Dpad = Dpad; sa.nhi = b.nhi; sa.nph = b.nph;
    sa.bin_lo = bin_lo; sa.bin_hi = bin_hi; sa.chunk0 = b.chunk0; sa.n_chunks = b.n_chunks;
}
// both kernels of the Capon spectrum (timing slot 3), arguments checked by the caller
int launch_spectrum(mca_hip_mvdr_ctx *c, int n_streams, float *spectrum, float *peak_doa, float *peak_val, hipStream_t st)
{
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const MvdrScanPlan p = plan_mvdr_spectrum(*c, c->spec.bin_lo, c->spec.bin_hi, c->spec_dpad, n_streams);
    MvdrSpectrumArgs sa{};
    scan_args(c, sa, p.b, c->d_spec_T, c->spec.n_angles, c->spec_dpad, c->spec.bin_lo, c->spec.bin_hi);
    sa.power = c->spec.weighting == MCA_HIP_MVDR_SPECTRUM_POWER; sa.loading = (float)c->cfg.loading;
    if (const int rc = grow_ws(c, c->d_spec_part, p.per_part * n_streams, "partial sums of the spectrum", true)) return rc;
    sa.part = c->d_spec_part;
    MvdrSpectrumPickArgs pa{};
    pa.part = c->d_spec_part; pa.grid = c->d_spec_grid; pa.n_slices = p.b.n_slices; pa.D = sa.D; pa.Dpad = sa.Dpad; pa.n_peaks = c->spec.n_peaks;
    pa.circular = c->geo_mode == MCA_HIP_MVDR_GEOMETRY_XYZ ? 1 : 0;
    pa.spectrum = spectrum; pa.peak_doa = peak_doa; pa.peak_val = peak_val;
    t_begin(c, T_SPECTRUM, st);
    const int rc = launch(c, mvdr_spectrum_kernel(c->Q()), p.grid(p.wg_scan, n_streams), dim3(256), p.lds, &sa, T_NONE, st);
    if (!rc) launch(c, kptr(k_mvdr_spectrum_pick), dim3(n_streams), dim3(256), 0, &pa, T_NONE, st);
    t_end(c, st);
    if (rc) return rc;
    HIP_TRY(c, hipGetLastError());
    return MCA_HIP_OK;
}
}  // namespace
}  // extern "C++"

int mca_hip_mvdr_spectrum_dev(mca_hip_mvdr_ctx *c, int n_streams, float *spectrum, float *peak_doa, float *peak_val, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!c->spec_set) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "mca_hip_mvdr_spectrum_configure first");
    if (n_streams < 1 || n_streams > c->cfg.max_streams) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_streams outside [1, max_streams]");
    if (!spectrum && !peak_doa && !peak_val) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "spectrum_dev, peak_doa_dev and peak_val_dev are all NULL");
    return launch_spectrum(c, n_streams, spectrum, peak_doa, peak_val, (hipStream_t)stream);
}

int mca_hip_mvdr_spectrum_host(mca_hip_mvdr_ctx *c, int n_streams, float *spectrum, float *peak_doa, float *peak_val)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!c->spec_set) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "mca_hip_mvdr_spectrum_configure first");
    if (n_streams < 1 || n_streams > c->cfg.max_streams) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_streams outside [1, max_streams]");
    if (!spectrum && !peak_doa && !peak_val) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "spectrum, peak_doa and peak_val are all NULL");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t sb = (size_t)n_streams * c->spec.n_angles * 4, pb = (size_t)n_streams * c->spec.n_peaks * 4;
    StageBuf b[] = {{SG_SCAN, spectrum, sb, STAGE_OUT}, {SG_AUX1, peak_doa, pb, STAGE_OUT}, {SG_AUX2, peak_val, pb, STAGE_OUT}};
    return staged(c, b, [&] { return mca_hip_mvdr_spectrum_dev(c, n_streams, (float *)b[0].dev, (float *)b[1].dev, (float *)b[2].dev, nullptr); });
}

// ---- the azimuth x elevation Capon map (kernels_mvdr_map.hip) ----
int mca_hip_mvdr_map_configure(mca_hip_mvdr_ctx *c, const mca_hip_mvdr_map_config *cfg)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!cfg) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (cfg->struct_size != (int)sizeof(mca_hip_mvdr_map_config)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "struct_size mismatch");
    if (c->geo_mode != MCA_HIP_MVDR_GEOMETRY_XYZ) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "the map needs XYZ geometry (mca_hip_mvdr_set_geometry)");
    if (cfg->n_az < 3 || cfg->n_az > 360) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_az must be in [3,360]");
    if (cfg->n_el < 1 || cfg->n_el > 91) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_el must be in [1,91]");
    if (cfg->n_az * cfg->n_el > MVDR_MAP_MAX_DIRS) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_az n_el must be at most 2048");
    if (!std::isfinite(cfg->el_lo_rad) || !std::isfinite(cfg->el_hi_rad) || cfg->el_lo_rad < -M_PI / 2 || cfg->el_hi_rad > M_PI / 2 || cfg->el_lo_rad > cfg->el_hi_rad)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "the elevations must satisfy -pi/2 <= el_lo_rad <= el_hi_rad <= pi/2");
    if (cfg->n_el == 1 && cfg->el_lo_rad != cfg->el_hi_rad) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_el == 1 needs el_lo_rad == el_hi_rad");
    if (cfg->bin_lo < 0 || cfg->bin_lo > cfg->bin_hi || cfg->bin_hi > c->N / 2)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "the band must satisfy 0 <= bin_lo <= bin_hi <= N/2");
    if (cfg->weighting != MCA_HIP_MVDR_SPECTRUM_POWER && cfg->weighting != MCA_HIP_MVDR_SPECTRUM_NORMALISED)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "weighting must be 0 (power) or 1 (normalised)");
    if (cfg->n_peaks < 1 || cfg->n_peaks > MCA_MAX_SOURCES) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_peaks must be in [1,4]");
    if (c->map_set && cfg->n_az == c->map.n_az && cfg->n_el == c->map.n_el && cfg->el_lo_rad == c->map.el_lo_rad && cfg->el_hi_rad == c->map.el_hi_rad) {
        c->map = *cfg;                                          // the grid and its phasors stay
        return MCA_HIP_OK;
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    // grid and phasors in double: theta_i = -pi + i 2 pi / n_az, eps_j = el_lo + j (el_hi - el_lo)/(n_el - 1), direction j n_az + i;
    // the layout and the factors are the spectrum's (mca_hip_mvdr_spectrum_configure), the surplus lanes repeat the last direction
    const int n_az = cfg->n_az, n_el = cfg->n_el, D = n_az * n_el, Dpad = (D + 63) & ~63, nhi = c->N / 64 + 1, nph = nhi + 32, M = c->M;
    const double step = n_el > 1 ? (cfg->el_hi_rad - cfg->el_lo_rad) / (double)(n_el - 1) : 0.0;
    std::vector<float> az(n_az), el(n_el);
    std::vector<double> azd(n_az), ce(n_el), se(n_el);
    for (int i = 0; i < n_az; ++i) { azd[i] = -M_PI + (double)i * (2.0 * M_PI) / (double)n_az; az[i] = (float)azd[i]; }
    for (int j = 0; j < n_el; ++j) {
        const double eps = cfg->el_lo_rad + (double)j * step;
        el[j] = (float)eps; ce[j] = std::cos(eps); se[j] = std::sin(eps);
    }
    std::vector<float2> T((size_t)M * nph * Dpad);
    for (int d = 0; d < Dpad; ++d) {
        const int dd = d < D ? d : D - 1, j = dd / n_az, i = dd - j * n_az;
        for (int m = 0; m < M; ++m) host_phasors(host_projection_xyz(c, m, azd[i], ce[j], se[j]), nhi, nph, &T[(size_t)m * nph * Dpad + d], Dpad);
    }
    // the former tables and map_set stay when the new ones fail; else they go, behind the wait
    DevBuf<float> na, ne;
    DevBuf<float2> nT;
    hipError_t e = na.upload(az.data(), az.size());
    if (e == hipSuccess) e = ne.upload(el.data(), el.size());
    if (e == hipSuccess) e = nT.upload(T.data(), T.size());
    if (e == hipSuccess) e = hipDeviceSynchronize();            // no map call in flight reads the former tables
    if (e != hipSuccess) return hip_fail(c, e, "steering tables of the map");
    c->d_map_az.swap(na); c->d_map_el.swap(ne); c->d_map_T.swap(nT); c->map_az.swap(az); c->map_el.swap(el);
    c->map_dpad = Dpad; c->map = *cfg; c->map_set = true; c->map_ever = true;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_map_get_grid(const mca_hip_mvdr_ctx *c, float *az, float *el)
{
    if (!c || (!az && !el) || !c->map_set) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (az) std::memcpy(az, c->map_az.data(), c->map_az.size() * 4);
    if (el) std::memcpy(el, c->map_el.data(), c->map_el.size() * 4);
    return MCA_HIP_OK;
}

int mca_hip_mvdr_map_dev(mca_hip_mvdr_ctx *c, int n_streams, float *map, float *peak_az, float *peak_el, float *peak_val, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!c->map_set) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "mca_hip_mvdr_map_configure first");
    if (n_streams < 1 || n_streams > c->cfg.max_streams) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_streams outside [1, max_streams]");
    if (!map && !peak_az && !peak_el && !peak_val) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "map_dev, peak_az_dev, peak_el_dev and peak_val_dev are all NULL");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    const int D = c->map.n_az * c->map.n_el;
    // the partial sums are taken in passes of streams under the workspace cap (MvdrScanPlan): 288 KiB per stream at 2048 directions and N = 1024
    const MvdrScanPlan p = plan_mvdr_map(*c, c->map.bin_lo, c->map.bin_hi, c->map_dpad, n_streams, c->plane_cap_cells);
    if (const int rc = grow_ws(c, c->d_map_part, p.per_part * p.pass, "partial sums of the map", true)) return rc;
    MvdrMapScanArgs ma{};
    MvdrSpectrumArgs &sa = ma.s;
    sa.power = c->map.weighting == MCA_HIP_MVDR_SPECTRUM_POWER; sa.loading = (float)c->cfg.loading; sa.part = c->d_map_part;
    ma.n_tiles = p.b.n_tiles;
    MvdrMapPickArgs pa{};
    pa.part = c->d_map_part; pa.az = c->d_map_az; pa.el = c->d_map_el; pa.n_slices = p.b.n_slices;
    pa.n_az = c->map.n_az; pa.n_el = c->map.n_el; pa.Dpad = c->map_dpad; pa.n_peaks = c->map.n_peaks; pa.ctx_el = (float)c->geo_elevation;
    int rc = MCA_HIP_OK;
    t_begin(c, T_MAP, st);
    for (int s0 = 0; s0 < n_streams && !rc; s0 += p.pass) {
        const int ns = std::min(p.pass, n_streams - s0);
        scan_args(c, sa, p.b, c->d_map_T, D, c->map_dpad, c->map.bin_lo, c->map.bin_hi, s0);
        pa.map = map ? map + (size_t)s0 * D : nullptr;
        pa.peak_az = peak_az ? peak_az + (size_t)s0 * pa.n_peaks : nullptr;
        pa.peak_el = peak_el ? peak_el + (size_t)s0 * pa.n_peaks : nullptr;
        pa.peak_val = peak_val ? peak_val + (size_t)s0 * pa.n_peaks : nullptr;
        ma.n_streams = ns;
        rc = launch(c, mvdr_map_scan_kernel(c->Q()), p.grid(p.wg_scan, ns), dim3(256), p.lds, &ma, T_NONE, st);
        if (!rc) launch(c, kptr(k_mvdr_map_pick), dim3(ns), dim3(256), 0, &pa, T_NONE, st);
    }
    t_end(c, st);
    if (rc) return rc;
    HIP_TRY(c, hipGetLastError());
    return MCA_HIP_OK;
}

int mca_hip_mvdr_map_host(mca_hip_mvdr_ctx *c, int n_streams, float *map, float *peak_az, float *peak_el, float *peak_val)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!c->map_set) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "mca_hip_mvdr_map_configure first");
    if (n_streams < 1 || n_streams > c->cfg.max_streams) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_streams outside [1, max_streams]");
    if (!map && !peak_az && !peak_el && !peak_val) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "map, peak_az, peak_el and peak_val are all NULL");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t mb = (size_t)n_streams * c->map.n_az * c->map.n_el * 4, pb = (size_t)n_streams * c->map.n_peaks * 4;
    StageBuf b[] = {{SG_SCAN, map, mb, STAGE_OUT}, {SG_AUX1, peak_az, pb, STAGE_OUT}, {SG_AUX2, peak_el, pb, STAGE_OUT}, {SG_WEIGHTS, peak_val, pb, STAGE_OUT}};
    return staged(c, b, [&] { return mca_hip_mvdr_map_dev(c, n_streams, (float *)b[0].dev, (float *)b[1].dev, (float *)b[2].dev, (float *)b[3].dev, nullptr); });
}

// ---- an elevation per look-direction slot ----
extern "C++" {
namespace {
int elevations_ready(mca_hip_mvdr_ctx *c, int n_streams, const void *ptr)
{
    if (n_streams < 1 || n_streams > c->cfg.max_streams) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_streams outside [1, max_streams]");
    if (!ptr) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "the elevations array is NULL");
    return MCA_HIP_OK;
}
}  // namespace
}  // extern "C++"

int mca_hip_mvdr_set_elevations_host(mca_hip_mvdr_ctx *c, int n_streams, const float *elev_rad)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = elevations_ready(c, n_streams, elev_rad)) return rc;
    const int S = c->max_sources;
    const float half_pi_f = 1.57079637f;                        // (float) pi/2: the largest float the call accepts
    for (int e = 0; e < n_streams * S; ++e)
        if (!std::isnan(elev_rad[e]) && !(std::fabs(elev_rad[e]) <= half_pi_f))
            return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "an elevation must be NaN (the context's) or within [-pi/2, pi/2]");
    // the pairs with the host functions of mca_hip_mvdr_set_geometry; a NaN takes the context's pair, bit for bit
    const double ce = std::cos(c->geo_elevation), se = std::sin(c->geo_elevation);
    std::vector<double2> pairs((size_t)n_streams * S);
    for (size_t e = 0; e < pairs.size(); ++e) {
        const double eps = std::min(std::max((double)elev_rad[e], -M_PI / 2), M_PI / 2);
        pairs[e] = std::isnan(elev_rad[e]) ? make_double2(ce, se) : make_double2(std::cos(eps), std::sin(eps));
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipDeviceSynchronize());                       // no call in flight reads the pairs that change here
    HIP_TRY(c, hipMemcpy2D(c->d_slot_el, MCA_MAX_SOURCES * sizeof(double2), pairs.data(), S * sizeof(double2), S * sizeof(double2), (size_t)n_streams, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy2D(c->d_slot_val, MCA_MAX_SOURCES * sizeof(float), elev_rad, S * sizeof(float), S * sizeof(float), (size_t)n_streams, hipMemcpyHostToDevice));
    tracks_off(c);                                             // they follow azimuths at the context's elevation: a slot with one of its own ends them
    return MCA_HIP_OK;
}

int mca_hip_mvdr_set_elevations_dev(mca_hip_mvdr_ctx *c, int n_streams, const float *elev_rad, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = elevations_ready(c, n_streams, elev_rad)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    MvdrElevationsArgs ea{elev_rad, c->d_slot_el, c->d_slot_val, n_streams * c->max_sources, c->max_sources, std::cos(c->geo_elevation), std::sin(c->geo_elevation)};
    launch(c, kptr(k_mvdr_elevations), grid_for(ea.n, 256), dim3(256), 0, &ea, T_NONE, (hipStream_t)stream);
    HIP_TRY(c, hipGetLastError());
    tracks_off(c);
    return MCA_HIP_OK;
}

int mca_hip_mvdr_get_elevations(mca_hip_mvdr_ctx *c, int n_streams, float *elev_rad)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = elevations_ready(c, n_streams, elev_rad)) return rc;
    const int S = c->max_sources;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemcpy2D(elev_rad, S * sizeof(float), c->d_slot_val, MCA_MAX_SOURCES * sizeof(float), S * sizeof(float), (size_t)n_streams, hipMemcpyDeviceToHost));
    return MCA_HIP_OK;
}

// ---- tracks of the look directions (kernels_mvdr_track.hip) ----
extern "C++" {
namespace {
MvdrTrackState track_state(mca_hip_mvdr_ctx *c)
{
    const size_t n = (size_t)c->cfg.max_streams * MCA_MAX_SOURCES;
    return MvdrTrackState{c->d_trk_theta, c->d_trk_int, c->d_trk_int + n, c->d_trk_int + 2 * n};
}
// the calls on one angle: refused in map mode, where they would leave eps undefined
int tracks_ready_1d(mca_hip_mvdr_ctx *c)
{
    if (c->trk_map_on) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "the tracks are in map mode: use the _map call (mca_hip_mvdr_tracks_set_map)");
    return MCA_HIP_OK;
}
MvdrTrk2State track_state_map(mca_hip_mvdr_ctx *c, int first_stream = 0)
{
    const size_t n = (size_t)c->cfg.max_streams * MCA_MAX_SOURCES, o = (size_t)first_stream * MCA_MAX_SOURCES;
    return MvdrTrk2State{c->d_trk_theta + o, c->d_trk_eps + o, c->d_trk_int + o, c->d_trk_int + n + o, c->d_trk_int + 2 * n + o};
}
int tracks_ready(mca_hip_mvdr_ctx *c, int n_streams)
{
    if (!c->trk_on) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "mca_hip_mvdr_tracks_configure first (with enable = 1)");
    if (n_streams < 1 || n_streams > c->cfg.max_streams) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_streams outside [1, max_streams]");
    return MCA_HIP_OK;
}
// the association's part of the pick kernel's arguments
MvdrTrackPickArgs track_pick_args(mca_hip_mvdr_ctx *c)
{
    MvdrTrackPickArgs pa{};
    pa.st = track_state(c);
    pa.grid = c->d_spec_grid; pa.D = c->spec.n_angles; pa.Dpad = c->spec_dpad;
    pa.n_tracks = c->trk.n_tracks; pa.n_own = c->trk.n_own; pa.hold = c->trk.hold;
    pa.max_step = (float)c->trk.max_step_rad; pa.min_sep = (float)c->trk.min_sep_rad;
    pa.psi = c->rtf_on ? c->d_psi : nullptr; pa.cpsi = c->rtf_on ? c->d_cpsi : nullptr;
    pa.slots = c->max_sources; pa.K = c->K; pa.tri = c->tri;
    pa.circular = c->geo_mode == MCA_HIP_MVDR_GEOMETRY_XYZ ? 1 : 0;
    return pa;
}
}  // namespace
}  // extern "C++"

int mca_hip_mvdr_tracks_configure(mca_hip_mvdr_ctx *c, const mca_hip_mvdr_tracks_config *cfg)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!cfg) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (cfg->struct_size != (int)sizeof(mca_hip_mvdr_tracks_config)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "struct_size mismatch");
    if (!c->spec_set) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "mca_hip_mvdr_spectrum_configure first: the tracks use its grid, band and n_peaks");
    if (cfg->enable != 0 && cfg->enable != 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "enable must be 0 or 1");
    if (cfg->n_tracks < 1 || cfg->n_tracks > c->max_sources) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_tracks must be in [1, max_sources]");
    if (cfg->n_own < 0 || cfg->n_own > cfg->n_tracks) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_own must be in [0, n_tracks]");
    if (cfg->n_own > 0 && !c->rtf_on) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_own > 0 needs RTF enabled (mca_hip_mvdr_set_rtf): an own track follows its target covariance");
    if (!std::isfinite(cfg->max_step_rad) || !(cfg->max_step_rad > 0.0) || cfg->max_step_rad > M_PI)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "max_step_rad must be finite and in (0, pi]");
    if (!std::isfinite(cfg->min_sep_rad) || cfg->min_sep_rad < 0.0 || cfg->min_sep_rad > M_PI)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "min_sep_rad must be finite and in [0, pi]");
    if (cfg->hold < 0 || cfg->hold > 1000) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "hold must be in [0,1000]");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t n = (size_t)c->cfg.max_streams * MCA_MAX_SOURCES;
    if (!c->d_trk_theta) {
        DevBuf<float> nth, npk;
        DevBuf<int> ni;
        DevBuf<float2> nt0;
        hipError_t e = nth.alloc(n);
        if (e == hipSuccess) e = ni.alloc(n * 3);
        if (e == hipSuccess) e = npk.alloc(n * 2);
        if (e == hipSuccess) e = nt0.alloc(n * c->M * (c->N / 64 + 33));
        if (e != hipSuccess) return hip_fail(c, e, "track state");
        c->d_trk_theta.swap(nth); c->d_trk_int.swap(ni); c->d_trk_peak.swap(npk); c->d_trk_T0.swap(nt0);
    }
    HIP_TRY(c, hipDeviceSynchronize());                       // no update in flight writes what is cleared here
    HIP_TRY(c, hipMemset(c->d_trk_theta, 0, c->d_trk_theta.bytes()));
    HIP_TRY(c, hipMemset(c->d_trk_int, 0, c->d_trk_int.bytes()));
    if (cfg->enable == 1) HIP_TRY(c, reset_elevations(c));   // the tracks live at the context's elevation: every slot back to unset
    if (c->d_trk_eps) HIP_TRY(c, hipMemset(c->d_trk_eps, 0, c->d_trk_eps.bytes()));
    c->trk = *cfg; c->trk_on = cfg->enable == 1;
    c->trk_map_on = false;                                      // map mode is entered anew (mca_hip_mvdr_tracks_set_map)
    c->trk_ever = true;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_tracks_get_config(const mca_hip_mvdr_ctx *c, mca_hip_mvdr_tracks_config *cfg)
{
    if (!c || !cfg) return MCA_HIP_ERR_INVALID_ARGUMENT;
    *cfg = c->trk;
    cfg->struct_size = (int)sizeof(mca_hip_mvdr_tracks_config);
    cfg->enable = c->trk_on ? 1 : 0;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_tracks_seed_dev(mca_hip_mvdr_ctx *c, int n_streams, const float *doa, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = tracks_ready(c, n_streams)) return rc;
    if (const int rc = tracks_ready_1d(c)) return rc;
    if (!doa) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "doa_dev is NULL");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    MvdrTrackSeedArgs sa{track_state(c), doa, n_streams, c->trk.n_tracks, c->geo_mode == MCA_HIP_MVDR_GEOMETRY_XYZ ? 1 : 0};
    launch(c, kptr(k_mvdr_track_seed), grid_for(n_streams * c->trk.n_tracks, 256), dim3(256), 0, &sa, T_TRACKS, st);
    HIP_TRY(c, hipGetLastError());
    return MCA_HIP_OK;
}

int mca_hip_mvdr_tracks_seed_host(mca_hip_mvdr_ctx *c, int n_streams, const float *doa)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = tracks_ready(c, n_streams)) return rc;
    if (const int rc = tracks_ready_1d(c)) return rc;
    if (!doa) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "doa is NULL");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    StageBuf b[] = {{SG_AUX2, doa, (size_t)n_streams * c->trk.n_tracks * 4, STAGE_IN}};
    return staged(c, b, [&] { return mca_hip_mvdr_tracks_seed_dev(c, n_streams, (float *)b[0].dev, nullptr); });
}

int mca_hip_mvdr_tracks_update_dev(mca_hip_mvdr_ctx *c, int n_streams, float *own_spectrum, unsigned char *own_used, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = tracks_ready(c, n_streams)) return rc;
    if (const int rc = tracks_ready_1d(c)) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int n_own = c->trk.n_own;
    const MvdrScanPlan p = plan_mvdr_tracks(*c, c->spec.bin_lo, c->spec.bin_hi, c->spec_dpad, n_own, n_streams);
    if (const int rc = grow_ws(c, c->d_trk_part, p.per_part * n_streams, "partial sums of the own tracks", true)) return rc;
    // the Capon peaks: the kernels of mca_hip_mvdr_spectrum_dev, into the context's own rows.  Not launched where every slot is an own
    // track: a peak then changes no track (it is within min_sep of an own track and skipped, or waits as a birth no slot takes)
    float *pk_doa = c->d_trk_peak, *pk_val = c->d_trk_peak + (size_t)c->cfg.max_streams * MCA_MAX_SOURCES;
    const bool capon = n_own < c->trk.n_tracks;
    if (capon)
        if (const int rc = launch_spectrum(c, n_streams, nullptr, pk_doa, pk_val, st)) return rc;
    MvdrTrackPickArgs pa = track_pick_args(c);
    pa.cand_doa = pk_doa; pa.cand_val = pk_val; pa.n_cand = capon ? c->spec.n_peaks : 0;
    if (n_own > 0 && own_used) HIP_TRY(c, hipMemsetAsync(own_used, 0, (size_t)n_streams * n_own * c->K, st));      // the bins outside the band's chunks
    t_begin(c, T_TRACKS, st);
    if (n_own > 0) {
        MvdrTrackTablesArgs ta{c->d_trk_theta, c->d_trk_T0, c->d_micx, (double)c->cfg.sample_rate / (double)c->N / 346.1, c->N, c->M, n_own, geometry_args(c)};
        launch(c, kptr(k_mvdr_track_tables), p.grid(p.wg_tables, n_streams), dim3(256), 0, &ta, T_NONE, st);
        MvdrTrackSpectrumArgs sa{};
        scan_args(c, sa, p.b, c->d_spec_T, c->spec.n_angles, c->spec_dpad, c->spec.bin_lo, c->spec.bin_hi);
        sa.psi = c->d_psi; sa.cpsi = c->d_cpsi; sa.cphi = c->d_cphi;
        sa.T0 = c->d_trk_T0; sa.alive = track_state(c).alive; sa.part = c->d_trk_part; sa.used = own_used;
        sa.n_own = n_own; sa.slots = c->max_sources;
        sa.min_share = (float)c->rtf_min_share; sa.iterations = c->rtf_iterations; sa.ref_mic = c->rtf_ref;
        launch(c, mvdr_track_spectrum_kernel(c->Q()), p.grid(p.wg_scan, n_streams), dim3(256), 0, &sa, T_NONE, st);
        pa.part = c->d_trk_part; pa.n_slices = p.b.n_slices; pa.own_spectrum = own_spectrum;
    }
    launch(c, kptr(k_mvdr_track_pick), dim3(n_streams), dim3(256), 0, &pa, T_NONE, st);
    t_end(c, st);
    HIP_TRY(c, hipGetLastError());
    return MCA_HIP_OK;
}

int mca_hip_mvdr_tracks_update_host(mca_hip_mvdr_ctx *c, int n_streams, float *own_spectrum, unsigned char *own_used)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = tracks_ready(c, n_streams)) return rc;
    if (const int rc = tracks_ready_1d(c)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t sb = (size_t)n_streams * c->trk.n_own * c->spec.n_angles * 4, ub = (size_t)n_streams * c->trk.n_own * c->K;
    StageBuf b[] = {{SG_SCAN, own_spectrum, sb, STAGE_OUT}, {SG_AUX1, own_used, ub, STAGE_OUT}};      // (n_own == 0: nothing of either)
    return staged(c, b, [&] { return mca_hip_mvdr_tracks_update_dev(c, n_streams, (float *)b[0].dev, (unsigned char *)b[1].dev, nullptr); });
}

int mca_hip_mvdr_tracks_associate_dev(mca_hip_mvdr_ctx *c, int n_streams, const float *own_doa, int n_cand, const float *cand_doa, const float *cand_val,
                                      void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = tracks_ready(c, n_streams)) return rc;
    if (const int rc = tracks_ready_1d(c)) return rc;
    if (n_cand < 1 || n_cand > MVDR_TRACK_MAX_CAND) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_cand must be in [1,8]");
    if (!cand_doa || !cand_val) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "cand_doa_dev / cand_val_dev is NULL");
    if (c->trk.n_own > 0 && !own_doa) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "own_doa_dev is NULL on tracks with n_own > 0");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    MvdrTrackPickArgs pa = track_pick_args(c);
    pa.own_doa = own_doa; pa.cand_doa = cand_doa; pa.cand_val = cand_val; pa.n_cand = n_cand;
    launch(c, kptr(k_mvdr_track_pick), dim3(n_streams), dim3(256), 0, &pa, T_TRACKS, st);
    HIP_TRY(c, hipGetLastError());
    return MCA_HIP_OK;
}

int mca_hip_mvdr_tracks_fill_dev(mca_hip_mvdr_ctx *c, int n_streams, int n_frames, float *doa_rad, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = tracks_ready(c, n_streams)) return rc;
    if (n_frames < 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_frames < 1");
    if (!doa_rad) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "doa_rad_dev is NULL");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const dim3 grid = grid_for((long long)n_streams * n_frames, 256);
    if (c->trk_map_on) {
        // map mode: the elevations of the slots travel with the azimuths, on the same stream
        MvdrTrk2FillArgs fa{track_state_map(c), doa_rad, n_streams, n_frames, c->trk.n_tracks, c->d_slot_el, c->d_slot_val, std::cos(c->geo_elevation), std::sin(c->geo_elevation)};
        launch(c, kptr(k_mvdr_trk2_fill), grid, dim3(256), 0, &fa, T_TRACKS_MAP, st);
    } else {
        MvdrTrackFillArgs fa{track_state(c), doa_rad, n_streams, n_frames, c->trk.n_tracks};
        launch(c, kptr(k_mvdr_track_fill), grid, dim3(256), 0, &fa, T_TRACKS, st);
    }
    HIP_TRY(c, hipGetLastError());
    return MCA_HIP_OK;
}

int mca_hip_mvdr_tracks_fill_host(mca_hip_mvdr_ctx *c, int n_streams, int n_frames, float *doa_rad)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = tracks_ready(c, n_streams)) return rc;
    if (n_frames < 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_frames < 1");
    if (!doa_rad) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "doa_rad is NULL");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    StageBuf b[] = {{SG_AUX2, doa_rad, (size_t)n_streams * n_frames * c->trk.n_tracks * 4, STAGE_OUT}};
    return staged(c, b, [&] { return mca_hip_mvdr_tracks_fill_dev(c, n_streams, n_frames, (float *)b[0].dev, nullptr); });
}

int mca_hip_mvdr_tracks_get(mca_hip_mvdr_ctx *c, int n_streams, float *theta, int *alive, int *miss, int *gen)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = tracks_ready(c, n_streams)) return rc;
    if (!theta && !alive && !miss && !gen) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "theta, alive, miss and gen are all NULL");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipDeviceSynchronize());
    const size_t n = (size_t)n_streams * MCA_MAX_SOURCES, all = (size_t)c->cfg.max_streams * MCA_MAX_SOURCES;
    std::vector<float> hf(n);
    std::vector<int> hi(n);
    const int T = c->trk.n_tracks;
    if (theta) {
        HIP_TRY(c, hipMemcpy(hf.data(), c->d_trk_theta, n * 4, hipMemcpyDeviceToHost));
        for (int a = 0; a < n_streams; ++a)
            for (int s = 0; s < T; ++s) theta[a * T + s] = hf[(size_t)a * MCA_MAX_SOURCES + s];
    }
    int *outs[3] = {alive, miss, gen};
    for (int j = 0; j < 3; ++j)
        if (outs[j]) {
            HIP_TRY(c, hipMemcpy(hi.data(), c->d_trk_int + j * all, n * 4, hipMemcpyDeviceToHost));
            for (int a = 0; a < n_streams; ++a)
                for (int s = 0; s < T; ++s) outs[j][a * T + s] = hi[(size_t)a * MCA_MAX_SOURCES + s];
        }
    return MCA_HIP_OK;
}

// ---- the tracks' map mode: azimuth and elevation, fed by the Capon map (kernels_mvdr_trk2.hip) ----
extern "C++" {
namespace {
int tracks_map_ready(mca_hip_mvdr_ctx *c, int n_streams)
{
    if (const int rc = tracks_ready(c, n_streams)) return rc;
    if (!c->trk_map_on) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "mca_hip_mvdr_tracks_set_map first (with enable = 1)");
    if (!c->map_set) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "mca_hip_mvdr_map_configure first");
    return MCA_HIP_OK;
}
// the association's part of the pick kernel's arguments, for the streams from first_stream on
MvdrTrk2PickArgs trk2_pick_args(mca_hip_mvdr_ctx *c, int first_stream)
{
    MvdrTrk2PickArgs pa{};
    pa.st = track_state_map(c, first_stream);
    pa.az = c->d_map_az; pa.el = c->d_map_el; pa.n_az = c->map.n_az; pa.n_el = c->map.n_el; pa.Dpad = c->map_dpad;
    pa.n_tracks = c->trk.n_tracks; pa.n_own = c->trk.n_own; pa.hold = c->trk.hold;
    pa.max_step = (float)c->trk.max_step_rad; pa.min_sep = (float)c->trk.min_sep_rad;
    pa.max_step_el = (float)c->trkm.max_step_el_rad; pa.min_sep_el = (float)c->trkm.min_sep_el_rad;
    pa.slots = c->max_sources; pa.K = c->K; pa.tri = c->tri;
    if (c->rtf_on) {
        pa.psi = c->d_psi + (size_t)first_stream * pa.slots * c->K * c->tri;
        pa.cpsi = c->d_cpsi + (size_t)first_stream * pa.slots * c->K;
    }
    return pa;
}
}  // namespace
}  // extern "C++"

int mca_hip_mvdr_tracks_set_map(mca_hip_mvdr_ctx *c, const mca_hip_mvdr_tracks_map_config *cfg)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!cfg) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (cfg->struct_size != (int)sizeof(mca_hip_mvdr_tracks_map_config)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "struct_size mismatch");
    if (cfg->enable != 0 && cfg->enable != 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "enable must be 0 or 1");
    if (!std::isfinite(cfg->max_step_el_rad) || cfg->max_step_el_rad < 0.0 || cfg->max_step_el_rad > M_PI)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "max_step_el_rad must be finite and in [0, pi]");
    if (!std::isfinite(cfg->min_sep_el_rad) || cfg->min_sep_el_rad < 0.0 || cfg->min_sep_el_rad > M_PI)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "min_sep_el_rad must be finite and in [0, pi]");
    if (cfg->enable == 1) {
        if (c->geo_mode != MCA_HIP_MVDR_GEOMETRY_XYZ) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "map mode needs XYZ geometry (mca_hip_mvdr_set_geometry)");
        if (!c->trk_on) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "mca_hip_mvdr_tracks_configure first (with enable = 1)");
        if (!c->map_set) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "mca_hip_mvdr_map_configure first: map mode uses its grid, band and n_peaks");
    }
    if (cfg->enable == 0 && !c->trk_map_on) { c->trkm = *cfg; return MCA_HIP_OK; }      // nothing to leave
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t n = (size_t)c->cfg.max_streams * MCA_MAX_SOURCES;
    if (!c->d_trk_eps) {
        DevBuf<float> ne, npk;
        hipError_t e = ne.alloc(n);
        if (e == hipSuccess) e = npk.alloc(n * 3);
        if (e != hipSuccess) return hip_fail(c, e, "track state of the map mode");
        c->d_trk_eps.swap(ne); c->d_trk2_peak.swap(npk);
    }
    // entering and leaving alike: the angles change meaning, so every slot starts from nothing
    HIP_TRY(c, hipDeviceSynchronize());                       // no update in flight writes what is cleared here
    HIP_TRY(c, hipMemset(c->d_trk_theta, 0, c->d_trk_theta.bytes()));
    HIP_TRY(c, hipMemset(c->d_trk_eps, 0, c->d_trk_eps.bytes()));
    HIP_TRY(c, hipMemset(c->d_trk_int, 0, c->d_trk_int.bytes()));
    if (cfg->enable == 0) HIP_TRY(c, reset_elevations(c));    // the tracks on one angle live at the context's elevation
    c->trkm = *cfg; c->trk_map_on = cfg->enable == 1;
    if (c->trk_map_on) c->trk_map_ever = true;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_tracks_get_map_config(const mca_hip_mvdr_ctx *c, mca_hip_mvdr_tracks_map_config *cfg)
{
    if (!c || !cfg) return MCA_HIP_ERR_INVALID_ARGUMENT;
    *cfg = c->trkm;
    cfg->struct_size = (int)sizeof(mca_hip_mvdr_tracks_map_config);
    cfg->enable = c->trk_map_on ? 1 : 0;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_tracks_seed_map_dev(mca_hip_mvdr_ctx *c, int n_streams, const float *az, const float *el, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = tracks_map_ready(c, n_streams)) return rc;
    if (!az || !el) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "az_dev / el_dev is NULL");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    MvdrTrk2SeedArgs sa{track_state_map(c), az, el, n_streams, c->trk.n_tracks};
    launch(c, kptr(k_mvdr_trk2_seed), grid_for(n_streams * c->trk.n_tracks, 256), dim3(256), 0, &sa, T_TRACKS_MAP, st);
    HIP_TRY(c, hipGetLastError());
    return MCA_HIP_OK;
}

int mca_hip_mvdr_tracks_seed_map_host(mca_hip_mvdr_ctx *c, int n_streams, const float *az, const float *el)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = tracks_map_ready(c, n_streams)) return rc;
    if (!az || !el) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "az / el is NULL");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t bytes = (size_t)n_streams * c->trk.n_tracks * 4;
    StageBuf b[] = {{SG_AUX1, az, bytes, STAGE_IN}, {SG_AUX2, el, bytes, STAGE_IN}};
    return staged(c, b, [&] { return mca_hip_mvdr_tracks_seed_map_dev(c, n_streams, (float *)b[0].dev, (float *)b[1].dev, nullptr); });
}

int mca_hip_mvdr_tracks_update_map_dev(mca_hip_mvdr_ctx *c, int n_streams, float *own_map, unsigned char *own_used, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = tracks_map_ready(c, n_streams)) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int n_own = c->trk.n_own, K = c->K, M = c->M, D = c->map.n_az * c->map.n_el;
    // the map's peaks: the kernels of mca_hip_mvdr_map_dev (timing slot 8), into the context's own rows.  Not launched where every slot
    // is an own track: a peak then changes no track
    const size_t row = (size_t)c->cfg.max_streams * MCA_MAX_SOURCES;
    float *pk_az = c->d_trk2_peak, *pk_el = c->d_trk2_peak + row, *pk_val = c->d_trk2_peak + 2 * row;
    const bool capon = n_own < c->trk.n_tracks;
    const int n_cand = capon ? c->map.n_peaks : 0;
    if (capon)
        if (const int rc = mca_hip_mvdr_map_dev(c, n_streams, nullptr, pk_az, pk_el, pk_val, stream)) return rc;
    // u, the flags and the partial sums are taken in passes of streams under the workspace cap (MvdrScanPlan)
    const MvdrScanPlan p = plan_mvdr_tracks_map(*c, c->map.bin_lo, c->map.bin_hi, c->map_dpad, n_own, n_streams, c->plane_cap_cells);
    const int pass = p.pass;
    if (n_own > 0) {
        if (const int rc = grow_ws(c, c->d_trk2_U, p.per_u * pass, "steering vectors of the own tracks", true)) return rc;
        if (const int rc = grow_ws(c, c->d_trk2_F, p.per_f * pass, "used flags of the own tracks", true)) return rc;
        if (const int rc = grow_ws(c, c->d_trk2_part, p.per_part * pass, "partial sums of the own tracks", true)) return rc;
        if (own_used) HIP_TRY(c, hipMemsetAsync(own_used, 0, (size_t)n_streams * n_own * K, st));      // the bins outside the band's chunks, the dead slots
    }
    t_begin(c, T_TRACKS_MAP, st);
    for (int s0 = 0; s0 < n_streams; s0 += pass) {
        const int ns = std::min(pass, n_streams - s0);
        MvdrTrk2PickArgs pa = trk2_pick_args(c, s0);
        pa.cand_az = pk_az + (size_t)s0 * n_cand; pa.cand_el = pk_el + (size_t)s0 * n_cand; pa.cand_val = pk_val + (size_t)s0 * n_cand; pa.n_cand = n_cand;
        if (n_own > 0) {
            const MvdrTrk2State ts = track_state_map(c, s0);
            float2 *T0 = c->d_trk_T0 + (size_t)s0 * n_own * M * p.b.nph;
            MvdrTrk2TablesArgs ta{ts.theta, ts.eps, ts.alive, T0, c->N, M, n_own, geometry_args(c)};
            launch(c, kptr(k_mvdr_trk2_tables), p.grid(p.wg_tables, ns), dim3(256), 0, &ta, T_NONE, st);
            MvdrTrk2ScanArgs sa{};
            MvdrTrackSpectrumArgs &sp = sa.s;
            scan_args(c, sp, p.b, c->d_map_T, D, c->map_dpad, c->map.bin_lo, c->map.bin_hi, s0);
            sp.cphi = c->d_cphi + (size_t)s0 * K;
            sp.psi = c->d_psi + (size_t)s0 * c->max_sources * K * c->tri; sp.cpsi = c->d_cpsi + (size_t)s0 * c->max_sources * K;
            sp.T0 = T0; sp.alive = ts.alive; sp.part = c->d_trk2_part;
            sp.used = own_used ? own_used + (size_t)s0 * n_own * K : nullptr;
            sp.n_own = n_own; sp.slots = c->max_sources;
            sp.min_share = (float)c->rtf_min_share; sp.iterations = c->rtf_iterations; sp.ref_mic = c->rtf_ref;
            sa.U = c->d_trk2_U; sa.F = c->d_trk2_F; sa.az = c->d_map_az; sa.el = c->d_map_el; sa.theta = ts.theta; sa.eps = ts.eps;
            sa.max_step = pa.max_step; sa.max_step_el = pa.max_step_el; sa.n_az = c->map.n_az; sa.n_tiles = p.b.n_tiles; sa.n_streams = ns;
            sa.skip = own_map ? 0 : 1;
            launch(c, mvdr_trk2_vectors_kernel(c->Q()), p.grid(p.wg_vectors, ns), dim3(256), 0, &sa, T_NONE, st);
            launch(c, kptr(k_mvdr_trk2_scan), p.grid(p.wg_scan, ns), dim3(256), 0, &sa, T_NONE, st);
            pa.part = c->d_trk2_part; pa.n_slices = p.b.n_slices;
            pa.own_map = own_map ? own_map + (size_t)s0 * n_own * D : nullptr;
        }
        launch(c, kptr(k_mvdr_trk2_pick), dim3(ns), dim3(256), 0, &pa, T_NONE, st);
    }
    t_end(c, st);
    HIP_TRY(c, hipGetLastError());
    return MCA_HIP_OK;
}

int mca_hip_mvdr_tracks_update_map_host(mca_hip_mvdr_ctx *c, int n_streams, float *own_map, unsigned char *own_used)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = tracks_map_ready(c, n_streams)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t mb = (size_t)n_streams * c->trk.n_own * c->map.n_az * c->map.n_el * 4, ub = (size_t)n_streams * c->trk.n_own * c->K;
    StageBuf b[] = {{SG_SCAN, own_map, mb, STAGE_OUT}, {SG_AUX1, own_used, ub, STAGE_OUT}};      // (n_own == 0: nothing of either)
    return staged(c, b, [&] { return mca_hip_mvdr_tracks_update_map_dev(c, n_streams, (float *)b[0].dev, (unsigned char *)b[1].dev, nullptr); });
}

int mca_hip_mvdr_tracks_associate_map_dev(mca_hip_mvdr_ctx *c, int n_streams, const float *own_az, const float *own_el, int n_cand, const float *cand_az,
                                          const float *cand_el, const float *cand_val, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = tracks_map_ready(c, n_streams)) return rc;
    if (n_cand < 1 || n_cand > MVDR_TRACK_MAX_CAND) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_cand must be in [1,8]");
    if (!cand_az || !cand_el || !cand_val) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "cand_az_dev / cand_el_dev / cand_val_dev is NULL");
    if (c->trk.n_own > 0 && (!own_az || !own_el)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "own_az_dev / own_el_dev is NULL on tracks with n_own > 0");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    MvdrTrk2PickArgs pa = trk2_pick_args(c, 0);
    pa.own_az = c->trk.n_own > 0 ? own_az : nullptr; pa.own_el = c->trk.n_own > 0 ? own_el : nullptr;
    pa.cand_az = cand_az; pa.cand_el = cand_el; pa.cand_val = cand_val; pa.n_cand = n_cand;
    launch(c, kptr(k_mvdr_trk2_pick), dim3(n_streams), dim3(256), 0, &pa, T_TRACKS_MAP, st);
    HIP_TRY(c, hipGetLastError());
    return MCA_HIP_OK;
}

int mca_hip_mvdr_tracks_get_map(mca_hip_mvdr_ctx *c, int n_streams, float *theta, float *eps, int *alive, int *miss, int *gen)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (const int rc = tracks_map_ready(c, n_streams)) return rc;
    if (!theta && !eps && !alive && !miss && !gen) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "theta, eps, alive, miss and gen are all NULL");
    if (theta || alive || miss || gen)
        if (const int rc = mca_hip_mvdr_tracks_get(c, n_streams, theta, alive, miss, gen)) return rc;
    if (eps) {
        HIP_TRY(c, hipSetDevice(c->cfg.device));
        HIP_TRY(c, hipDeviceSynchronize());
        std::vector<float> hf((size_t)n_streams * MCA_MAX_SOURCES);
        HIP_TRY(c, hipMemcpy(hf.data(), c->d_trk_eps, hf.size() * 4, hipMemcpyDeviceToHost));
        const int T = c->trk.n_tracks;
        for (int a = 0; a < n_streams; ++a)
            for (int s = 0; s < T; ++s) eps[a * T + s] = hf[(size_t)a * MCA_MAX_SOURCES + s];
    }
    return MCA_HIP_OK;
}

extern "C++" {
namespace {
// the covariance [K][tri] of one stream or slot (the lower triangle, row by row) read back as the Hermitian [K][M][M] in double
int read_hermitian(mca_hip_mvdr_ctx *c, const float2 *tri_dev, double *out)
{
    const int M = c->M;
    std::vector<float2> h((size_t)c->K * c->tri);
    HIP_TRY(c, hipMemcpy(h.data(), tri_dev, h.size() * sizeof(float2), hipMemcpyDeviceToHost));
    for (int k = 0; k < c->K; ++k)
        for (int i = 0; i < M; ++i)
            for (int j = 0; j <= i; ++j) {
                const float2 v = h[(size_t)k * c->tri + i * (i + 1) / 2 + j];
                double *lo = out + (((size_t)k * M + i) * M + j) * 2, *up = out + (((size_t)k * M + j) * M + i) * 2;
                lo[0] = v.x; lo[1] = i == j ? 0.0 : v.y;
                up[0] = v.x; up[1] = i == j ? 0.0 : -(double)v.y;
            }
    return MCA_HIP_OK;
}
}  // namespace
}  // extern "C++"

int mca_hip_mvdr_get_covariance(mca_hip_mvdr_ctx *c, int s, double *out)
{
    if (!c || !out) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (s < 0 || s >= c->cfg.max_streams) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "stream_index out of range");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipDeviceSynchronize());
    return read_hermitian(c, c->d_phi + (size_t)s * c->K * c->tri, out);
}

int mca_hip_mvdr_get_target_covariance(mca_hip_mvdr_ctx *c, int s, int source, double *out, double *norm)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!out && !norm) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "out and norm are both NULL");
    if (!c->rtf_on) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "RTF is not enabled on this context (mca_hip_mvdr_set_rtf)");
    if (s < 0 || s >= c->cfg.max_streams) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "stream_index out of range");
    if (source < 0 || source >= c->max_sources) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "source outside [0, max_sources)");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipDeviceSynchronize());
    const size_t slot = (size_t)s * c->max_sources + source;
    if (out)
        if (const int rc = read_hermitian(c, c->d_psi + slot * c->K * c->tri, out)) return rc;
    if (norm) {
        std::vector<float> h((size_t)c->K);
        HIP_TRY(c, hipMemcpy(h.data(), c->d_cpsi + slot * c->K, h.size() * 4, hipMemcpyDeviceToHost));
        for (int k = 0; k < c->K; ++k) norm[k] = h[k];
    }
    return MCA_HIP_OK;
}

int mca_hip_mvdr_get_steering(mca_hip_mvdr_ctx *c, int s, int source, double doa_rad, double *out, unsigned char *estimated)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!out && !estimated) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "out and estimated are both NULL");
    if (!c->rtf_on) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "RTF is not enabled on this context (mca_hip_mvdr_set_rtf)");
    if (s < 0 || s >= c->cfg.max_streams) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "stream_index out of range");
    if (source < 0 || source >= c->max_sources) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "source outside [0, max_sources)");
    if (!std::isfinite(doa_rad)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "doa_rad is not finite");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipDeviceSynchronize());
    // the factored phasors of the look direction, as the analysis forms them (MvdrAnalyseArgs::T), the phase in double
    const int M = c->M, K = c->K, nhi = c->N / 64 + 1, nph = nhi + 32;
    // (XYZ mode: at the elevation of the slot, mca_hip_mvdr_set_elevations_*)
    const bool xyz = c->geo_mode == MCA_HIP_MVDR_GEOMETRY_XYZ;
    double2 el = make_double2(1.0, 0.0);
    if (xyz) HIP_TRY(c, hipMemcpy(&el, c->d_slot_el + (size_t)s * MCA_MAX_SOURCES + source, sizeof(double2), hipMemcpyDeviceToHost));
    std::vector<float2> T((size_t)M * nph);
    for (int m = 0; m < M; ++m)
        for (int e = 0; e < nph; ++e) {
            double t = (e < nhi ? 32.0 * e : (double)(e - nhi)) * (xyz ? host_projection_xyz(c, m, doa_rad, el.x, el.y) : host_projection(c, m, doa_rad));
            t -= std::rint(t);
            T[(size_t)m * nph + e] = make_float2((float)std::cos(2.0 * M_PI * t), (float)(-std::sin(2.0 * M_PI * t)));
        }
    const size_t tb = T.size() * sizeof(float2), ob = (size_t)K * M * sizeof(float2);
    DevBuf<char> buf;                                           // T, the vectors, the flags
    if (const hipError_t e = buf.alloc(tb + ob + (size_t)K)) return hip_fail(c, e, "steering vectors");
    MvdrRtfSteerArgs ga{};
    const size_t slot = (size_t)s * c->max_sources + source;
    ga.phi = c->d_phi + (size_t)s * K * c->tri; ga.psi = c->d_psi + slot * K * c->tri;
    ga.cpsi = c->d_cpsi + slot * K; ga.cphi = c->d_cphi + (size_t)s * K;
    ga.T = reinterpret_cast<float2 *>(buf.p); ga.K = K; ga.M = M;
    ga.min_share = (float)c->rtf_min_share; ga.iterations = c->rtf_iterations; ga.ref_mic = c->rtf_ref;
    ga.out = reinterpret_cast<float2 *>(buf + tb); ga.estimated = reinterpret_cast<unsigned char *>(buf + tb + ob);
    std::vector<float2> h((size_t)K * M);
    std::vector<unsigned char> he((size_t)K);
    const int Q = (M + 3) / 4;
    void *kargs[1] = {&ga};
    hipError_t e = hipMemcpy(buf, T.data(), tb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipLaunchKernel(mvdr_rtf_kernel(Q, true), dim3((unsigned)((K + 63) / 64)), dim3(256), kargs, 0, nullptr);
    if (e == hipSuccess) e = hipMemcpy(h.data(), buf + tb, ob, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(he.data(), buf + tb + ob, (size_t)K, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, MCA_HIP_ERR_HIP, std::string("steering vectors: ") + hipGetErrorString(e));
    if (out)
        for (size_t i = 0; i < h.size(); ++i) { out[2 * i] = h[i].x; out[2 * i + 1] = h[i].y; }
    if (estimated) std::memcpy(estimated, he.data(), (size_t)K);
    return MCA_HIP_OK;
}

extern "C++" {
namespace {
constexpr unsigned MVDR_MAGIC = 0x4d435644u;   // "MCVD"
std::vector<BlobPart> mvdr_parts(mca_hip_mvdr_ctx *c)
{
    DevBuf<float> &tail = c->d_tail[c->tail_cur];
    std::vector<BlobPart> parts{{c->d_phi.p, c->d_phi.bytes()}, {c->d_trace.p, c->d_trace.bytes()}, {tail.p, tail.bytes()}};
    if (c->pf_on) parts.push_back({c->d_pf_A.p, c->d_pf_A.bytes()});
    if (c->rtf_on) {
        parts.push_back({c->d_psi.p, c->d_psi.bytes()});
        parts.push_back({c->d_cpsi.p, c->d_cpsi.bytes()});
        parts.push_back({c->d_cphi.p, c->d_cphi.bytes()});
    }
    return parts;
}
unsigned mvdr_cfg_hash(const mca_hip_mvdr_ctx *c)
{
    const int v[5] = {c->N, c->M, c->cfg.max_streams, c->cfg.sample_rate, 0};
    unsigned h = blob_fnv(v, sizeof(v));
    h = blob_fnv(&c->cfg.alpha, sizeof(double), h);
    return blob_fnv(&c->cfg.loading, sizeof(double), h);
}
}  // namespace
}  // extern "C++"

long long mca_hip_mvdr_state_size(const mca_hip_mvdr_ctx *c) { return state_size(c, c ? mvdr_parts(const_cast<mca_hip_mvdr_ctx *>(c)) : std::vector<BlobPart>()); }

int mca_hip_mvdr_state_save(mca_hip_mvdr_ctx *c, void *blob, long long bytes)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    // version 1: one tail per stream (a context that never raised max_sources writes what it always wrote);
    // version 2: max_sources tails per stream, the maximum in host[0];
    // version 3: a context with the post-filter enabled -- the same and A behind the tails, the maximum in host[0], 1 in host[1]
    BlobHeader h{MVDR_MAGIC, c->max_sources > 1 ? 2 : 1, mvdr_cfg_hash(c), 0, {c->max_sources > 1 ? c->max_sources : 0, 0, 0, 0}};
    if (c->pf_on) { h.version = 3; h.host[0] = c->max_sources; h.host[1] = 1; }
    // version 4: a context with RTF enabled -- the same (A only with the post-filter, 1 in host[1] then), Psi, cpsi and cphi behind it, 1 in host[2]
    if (c->rtf_on) { h.version = 4; h.host[0] = c->max_sources; h.host[1] = c->pf_on ? 1 : 0; h.host[2] = 1; }
    return state_save(c, mvdr_parts(c), h, blob, bytes);
}

int mca_hip_mvdr_state_load(mca_hip_mvdr_ctx *c, const void *blob, long long bytes)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    BlobHeader h;
    if (blob && bytes >= (long long)sizeof(BlobHeader)) {      // the feature parts: what the blob holds is what the context has
        std::memcpy(&h, blob, sizeof(h));
        const int blob_max = h.version >= 2 && h.version <= 4 ? (int)h.host[0] : 1;
        const bool blob_pf = h.version == 3 || (h.version == 4 && h.host[1] != 0), known = h.magic == MVDR_MAGIC && h.version >= 1 && h.version <= 4;
        if (known && (h.version == 4) != c->rtf_on)
            return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, h.version == 4 ? "state blob was saved with RTF enabled, this context has it disabled"
                                                                         : "state blob was saved without RTF, this context has it enabled");
        if (known && blob_pf != c->pf_on)
            return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, blob_pf ? "state blob was saved with the post-filter enabled, this context has it disabled"
                                                                  : "state blob was saved without the post-filter, this context has it enabled");
        if (known && blob_max != c->max_sources)
            return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "state blob was saved by a context with max_sources = " + std::to_string(blob_max) +
                                                              ", this one has " + std::to_string(c->max_sources));
    }
    const int rc = state_load(c, mvdr_parts(c), MVDR_MAGIC, c->rtf_on ? 4 : c->pf_on ? 3 : c->max_sources > 1 ? 2 : 1, mvdr_cfg_hash(c), blob, bytes, &h);
    if (!rc && c->d_trk_theta) {
        // the tracks are no part of a blob: a loaded context starts without them and is seeded again
        HIP_TRY(c, hipMemset(c->d_trk_theta, 0, c->d_trk_theta.bytes()));
        HIP_TRY(c, hipMemset(c->d_trk_int, 0, c->d_trk_int.bytes()));
        if (c->d_trk_eps) HIP_TRY(c, hipMemset(c->d_trk_eps, 0, c->d_trk_eps.bytes()));
    }
    return rc;
}

int mca_hip_mvdr_set_timing(mca_hip_mvdr_ctx *c, int enable)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    c->timing = enable != 0;
    return MCA_HIP_OK;
}

int mca_hip_mvdr_get_timing(mca_hip_mvdr_ctx *c, int kernel_id, int *launches, double *total_ms)
{
    // slot -> the flag that opens it: a slot of a feature exists once the feature was ever on (a context that never had it refuses the id as it always did)
    static bool mca_hip_mvdr_ctx::*const opens[T_COUNT] = {nullptr, nullptr, nullptr, nullptr, &mca_hip_mvdr_ctx::pf_ever, &mca_hip_mvdr_ctx::rtf_ever, &mca_hip_mvdr_ctx::em_ever,
                                                           &mca_hip_mvdr_ctx::trk_ever, &mca_hip_mvdr_ctx::map_ever, &mca_hip_mvdr_ctx::trk_map_ever};
    if (!c || kernel_id < 0 || kernel_id >= T_COUNT || (opens[kernel_id] && !(c->*opens[kernel_id]))) return MCA_HIP_ERR_INVALID_ARGUMENT;
    for (auto &e : c->events) {
        HIP_TRY(c, hipEventSynchronize(e.b));
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, e.a, e.b));
        c->t_ms[e.id] += ms; c->t_launches[e.id] += 1;
        (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b);
    }
    c->events.clear();
    if (launches) *launches = c->t_launches[kernel_id];
    if (total_ms) *total_ms = c->t_ms[kernel_id];
    return MCA_HIP_OK;
}

}  // extern "C"
