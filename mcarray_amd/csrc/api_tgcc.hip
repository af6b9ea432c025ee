// api_tgcc.hip -- C ABI of the time-domain 2-microphone localiser (include/mcarray_hip.h, mca_hip_tgcc_*).
// Host side only: the geometry the reference's constructor computes (BinauralLocalisation.cpp:66-101), the per-array
// state, the frame hook's own state, and the launches of kernels_tgcc.hip.  No CPU fallback.
#include "../../include/mcarray_hip.h"
#include "host_common.h"
#include "kernels.h"
#include "module_plan.h"

#include <cmath>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

using namespace mca;

struct mca_hip_tgcc_ctx {
    mca_hip_tgcc_config cfg{};
    double dist = 0;
    int W = 0, hop = 0, nd = 0, W8 = 0, needed = 0, rem = 0;
    DevBuf<double> d_state;                        // [max_arrays][TGCC_STATE]
    DevBuf<double> d_hook_state;                   // [TGCC_STATE] the frame hook's module
    DevBuf<double> d_hook_in;                      // padded channels of one double frame
    DevBuf<double> d_hook_res, d_hook_out, d_hook_index;
    DevBuf<double> d_res;                          // workspace: [rows][TGCC_RES]
    StagePool stage;
    std::string err;
};

namespace {

mca_hip_tgcc_ctx *const NO_CTX = nullptr;        // a failing create: the text goes to the module's creation error
enum TgccStageSlot { SG_PCM, SG_DOA, SG_PROB, SG_POWER, SG_VOICED, SG_DELAY, SG_INDEX };      // the staging-pool slots of the host-pointer call: the numbers stay

// _currentDOA = 0, _prob = -1 (:88-89), _powerFloor = 0, nothing consumed, not estimated
int init_state(mca_hip_tgcc_ctx *c, hipStream_t st)
{
    const size_t na = (size_t)c->cfg.max_arrays;
    std::vector<double> s((na + 1) * TGCC_STATE, 0.0);
    for (size_t a = 0; a <= na; ++a) s[a * TGCC_STATE + 1] = -1.0;
    HIP_TRY(c, hipMemcpyAsync(c->d_state, s.data(), c->d_state.bytes(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_hook_state, s.data() + na * TGCC_STATE, c->d_hook_state.bytes(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return MCA_HIP_OK;
}

int ensure_ws(mca_hip_tgcc_ctx *c, size_t rows)
{
    HIP_TRY(c, c->d_res.grow(rows * TGCC_RES));
    return MCA_HIP_OK;
}

}  // namespace

extern "C" {

const char *mca_hip_tgcc_last_error(const mca_hip_tgcc_ctx *ctx) { return last_error(ctx); }

int mca_hip_tgcc_create(const mca_hip_tgcc_config *cfg, mca_hip_tgcc_ctx **out)
{
    if (!cfg || !out) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "cfg/out is NULL");
    *out = nullptr;
    if (cfg->struct_size != (int)sizeof(mca_hip_tgcc_config)) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "struct_size mismatch");
    if (cfg->sample_rate <= 0 || cfg->sample_rate > 96000) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "sample_rate must be in [1, 96000]");
    if (cfg->max_arrays < 1 || cfg->max_arrays > 65535) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "max_arrays must be in [1, 65535]");
    const double *x = &cfg->mic_xyz[0][0];
    const double dist = std::sqrt(std::pow(x[3] - x[0], 2) + std::pow(x[4] - x[1], 2) + std::pow(x[5] - x[2], 2));   // distance(0,1)
    if (!(dist > 0)) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "the two microphones coincide");
    const double c_sound = 346.1;                                               // getSpeedOfSound()
    const int nd = (int)(dist * cfg->sample_rate / c_sound);                    // _ndelays (:71)
    if (nd < 2) {                                                               // :76-80 (samples2Degrees divides by nd - 1)
        std::ostringstream oss;
        oss << "Sample frequency has to be a least " << c_sound * 2 / dist;
        return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, oss.str());
    }
    if (nd > TGCC_MAX_ND) {
        std::ostringstream oss;
        oss << "distance(0,1) * sample_rate / 346.1 = " << nd << " delay pairs; the kernels support at most " << TGCC_MAX_ND;
        return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, oss.str());
    }
    if (const int rc = check_device(NO_CTX, cfg->device)) return rc;

    mca_hip_tgcc_ctx *c = new mca_hip_tgcc_ctx();
    c->cfg = *cfg;
    c->dist = dist;
    c->W = (int)(2 * (0.075 * cfg->sample_rate));                               // window = analysis length (:68, .h:52)
    c->hop = c->W / 2;                                                          // [BUILD-DEFINES] framing
    c->nd = nd;
    c->W8 = (c->W + 7) / 8 * 8;
    c->needed = (int)(3 * cfg->sample_rate);                                    // _durationToEstimatePowerFloor
    c->rem = c->needed % c->W;
    int rc = MCA_HIP_OK;
    auto setup = [&]() -> int {
        HIP_TRY(c, c->d_state.alloc((size_t)cfg->max_arrays * TGCC_STATE));      // (the state arrays at exactly their state sizes, tgcc_parts)
        HIP_TRY(c, c->d_hook_state.alloc(TGCC_STATE));
        HIP_TRY(c, c->d_hook_in.alloc((size_t)(2 * c->W8 + TGCC_RPAD_FRONT + TGCC_RPAD_BACK)));
        HIP_TRY(c, c->d_hook_res.alloc(TGCC_RES));
        HIP_TRY(c, c->d_hook_out.alloc(5));
        HIP_TRY(c, c->d_hook_index.alloc((size_t)nd));
        return init_state(c, nullptr);
    };
    if ((rc = setup())) return create_failed(c, rc, [](mca_hip_tgcc_ctx *x) { delete x; });
    *out = c;
    return MCA_HIP_OK;
}

void mca_hip_tgcc_destroy(mca_hip_tgcc_ctx *c)
{
    destroy_ctx(c, [](mca_hip_tgcc_ctx *x) { delete x; });      // every device buffer goes with its member
}

int mca_hip_tgcc_get_geometry(const mca_hip_tgcc_ctx *c, int *window, int *hop, int *nd)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (window) *window = c->W;
    if (hop) *hop = c->hop;
    if (nd) *nd = c->nd;
    return MCA_HIP_OK;
}

int mca_hip_tgcc_reset(mca_hip_tgcc_ctx *c, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return init_state(c, (hipStream_t)stream);
}

int mca_hip_tgcc_frames_dev(mca_hip_tgcc_ctx *c, const float *pcm, long long array_stride, long long ch_stride, int n_arrays,
                            int n_frames, float *doa_deg, float *prob, unsigned char *voiced, float *power, int *delay_idx,
                            double *index, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!pcm || !doa_deg) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "pcm_dev / doa_deg_dev is NULL");
    if (n_arrays < 1 || n_arrays > c->cfg.max_arrays) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_arrays outside [1, max_arrays]");
    if (n_frames < 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_frames < 1");
    const long long need = (long long)(n_frames - 1) * c->hop + c->W;
    if (ch_stride < need) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "ch_stride shorter than (n_frames-1)*hop + window samples");
    if (n_arrays > 1 && array_stride < ch_stride + need) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "array_stride too short");
    hipStream_t st = (hipStream_t)stream;
    int rc = ensure_ws(c, (size_t)n_arrays * n_frames);
    if (rc) return rc;

    TgccFrameArgs fa{};
    fa.pcm = pcm; fa.array_stride = array_stride; fa.ch_stride = ch_stride;
    fa.n_frames = n_frames; fa.W = c->W; fa.hop = c->hop; fa.nd = c->nd; fa.rem = c->rem;
    fa.res = c->d_res; fa.index = index;
    const Launch lf = plan_tgcc_frames(c->W8, c->nd, n_arrays, n_frames), lg = plan_tgcc_gate(n_arrays);
    if ((rc = launch_kernel(c, k_tgcc_frames, lf.grid, lf.block, lf.lds, st, fa))) return rc;

    TgccGateArgs ga{};
    ga.res = c->d_res; ga.state = c->d_state;
    ga.n_arrays = n_arrays; ga.n_frames = n_frames; ga.W = c->W; ga.needed = c->needed; ga.use_floor = c->cfg.use_power_floor;
    ga.doa_deg = doa_deg; ga.prob = prob; ga.power = power; ga.voiced = voiced; ga.delay_idx = delay_idx; ga.out_f64 = nullptr;
    if ((rc = launch_kernel(c, k_tgcc_gate, lg.grid, lg.block, lg.lds, st, ga))) return rc;
    HIP_TRY(c, hipGetLastError());
    return MCA_HIP_OK;
}

int mca_hip_tgcc_frames_host(mca_hip_tgcc_ctx *c, const float *pcm, int n_arrays, int n_frames, float *doa_deg, float *prob,
                             unsigned char *voiced, float *power, int *delay_idx, double *index)
{
    if (!c || !pcm || !doa_deg) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_arrays < 1 || n_frames < 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_arrays/n_frames < 1");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const long long cs = (long long)(n_frames - 1) * c->hop + c->W, as = 2 * cs;
    const size_t nf = (size_t)n_arrays * n_frames;
    // (the _dev call gets a buffer for every optional output but the index, whatever the caller takes back)
    StageBuf b[] = {{SG_PCM, pcm, (size_t)as * n_arrays * 4, STAGE_IN}, {SG_DOA, doa_deg, nf * 4, STAGE_OUT}, {SG_PROB, prob, nf * 4, STAGE_OUT | STAGE_ALWAYS},
                    {SG_VOICED, voiced, nf, STAGE_OUT | STAGE_ALWAYS}, {SG_POWER, power, nf * 4, STAGE_OUT | STAGE_ALWAYS}, {SG_DELAY, delay_idx, nf * 4, STAGE_OUT | STAGE_ALWAYS},
                    {SG_INDEX, index, nf * c->nd * 8, STAGE_OUT}};
    return staged(c, b, [&] {
        return mca_hip_tgcc_frames_dev(c, (float *)b[0].dev, as, cs, n_arrays, n_frames, (float *)b[1].dev, (float *)b[2].dev, (unsigned char *)b[3].dev, (float *)b[4].dev,
                                       (int *)b[5].dev, (double *)b[6].dev, nullptr);
    });
}

int mca_hip_tgcc_process_frame(mca_hip_tgcc_ctx *c, const double *const *frames, int length, int *voiced, double *doa_deg,
                               double *prob, double *power, int *delay_idx, double *index)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!frames || !frames[0] || !frames[1]) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "frames is NULL");
    if (length != c->W) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "length must be the module's analysis length (window size)");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int RL = TGCC_RPAD_FRONT + c->W8 + TGCC_RPAD_BACK;
    std::vector<double> buf((size_t)c->W8 + RL, 0.0);
    std::memcpy(buf.data(), frames[0], (size_t)c->W * 8);
    std::memcpy(buf.data() + c->W8 + TGCC_RPAD_FRONT, frames[1], (size_t)c->W * 8);
    HIP_TRY(c, hipMemcpy(c->d_hook_in, buf.data(), buf.size() * 8, hipMemcpyHostToDevice));
    const Launch lh = plan_tgcc_hook(c->nd), lg = plan_tgcc_gate(1);
    int rc = launch_kernel(c, k_tgcc_frame_f64, lh.grid, lh.block, lh.lds, nullptr, c->d_hook_in, c->d_hook_in + c->W8, c->W, c->nd, c->rem, c->d_hook_res, c->d_hook_index);
    if (rc) return rc;
    TgccGateArgs ga{};
    ga.res = c->d_hook_res; ga.state = c->d_hook_state;
    ga.n_arrays = 1; ga.n_frames = 1; ga.W = c->W; ga.needed = c->needed; ga.use_floor = c->cfg.use_power_floor;
    ga.out_f64 = c->d_hook_out;
    if ((rc = launch_kernel(c, k_tgcc_gate, lg.grid, lg.block, lg.lds, nullptr, ga))) return rc;
    HIP_TRY(c, hipGetLastError());
    double o[5];
    HIP_TRY(c, hipMemcpy(o, c->d_hook_out, sizeof(o), hipMemcpyDeviceToHost));
    if (index) HIP_TRY(c, hipMemcpy(index, c->d_hook_index, (size_t)c->nd * 8, hipMemcpyDeviceToHost));
    if (voiced) *voiced = o[0] != 0.0 ? 1 : 0;
    if (doa_deg) *doa_deg = o[1];
    if (prob) *prob = o[2];
    if (power) *power = o[3];
    if (delay_idx) *delay_idx = (int)o[4];
    return MCA_HIP_OK;
}

extern "C++" {
namespace {
constexpr unsigned TGCC_MAGIC = 0x4d435447u;     // "MCTG"
std::vector<BlobPart> tgcc_parts(mca_hip_tgcc_ctx *c)
{
    return {blob_part(c->d_state), blob_part(c->d_hook_state)};
}
unsigned tgcc_cfg_hash(const mca_hip_tgcc_ctx *c)
{
    const int v[6] = {c->W, c->nd, c->needed, c->cfg.max_arrays, c->cfg.sample_rate, c->cfg.use_power_floor};
    return blob_fnv(&c->dist, sizeof(c->dist), blob_fnv(v, sizeof(v)));
}
}  // namespace
}  // extern "C++"

long long mca_hip_tgcc_state_size(const mca_hip_tgcc_ctx *c) { return state_size(c, c ? tgcc_parts(const_cast<mca_hip_tgcc_ctx *>(c)) : std::vector<BlobPart>()); }

int mca_hip_tgcc_state_save(mca_hip_tgcc_ctx *c, void *blob, long long bytes)
{
    return c ? state_save(c, tgcc_parts(c), BlobHeader{TGCC_MAGIC, 1, tgcc_cfg_hash(c), 0, {0, 0, 0, 0}}, blob, bytes) : MCA_HIP_ERR_INVALID_ARGUMENT;
}

int mca_hip_tgcc_state_load(mca_hip_tgcc_ctx *c, const void *blob, long long bytes)
{
    BlobHeader h;
    return c ? state_load(c, tgcc_parts(c), TGCC_MAGIC, 1, tgcc_cfg_hash(c), blob, bytes, &h) : MCA_HIP_ERR_INVALID_ARGUMENT;
}

}  // extern "C"
