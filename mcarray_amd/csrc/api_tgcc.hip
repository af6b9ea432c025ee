// api_tgcc.hip -- C ABI of the time-domain 2-microphone localiser (include/mcarray_hip.h, mca_hip_tgcc_*).
// Host side only: the geometry the reference's constructor computes (BinauralLocalisation.cpp:66-101), the per-array
// state, the frame hook's own state, and the launches of kernels_tgcc.hip.  No CPU fallback.
#include "../../include/mcarray_hip.h"
#include "kernels.h"
#include "stage.h"
#include "state_blob.h"

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
    size_t smem = 0, smem_hook = 0;
    DevBuf<double> d_state;                        // [max_arrays][TGCC_STATE]
    DevBuf<double> d_hook_state;                   // [TGCC_STATE] the frame hook's module
    DevBuf<double> d_hook_in;                      // padded channels of one double frame
    DevBuf<double> d_hook_res, d_hook_out, d_hook_index;
    DevBuf<double> d_res;                          // workspace: [rows][TGCC_RES]
    StagePool stage;
    std::string err;
};

namespace {

std::string g_tgcc_create_error;

int tfail(mca_hip_tgcc_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg; else g_tgcc_create_error = msg;
    return code;
}

#define THIP_TRY(ctx, expr)                                                                             \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return tfail(ctx, _e == hipErrorOutOfMemory ? MCA_HIP_ERR_OUT_OF_MEMORY : MCA_HIP_ERR_HIP,  \
                         std::string(#expr) + ": " + hipGetErrorString(_e));                           \
    } while (0)

// _currentDOA = 0, _prob = -1 (:88-89), _powerFloor = 0, nothing consumed, not estimated
int init_state(mca_hip_tgcc_ctx *c, hipStream_t st)
{
    const size_t na = (size_t)c->cfg.max_arrays;
    std::vector<double> s((na + 1) * TGCC_STATE, 0.0);
    for (size_t a = 0; a <= na; ++a) s[a * TGCC_STATE + 1] = -1.0;
    THIP_TRY(c, hipMemcpyAsync(c->d_state, s.data(), c->d_state.bytes(), hipMemcpyHostToDevice, st));
    THIP_TRY(c, hipMemcpyAsync(c->d_hook_state, s.data() + na * TGCC_STATE, c->d_hook_state.bytes(), hipMemcpyHostToDevice, st));
    THIP_TRY(c, hipStreamSynchronize(st));
    return MCA_HIP_OK;
}

int ensure_ws(mca_hip_tgcc_ctx *c, size_t rows)
{
    THIP_TRY(c, c->d_res.grow(rows * TGCC_RES));
    return MCA_HIP_OK;
}

}  // namespace

extern "C" {

const char *mca_hip_tgcc_last_error(const mca_hip_tgcc_ctx *ctx) { return ctx ? ctx->err.c_str() : g_tgcc_create_error.c_str(); }

int mca_hip_tgcc_create(const mca_hip_tgcc_config *cfg, mca_hip_tgcc_ctx **out)
{
    if (!cfg || !out) return tfail(nullptr, MCA_HIP_ERR_INVALID_ARGUMENT, "cfg/out is NULL");
    *out = nullptr;
    if (cfg->struct_size != (int)sizeof(mca_hip_tgcc_config)) return tfail(nullptr, MCA_HIP_ERR_INVALID_ARGUMENT, "struct_size mismatch");
    if (cfg->sample_rate <= 0 || cfg->sample_rate > 96000) return tfail(nullptr, MCA_HIP_ERR_INVALID_ARGUMENT, "sample_rate must be in [1, 96000]");
    if (cfg->max_arrays < 1 || cfg->max_arrays > 65535) return tfail(nullptr, MCA_HIP_ERR_INVALID_ARGUMENT, "max_arrays must be in [1, 65535]");
    const double *x = &cfg->mic_xyz[0][0];
    const double dist = std::sqrt(std::pow(x[3] - x[0], 2) + std::pow(x[4] - x[1], 2) + std::pow(x[5] - x[2], 2));   // distance(0,1)
    if (!(dist > 0)) return tfail(nullptr, MCA_HIP_ERR_INVALID_ARGUMENT, "the two microphones coincide");
    const double c_sound = 346.1;                                               // getSpeedOfSound()
    const int nd = (int)(dist * cfg->sample_rate / c_sound);                    // _ndelays (:71)
    if (nd < 2) {                                                               // :76-80 (samples2Degrees divides by nd - 1)
        std::ostringstream oss;
        oss << "Sample frequency has to be a least " << c_sound * 2 / dist;
        return tfail(nullptr, MCA_HIP_ERR_INVALID_ARGUMENT, oss.str());
    }
    if (nd > TGCC_MAX_ND) {
        std::ostringstream oss;
        oss << "distance(0,1) * sample_rate / 346.1 = " << nd << " delay pairs; the kernels support at most " << TGCC_MAX_ND;
        return tfail(nullptr, MCA_HIP_ERR_INVALID_ARGUMENT, oss.str());
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return tfail(nullptr, MCA_HIP_ERR_NO_DEVICE, "no HIP device visible; libmcarray_hip has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return tfail(nullptr, MCA_HIP_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    if (hipSetDevice(cfg->device) != hipSuccess) return tfail(nullptr, MCA_HIP_ERR_HIP, "hipSetDevice failed");

    mca_hip_tgcc_ctx *c = new mca_hip_tgcc_ctx();
    c->cfg = *cfg;
    c->dist = dist;
    c->W = (int)(2 * (0.075 * cfg->sample_rate));                               // window = analysis length (:68, .h:52)
    c->hop = c->W / 2;                                                          // [BUILD-DEFINES] framing
    c->nd = nd;
    c->W8 = (c->W + 7) / 8 * 8;
    c->needed = (int)(3 * cfg->sample_rate);                                    // _durationToEstimatePowerFloor
    c->rem = c->needed % c->W;
    c->smem_hook = (size_t)tgcc_frame_ws_doubles(nd) * 8;
    c->smem = c->smem_hook + (size_t)4 * (2 * c->W8 + TGCC_RPAD_FRONT + TGCC_RPAD_BACK);
    int rc = MCA_HIP_OK;
    auto setup = [&]() -> int {
        THIP_TRY(c, c->d_state.alloc((size_t)cfg->max_arrays * TGCC_STATE));      // (the state arrays at exactly their state sizes, tgcc_parts)
        THIP_TRY(c, c->d_hook_state.alloc(TGCC_STATE));
        THIP_TRY(c, c->d_hook_in.alloc((size_t)(2 * c->W8 + TGCC_RPAD_FRONT + TGCC_RPAD_BACK)));
        THIP_TRY(c, c->d_hook_res.alloc(TGCC_RES));
        THIP_TRY(c, c->d_hook_out.alloc(5));
        THIP_TRY(c, c->d_hook_index.alloc((size_t)nd));
        return init_state(c, nullptr);
    };
    if ((rc = setup())) { g_tgcc_create_error = c->err; delete c; return rc; }
    *out = c;
    return MCA_HIP_OK;
}

void mca_hip_tgcc_destroy(mca_hip_tgcc_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    (void)hipDeviceSynchronize();
    delete c;                                 // every device buffer goes with its member
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
    THIP_TRY(c, hipSetDevice(c->cfg.device));
    return init_state(c, (hipStream_t)stream);
}

int mca_hip_tgcc_frames_dev(mca_hip_tgcc_ctx *c, const float *pcm, long long array_stride, long long ch_stride, int n_arrays,
                            int n_frames, float *doa_deg, float *prob, unsigned char *voiced, float *power, int *delay_idx,
                            double *index, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!pcm || !doa_deg) return tfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "pcm_dev / doa_deg_dev is NULL");
    if (n_arrays < 1 || n_arrays > c->cfg.max_arrays) return tfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_arrays outside [1, max_arrays]");
    if (n_frames < 1) return tfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_frames < 1");
    const long long need = (long long)(n_frames - 1) * c->hop + c->W;
    if (ch_stride < need) return tfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "ch_stride shorter than (n_frames-1)*hop + window samples");
    if (n_arrays > 1 && array_stride < ch_stride + need) return tfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "array_stride too short");
    hipStream_t st = (hipStream_t)stream;
    int rc = ensure_ws(c, (size_t)n_arrays * n_frames);
    if (rc) return rc;

    TgccFrameArgs fa{};
    fa.pcm = pcm; fa.array_stride = array_stride; fa.ch_stride = ch_stride;
    fa.n_frames = n_frames; fa.W = c->W; fa.hop = c->hop; fa.nd = c->nd; fa.rem = c->rem;
    fa.res = c->d_res; fa.index = index;
    // the kernel's LDS limit is per function: set on every call (another context may have set it for a shorter window)
    THIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_tgcc_frames), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->smem));
    hipLaunchKernelGGL(k_tgcc_frames, dim3(n_frames, n_arrays), dim3(256), c->smem, st, fa);

    TgccGateArgs ga{};
    ga.res = c->d_res; ga.state = c->d_state;
    ga.n_arrays = n_arrays; ga.n_frames = n_frames; ga.W = c->W; ga.needed = c->needed; ga.use_floor = c->cfg.use_power_floor;
    ga.doa_deg = doa_deg; ga.prob = prob; ga.power = power; ga.voiced = voiced; ga.delay_idx = delay_idx; ga.out_f64 = nullptr;
    hipLaunchKernelGGL(k_tgcc_gate, dim3((n_arrays + 63) / 64), dim3(64), 0, st, ga);
    THIP_TRY(c, hipGetLastError());
    return MCA_HIP_OK;
}

int mca_hip_tgcc_frames_host(mca_hip_tgcc_ctx *c, const float *pcm, int n_arrays, int n_frames, float *doa_deg, float *prob,
                             unsigned char *voiced, float *power, int *delay_idx, double *index)
{
    if (!c || !pcm || !doa_deg) return tfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_arrays < 1 || n_frames < 1) return tfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_arrays/n_frames < 1");
    THIP_TRY(c, hipSetDevice(c->cfg.device));
    const long long cs = (long long)(n_frames - 1) * c->hop + c->W, as = 2 * cs;
    const size_t nf = (size_t)n_arrays * n_frames;
    const size_t n_ix = index ? nf * c->nd : 0;
    float *d_pcm = (float *)c->stage.get(0, (size_t)as * n_arrays * 4), *d_doa = (float *)c->stage.get(1, nf * 4);
    float *d_prob = (float *)c->stage.get(2, nf * 4), *d_pow = (float *)c->stage.get(3, nf * 4);
    unsigned char *d_v = (unsigned char *)c->stage.get(4, nf);
    int *d_k = (int *)c->stage.get(5, nf * 4);
    double *d_ix = (double *)c->stage.get(6, n_ix * 8);
    if (!d_pcm || !d_doa || !d_prob || !d_pow || !d_v || !d_k || (index && !d_ix))
        return tfail(c, MCA_HIP_ERR_OUT_OF_MEMORY, "device staging buffers for the host-pointer call");
    THIP_TRY(c, hipMemcpy(d_pcm, pcm, (size_t)as * n_arrays * 4, hipMemcpyHostToDevice));
    const int rc = mca_hip_tgcc_frames_dev(c, d_pcm, as, cs, n_arrays, n_frames, d_doa, d_prob, d_v, d_pow, d_k, index ? d_ix : nullptr, nullptr);
    if (rc) return rc;
    THIP_TRY(c, hipDeviceSynchronize());
    THIP_TRY(c, hipMemcpy(doa_deg, d_doa, nf * 4, hipMemcpyDeviceToHost));
    if (prob) THIP_TRY(c, hipMemcpy(prob, d_prob, nf * 4, hipMemcpyDeviceToHost));
    if (voiced) THIP_TRY(c, hipMemcpy(voiced, d_v, nf, hipMemcpyDeviceToHost));
    if (power) THIP_TRY(c, hipMemcpy(power, d_pow, nf * 4, hipMemcpyDeviceToHost));
    if (delay_idx) THIP_TRY(c, hipMemcpy(delay_idx, d_k, nf * 4, hipMemcpyDeviceToHost));
    if (index) THIP_TRY(c, hipMemcpy(index, d_ix, n_ix * 8, hipMemcpyDeviceToHost));
    return MCA_HIP_OK;
}

int mca_hip_tgcc_process_frame(mca_hip_tgcc_ctx *c, const double *const *frames, int length, int *voiced, double *doa_deg,
                               double *prob, double *power, int *delay_idx, double *index)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!frames || !frames[0] || !frames[1]) return tfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "frames is NULL");
    if (length != c->W) return tfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "length must be the module's analysis length (window size)");
    THIP_TRY(c, hipSetDevice(c->cfg.device));
    const int RL = TGCC_RPAD_FRONT + c->W8 + TGCC_RPAD_BACK;
    std::vector<double> buf((size_t)c->W8 + RL, 0.0);
    std::memcpy(buf.data(), frames[0], (size_t)c->W * 8);
    std::memcpy(buf.data() + c->W8 + TGCC_RPAD_FRONT, frames[1], (size_t)c->W * 8);
    THIP_TRY(c, hipMemcpy(c->d_hook_in, buf.data(), buf.size() * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_tgcc_frame_f64, dim3(1), dim3(256), c->smem_hook, nullptr, c->d_hook_in, c->d_hook_in + c->W8, c->W, c->nd,
                       c->rem, c->d_hook_res, c->d_hook_index);
    TgccGateArgs ga{};
    ga.res = c->d_hook_res; ga.state = c->d_hook_state;
    ga.n_arrays = 1; ga.n_frames = 1; ga.W = c->W; ga.needed = c->needed; ga.use_floor = c->cfg.use_power_floor;
    ga.out_f64 = c->d_hook_out;
    hipLaunchKernelGGL(k_tgcc_gate, dim3(1), dim3(64), 0, nullptr, ga);
    THIP_TRY(c, hipGetLastError());
    double o[5];
    THIP_TRY(c, hipMemcpy(o, c->d_hook_out, sizeof(o), hipMemcpyDeviceToHost));
    if (index) THIP_TRY(c, hipMemcpy(index, c->d_hook_index, (size_t)c->nd * 8, hipMemcpyDeviceToHost));
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

long long mca_hip_tgcc_state_size(const mca_hip_tgcc_ctx *c)
{
    return c ? blob_size(tgcc_parts(const_cast<mca_hip_tgcc_ctx *>(c))) : (long long)MCA_HIP_ERR_INVALID_ARGUMENT;
}

int mca_hip_tgcc_state_save(mca_hip_tgcc_ctx *c, void *blob, long long bytes)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    THIP_TRY(c, hipSetDevice(c->cfg.device));
    BlobHeader h{TGCC_MAGIC, 1, tgcc_cfg_hash(c), 0, {0, 0, 0, 0}};
    const int rc = blob_save(tgcc_parts(c), h, blob, bytes);
    return rc ? tfail(c, rc == 2 ? MCA_HIP_ERR_HIP : MCA_HIP_ERR_INVALID_ARGUMENT, blob_error(rc)) : MCA_HIP_OK;
}

int mca_hip_tgcc_state_load(mca_hip_tgcc_ctx *c, const void *blob, long long bytes)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    THIP_TRY(c, hipSetDevice(c->cfg.device));
    BlobHeader h;
    const int rc = blob_load(tgcc_parts(c), TGCC_MAGIC, tgcc_cfg_hash(c), blob, bytes, &h);
    return rc ? tfail(c, rc == 2 ? MCA_HIP_ERR_HIP : MCA_HIP_ERR_INVALID_ARGUMENT, blob_error(rc)) : MCA_HIP_OK;
}

}  // extern "C"
