// api_multiband.hip -- C ABI of the multiband 2-microphone localiser (include/mcarray_hip.h, mca_hip_mb_*).
// Host side only: builds the tables the reference builds in its constructor
// (MultibandBinarualLocalisation.cpp:52-123), owns the per-array state, enqueues the kernels.  No CPU fallback.
#include "../../include/mcarray_hip.h"
#include "fft512.h"
#include "host_common.h"
#include "kernels.h"
#include "module_plan.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace mca;

struct mca_hip_mb_ctx {
    mca_hip_mb_config cfg{};
    int N = 0, K = 0, H = 0, logH = 0, D = 0, nb = 0;
    float step = 0.f;
    std::vector<double> coef;                 // [nbins][K]
    std::vector<float> grid, delays;          // [D]
    DevBuf<float> d_window, d_coef, d_grid;
    DevBuf<float2> d_tw, d_T;
    DevBuf<int> d_lo, d_hi;
    DevBuf<float> d_corr[2]; int corr_cur = 0;    // the state: each array at exactly its state size (mb_parts)
    DevBuf<double> d_gate; DevBuf<float> d_cur;
    // workspace: each buffer grows on its own need
    DevBuf<float> d_raw, d_be, d_pf, d_ph, d_hprob; DevBuf<int> d_hidx;
    StagePool stage;
    std::string err;
};

namespace {

mca_hip_mb_ctx *const NO_CTX = nullptr;          // a failing create: the text goes to the module's creation error
enum MbStageSlot { SG_PCM, SG_DOA, SG_PROB, SG_POWER, SG_VOICED, SG_BAND_IDX, SG_ENERGY, SG_BAND_CORR };      // the staging-pool slots of the host-pointer call: the numbers stay
void free_mb(mca_hip_mb_ctx *c) { delete c; }      // every device buffer goes with its member

int init_state(mca_hip_mb_ctx *c, hipStream_t st)
{
    const size_t na = (size_t)c->cfg.max_arrays;
    for (int i = 0; i < 2; ++i) HIP_TRY(c, c->d_corr[i].zero_async(st));   // :106-110
    HIP_TRY(c, c->d_gate.zero_async(st));
    std::vector<float> cur(na * 2);
    for (size_t a = 0; a < na; ++a) { cur[2 * a] = 0.f; cur[2 * a + 1] = -1.f; }                            // :81-82
    HIP_TRY(c, hipMemcpyAsync(c->d_cur, cur.data(), cur.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return MCA_HIP_OK;
}

int ensure_ws(mca_hip_mb_ctx *c, size_t rows)
{
    hipError_t e;
    if ((e = c->d_raw.grow(rows * c->nb * c->D)) || (e = c->d_be.grow(rows * c->nb)) || (e = c->d_pf.grow(rows)) || (e = c->d_ph.grow(rows)) ||
        (e = c->d_hprob.grow(rows)) || (e = c->d_hidx.grow(rows))) return hip_fail(c, e, "the workspace of the call");
    return MCA_HIP_OK;
}

}  // namespace

extern "C" {

const char *mca_hip_mb_last_error(const mca_hip_mb_ctx *ctx) { return last_error(ctx); }

int mca_hip_mb_create(const mca_hip_mb_config *cfg, mca_hip_mb_ctx **out)
{
    if (!cfg || !out) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "cfg/out is NULL");
    *out = nullptr;
    if (cfg->struct_size != (int)sizeof(mca_hip_mb_config)) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "struct_size mismatch");
    if (cfg->fft_size < 64 || (cfg->fft_size & (cfg->fft_size - 1)) || cfg->fft_size > 8192) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "fft_size must be a power of two in [64,8192]");
    if (cfg->sample_rate <= 0) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "sample_rate <= 0");
    if (!cfg->mic_xyz) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "mic_xyz is NULL");
    if (cfg->nbins < 1 || cfg->nbins > 27) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "nbins must be in [1,27] (nbins x 37 delays <= 1024 threads)");
    if (cfg->max_arrays < 1) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "max_arrays < 1");
    const double *x = cfg->mic_xyz;
    const double dist = std::sqrt(std::pow(x[3] - x[0], 2) + std::pow(x[4] - x[1], 2) + std::pow(x[5] - x[2], 2));   // distance(0,1) :61
    if (!(dist > 0)) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "the two microphones coincide");
    if (const int rc = check_device(NO_CTX, cfg->device)) return rc;

    mca_hip_mb_ctx *c = new mca_hip_mb_ctx();
    c->cfg = *cfg; c->cfg.mic_xyz = nullptr;
    c->N = cfg->fft_size; c->H = c->N / 2; c->K = c->H + 1; c->nb = cfg->nbins;
    while ((1 << c->logH) < c->H) ++c->logH;
    c->step = (float)(5 * M_PI / 180);                                          // :62
    c->D = (int)(std::floor(M_PI / (double)c->step) + 1);                       // :63
    const int K = c->K, D = c->D, nb = c->nb;
    // [BUILD-DEFINES] LINEAR filter bank of dsp::SubBandSTFTAnalysis(nbins, fs, order, 2, 100, fmax, LINEAR) (:54-60):
    // unit-peak triangles, edges linearly spaced between 100 Hz and maxFreqForSpatialAliasing (float in, float out)
    const double fmin = 100.0;
    const double fmax = (double)(float)(346.1 / (double)(2 * (float)dist));     // microhponeArrayHelpers.cpp:85-89
    c->coef.assign((size_t)nb * K, 0.0);
    std::vector<int> lo(nb), hi(nb);
    std::vector<float> coef_f((size_t)nb * K);
    for (int b = 0; b < nb; ++b) {
        const double f0 = fmin + (fmax - fmin) * (double)b / (double)(nb + 1);
        const double f1 = fmin + (fmax - fmin) * (double)(b + 1) / (double)(nb + 1);
        const double f2 = fmin + (fmax - fmin) * (double)(b + 2) / (double)(nb + 1);
        lo[b] = K; hi[b] = -1;
        for (int k = 0; k < K; ++k) {
            const double f = (double)k * (double)cfg->sample_rate / (double)c->N;
            double h = 0;
            if (f > f0 && f <= f1) h = (f - f0) / (f1 - f0);
            else if (f > f1 && f < f2) h = (f2 - f) / (f2 - f1);
            c->coef[(size_t)b * K + k] = h;
            coef_f[(size_t)b * K + k] = (float)h;
            if (h > 0) { lo[b] = std::min(lo[b], k); hi[b] = std::max(hi[b], k); }
        }
    }
    // delay grid (:101-104) with the class's own float doaIdx2angle (MultibandBinarualLocalisation.h:96-100)
    c->grid.resize(D); c->delays.resize(D);
    for (int i = 0; i < D; ++i) {
        const float ang = (float)((double)((float)i * c->step) - M_PI_2);
        c->grid[i] = ang;
        const float tsec = (float)(((double)(float)dist * std::sin((double)ang)) / 346.1);   // doaToDelayFarField :46-67
        c->delays[i] = tsec * (float)cfg->sample_rate;                                       // :69-72
    }
    std::vector<float2> T((size_t)K * D);
    for (int k = 0; k < K; ++k)
        for (int d = 0; d < D; ++d) {
            const double ph = 2.0 * M_PI * (double)k * (double)c->delays[d] / (double)c->N;
            T[(size_t)k * D + d] = make_float2((float)std::cos(ph), (float)std::sin(ph));
        }
    std::vector<float> win(c->N);
    for (int n = 0; n < c->N; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / c->N));
    std::vector<float2> tw(c->N / 2);
    for (int i = 0; i < c->N / 2; ++i) tw[i] = make_float2((float)std::cos(2.0 * M_PI * i / c->N), (float)(-std::sin(2.0 * M_PI * i / c->N)));

    const size_t na = (size_t)cfg->max_arrays;
    hipError_t e;
    int rc = MCA_HIP_OK;
    if ((e = c->d_window.upload(win.data(), win.size())) || (e = c->d_tw.upload(tw.data(), tw.size())) ||
        (e = c->d_coef.upload(coef_f.data(), coef_f.size())) || (e = c->d_grid.upload(c->grid.data(), D)) ||
        (e = c->d_T.upload(T.data(), T.size())) || (e = c->d_lo.upload(lo.data(), nb)) || (e = c->d_hi.upload(hi.data(), nb)) ||
        (e = c->d_corr[0].alloc_zero(na * nb * D)) || (e = c->d_corr[1].alloc_zero(na * nb * D)) ||
        (e = c->d_gate.alloc_zero(na * 4)) || (e = c->d_cur.alloc_zero(na * 2))) rc = hip_fail(c, e, "device memory for the tables and the state of the context");
    if (rc || (rc = init_state(c, nullptr))) return create_failed(c, rc, free_mb);
    *out = c;
    return MCA_HIP_OK;
}

void mca_hip_mb_destroy(mca_hip_mb_ctx *c) { destroy_ctx(c, free_mb); }

int mca_hip_mb_num_steps(const mca_hip_mb_ctx *c) { return c ? c->D : MCA_HIP_ERR_INVALID_ARGUMENT; }

int mca_hip_mb_get_filters(const mca_hip_mb_ctx *c, double *out)
{
    if (!c || !out) return MCA_HIP_ERR_INVALID_ARGUMENT;
    std::memcpy(out, c->coef.data(), c->coef.size() * sizeof(double));
    return MCA_HIP_OK;
}

int mca_hip_mb_reset(mca_hip_mb_ctx *c, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return init_state(c, (hipStream_t)stream);
}

int mca_hip_mb_frames_dev(mca_hip_mb_ctx *c, const float *pcm, long long array_stride, long long ch_stride, int n_arrays,
                          int n_frames, float *doa_rad, float *prob, unsigned char *voiced, float *power, int *band_idx,
                          float *energy_in_doa, float *band_corr, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!pcm || !doa_rad || !prob) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "pcm_dev / doa_rad_dev / prob_dev is NULL");
    if (n_arrays < 1 || n_arrays > c->cfg.max_arrays) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_arrays outside [1, max_arrays]");
    if (n_frames < 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_frames < 1");
    const long long need = (long long)(n_frames + 1) * c->H;
    if (ch_stride < need) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "ch_stride shorter than (n_frames+1)*hop samples");
    if (n_arrays > 1 && array_stride < ch_stride + need) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "array_stride too short");
    if ((ch_stride & 1) || (array_stride & 1) || (reinterpret_cast<uintptr_t>(pcm) & 7))
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "pcm_dev must be 8-byte aligned with even strides (float2 loads)");
    hipStream_t st = (hipStream_t)stream;
    int rc = ensure_ws(c, (size_t)n_arrays * n_frames);
    if (rc) return rc;

    MbAnalyseArgs aa{};
    aa.pcm = pcm; aa.array_stride = array_stride; aa.ch_stride = ch_stride; aa.n_frames = n_frames;
    aa.N = c->N; aa.logH = c->logH; aa.nbins = c->nb; aa.D = c->D;
    aa.window = c->d_window; aa.tw = c->d_tw; aa.coef = c->d_coef; aa.lo = c->d_lo; aa.hi = c->d_hi; aa.T = c->d_T;
    aa.raw = c->d_raw; aa.band_energy = c->d_be; aa.p_full = c->d_pf; aa.p_half = c->d_ph;
    const MbAnalysePlan pa = plan_mb_analyse(c->N, n_arrays, n_frames);
    if (pa.form == FORM_GEN) rc = launch_kernel(c, k_mb_analyse, pa.l.grid, pa.l.block, pa.l.lds, st, aa);
    else rc = launch_kernel(c, pa.form == FORM_A ? k_mb_analyse_1024 : k_mb_analyse_512, pa.l.grid, pa.l.block, pa.l.lds, st, aa, pa.fpb);
    if (rc) return rc;

    MbScanArgs sa{};
    sa.raw = c->d_raw; sa.band_energy = c->d_be; sa.n_frames = n_frames; sa.nbins = c->nb; sa.D = c->D;
    const MbScanPlan ps = plan_mb_scan(c->nb, c->D, n_arrays, n_frames);
    sa.chunk = ps.chunk;
    const float mem = 0.4f;                                                     // _corrMemoryFactor (MultibandBinarualLocalisation.h:46)
    sa.mem = mem; sa.one_minus_mem = 1 - mem;
    sa.corr_in = c->d_corr[c->corr_cur]; sa.corr_out = c->d_corr[c->corr_cur ^ 1];
    sa.hist_idx = c->d_hidx; sa.hist_prob = c->d_hprob;
    sa.band_idx = band_idx; sa.energy_in_doa = energy_in_doa; sa.band_corr = band_corr;
    if ((rc = launch_kernel(c, k_mb_scan, ps.l.grid, ps.l.block, ps.l.lds, st, sa))) return rc;

    MbSummaryArgs ma{};
    ma.p_full = c->d_pf; ma.p_half = c->d_ph; ma.hist_idx = c->d_hidx; ma.hist_prob = c->d_hprob;
    ma.n_frames = n_frames; ma.K = c->K; ma.needed_samples = (int)(3.0 * c->cfg.sample_rate);   // SoundLocalisationImpl.h:77
    ma.use_floor = c->cfg.use_power_floor; ma.margin_db = 3.0f;                 // _noiseMarginDB (.h:47)
    ma.grid = c->d_grid; ma.gate = c->d_gate; ma.cur = c->d_cur;
    ma.doa_rad = doa_rad; ma.prob = prob; ma.power = power; ma.voiced = voiced;
    const Launch pm = plan_mb_summary(n_arrays);
    if ((rc = launch_kernel(c, k_mb_summary, pm.grid, pm.block, pm.lds, st, ma))) return rc;
    HIP_TRY(c, hipGetLastError());
    c->corr_cur ^= 1;
    return MCA_HIP_OK;
}

extern "C++" {
namespace {
constexpr unsigned MB_MAGIC = 0x4d434d42u;     // "MCMB"
std::vector<BlobPart> mb_parts(mca_hip_mb_ctx *c)
{
    return {blob_part(c->d_corr[c->corr_cur]), blob_part(c->d_gate), blob_part(c->d_cur)};
}
unsigned mb_cfg_hash(const mca_hip_mb_ctx *c)
{
    const int v[6] = {c->N, c->nb, c->D, c->cfg.max_arrays, c->cfg.sample_rate, c->cfg.use_power_floor};
    return blob_fnv(c->delays.data(), c->delays.size() * sizeof(float), blob_fnv(v, sizeof(v)));
}
}  // namespace
}  // extern "C++"

long long mca_hip_mb_state_size(const mca_hip_mb_ctx *c) { return state_size(c, c ? mb_parts(const_cast<mca_hip_mb_ctx *>(c)) : std::vector<BlobPart>()); }

int mca_hip_mb_state_save(mca_hip_mb_ctx *c, void *blob, long long bytes)
{
    return c ? state_save(c, mb_parts(c), BlobHeader{MB_MAGIC, 1, mb_cfg_hash(c), 0, {0, 0, 0, 0}}, blob, bytes) : MCA_HIP_ERR_INVALID_ARGUMENT;
}

int mca_hip_mb_state_load(mca_hip_mb_ctx *c, const void *blob, long long bytes)
{
    BlobHeader h;
    return c ? state_load(c, mb_parts(c), MB_MAGIC, 1, mb_cfg_hash(c), blob, bytes, &h) : MCA_HIP_ERR_INVALID_ARGUMENT;
}

int mca_hip_mb_frames_host(mca_hip_mb_ctx *c, const float *pcm, int n_arrays, int n_frames, float *doa_rad, float *prob,
                           unsigned char *voiced, float *power, int *band_idx, float *energy_in_doa, float *band_corr)
{
    if (!c || !pcm || !doa_rad || !prob) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_arrays < 1 || n_frames < 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_arrays/n_frames < 1");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const long long cs = (long long)(n_frames + 1) * c->H, as = 2 * cs;
    const size_t nf = (size_t)n_arrays * n_frames;
    // (the _dev call gets a buffer for voiced and power whatever the caller takes back)
    StageBuf b[] = {{SG_PCM, pcm, (size_t)as * n_arrays * 4, STAGE_IN}, {SG_DOA, doa_rad, nf * 4, STAGE_OUT}, {SG_PROB, prob, nf * 4, STAGE_OUT},
                    {SG_VOICED, voiced, nf, STAGE_OUT | STAGE_ALWAYS}, {SG_POWER, power, nf * 4, STAGE_OUT | STAGE_ALWAYS}, {SG_BAND_IDX, band_idx, nf * c->nb * 4, STAGE_OUT},
                    {SG_ENERGY, energy_in_doa, nf * c->D * 4, STAGE_OUT}, {SG_BAND_CORR, band_corr, nf * c->nb * c->D * 4, STAGE_OUT}};
    return staged(c, b, [&] {
        return mca_hip_mb_frames_dev(c, (float *)b[0].dev, as, cs, n_arrays, n_frames, (float *)b[1].dev, (float *)b[2].dev, (unsigned char *)b[3].dev, (float *)b[4].dev,
                                     (int *)b[5].dev, (float *)b[6].dev, (float *)b[7].dev, nullptr);
    });
}

}  // extern "C"
