// api_bmask.hip -- C ABI of the filter-bank binaural masking module (include/mcarray_hip.h, mca_hip_bmask_*).
// Host side only: builds the filter bank, the thresholds and the per-bin tables, owns the per-stream state and the
// workspace between the three launches, enqueues the kernels.  No CPU fallback.
#include "../../include/mcarray_hip.h"
#include "bmask.h"
#include "fft512.h"
#include "host_common.h"
#include "module_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

using namespace mca;

struct mca_hip_bmask_ctx {
    mca_hip_bmask_config cfg{};
    int N = 0, K = 0, hop = 0, logH = 0;
    std::vector<double> H, center, thr;        // [45][K], [45], [45]
    std::vector<int> lo, hi;
    BmaskTables tab{};
    DevBuf<float> d_window, d_thr;
    DevBuf<float2> d_tw, d_kw, d_kp;
    DevBuf<int> d_kb, d_lo, d_hi;
    DevBuf<double> d_Q;                        // the state: each array at exactly its state size (bmask_parts)
    DevBuf<float> d_tail[2];
    DevBuf<long long> d_frames;
    int tail_cur = 0;
    // frame hooks (double)
    DevBuf<double> d_thr64, d_Q64, d_h, d_x, d_ana;   // d_h [45][N] impulse responses (built at the first frameAnalysis), d_ana [2][46 N]
    DevBuf<int> d_dec;
    StagePool stage;                           // (BmaskStageSlot)
    std::string err;
};

namespace {

// the module's constants (BinauralMaskingImpl.h:142-155)
constexpr float kForgetting = 0.04f, kScaling = 0.01f, kTemporalFactor = 1.f, kSpatialFactor = 1.f, kEnhanceFactor = 1.f;
constexpr double kPhi = 10 * M_PI / 180, kThresholdScale = 0.9, kSpeedOfSound = 346.1;

mca_hip_bmask_ctx *const NO_CTX = nullptr;       // a failing create: the text goes to the module's creation error
enum BmaskStageSlot { SG_PCM, SG_OUT, SG_DECISIONS, SG_SUMS, SG_GAINS };      // the staging pool: the host-pointer call's buffers, the band sums and gains of a call; the numbers stay
void free_bmask(mca_hip_bmask_ctx *c) { delete c; }      // every device buffer goes with its member

double hz2mel(double f) { return 2595.0 * std::log10(1.0 + f / 700.0); }
double mel2hz(double m) { return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0); }

// [BUILD-DEFINES] stand-in for dsp::FilterBankFFTWMelScale(order, 45, fs, fmin, fmax) (BinauralMaskingImpl.cpp:80-81), the
// filters of the FastBinauralMasking context: 45 unit-peak triangles with HTK-mel spaced edges on the K bin frequencies
void mel_filterbank(int N, int nb, int fs, double fmin, double fmax, std::vector<double> &H, std::vector<double> &center)
{
    const int K = N / 2 + 1;
    std::vector<double> edge(nb + 2);
    const double mlo = hz2mel(fmin), mhi = hz2mel(fmax);
    for (int i = 0; i < nb + 2; ++i) edge[i] = mel2hz(mlo + (mhi - mlo) * (double)i / (double)(nb + 1));
    H.assign((size_t)nb * K, 0.0);
    center.resize(nb);
    for (int b = 0; b < nb; ++b) {
        const double f0 = edge[b], f1 = edge[b + 1], f2 = edge[b + 2];
        center[b] = f1 / (double)fs;
        for (int k = 0; k < K; ++k) {
            const double f = (double)k * (double)fs / (double)N;
            double h = 0;
            if (f > f0 && f <= f1) h = (f - f0) / (f1 - f0);
            else if (f > f1 && f < f2) h = (f2 - f) / (f2 - f1);
            H[(size_t)b * K + k] = h;
        }
    }
}

// h_b = irfft(H_b), [45][N] in double, uploaded once: h_b[n] = (1 / N) sum_k c_k H_b[k] cos(2 pi k n / N) over the band's support
int build_impulse_responses(mca_hip_bmask_ctx *c)
{
    if (c->d_h) return MCA_HIP_OK;
    const int N = c->N, K = c->K;
    std::vector<double> cs(N), h((size_t)BM_BANDS * N, 0.0);
    for (int i = 0; i < N; ++i) cs[i] = std::cos(2.0 * M_PI * (double)i / (double)N);
    for (int b = 0; b < BM_BANDS; ++b)
        for (int n = 0; n < N; ++n) {
            double acc = 0;
            for (int k = c->lo[b]; k <= c->hi[b]; ++k) {
                const double ck = (k == 0 || k == K - 1) ? 1.0 : 2.0;
                acc += ck * c->H[(size_t)b * K + k] * cs[(int)(((long long)k * n) & (N - 1))];
            }
            h[(size_t)b * N + n] = acc / (double)N;
        }
    HIP_TRY(c, c->d_h.upload(h.data(), h.size()));
    return MCA_HIP_OK;
}

// the kernels of a frame length, by the plan's form (module_plan.h): 1024, 2048, any other power of two
typedef void (*BmaskKernel)(BmaskStreamArgs);
const BmaskKernel kAnalyse[3] = {k_bmask_analyse_1024, k_bmask_analyse_2048, k_bmask_analyse_gen}, kSynth[3] = {k_bmask_synth_1024, k_bmask_synth_2048, k_bmask_synth_gen};

int fits(const mca_hip_bmask_ctx *c, int analysis_length) { return analysis_length < 0 ? 0 : std::min(BM_BANDS, analysis_length / c->N); }

}  // namespace

extern "C" {

const char *mca_hip_bmask_last_error(const mca_hip_bmask_ctx *ctx) { return last_error(ctx); }

int mca_hip_bmask_create(const mca_hip_bmask_config *cfg, mca_hip_bmask_ctx **out)
{
    if (!cfg || !out) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "cfg/out is NULL");
    *out = nullptr;
    if (cfg->struct_size != (int)sizeof(mca_hip_bmask_config)) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "struct_size mismatch");
    if (cfg->frame_size < 256 || (cfg->frame_size & (cfg->frame_size - 1)) || cfg->frame_size > 8192) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "frame_size must be a power of two in [256,8192]");
    if (cfg->sample_rate <= 0 || !(cfg->micro_distance > 0)) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "sample_rate / micro_distance must be positive");
    if (!(cfg->low_freq >= 0) || !(cfg->high_freq > cfg->low_freq) || cfg->high_freq > 0.5f * cfg->sample_rate) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "need 0 <= low_freq < high_freq <= fs/2");
    const int m = cfg->method;
    if (!(m == 0 || m == 1 || m == 3)) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "bad masking method (FACTOR 0, RELATIVE 1, FULL 3)");
    if (cfg->max_streams < 1) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "max_streams < 1");
    if (const int rc = check_device(NO_CTX, cfg->device)) return rc;

    mca_hip_bmask_ctx *c = new mca_hip_bmask_ctx();
    c->cfg = *cfg; c->N = cfg->frame_size; c->K = c->N / 2 + 1; c->hop = c->N / 2;
    while ((1 << c->logH) < c->hop) ++c->logH;
    const int N = c->N, K = c->K;
    mel_filterbank(N, BM_BANDS, cfg->sample_rate, (double)cfg->low_freq, (double)cfg->high_freq, c->H, c->center);
    c->thr.resize(BM_BANDS);
    for (int b = 0; b < BM_BANDS; ++b) {                                          // calculateThresholds :237-261
        const double wfreq = c->center[b] * cfg->sample_rate * 2 * M_PI;
        c->thr[b] = std::cos(wfreq * cfg->micro_distance * std::sin(kPhi) / kSpeedOfSound) * kThresholdScale;
    }
    // every bin is covered by at most two adjacent triangles
    bool compact_ok = true;
    std::vector<int> kb(K, -1);
    std::vector<float2> kw(K, make_float2(0.f, 0.f)), kp(K, make_float2(0.f, 0.f));
    std::vector<float> thr32(BM_BANDS);
    c->lo.assign(BM_BANDS, 1); c->hi.assign(BM_BANDS, 0);
    for (int b = 0; b < BM_BANDS; ++b) thr32[b] = (float)c->thr[b];
    const double inv_n2 = 1.0 / ((double)N * (double)N);
    for (int k = 0; k < K; ++k) {
        const double ck = (k == 0 || k == K - 1) ? 1.0 : 2.0;
        int nfound = 0;
        for (int b = 0; b < BM_BANDS; ++b) {
            const double h = c->H[(size_t)b * K + k];
            if (h > 0) {
                if (nfound == 0) { kb[k] = b; kw[k].x = (float)h; kp[k].x = (float)(ck * h * h * inv_n2); }
                else if (nfound == 1 && b == kb[k] + 1) { kw[k].y = (float)h; kp[k].y = (float)(ck * h * h * inv_n2); }
                else compact_ok = false;
                ++nfound;
                if (c->lo[b] > c->hi[b]) c->lo[b] = k;
                c->hi[b] = k;
            }
        }
    }
    if (!compact_ok) { delete c; return fail(NO_CTX, MCA_HIP_ERR_UNSUPPORTED, "a bin is covered by more than two adjacent bands"); }
    const size_t ns = (size_t)cfg->max_streams;
    std::vector<float> win(N);
    for (int n = 0; n < N; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / N));
    std::vector<float2> tw(N / 2);
    for (int i = 0; i < N / 2; ++i) tw[i] = make_float2((float)std::cos(2.0 * M_PI * i / N), (float)(-std::sin(2.0 * M_PI * i / N)));
    auto body = [&]() -> int {
        HIP_TRY(c, c->d_window.upload(win.data(), win.size()));
        HIP_TRY(c, c->d_tw.upload(tw.data(), tw.size()));
        HIP_TRY(c, c->d_kw.upload(kw.data(), kw.size())); HIP_TRY(c, c->d_kp.upload(kp.data(), kp.size())); HIP_TRY(c, c->d_kb.upload(kb.data(), kb.size()));
        HIP_TRY(c, c->d_lo.upload(c->lo.data(), BM_BANDS)); HIP_TRY(c, c->d_hi.upload(c->hi.data(), BM_BANDS));
        HIP_TRY(c, c->d_thr.upload(thr32.data(), BM_BANDS));
        HIP_TRY(c, c->d_Q.alloc_zero(ns * BM_BANDS));
        for (int i = 0; i < 2; ++i) HIP_TRY(c, c->d_tail[i].alloc_zero(ns * 2 * c->hop));
        HIP_TRY(c, c->d_frames.alloc_zero(ns));
        HIP_TRY(c, c->d_thr64.upload(c->thr.data(), BM_BANDS));
        HIP_TRY(c, c->d_Q64.alloc_zero(BM_BANDS));
        HIP_TRY(c, c->d_x.alloc_zero((size_t)N));
        HIP_TRY(c, c->d_ana.alloc_zero((size_t)2 * (BM_BANDS + 1) * N));
        HIP_TRY(c, c->d_dec.alloc_zero(BM_BANDS));
        return MCA_HIP_OK;
    };
    const int rc = body();
    if (rc) return create_failed(c, rc, free_bmask);
    BmaskTables &t = c->tab;
    t.window = c->d_window; t.tw = c->d_tw; t.kb = c->d_kb; t.kw = c->d_kw; t.kp = c->d_kp; t.lo = c->d_lo; t.hi = c->d_hi;
    t.N = N; t.logH = c->logH;
    *out = c;
    return MCA_HIP_OK;
}

void mca_hip_bmask_destroy(mca_hip_bmask_ctx *c) { destroy_ctx(c, free_bmask); }

int mca_hip_bmask_reset(mca_hip_bmask_ctx *c)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemset(c->d_Q, 0, c->d_Q.bytes()));
    for (int i = 0; i < 2; ++i) HIP_TRY(c, hipMemset(c->d_tail[i], 0, c->d_tail[i].bytes()));
    HIP_TRY(c, hipMemset(c->d_frames, 0, c->d_frames.bytes()));
    HIP_TRY(c, hipMemset(c->d_Q64, 0, c->d_Q64.bytes()));
    return MCA_HIP_OK;
}

int mca_hip_bmask_get_thresholds(const mca_hip_bmask_ctx *c, double *thresholds, double *center_freqs)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (thresholds) std::memcpy(thresholds, c->thr.data(), BM_BANDS * 8);
    if (center_freqs) std::memcpy(center_freqs, c->center.data(), BM_BANDS * 8);
    return MCA_HIP_OK;
}

int mca_hip_bmask_frames_dev(mca_hip_bmask_ctx *c, const float *pcm, long long stream_stride, long long ch_stride,
                             int n_streams, int n_frames, float *out_pcm, int *decisions, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!pcm || !out_pcm) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "pcm_dev/out_pcm_dev is NULL");
    if (n_streams < 1 || n_streams > c->cfg.max_streams) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_streams outside [1, max_streams]");
    if (n_frames < 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_frames < 1");
    const long long need = (long long)(n_frames + 1) * c->hop;
    if (ch_stride < need || (n_streams > 1 && stream_stride < ch_stride + need)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "strides shorter than (n_frames+1)*hop samples");
    if ((ch_stride & 1) || (stream_stride & 1) || (reinterpret_cast<uintptr_t>(pcm) & 7)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "pcm_dev must be 8-byte aligned with even strides");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    // the band sums and gains of the call, [streams][n_frames][45]; grow-only
    const size_t cells = (size_t)n_streams * n_frames * BM_BANDS;
    float4 *d_sums = (float4 *)c->stage.get(SG_SUMS, cells * sizeof(float4));
    float2 *d_gains = (float2 *)c->stage.get(SG_GAINS, cells * sizeof(float2));
    if (!d_sums || !d_gains) return fail(c, MCA_HIP_ERR_OUT_OF_MEMORY, "workspace for the band sums and gains");

    BmaskStreamArgs a{};
    a.t = c->tab; a.pcm = pcm; a.stream_stride = stream_stride; a.ch_stride = ch_stride; a.n_frames = n_frames;
    a.sums = d_sums; a.gains = d_gains;
    a.tail_in = c->d_tail[c->tail_cur]; a.tail_out = c->d_tail[c->tail_cur ^ 1]; a.out = out_pcm;
    const BmaskPlan p = plan_bmask(c->N, n_streams, n_frames);
    a.ft = p.ft;

    BmaskScanArgs sa{};
    sa.sums = d_sums; sa.n_frames = n_frames; sa.method = c->cfg.method; sa.thr = c->d_thr;
    sa.lambda = (double)kForgetting; sa.one_minus_lambda = (double)(1 - kForgetting); sa.rho = kScaling;
    sa.inv_spatial = 1.f / kSpatialFactor; sa.inv_temporal = 1.f / kTemporalFactor; sa.enhance = kEnhanceFactor;
    sa.Q = c->d_Q; sa.frames = c->d_frames; sa.gains = d_gains; sa.decisions = decisions;
    int rc;
    if ((rc = launch_kernel(c, kAnalyse[p.form], p.analyse.grid, p.analyse.block, p.analyse.lds, st, a))) return rc;
    if ((rc = launch_kernel(c, k_bmask_scan, p.scan.grid, p.scan.block, p.scan.lds, st, sa))) return rc;
    if ((rc = launch_kernel(c, kSynth[p.form], p.synth.grid, p.synth.block, p.synth.lds, st, a))) return rc;
    HIP_TRY(c, hipGetLastError());
    c->tail_cur ^= 1;
    if (n_streams < c->cfg.max_streams) {
        // the streams beyond n_streams did not run: their carries move to the new buffer unchanged
        const size_t off = (size_t)n_streams * 2 * c->hop, cnt = ((size_t)c->cfg.max_streams - n_streams) * 2 * c->hop;
        HIP_TRY(c, hipMemcpyAsync(c->d_tail[c->tail_cur] + off, c->d_tail[c->tail_cur ^ 1] + off, cnt * 4, hipMemcpyDeviceToDevice, st));
    }
    return MCA_HIP_OK;
}

int mca_hip_bmask_frames_host(mca_hip_bmask_ctx *c, const float *pcm, int n_streams, int n_frames, float *out_pcm, int *decisions)
{
    if (!c || !pcm || !out_pcm) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_streams < 1 || n_frames < 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_streams/n_frames < 1");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const long long cs = (long long)(n_frames + 1) * c->hop, ss = 2 * cs;
    const size_t n_out = (size_t)n_streams * 2 * n_frames * c->hop, n_dec = (size_t)n_streams * n_frames * BM_BANDS;
    StageBuf b[] = {{SG_PCM, pcm, (size_t)ss * n_streams * 4, STAGE_IN}, {SG_OUT, out_pcm, n_out * 4, STAGE_OUT}, {SG_DECISIONS, decisions, n_dec * 4, STAGE_OUT}};
    return staged(c, b, [&] { return mca_hip_bmask_frames_dev(c, (float *)b[0].dev, ss, cs, n_streams, n_frames, (float *)b[1].dev, (int *)b[2].dev, nullptr); });
}

int mca_hip_bmask_frame_analysis(mca_hip_bmask_ctx *c, const double *in_frame, double *analysis, int frame_length, int analysis_length, int channel)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!in_frame || !analysis) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "in_frame/analysis is NULL");
    if (frame_length != c->N) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "frame_length != frame_size");
    if (channel < 0 || channel > 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "Sound localisation is only working for 2 channels by now.");
    const int nb = fits(c, analysis_length);
    if (nb == 0) return MCA_HIP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int rc = build_impulse_responses(c);
    if (rc) return rc;
    const int N = c->N;
    const bool residual = (long long)analysis_length >= (long long)(BM_BANDS + 1) * N;
    HIP_TRY(c, hipMemcpy(c->d_x, in_frame, (size_t)N * 8, hipMemcpyHostToDevice));
    int lrc = launch_kernel(c, k_bmask_hook_analysis, dim3(grid_for(N, 256).x, nb), dim3(256), 0, nullptr, c->d_x, c->d_h, c->d_ana, N, nb);
    if (!lrc && residual) lrc = launch_kernel(c, k_bmask_hook_residual, grid_for(N, 256), dim3(256), 0, nullptr, c->d_x, c->d_ana, N);
    if (lrc) return lrc;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpy(analysis, c->d_ana, (size_t)(nb + (residual ? 1 : 0)) * N * 8, hipMemcpyDeviceToHost));
    return MCA_HIP_OK;
}

int mca_hip_bmask_process_frame(mca_hip_bmask_ctx *c, double *left, double *right, int analysis_length, int *decisions)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!left || !right) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "left/right is NULL");
    if ((long long)analysis_length < (long long)BM_BANDS * c->N) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "analysis_length < 45 * frame_size");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t nb = (size_t)BM_BANDS * c->N * 8, slot = (size_t)(BM_BANDS + 1) * c->N;
    HIP_TRY(c, hipMemcpy(c->d_ana, left, nb, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_ana + slot, right, nb, hipMemcpyHostToDevice));
    BmaskHookArgs a{};
    a.L = c->d_ana; a.R = c->d_ana + slot; a.W = c->N; a.method = c->cfg.method; a.thr = c->d_thr64; a.Q = c->d_Q64;
    a.lambda = (double)kForgetting; a.one_minus_lambda = (double)(1 - kForgetting); a.rho = (double)kScaling;
    a.spatial = (double)kSpatialFactor; a.temporal = (double)kTemporalFactor; a.enhance = (double)kEnhanceFactor;
    a.decisions = c->d_dec;
    if (const int rc = launch_kernel(c, k_bmask_hook_param, dim3(BM_BANDS), dim3(256), 0, nullptr, a)) return rc;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpy(left, a.L, nb, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(right, a.R, nb, hipMemcpyDeviceToHost));
    if (decisions) HIP_TRY(c, hipMemcpy(decisions, c->d_dec, BM_BANDS * 4, hipMemcpyDeviceToHost));
    return MCA_HIP_OK;
}

int mca_hip_bmask_frame_synthesis(mca_hip_bmask_ctx *c, double *out_frame, const double *analysis, int frame_length, int analysis_length, int channel)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!out_frame || !analysis) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "out_frame/analysis is NULL");
    if (frame_length != c->N) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "frame_length != frame_size");
    if (channel < 0 || channel > 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "Sound localisation is only working for 2 channels by now.");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int N = c->N;
    // the slots the literal loop reads: slot * N < analysis_length - N, at most 46
    long long n_slots = 0;
    while (n_slots <= BM_BANDS && n_slots * N < (long long)analysis_length - N) ++n_slots;
    if (n_slots) HIP_TRY(c, hipMemcpy(c->d_ana, analysis, (size_t)n_slots * N * 8, hipMemcpyHostToDevice));
    if (const int rc = launch_kernel(c, k_bmask_hook_synth, grid_for(N, 256), dim3(256), 0, nullptr, c->d_x, c->d_ana, N, analysis_length)) return rc;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpy(out_frame, c->d_x, (size_t)N * 8, hipMemcpyDeviceToHost));
    return MCA_HIP_OK;
}

extern "C++" {
namespace {
constexpr unsigned BMASK_MAGIC = 0x4d43424du;   // "MCBM"
std::vector<BlobPart> bmask_parts(mca_hip_bmask_ctx *c)
{
    return {blob_part(c->d_Q), blob_part(c->d_tail[c->tail_cur]), blob_part(c->d_frames), blob_part(c->d_Q64)};
}
unsigned bmask_cfg_hash(const mca_hip_bmask_ctx *c)
{
    const int v[4] = {c->N, c->cfg.sample_rate, c->cfg.method, c->cfg.max_streams};
    unsigned h = blob_fnv(v, sizeof(v));
    h = blob_fnv(&c->cfg.micro_distance, sizeof(double), h);
    h = blob_fnv(&c->cfg.low_freq, sizeof(float), h);
    return blob_fnv(&c->cfg.high_freq, sizeof(float), h);
}
}  // namespace
}  // extern "C++"

long long mca_hip_bmask_state_size(const mca_hip_bmask_ctx *c) { return state_size(c, c ? bmask_parts(const_cast<mca_hip_bmask_ctx *>(c)) : std::vector<BlobPart>()); }

int mca_hip_bmask_state_save(mca_hip_bmask_ctx *c, void *blob, long long bytes)
{
    return c ? state_save(c, bmask_parts(c), BlobHeader{BMASK_MAGIC, 1, bmask_cfg_hash(c), 0, {0, 0, 0, 0}}, blob, bytes) : MCA_HIP_ERR_INVALID_ARGUMENT;
}

int mca_hip_bmask_state_load(mca_hip_bmask_ctx *c, const void *blob, long long bytes)
{
    BlobHeader h;
    return c ? state_load(c, bmask_parts(c), BMASK_MAGIC, 1, bmask_cfg_hash(c), blob, bytes, &h) : MCA_HIP_ERR_INVALID_ARGUMENT;
}

}  // extern "C"
