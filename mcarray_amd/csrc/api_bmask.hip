// api_bmask.hip -- C ABI of the filter-bank binaural masking module (include/mcarray_hip.h, mca_hip_bmask_*).
// Host side only: builds the filter bank, the thresholds and the per-bin tables, owns the per-stream state and the
// workspace between the three launches, enqueues the kernels.  No CPU fallback.
#include "../../include/mcarray_hip.h"
#include "bmask.h"
#include "fft512.h"
#include "stage.h"
#include "state_blob.h"

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
    StagePool stage;                           // 0..2 host-pointer staging, 3 sums, 4 gains
    std::string err;
};

namespace {

// the module's constants (BinauralMaskingImpl.h:142-155)
constexpr float kForgetting = 0.04f, kScaling = 0.01f, kTemporalFactor = 1.f, kSpatialFactor = 1.f, kEnhanceFactor = 1.f;
constexpr double kPhi = 10 * M_PI / 180, kThresholdScale = 0.9, kSpeedOfSound = 346.1;

std::string g_bmask_create_error;

int bfail(mca_hip_bmask_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg; else g_bmask_create_error = msg;
    return code;
}

#define BHIP_TRY(ctx, expr)                                                                             \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return bfail(ctx, _e == hipErrorOutOfMemory ? MCA_HIP_ERR_OUT_OF_MEMORY : MCA_HIP_ERR_HIP,  \
                         std::string(#expr) + ": " + hipGetErrorString(_e));                           \
    } while (0)

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
    BHIP_TRY(c, c->d_h.upload(h.data(), h.size()));
    return MCA_HIP_OK;
}

// dynamic LDS of the analysis and the synthesis kernel of frame length N
size_t smem_analyse(int N)
{
    if (N == 1024) return (size_t)(BM_FPB_1024 * 2 * FFT_SCRATCH + TW_WIN) * sizeof(float2);
    if (N == 2048) return (size_t)(16 * N512_ROW + 8 * FFT_SCRATCH + TW_WIN) * sizeof(float2);
    return (size_t)2 * (N / 2 + 1) * sizeof(float2);
}
size_t smem_synth(int N)
{
    if (N == 1024) return smem_analyse(N) + (size_t)BM_FPB_1024 * 48 * sizeof(float2);
    if (N == 2048) return smem_analyse(N) + (size_t)BM_FPB_2048 * 48 * sizeof(float2);
    return smem_analyse(N) + (size_t)2 * (N / 2) * sizeof(float) + 48 * sizeof(float2);
}

int fits(const mca_hip_bmask_ctx *c, int analysis_length) { return analysis_length < 0 ? 0 : std::min(BM_BANDS, analysis_length / c->N); }

}  // namespace

extern "C" {

const char *mca_hip_bmask_last_error(const mca_hip_bmask_ctx *ctx) { return ctx ? ctx->err.c_str() : g_bmask_create_error.c_str(); }

int mca_hip_bmask_create(const mca_hip_bmask_config *cfg, mca_hip_bmask_ctx **out)
{
    if (!cfg || !out) return bfail(nullptr, MCA_HIP_ERR_INVALID_ARGUMENT, "cfg/out is NULL");
    *out = nullptr;
    if (cfg->struct_size != (int)sizeof(mca_hip_bmask_config)) return bfail(nullptr, MCA_HIP_ERR_INVALID_ARGUMENT, "struct_size mismatch");
    if (cfg->frame_size < 256 || (cfg->frame_size & (cfg->frame_size - 1)) || cfg->frame_size > 8192) return bfail(nullptr, MCA_HIP_ERR_INVALID_ARGUMENT, "frame_size must be a power of two in [256,8192]");
    if (cfg->sample_rate <= 0 || !(cfg->micro_distance > 0)) return bfail(nullptr, MCA_HIP_ERR_INVALID_ARGUMENT, "sample_rate / micro_distance must be positive");
    if (!(cfg->low_freq >= 0) || !(cfg->high_freq > cfg->low_freq) || cfg->high_freq > 0.5f * cfg->sample_rate) return bfail(nullptr, MCA_HIP_ERR_INVALID_ARGUMENT, "need 0 <= low_freq < high_freq <= fs/2");
    const int m = cfg->method;
    if (!(m == 0 || m == 1 || m == 3)) return bfail(nullptr, MCA_HIP_ERR_INVALID_ARGUMENT, "bad masking method (FACTOR 0, RELATIVE 1, FULL 3)");
    if (cfg->max_streams < 1) return bfail(nullptr, MCA_HIP_ERR_INVALID_ARGUMENT, "max_streams < 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return bfail(nullptr, MCA_HIP_ERR_NO_DEVICE, "no HIP device visible; libmcarray_hip has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return bfail(nullptr, MCA_HIP_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    if (hipSetDevice(cfg->device) != hipSuccess) return bfail(nullptr, MCA_HIP_ERR_HIP, "hipSetDevice failed");

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
    if (!compact_ok) { delete c; return bfail(nullptr, MCA_HIP_ERR_UNSUPPORTED, "a bin is covered by more than two adjacent bands"); }
    const size_t ns = (size_t)cfg->max_streams;
    std::vector<float> win(N);
    for (int n = 0; n < N; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / N));
    std::vector<float2> tw(N / 2);
    for (int i = 0; i < N / 2; ++i) tw[i] = make_float2((float)std::cos(2.0 * M_PI * i / N), (float)(-std::sin(2.0 * M_PI * i / N)));
    auto body = [&]() -> int {
        BHIP_TRY(c, c->d_window.upload(win.data(), win.size()));
        BHIP_TRY(c, c->d_tw.upload(tw.data(), tw.size()));
        BHIP_TRY(c, c->d_kw.upload(kw.data(), kw.size())); BHIP_TRY(c, c->d_kp.upload(kp.data(), kp.size())); BHIP_TRY(c, c->d_kb.upload(kb.data(), kb.size()));
        BHIP_TRY(c, c->d_lo.upload(c->lo.data(), BM_BANDS)); BHIP_TRY(c, c->d_hi.upload(c->hi.data(), BM_BANDS));
        BHIP_TRY(c, c->d_thr.upload(thr32.data(), BM_BANDS));
        BHIP_TRY(c, c->d_Q.alloc_zero(ns * BM_BANDS));
        for (int i = 0; i < 2; ++i) BHIP_TRY(c, c->d_tail[i].alloc_zero(ns * 2 * c->hop));
        BHIP_TRY(c, c->d_frames.alloc_zero(ns));
        BHIP_TRY(c, c->d_thr64.upload(c->thr.data(), BM_BANDS));
        BHIP_TRY(c, c->d_Q64.alloc_zero(BM_BANDS));
        BHIP_TRY(c, c->d_x.alloc_zero((size_t)N));
        BHIP_TRY(c, c->d_ana.alloc_zero((size_t)2 * (BM_BANDS + 1) * N));
        BHIP_TRY(c, c->d_dec.alloc_zero(BM_BANDS));
        return MCA_HIP_OK;
    };
    const int rc = body();
    if (rc) { g_bmask_create_error = c->err; delete c; return rc; }
    // kernels that take more than 64 KiB of dynamic LDS are told so once, here
    if (smem_synth(N) > 64 * 1024) {
        const void *ka = N == 2048 ? reinterpret_cast<const void *>(k_bmask_analyse_2048) : reinterpret_cast<const void *>(k_bmask_analyse_gen);
        const void *ks = N == 2048 ? reinterpret_cast<const void *>(k_bmask_synth_2048) : reinterpret_cast<const void *>(k_bmask_synth_gen);
        hipError_t e = hipFuncSetAttribute(ka, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_analyse(N));
        if (e == hipSuccess) e = hipFuncSetAttribute(ks, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_synth(N));
        if (e != hipSuccess) { delete c; return bfail(nullptr, MCA_HIP_ERR_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e)); }
    }
    BmaskTables &t = c->tab;
    t.window = c->d_window; t.tw = c->d_tw; t.kb = c->d_kb; t.kw = c->d_kw; t.kp = c->d_kp; t.lo = c->d_lo; t.hi = c->d_hi;
    t.N = N; t.logH = c->logH;
    *out = c;
    return MCA_HIP_OK;
}

void mca_hip_bmask_destroy(mca_hip_bmask_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    (void)hipDeviceSynchronize();
    delete c;                                 // every device buffer goes with its member
}

int mca_hip_bmask_reset(mca_hip_bmask_ctx *c)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    BHIP_TRY(c, hipSetDevice(c->cfg.device));
    BHIP_TRY(c, hipDeviceSynchronize());
    BHIP_TRY(c, hipMemset(c->d_Q, 0, c->d_Q.bytes()));
    for (int i = 0; i < 2; ++i) BHIP_TRY(c, hipMemset(c->d_tail[i], 0, c->d_tail[i].bytes()));
    BHIP_TRY(c, hipMemset(c->d_frames, 0, c->d_frames.bytes()));
    BHIP_TRY(c, hipMemset(c->d_Q64, 0, c->d_Q64.bytes()));
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
    if (!pcm || !out_pcm) return bfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "pcm_dev/out_pcm_dev is NULL");
    if (n_streams < 1 || n_streams > c->cfg.max_streams) return bfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_streams outside [1, max_streams]");
    if (n_frames < 1) return bfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_frames < 1");
    const long long need = (long long)(n_frames + 1) * c->hop;
    if (ch_stride < need || (n_streams > 1 && stream_stride < ch_stride + need)) return bfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "strides shorter than (n_frames+1)*hop samples");
    if ((ch_stride & 1) || (stream_stride & 1) || (reinterpret_cast<uintptr_t>(pcm) & 7)) return bfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "pcm_dev must be 8-byte aligned with even strides");
    BHIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    // the band sums and gains of the call, [streams][n_frames][45]; grow-only
    const size_t cells = (size_t)n_streams * n_frames * BM_BANDS;
    float4 *d_sums = (float4 *)c->stage.get(3, cells * sizeof(float4));
    float2 *d_gains = (float2 *)c->stage.get(4, cells * sizeof(float2));
    if (!d_sums || !d_gains) return bfail(c, MCA_HIP_ERR_OUT_OF_MEMORY, "workspace for the band sums and gains");

    BmaskStreamArgs a{};
    a.t = c->tab; a.pcm = pcm; a.stream_stride = stream_stride; a.ch_stride = ch_stride; a.n_frames = n_frames;
    a.sums = d_sums; a.gains = d_gains;
    a.tail_in = c->d_tail[c->tail_cur]; a.tail_out = c->d_tail[c->tail_cur ^ 1]; a.out = out_pcm;
    // runs of up to 256 frames (every run but the first re-synthesises one frame for the overlap-add carry), shorter ones for
    // small batches so that two workgroups per CU exist
    a.ft = 256;
    while (a.ft > 16 && (long long)n_streams * ((n_frames + a.ft - 1) / a.ft) < 512) a.ft >>= 1;
    const int n_runs = (n_frames + a.ft - 1) / a.ft;

    BmaskScanArgs sa{};
    sa.sums = d_sums; sa.n_frames = n_frames; sa.method = c->cfg.method; sa.thr = c->d_thr;
    sa.lambda = (double)kForgetting; sa.one_minus_lambda = (double)(1 - kForgetting); sa.rho = kScaling;
    sa.inv_spatial = 1.f / kSpatialFactor; sa.inv_temporal = 1.f / kTemporalFactor; sa.enhance = kEnhanceFactor;
    sa.Q = c->d_Q; sa.frames = c->d_frames; sa.gains = d_gains; sa.decisions = decisions;
    const dim3 scan_grid(n_streams);
    const size_t smem_a = smem_analyse(c->N), smem_s = smem_synth(c->N);

    if (c->N == 1024) {
        hipLaunchKernelGGL(k_bmask_analyse_1024, dim3((n_frames + BM_FPB_1024 - 1) / BM_FPB_1024, n_streams), dim3(512), smem_a, st, a);
        hipLaunchKernelGGL(k_bmask_scan, scan_grid, dim3(BM_SCAN_THREADS), 0, st, sa);
        hipLaunchKernelGGL(k_bmask_synth_1024, dim3(n_runs, n_streams), dim3(512), smem_s, st, a);
    } else if (c->N == 2048) {
        hipLaunchKernelGGL(k_bmask_analyse_2048, dim3((n_frames + BM_FPB_2048 - 1) / BM_FPB_2048, n_streams), dim3(512), smem_a, st, a);
        hipLaunchKernelGGL(k_bmask_scan, scan_grid, dim3(BM_SCAN_THREADS), 0, st, sa);
        hipLaunchKernelGGL(k_bmask_synth_2048, dim3(n_runs, n_streams), dim3(512), smem_s, st, a);
    } else {
        hipLaunchKernelGGL(k_bmask_analyse_gen, dim3(n_frames, n_streams), dim3(256), smem_a, st, a);
        hipLaunchKernelGGL(k_bmask_scan, scan_grid, dim3(BM_SCAN_THREADS), 0, st, sa);
        hipLaunchKernelGGL(k_bmask_synth_gen, dim3(n_runs, n_streams), dim3(256), smem_s, st, a);
    }
    BHIP_TRY(c, hipGetLastError());
    c->tail_cur ^= 1;
    if (n_streams < c->cfg.max_streams) {
        // the streams beyond n_streams did not run: their carries move to the new buffer unchanged
        const size_t off = (size_t)n_streams * 2 * c->hop, cnt = ((size_t)c->cfg.max_streams - n_streams) * 2 * c->hop;
        BHIP_TRY(c, hipMemcpyAsync(c->d_tail[c->tail_cur] + off, c->d_tail[c->tail_cur ^ 1] + off, cnt * 4, hipMemcpyDeviceToDevice, st));
    }
    return MCA_HIP_OK;
}

int mca_hip_bmask_frames_host(mca_hip_bmask_ctx *c, const float *pcm, int n_streams, int n_frames, float *out_pcm, int *decisions)
{
    if (!c || !pcm || !out_pcm) return bfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_streams < 1 || n_frames < 1) return bfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_streams/n_frames < 1");
    BHIP_TRY(c, hipSetDevice(c->cfg.device));
    const long long cs = (long long)(n_frames + 1) * c->hop, ss = 2 * cs;
    const size_t n_out = (size_t)n_streams * 2 * n_frames * c->hop, n_dec = decisions ? (size_t)n_streams * n_frames * BM_BANDS : 0;
    float *d_pcm = (float *)c->stage.get(0, (size_t)ss * n_streams * 4), *d_out = (float *)c->stage.get(1, n_out * 4);
    int *d_dec = (int *)c->stage.get(2, n_dec * 4);
    if (!d_pcm || !d_out || (decisions && !d_dec)) return bfail(c, MCA_HIP_ERR_OUT_OF_MEMORY, "device staging buffers for the host-pointer call");
    BHIP_TRY(c, hipMemcpy(d_pcm, pcm, (size_t)ss * n_streams * 4, hipMemcpyHostToDevice));
    const int rc = mca_hip_bmask_frames_dev(c, d_pcm, ss, cs, n_streams, n_frames, d_out, d_dec, nullptr);
    if (rc) return rc;
    BHIP_TRY(c, hipDeviceSynchronize());
    BHIP_TRY(c, hipMemcpy(out_pcm, d_out, n_out * 4, hipMemcpyDeviceToHost));
    if (decisions) BHIP_TRY(c, hipMemcpy(decisions, d_dec, n_dec * 4, hipMemcpyDeviceToHost));
    return MCA_HIP_OK;
}

int mca_hip_bmask_frame_analysis(mca_hip_bmask_ctx *c, const double *in_frame, double *analysis, int frame_length, int analysis_length, int channel)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!in_frame || !analysis) return bfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "in_frame/analysis is NULL");
    if (frame_length != c->N) return bfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "frame_length != frame_size");
    if (channel < 0 || channel > 1) return bfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "Sound localisation is only working for 2 channels by now.");
    const int nb = fits(c, analysis_length);
    if (nb == 0) return MCA_HIP_OK;
    BHIP_TRY(c, hipSetDevice(c->cfg.device));
    const int rc = build_impulse_responses(c);
    if (rc) return rc;
    const int N = c->N;
    const bool residual = (long long)analysis_length >= (long long)(BM_BANDS + 1) * N;
    BHIP_TRY(c, hipMemcpy(c->d_x, in_frame, (size_t)N * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_bmask_hook_analysis, dim3(N / 256, nb), dim3(256), 0, 0, c->d_x, c->d_h, c->d_ana, N, nb);
    if (residual) hipLaunchKernelGGL(k_bmask_hook_residual, dim3(N / 256), dim3(256), 0, 0, c->d_x, c->d_ana, N);
    BHIP_TRY(c, hipGetLastError());
    BHIP_TRY(c, hipMemcpy(analysis, c->d_ana, (size_t)(nb + (residual ? 1 : 0)) * N * 8, hipMemcpyDeviceToHost));
    return MCA_HIP_OK;
}

int mca_hip_bmask_process_frame(mca_hip_bmask_ctx *c, double *left, double *right, int analysis_length, int *decisions)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!left || !right) return bfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "left/right is NULL");
    if ((long long)analysis_length < (long long)BM_BANDS * c->N) return bfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "analysis_length < 45 * frame_size");
    BHIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t nb = (size_t)BM_BANDS * c->N * 8, slot = (size_t)(BM_BANDS + 1) * c->N;
    BHIP_TRY(c, hipMemcpy(c->d_ana, left, nb, hipMemcpyHostToDevice));
    BHIP_TRY(c, hipMemcpy(c->d_ana + slot, right, nb, hipMemcpyHostToDevice));
    BmaskHookArgs a{};
    a.L = c->d_ana; a.R = c->d_ana + slot; a.W = c->N; a.method = c->cfg.method; a.thr = c->d_thr64; a.Q = c->d_Q64;
    a.lambda = (double)kForgetting; a.one_minus_lambda = (double)(1 - kForgetting); a.rho = (double)kScaling;
    a.spatial = (double)kSpatialFactor; a.temporal = (double)kTemporalFactor; a.enhance = (double)kEnhanceFactor;
    a.decisions = c->d_dec;
    hipLaunchKernelGGL(k_bmask_hook_param, dim3(BM_BANDS), dim3(256), 0, 0, a);
    BHIP_TRY(c, hipGetLastError());
    BHIP_TRY(c, hipMemcpy(left, a.L, nb, hipMemcpyDeviceToHost));
    BHIP_TRY(c, hipMemcpy(right, a.R, nb, hipMemcpyDeviceToHost));
    if (decisions) BHIP_TRY(c, hipMemcpy(decisions, c->d_dec, BM_BANDS * 4, hipMemcpyDeviceToHost));
    return MCA_HIP_OK;
}

int mca_hip_bmask_frame_synthesis(mca_hip_bmask_ctx *c, double *out_frame, const double *analysis, int frame_length, int analysis_length, int channel)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!out_frame || !analysis) return bfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "out_frame/analysis is NULL");
    if (frame_length != c->N) return bfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "frame_length != frame_size");
    if (channel < 0 || channel > 1) return bfail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "Sound localisation is only working for 2 channels by now.");
    BHIP_TRY(c, hipSetDevice(c->cfg.device));
    const int N = c->N;
    // the slots the literal loop reads: slot * N < analysis_length - N, at most 46
    long long n_slots = 0;
    while (n_slots <= BM_BANDS && n_slots * N < (long long)analysis_length - N) ++n_slots;
    if (n_slots) BHIP_TRY(c, hipMemcpy(c->d_ana, analysis, (size_t)n_slots * N * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_bmask_hook_synth, dim3(N / 256), dim3(256), 0, 0, c->d_x, c->d_ana, N, analysis_length);
    BHIP_TRY(c, hipGetLastError());
    BHIP_TRY(c, hipMemcpy(out_frame, c->d_x, (size_t)N * 8, hipMemcpyDeviceToHost));
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

long long mca_hip_bmask_state_size(const mca_hip_bmask_ctx *c)
{
    return c ? blob_size(bmask_parts(const_cast<mca_hip_bmask_ctx *>(c))) : (long long)MCA_HIP_ERR_INVALID_ARGUMENT;
}

int mca_hip_bmask_state_save(mca_hip_bmask_ctx *c, void *blob, long long bytes)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    BHIP_TRY(c, hipSetDevice(c->cfg.device));
    BlobHeader h{BMASK_MAGIC, 1, bmask_cfg_hash(c), 0, {0, 0, 0, 0}};
    const int rc = blob_save(bmask_parts(c), h, blob, bytes);
    return rc ? bfail(c, rc == 2 ? MCA_HIP_ERR_HIP : MCA_HIP_ERR_INVALID_ARGUMENT, blob_error(rc)) : MCA_HIP_OK;
}

int mca_hip_bmask_state_load(mca_hip_bmask_ctx *c, const void *blob, long long bytes)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    BHIP_TRY(c, hipSetDevice(c->cfg.device));
    BlobHeader h;
    const int rc = blob_load(bmask_parts(c), BMASK_MAGIC, bmask_cfg_hash(c), blob, bytes, &h);
    return rc ? bfail(c, rc == 2 ? MCA_HIP_ERR_HIP : MCA_HIP_ERR_INVALID_ARGUMENT, blob_error(rc)) : MCA_HIP_OK;
}

}  // extern "C"
