// api_mask.hip -- C ABI of the binaural masking module (include/mcarray_hip.h, mca_hip_mask_*).
// Host side only: builds the mel filter bank and thresholds the reference builds in its
// constructor, owns the per-stream state, enqueues the kernels.  No CPU fallback.
#include "../../include/mcarray_hip.h"
#include "fft512.h"
#include "host_common.h"
#include "kernels.h"
#include "module_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace mca;

struct mca_hip_mask_ctx {
    mca_hip_mask_config cfg{};
    int N = 0, K = 0;
    std::vector<double> H, center, thr;       // [45][K], [45], [45]
    MaskParams hp{};
    DevBuf<MaskParams> d_mp;
    DevBuf<float> d_window;
    DevBuf<float2> d_tw, d_kw; DevBuf<int> d_kb;   // any-length stream kernel
    int hop = 0, logH = 0;
    DevBuf<float> d_Q[2], d_noise, d_tail[2];      // the state: each array at exactly its state size (mask_parts)
    int q_cur = 0, tail_cur = 0;
    long long frames_done = 0;
    int streams_in_use = 0;           // n_streams of the first stream call after create / reset: the context counts frames once for all streams
    // frame API (double)
    DevBuf<double> d_H, d_thr, d_Q64, d_noise64, d_io;   // d_io: L, R, outL, outR
    DevBuf<int> d_dec;
    int first_call = 0;
    StagePool stage;
    std::string err;
};

namespace {

mca_hip_mask_ctx *const NO_CTX = nullptr;        // a failing create: the text goes to the module's creation error
enum MaskStageSlot { SG_PCM, SG_OUT, SG_DECISIONS };      // the staging-pool slots of the host-pointer call: the numbers stay
void free_mask(mca_hip_mask_ctx *c) { delete c; }      // every device buffer goes with its member

double hz2mel(double f) { return 2595.0 * std::log10(1.0 + f / 700.0); }
double mel2hz(double m) { return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0); }

// [BUILD-DEFINES] stand-in for dsp::FilterBankFFTWMelScale(order, 45, fs, fmin, fmax) (FastBinauralMasking.cpp:95):
// 45 unit-peak triangles with HTK-mel spaced edges, sampled on the K = N/2+1 bin frequencies.
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

}  // namespace

extern "C" {

const char *mca_hip_mask_last_error(const mca_hip_mask_ctx *ctx) { return last_error(ctx); }

int mca_hip_mask_create(const mca_hip_mask_config *cfg, mca_hip_mask_ctx **out)
{
    if (!cfg || !out) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "cfg/out is NULL");
    *out = nullptr;
    if (cfg->struct_size != (int)sizeof(mca_hip_mask_config)) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "struct_size mismatch");
    if (cfg->fft_size < 64 || (cfg->fft_size & (cfg->fft_size - 1)) || cfg->fft_size > 16384) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "fft_size must be a power of two in [64,16384]");
    if (cfg->sample_rate <= 0 || !(cfg->micro_distance > 0)) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "sample_rate / micro_distance must be positive");
    if (!(cfg->low_freq >= 0) || !(cfg->high_freq > cfg->low_freq) || cfg->high_freq > 0.5f * cfg->sample_rate) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "need 0 <= low_freq < high_freq <= fs/2");
    const int m = cfg->method;
    if (!(m == 0 || m == 1 || m == 3 || m == 4 || m == 5)) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "bad masking method");
    if (cfg->algorithm < 0 || cfg->algorithm > 2) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "bad masking algorithm");
    if (cfg->max_streams < 1) return fail(NO_CTX, MCA_HIP_ERR_INVALID_ARGUMENT, "max_streams < 1");
    if (const int rc = check_device(NO_CTX, cfg->device)) return rc;

    mca_hip_mask_ctx *c = new mca_hip_mask_ctx();
    c->cfg = *cfg; c->N = cfg->fft_size; c->K = c->N / 2 + 1; c->hop = c->N / 2;
    while ((1 << c->logH) < c->hop) ++c->logH;
    mel_filterbank(c->N, 45, cfg->sample_rate, (double)cfg->low_freq, (double)cfg->high_freq, c->H, c->center);
    c->thr.resize(45);
    const double phi = 10 * M_PI / 180;                                           // FastBinauralMasking.h:113
    for (int b = 0; b < 45; ++b) {                                                // calculateThresholds :342-366
        const double wfreq = c->center[b] * cfg->sample_rate * 2 * M_PI;
        c->thr[b] = std::cos(wfreq * cfg->micro_distance * std::sin(phi) / 346.1);
    }
    const float lam = 0.04f, rej = 0.999f, rho = 0.01f;                           // FastBinauralMasking.h:114,128,124
    MaskParams &hp = c->hp;
    hp.lambda = lam; hp.one_minus_lambda = 1 - lam; hp.reject = rej; hp.rho = rho; hp.method = cfg->method; hp.alg = cfg->algorithm;
    // every bin is covered by at most two adjacent triangles: (first band, its weight, the next band's weight) per bin
    bool compact_ok = true;
    std::vector<int> kb(c->K, -1);
    std::vector<float2> kw(c->K, make_float2(0.f, 0.f));
    for (int b = 0; b < 45; ++b) { hp.thr[b] = (float)c->thr[b]; hp.lo[b] = 1; hp.hi[b] = 0; }
    for (int k = 0; k < c->K; ++k) {
        int nfound = 0;
        for (int b = 0; b < 45; ++b) {
            const double h = c->H[(size_t)b * c->K + k];
            if (h > 0) {
                if (nfound == 0) { kb[k] = b; kw[k].x = (float)h; }
                else if (nfound == 1 && b == kb[k] + 1) kw[k].y = (float)h;
                else compact_ok = false;
                ++nfound;
                if (hp.lo[b] > hp.hi[b]) hp.lo[b] = k;
                hp.hi[b] = k;
            }
        }
    }
    if (!compact_ok) { delete c; return fail(NO_CTX, MCA_HIP_ERR_UNSUPPORTED, "a bin is covered by more than two adjacent bands"); }
    if (c->N == FFT_N)
        for (int k = 0; k < c->K; ++k) { hp.kb[k] = kb[k]; hp.kw0[k] = kw[k].x; hp.kw1[k] = kw[k].y; }
    const size_t ns = (size_t)cfg->max_streams;
    std::vector<float> win(c->N);
    for (int n = 0; n < c->N; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / c->N));
    std::vector<float2> tw(c->N / 2);
    for (int i = 0; i < c->N / 2; ++i) tw[i] = make_float2((float)std::cos(2.0 * M_PI * i / c->N), (float)(-std::sin(2.0 * M_PI * i / c->N)));
    auto body = [&]() -> int {
        HIP_TRY(c, c->d_mp.upload(&c->hp, 1));
        HIP_TRY(c, c->d_window.upload(win.data(), win.size()));
        HIP_TRY(c, c->d_tw.upload(tw.data(), tw.size())); HIP_TRY(c, c->d_kw.upload(kw.data(), kw.size())); HIP_TRY(c, c->d_kb.upload(kb.data(), kb.size()));
        for (int i = 0; i < 2; ++i) { HIP_TRY(c, c->d_Q[i].alloc_zero(ns * 45)); HIP_TRY(c, c->d_tail[i].alloc_zero(ns * 2 * c->hop)); }
        HIP_TRY(c, c->d_noise.alloc_zero(ns * 45));
        HIP_TRY(c, c->d_H.upload(c->H.data(), c->H.size()));
        HIP_TRY(c, c->d_thr.upload(c->thr.data(), 45));
        HIP_TRY(c, c->d_Q64.alloc_zero(45)); HIP_TRY(c, c->d_noise64.alloc_zero(45));
        HIP_TRY(c, c->d_io.alloc_zero((size_t)4 * (c->N + 2)));
        HIP_TRY(c, c->d_dec.alloc_zero(45));
        return MCA_HIP_OK;
    };
    const int rc = body();
    if (rc) return create_failed(c, rc, free_mask);
    *out = c;
    return MCA_HIP_OK;
}

void mca_hip_mask_destroy(mca_hip_mask_ctx *c) { destroy_ctx(c, free_mask); }

int mca_hip_mask_reset(mca_hip_mask_ctx *c)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    for (int i = 0; i < 2; ++i) { HIP_TRY(c, hipMemset(c->d_Q[i], 0, c->d_Q[i].bytes())); HIP_TRY(c, hipMemset(c->d_tail[i], 0, c->d_tail[i].bytes())); }
    HIP_TRY(c, hipMemset(c->d_noise, 0, c->d_noise.bytes()));
    HIP_TRY(c, hipMemset(c->d_Q64, 0, c->d_Q64.bytes())); HIP_TRY(c, hipMemset(c->d_noise64, 0, c->d_noise64.bytes()));
    c->frames_done = 0; c->first_call = 0; c->streams_in_use = 0;
    return MCA_HIP_OK;
}

int mca_hip_mask_get_thresholds(const mca_hip_mask_ctx *c, double *thresholds, double *center_freqs)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (thresholds) std::memcpy(thresholds, c->thr.data(), 45 * 8);
    if (center_freqs) std::memcpy(center_freqs, c->center.data(), 45 * 8);
    return MCA_HIP_OK;
}

int mca_hip_mask_frames_dev(mca_hip_mask_ctx *c, const float *pcm, long long stream_stride, long long ch_stride,
                            int n_streams, int n_frames, float *out_pcm, int *decisions, void *stream)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (c->N > 8192) return fail(c, MCA_HIP_ERR_UNSUPPORTED, "the stream API takes frame lengths up to 8192 (the frame hook takes any size)");
    if (!pcm || !out_pcm) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "pcm_dev/out_pcm_dev is NULL");
    if (n_streams < 1 || n_streams > c->cfg.max_streams) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_streams outside [1, max_streams]");
    if (n_frames < 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_frames < 1");
    // frames_done (first-frame behaviour of the Q recursion, NOISY's noise capture: FastBinauralMasking.cpp:186-197) is kept once
    // per context, so all streams of a context start together and advance together: a call with another number of streams
    // would give the late or missing slots the not-first-frame path
    if (c->streams_in_use && n_streams != c->streams_in_use)
        return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_streams differs from the first call after create / reset: the streams of a masking context advance together (mca_hip_mask_reset starts over)");
    const long long need = (long long)(n_frames + 1) * c->hop;
    if (ch_stride < need || (n_streams > 1 && stream_stride < ch_stride + need)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "strides shorter than (n_frames+1)*hop samples");
    if ((ch_stride & 1) || (stream_stride & 1) || (reinterpret_cast<uintptr_t>(pcm) & 7)) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "pcm_dev must be 8-byte aligned with even strides");
    hipStream_t st = (hipStream_t)stream;
    MaskArgs a{};
    a.pcm = pcm; a.stream_stride = stream_stride; a.ch_stride = ch_stride; a.n_frames = n_frames;
    // (the run length, NOISY's first call as one chunk, the LDS of the three forms: plan_mask_stream)
    const MaskStreamPlan p = plan_mask_stream(c->N, c->cfg.method == MCA_HIP_MASK_NOISY && c->frames_done == 0, n_streams, n_frames);
    a.ft = p.ft;
    a.frames_done = c->frames_done; a.window = c->d_window; a.mp = c->d_mp;
    a.Q_in = c->d_Q[c->q_cur]; a.Q_out = c->d_Q[c->q_cur ^ 1]; a.noise = c->d_noise;
    a.tail_in = c->d_tail[c->tail_cur]; a.tail_out = c->d_tail[c->tail_cur ^ 1];
    a.out = out_pcm; a.decisions = decisions;
    int rc;
    if (p.form == FORM_A) rc = launch_kernel(c, k_mask_stream, p.l.grid, p.l.block, p.l.lds, st, a);
    else {
        // 2048-sample frames (44.1 / 48 kHz): four 512-sample sub-sequences per frame on the wave-level transform; any other power of two: one
        // frame at a time, block-cooperative FFT (runs re-analyse MK_WARM + 1 frames)
        MaskGenArgs ga{};
        ga.a = a; ga.N = c->N; ga.logH = c->logH; ga.tw = c->d_tw; ga.kw = c->d_kw; ga.kb = c->d_kb;
        rc = launch_kernel(c, p.form == FORM_B ? k_mask_stream_2048 : k_mask_stream_gen, p.l.grid, p.l.block, p.l.lds, st, ga);
    }
    if (rc) return rc;
    HIP_TRY(c, hipGetLastError());
    c->q_cur ^= 1; c->tail_cur ^= 1;
    c->frames_done += n_frames; c->streams_in_use = n_streams;
    return MCA_HIP_OK;
}

int mca_hip_mask_frames_host(mca_hip_mask_ctx *c, const float *pcm, int n_streams, int n_frames, float *out_pcm, int *decisions)
{
    if (!c || !pcm || !out_pcm) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_streams < 1 || n_frames < 1) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "n_streams/n_frames < 1");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const long long cs = (long long)(n_frames + 1) * c->hop, ss = 2 * cs;
    const size_t n_out = (size_t)n_streams * 2 * n_frames * c->hop, n_dec = (size_t)n_streams * n_frames * 45;
    StageBuf b[] = {{SG_PCM, pcm, (size_t)ss * n_streams * 4, STAGE_IN}, {SG_OUT, out_pcm, n_out * 4, STAGE_OUT}, {SG_DECISIONS, decisions, n_dec * 4, STAGE_OUT}};
    return staged(c, b, [&] { return mca_hip_mask_frames_dev(c, (float *)b[0].dev, ss, cs, n_streams, n_frames, (float *)b[1].dev, (int *)b[2].dev, nullptr); });
}

extern "C++" {
namespace {
constexpr unsigned MASK_MAGIC = 0x4d434d4bu;   // "MCMK"
std::vector<BlobPart> mask_parts(mca_hip_mask_ctx *c)
{
    return {blob_part(c->d_Q[c->q_cur]), blob_part(c->d_noise), blob_part(c->d_tail[c->tail_cur]), blob_part(c->d_Q64), blob_part(c->d_noise64)};
}
unsigned mask_cfg_hash(const mca_hip_mask_ctx *c)
{
    const int v[5] = {c->N, c->cfg.sample_rate, c->cfg.method, c->cfg.algorithm, c->cfg.max_streams};
    unsigned h = blob_fnv(v, sizeof(v));
    h = blob_fnv(&c->cfg.micro_distance, sizeof(double), h);
    h = blob_fnv(&c->cfg.low_freq, sizeof(float), h);
    return blob_fnv(&c->cfg.high_freq, sizeof(float), h);
}
}  // namespace
}  // extern "C++"

long long mca_hip_mask_state_size(const mca_hip_mask_ctx *c) { return state_size(c, c ? mask_parts(const_cast<mca_hip_mask_ctx *>(c)) : std::vector<BlobPart>()); }

int mca_hip_mask_state_save(mca_hip_mask_ctx *c, void *blob, long long bytes)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    const BlobHeader h{MASK_MAGIC, 1, mask_cfg_hash(c), 0, {c->frames_done, (long long)c->first_call, (long long)c->streams_in_use, 0}};      // the host-side counters
    return state_save(c, mask_parts(c), h, blob, bytes);
}

int mca_hip_mask_state_load(mca_hip_mask_ctx *c, const void *blob, long long bytes)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    BlobHeader h;
    if (const int rc = state_load(c, mask_parts(c), MASK_MAGIC, 1, mask_cfg_hash(c), blob, bytes, &h)) return rc;
    c->frames_done = h.host[0]; c->first_call = (int)h.host[1]; c->streams_in_use = (int)h.host[2];
    return MCA_HIP_OK;
}

int mca_hip_mask_process_frame(mca_hip_mask_ctx *c, double *left, double *right, int ccs_len, int *decisions)
{
    if (!c) return MCA_HIP_ERR_INVALID_ARGUMENT;
    if (!left || !right) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "left/right is NULL");
    if (ccs_len != c->N + 2) return fail(c, MCA_HIP_ERR_INVALID_ARGUMENT, "ccs_len != fft_size + 2");
    if (c->cfg.method == MCA_HIP_MASK_NOTHING) return MCA_HIP_OK;              // :130-134
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t nb = (size_t)ccs_len * 8;
    HIP_TRY(c, hipMemcpy(c->d_io, left, nb, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_io + ccs_len, right, nb, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemset(c->d_io + 2 * ccs_len, 0, 2 * nb));                   // setZeros :142-143
    MaskFrameArgs a{};
    a.L = c->d_io; a.R = c->d_io + ccs_len; a.outL = c->d_io + 2 * ccs_len; a.outR = c->d_io + 3 * ccs_len;
    a.H = c->d_H; a.thr = c->d_thr; a.Q = c->d_Q64; a.noise = c->d_noise64;
    a.K = c->K; a.method = c->cfg.method; a.alg = c->cfg.algorithm; a.first_call = c->first_call;
    const float lam = 0.04f, rej = 0.999f, rho = 0.01f;
    a.lambda = (double)lam; a.one_minus_lambda = (double)(1 - lam); a.reject = (double)rej; a.rho = (double)rho;
    a.decisions = decisions ? c->d_dec : nullptr;
    if (const int rc = launch_kernel(c, k_mask_frame, dim3(1), dim3(256), 0, nullptr, a)) return rc;
    HIP_TRY(c, hipGetLastError());
    ++c->first_call;                                                             // :192
    HIP_TRY(c, hipMemcpy(left, a.outL, nb, hipMemcpyDeviceToHost));            // :199-200
    HIP_TRY(c, hipMemcpy(right, a.outR, nb, hipMemcpyDeviceToHost));
    if (decisions) HIP_TRY(c, hipMemcpy(decisions, c->d_dec, 45 * 4, hipMemcpyDeviceToHost));
    return MCA_HIP_OK;
}

}  // extern "C"
