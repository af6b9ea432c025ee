// kernels_bmask.hip -- filter-bank binaural masking (BinauralMaskingImpl, the time-domain formulation of the
// Kim / Kumar / Stern masking) on gfx950.
//
// The module filters every windowed frame through 45 mel triangles, takes four means over the W samples of every
// band signal pair (l, r), decides per band and scales the band.  Band b is the circular filtering irfft(X H_b), so
//   - the means are sums over the half spectrum (Parseval: weight 1 at DC and Nyquist, 2 elsewhere), and
//   - the re-summed frame is irfft(X sum_b g_b H_b): one inverse transform per channel, none per band.
//
// Stream path, fp32, three launches per call:
//   k_bmask_analyse_*   (stream, frames)  window, transform, the four band sums of every band -> sums
//   k_bmask_scan        (stream)          frames in order: Q recursion; decision and the two gains per cell -> gains, decisions
//   k_bmask_synth_*     (stream, run)     transform again, X sum_b g_b H_b, inverse, overlap-add
// Every (frame, band) sum is formed by the same eight lanes in the same order and the scan walks the frames of one call
// after those of the call before it with Q carried in memory, so the bits depend neither on the batch nor on the call split.
//
// Frame hooks, double: the circulant filter bank, the literal decision loop on band signals, the literal re-summation.
#include "bmask.h"
#include "fft_block.h"

namespace mca {

// sums of band b over its support for one frame: eight lanes (sub = 0..7) stride over the bins, xor-shuffle reduction
// (every lane of the group returns the total)
__device__ __forceinline__ float4 bm_band_sums(const BmaskTables &t, const float2 *L, const float2 *R, int b, int sub)
{
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    const int hi = t.hi[b];
    for (int k = t.lo[b] + sub; k <= hi; k += 8) {
        const float2 pw = t.kp[k];
        const float w = t.kb[k] == b ? pw.x : pw.y;
        const float2 l = L[k], r = R[k];
        const float mx = l.x + r.x, my = l.y + r.y;
        a0 += w * (l.x * l.x + l.y * l.y);
        a1 += w * (r.x * r.x + r.y * r.y);
        a2 += w * (l.x * r.x + l.y * r.y);
        a3 += w * (0.25f * (mx * mx + my * my));
    }
#pragma unroll
    for (int off = 4; off > 0; off >>= 1) {
        a0 += __shfl_xor(a0, off); a1 += __shfl_xor(a1, off); a2 += __shfl_xor(a2, off); a3 += __shfl_xor(a3, off);
    }
    return make_float4(a0, a1, a2, a3);
}

// sum_b g_b H_b[k] for channel ch; g: the 45 gain pairs of the frame
__device__ __forceinline__ float bm_bin_gain(const BmaskTables &t, const float2 *g, int ch, int k)
{
    const int b0 = t.kb[k];
    if (b0 < 0) return 0.f;
    const float2 hw = t.kw[k];
    const float2 ga = g[b0];
    float m = (ch ? ga.y : ga.x) * hw.x;
    if (b0 + 1 < BM_BANDS) {
        const float2 gb = g[b0 + 1];
        m += (ch ? gb.y : gb.x) * hw.y;
    }
    return m;
}

// ---------------------------------------------------------------------------------------
// W = 1024: wave = (frame slot, channel), the wave-level transform of fft512.h
// ---------------------------------------------------------------------------------------
// frames tb .. tb + nb - 1 of stream s -> spec[(slot * 2 + channel) * FFT_SCRATCH + k], k = 0..512.  Ends with a barrier.
__device__ __forceinline__ void bm_forward_1024(const BmaskStreamArgs &p, int s, int tb, int nb, const float2 (&wreg)[8], float2 *spec,
                                                int lane, int wave, const FftTw &tw)
{
    const int jw = wave >> 1, cw = wave & 1;
    if (jw < nb) {
        const float *base = p.pcm + (long long)s * p.stream_stride + (long long)cw * p.ch_stride;
        const float2 *src = reinterpret_cast<const float2 *>(base + (long long)(tb + jw) * FFT_H);
        float2 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float2 x = src[lane + 64 * r], w = wreg[r];
            v[r] = make_float2(x.x * w.x, x.y * w.y);
        }
        rfft1024(v, spec + (jw * 2 + cw) * FFT_SCRATCH, lane, tw);
    }
    __syncthreads();
}

__device__ __forceinline__ void bm_window_1024(const float *window, int lane, float2 (&wreg)[8])
{
#pragma unroll
    for (int r = 0; r < 8; ++r) {                          // halved: the 1/2 of rfft1024's split step
        const float2 w = reinterpret_cast<const float2 *>(window)[lane + 64 * r];
        wreg[r] = make_float2(0.5f * w.x, 0.5f * w.y);
    }
}

// grid (ceil(F / 4), streams), 512 threads, LDS 4 * 2 * FFT_SCRATCH + TW_WIN float2 (42.5 KiB)
__global__ __launch_bounds__(512) void k_bmask_analyse_1024(BmaskStreamArgs p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *spec = reinterpret_cast<float2 *>(smem_raw);                  // [4][2][FFT_SCRATCH]
    float2 *tab = spec + BM_FPB_1024 * 2 * FFT_SCRATCH;                   // [TW_WIN]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.y, tb = blockIdx.x * BM_FPB_1024, nb = min(BM_FPB_1024, p.n_frames - tb);
    fft_table_init(tab, nullptr, tid, 512);
    float2 wreg[8];
    bm_window_1024(p.t.window, lane, wreg);
    __syncthreads();
    FftTw tw{tab};
    bm_forward_1024(p, s, tb, nb, wreg, spec, lane, wave, tw);
    for (int q = tid >> 3; q < nb * BM_BANDS; q += 64) {
        const int j = q / BM_BANDS, b = q - j * BM_BANDS;
        const float4 a = bm_band_sums(p.t, spec + (j * 2) * FFT_SCRATCH, spec + (j * 2 + 1) * FFT_SCRATCH, b, tid & 7);
        if ((tid & 7) == 0) p.sums[((long long)s * p.n_frames + tb + j) * BM_BANDS + b] = a;
    }
}

// grid (runs of ft frames, streams), 512 threads.  A run starts one frame early (not at frame 0): that frame rebuilds the
// overlap-add carry and is not written.
__global__ __launch_bounds__(512) void k_bmask_synth_1024(BmaskStreamArgs p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *spec = reinterpret_cast<float2 *>(smem_raw);                  // [4][2][FFT_SCRATCH]
    float2 *tab = spec + BM_FPB_1024 * 2 * FFT_SCRATCH;                   // [TW_WIN]
    float2 *gl = tab + TW_WIN;                                            // [4][48] gains of the pass
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.y;
    const int t0 = blockIdx.x * p.ft, t1 = min(t0 + p.ft, p.n_frames);
    const int tbeg = t0 > 0 ? t0 - 1 : 0;
    fft_table_init(tab, nullptr, tid, 512);
    float2 wreg[8];
    bm_window_1024(p.t.window, lane, wreg);
    float carry[2] = {0.f, 0.f};
    if (t0 == 0) { carry[0] = p.tail_in[((long long)s * 2 + 0) * FFT_H + tid]; carry[1] = p.tail_in[((long long)s * 2 + 1) * FFT_H + tid]; }
    __syncthreads();
    FftTw tw{tab};
    const int jw = wave >> 1, cw = wave & 1;

    for (int tb = tbeg; tb < t1; tb += BM_FPB_1024) {
        const int nb = min(BM_FPB_1024, t1 - tb);
        for (int e = tid; e < nb * BM_BANDS; e += 512) {
            const int j = e / BM_BANDS, b = e - j * BM_BANDS;
            gl[j * 48 + b] = p.gains[((long long)s * p.n_frames + tb + j) * BM_BANDS + b];
        }
        bm_forward_1024(p, s, tb, nb, wreg, spec, lane, wave, tw);      // its barrier also publishes gl
        for (int e = tid; e < nb * 2 * FFT_K; e += 512) {
            const int jc = e / FFT_K, k = e - jc * FFT_K;
            const float m = bm_bin_gain(p.t, gl + (jc >> 1) * 48, jc & 1, k);
            const float2 x = spec[jc * FFT_SCRATCH + k];
            spec[jc * FFT_SCRATCH + k] = make_float2(x.x * m, x.y * m);
        }
        __syncthreads();
        if (jw < nb) irfft1024(spec + (jw * 2 + cw) * FFT_SCRATCH, lane, tw);
        __syncthreads();
        for (int j = 0; j < nb; ++j) {
            const int t = tb + j;
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                const float *y = reinterpret_cast<const float *>(spec + (j * 2 + ch) * FFT_SCRATCH);
                if (t >= t0) p.out[((long long)s * 2 + ch) * (long long)p.n_frames * FFT_H + (long long)t * FFT_H + tid] = carry[ch] + y[tid];
                carry[ch] = y[tid + FFT_H];
            }
        }
        __syncthreads();
    }
    if (t1 == p.n_frames) {
        p.tail_out[((long long)s * 2 + 0) * FFT_H + tid] = carry[0];
        p.tail_out[((long long)s * 2 + 1) * FFT_H + tid] = carry[1];
    }
}

// ---------------------------------------------------------------------------------------
// W = 2048: four 512-sample sub-sequences per frame (fft512.h), wave = (frame slot, channel, pair of sub-sequences)
// LDS: sub [2][2][4][N512_ROW] | scr [8][FFT_SCRATCH] (the spectra X [2][2][1026] take its place between the transforms) | tab
// ---------------------------------------------------------------------------------------
constexpr int BM_XR = 1026, BM_YT = 2064;

__device__ __forceinline__ void bm_window_2048(const float *window, int lane, int pr, float2 (&wreg)[8])
{
#pragma unroll
    for (int r = 0; r < 8; ++r) {                          // halved: the 1/2 of rfft512_pair
        const float2 w = reinterpret_cast<const float2 *>(window)[2 * (lane + 64 * r) + pr];
        wreg[r] = make_float2(0.5f * w.x, 0.5f * w.y);
    }
}

// frames tb .. tb + nb - 1 -> X[(slot * 2 + channel) * BM_XR + k], k = 0..1024.  Ends with a barrier.
__device__ __forceinline__ void bm_forward_2048(const BmaskStreamArgs &p, int s, int tb, int nb, const float2 (&wreg)[8], float2 *sub,
                                                float2 *scr, float2 *X, int tid, const FftTw &tw)
{
    const int lane = tid & 63, wave = tid >> 6;
    const int jw = wave >> 2, cw = (wave >> 1) & 1, pr = wave & 1;
    if (jw < nb) {
        const float *base = p.pcm + (long long)s * p.stream_stride + (long long)cw * p.ch_stride;
        const float2 *src = reinterpret_cast<const float2 *>(base + (long long)(tb + jw) * 1024);
        float2 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float2 x = src[2 * (lane + 64 * r) + pr], w = wreg[r];
            v[r] = make_float2(x.x * w.x, x.y * w.y);
        }
        float2 *S = sub + ((jw * 2 + cw) * 4 + 2 * pr) * N512_ROW;
        rfft512_pair(v, scr + wave * FFT_SCRATCH, S, S + N512_ROW, lane, tw);
    }
    __syncthreads();
    for (int e = tid; e < nb * 2 * 512; e += 512) {         // thread = (frame, channel, m): one radix-4 butterfly
        const int jc = e >> 9, m = e & 511;
        combine2048_m(sub + jc * 4 * N512_ROW, m, p.t.tw, X + jc * BM_XR);
    }
    __syncthreads();
}

// grid (ceil(F / 2), streams), 512 threads
__global__ __launch_bounds__(512) void k_bmask_analyse_2048(BmaskStreamArgs p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *sub = reinterpret_cast<float2 *>(smem_raw);
    float2 *scr = sub + 16 * N512_ROW;
    float2 *X = scr;
    float2 *tab = scr + 8 * FFT_SCRATCH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.y, tb = blockIdx.x * BM_FPB_2048, nb = min(BM_FPB_2048, p.n_frames - tb);
    fft_table_init(tab, nullptr, tid, 512);
    float2 wreg[8];
    bm_window_2048(p.t.window, lane, wave & 1, wreg);
    __syncthreads();
    FftTw tw{tab};
    bm_forward_2048(p, s, tb, nb, wreg, sub, scr, X, tid, tw);
    for (int q = tid >> 3; q < nb * BM_BANDS; q += 64) {
        const int j = q / BM_BANDS, b = q - j * BM_BANDS;
        const float4 a = bm_band_sums(p.t, X + (j * 2) * BM_XR, X + (j * 2 + 1) * BM_XR, b, tid & 7);
        if ((tid & 7) == 0) p.sums[((long long)s * p.n_frames + tb + j) * BM_BANDS + b] = a;
    }
}

// grid (runs of ft frames, streams), 512 threads
__global__ __launch_bounds__(512) void k_bmask_synth_2048(BmaskStreamArgs p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int H = 1024, K = 1025;
    float2 *sub = reinterpret_cast<float2 *>(smem_raw);
    float *yt = reinterpret_cast<float *>(sub);                            // [2][2][BM_YT] time-domain frames (after the inverse)
    float2 *scr = sub + 16 * N512_ROW;
    float2 *X = scr;
    float2 *tab = scr + 8 * FFT_SCRATCH;
    float2 *gl = tab + TW_WIN;                                             // [2][48]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.y;
    const int t0 = blockIdx.x * p.ft, t1 = min(t0 + p.ft, p.n_frames);
    const int tbeg = t0 > 0 ? t0 - 1 : 0;
    const int jw = wave >> 2, cw = (wave >> 1) & 1, pr = wave & 1;
    fft_table_init(tab, nullptr, tid, 512);
    float2 wreg[8];
    bm_window_2048(p.t.window, lane, pr, wreg);
    float carry[2][2] = {{0.f, 0.f}, {0.f, 0.f}};                          // samples tid, tid + 512 of the hop, per channel
    if (t0 == 0) {
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) { carry[ch][0] = p.tail_in[((long long)s * 2 + ch) * H + tid]; carry[ch][1] = p.tail_in[((long long)s * 2 + ch) * H + tid + 512]; }
    }
    __syncthreads();
    FftTw tw{tab};

    for (int tb = tbeg; tb < t1; tb += BM_FPB_2048) {
        const int nb = min(BM_FPB_2048, t1 - tb);
        for (int e = tid; e < nb * BM_BANDS; e += 512) {
            const int j = e / BM_BANDS, b = e - j * BM_BANDS;
            gl[j * 48 + b] = p.gains[((long long)s * p.n_frames + tb + j) * BM_BANDS + b];
        }
        bm_forward_2048(p, s, tb, nb, wreg, sub, scr, X, tid, tw);
        for (int e = tid; e < nb * 2 * K; e += 512) {
            const int jc = e / K, k = e - jc * K;
            const float m = bm_bin_gain(p.t, gl + (jc >> 1) * 48, jc & 1, k);
            const float2 x = X[jc * BM_XR + k];
            X[jc * BM_XR + k] = make_float2(x.x * m, x.y * m);
        }
        __syncthreads();
        for (int e = tid; e < nb * 2 * 257; e += 512) {                     // the four sub-spectra of every masked spectrum
            const int jc = e / 257, m = e - jc * 257;
            float2 o4[4];
            split2048_inv(X + jc * BM_XR, m, p.t.tw, o4);
#pragma unroll
            for (int r = 0; r < 4; ++r) sub[(jc * 4 + r) * N512_ROW + m] = o4[r];
        }
        __syncthreads();
        float2 v[8];
        if (jw < nb) {
            const float2 *Ya = sub + ((jw * 2 + cw) * 4 + 2 * pr) * N512_ROW;
            irfft512_pair(Ya, Ya + N512_ROW, scr + wave * FFT_SCRATCH, v, lane, tw);
        }
        __syncthreads();                                                    // every wave has read its sub-spectra: yt may overwrite them
        if (jw < nb) {
            float *y = yt + (jw * 2 + cw) * BM_YT;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int n = lane + 64 * br3(i);
                *reinterpret_cast<float2 *>(y + 4 * n + 2 * pr) = v[i];     // y[4 n + 2 pr], y[4 n + 2 pr + 1]
            }
        }
        __syncthreads();
        for (int j = 0; j < nb; ++j) {
            const int t = tb + j;
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                const float *y = yt + (j * 2 + ch) * BM_YT;
                if (t >= t0) {
                    float *o = p.out + ((long long)s * 2 + ch) * (long long)p.n_frames * H + (long long)t * H;
                    o[tid] = carry[ch][0] + y[tid]; o[tid + 512] = carry[ch][1] + y[tid + 512];
                }
                carry[ch][0] = y[H + tid]; carry[ch][1] = y[H + tid + 512];
            }
        }
        __syncthreads();
    }
    if (t1 == p.n_frames) {
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            p.tail_out[((long long)s * 2 + ch) * H + tid] = carry[ch][0];
            p.tail_out[((long long)s * 2 + ch) * H + tid + 512] = carry[ch][1];
        }
    }
}

// ---------------------------------------------------------------------------------------
// any other power of two: one frame at a time on the block-cooperative transform of fft_block.h
// LDS: spec [2][H + 1] float2 | carry [2][H] | gl [48] float2
// ---------------------------------------------------------------------------------------
// grid (F, streams), 256 threads
__global__ __launch_bounds__(256) void k_bmask_analyse_gen(BmaskStreamArgs p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int logH = p.t.logH, H = 1 << logH, zs = H + 1;
    float2 *spec = reinterpret_cast<float2 *>(smem_raw);
    const int tid = threadIdx.x, NT = blockDim.x;
    const int s = blockIdx.y, t = blockIdx.x;
    const float *base = p.pcm + (long long)s * p.stream_stride;
    load_frames(spec, zs, 2, logH, base, p.ch_stride, (long long)t, p.t.window, tid, NT);
    block_fft_dit(spec, zs, 2, logH, p.t.tw, p.t.N, tid, NT);
    split_forward(spec, zs, 2, logH, p.t.tw, tid, NT);
    for (int b = tid >> 3; b < BM_BANDS; b += NT >> 3) {
        const float4 a = bm_band_sums(p.t, spec, spec + zs, b, tid & 7);
        if ((tid & 7) == 0) p.sums[((long long)s * p.n_frames + t) * BM_BANDS + b] = a;
    }
}

// grid (runs of ft frames, streams), 256 threads
__global__ __launch_bounds__(256) void k_bmask_synth_gen(BmaskStreamArgs p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int logH = p.t.logH, H = 1 << logH, K = H + 1, zs = H + 1;
    float2 *spec = reinterpret_cast<float2 *>(smem_raw);                  // [2][H + 1]
    float *carry = reinterpret_cast<float *>(spec + 2 * zs);              // [2][H]
    float2 *gl = reinterpret_cast<float2 *>(carry + 2 * H);               // [48]
    const int tid = threadIdx.x, NT = blockDim.x;
    const int s = blockIdx.y;
    const int t0 = blockIdx.x * p.ft, t1 = min(t0 + p.ft, p.n_frames);
    const int tbeg = t0 > 0 ? t0 - 1 : 0;
    for (int e = tid; e < 2 * H; e += NT) carry[e] = t0 == 0 ? p.tail_in[(long long)s * 2 * H + e] : 0.f;
    const float *base = p.pcm + (long long)s * p.stream_stride;
    const float sc = 1.0f / (float)H;

    for (int t = tbeg; t < t1; ++t) {
        if (tid < BM_BANDS) gl[tid] = p.gains[((long long)s * p.n_frames + t) * BM_BANDS + tid];
        load_frames(spec, zs, 2, logH, base, p.ch_stride, (long long)t, p.t.window, tid, NT);
        block_fft_dit(spec, zs, 2, logH, p.t.tw, p.t.N, tid, NT);
        split_forward(spec, zs, 2, logH, p.t.tw, tid, NT);
        for (int e = tid; e < 2 * K; e += NT) {
            const int ch = e / K, k = e - ch * K;
            const float m = bm_bin_gain(p.t, gl, ch, k);
            const float2 x = spec[ch * zs + k];
            spec[ch * zs + k] = make_float2(x.x * m, x.y * m);
        }
        __syncthreads();
        // one-sided spectra -> packed Z (imaginary parts of DC and Nyquist ignored), inverse transform
        for (int e = tid; e < 2 * (H / 2 + 1); e += NT) {
            const int ch = e / (H / 2 + 1), k = e - ch * (H / 2 + 1);
            float2 *yy = spec + ch * zs;
            float2 xk = yy[k], xp = yy[H - k];
            if (k == 0) { xk.y = 0.f; xp.y = 0.f; }
            const float2 ev = make_float2(0.5f * (xk.x + xp.x), 0.5f * (xk.y - xp.y));
            const float2 df = make_float2(0.5f * (xk.x - xp.x), 0.5f * (xk.y + xp.y));
            const float2 od = cmulc(df, p.t.tw[k]);
            yy[k] = make_float2(ev.x - od.y, ev.y + od.x);
            if (k != 0 && k != H - k) yy[H - k] = make_float2(ev.x + od.y, -ev.y + od.x);
        }
        __syncthreads();
        block_ifft_dif(spec, zs, 2, logH, p.t.tw, p.t.N, tid, NT);
        for (int e = tid; e < 2 * (H / 2); e += NT) {
            const int ch = e / (H / 2), n = e - ch * (H / 2);
            const float2 lo = spec[ch * zs + (int)(__brev((unsigned)n) >> (32 - logH))];
            const float2 hi = spec[ch * zs + (int)(__brev((unsigned)(n + H / 2)) >> (32 - logH))];
            float *cr = carry + ch * H + 2 * n;
            if (t >= t0) {
                float *o = p.out + ((long long)s * 2 + ch) * (long long)p.n_frames * H + (long long)t * H + 2 * n;
                o[0] = cr[0] + lo.x * sc; o[1] = cr[1] + lo.y * sc;
            }
            cr[0] = hi.x * sc; cr[1] = hi.y * sc;
        }
        __syncthreads();
    }
    if (t1 == p.n_frames)
        for (int e = tid; e < 2 * H; e += NT) p.tail_out[(long long)s * 2 * H + e] = carry[e];
}

// ---------------------------------------------------------------------------------------
// the recursion over frames: block = stream (BM_SCAN_THREADS threads: the loads and the cells of a chunk are spread over all of
// them, a single workgroup being all that one stream has), chunks of BM_SCAN_CHUNK frames through LDS.  Only Q is sequential: thread = band
// walks the chunk's P values in order (the same recursion whatever the chunking or the call split: Q lives in memory between
// calls); the decisions and gains of the chunk's (frame, band) cells are then formed by all threads from the Q of their frame.
// Q is a double, as in the definition (Q = Q (double)0.04f + (double)(1 - 0.04f) P): 45 threads per stream carry it, and a
// band that falls silent keeps a Q above 0 (and so its temporal decision) for as long as the double twin's does.
// ---------------------------------------------------------------------------------------
constexpr int BM_SCAN_CHUNK = 48;

__global__ __launch_bounds__(BM_SCAN_THREADS) void k_bmask_scan(BmaskScanArgs p)
{
    __shared__ float4 sm[BM_SCAN_CHUNK * BM_BANDS];        // mean(l^2), mean(r^2), mean(l r), P
    __shared__ double sq[BM_SCAN_CHUNK * BM_BANDS];        // Q after each frame
    const int tid = threadIdx.x, s = blockIdx.x;
    double Q = tid < BM_BANDS ? p.Q[s * BM_BANDS + tid] : 0.0;
    const long long row0 = (long long)s * p.n_frames * BM_BANDS;
    for (int t0 = 0; t0 < p.n_frames; t0 += BM_SCAN_CHUNK) {
        const int nc = min(BM_SCAN_CHUNK, p.n_frames - t0), cells = nc * BM_BANDS;
        const long long base = row0 + (long long)t0 * BM_BANDS;
        for (int e = tid; e < cells; e += BM_SCAN_THREADS) sm[e] = p.sums[base + e];
        __syncthreads();
        if (tid < BM_BANDS) {
#pragma unroll 8
            for (int j = 0; j < nc; ++j) {
                Q = Q * p.lambda + p.one_minus_lambda * (double)sm[j * BM_BANDS + tid].w;     // temportalMasking: Q[m] = lambda Q[m-1] + (1 - lambda) P[m]
                sq[j * BM_BANDS + tid] = Q;
            }
        }
        __syncthreads();
        for (int e = tid; e < cells; e += BM_SCAN_THREADS) {
            const int b = e % BM_BANDS;
            const float4 m = sm[e];
            const double Qn = sq[e];
            const bool temp = (double)m.w < Qn;                  // the compare takes the updated Q
            const float den = sqrtf(m.x) * sqrtf(m.y);           // normaliseCorrelation
            const float nc_ = den == 0.f ? 1.f : m.z / den;
            const bool spat = nc_ < p.thr[b];
            const int dec = spat ? 2 : (temp ? 1 : 0);
            float gL = p.enhance, gR = p.enhance;
            if (dec != 0) {
                if (p.method == 3) gL = gR = 1.f / 1000.f;                                   // FULL: zeroFrame
                else if (p.method == 0) gL = gR = dec == 2 ? p.inv_spatial : p.inv_temporal;  // FACTOR
                else {                                                                       // RELATIVE, per channel, updated Q
                    double fl = (double)(p.rho * m.x), fr = (double)(p.rho * m.y);
                    if (Qn < 1e-10) { fl = (double)p.rho; fr = (double)p.rho; } else { fl /= Qn; fr /= Qn; }
                    gL = sqrtf((float)fl); gR = sqrtf((float)fr);
                }
            }
            p.gains[base + e] = make_float2(gL, gR);
            if (p.decisions) p.decisions[base + e] = dec;
        }
        __syncthreads();
    }
    if (tid < BM_BANDS) p.Q[s * BM_BANDS + tid] = Q;
    if (tid == 0) p.frames[s] += p.n_frames;
}

// ---------------------------------------------------------------------------------------
// frame hooks, double
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double bm_block_sum(double v, double *sred)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) sred[wave] = v;
    __syncthreads();
    double r = sred[0];
    for (int w = 1; w < nw; ++w) r += sred[w];
    return r;
}

// frameAnalysis: band b = the circular convolution of the frame with h_b = irfft(H_b).  grid (W / 256, n_bands), 256 threads;
// W is a power of two >= 256.
__global__ __launch_bounds__(256) void k_bmask_hook_analysis(const double *x, const double *h, double *analysis, int W, int n_bands)
{
    const int n = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (n >= W || b >= n_bands) return;
    const double *hb = h + (long long)b * W;
    double acc = 0;
    for (int m = 0; m < W; ++m) acc += hb[(n - m) & (W - 1)] * x[m];
    analysis[(long long)b * W + n] = acc;
}

// slot 45: the frame minus its 45 bands
__global__ __launch_bounds__(256) void k_bmask_hook_residual(const double *x, double *analysis, int W)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= W) return;
    double acc = 0;
    for (int b = 0; b < BM_BANDS; ++b) acc += analysis[(long long)b * W + n];
    analysis[(long long)BM_BANDS * W + n] = x[n] - acc;
}

// processParametrisation: block = band, 256 threads
__global__ __launch_bounds__(256) void k_bmask_hook_param(BmaskHookArgs p)
{
    __shared__ double sred[4];
    __shared__ double sg[2];
    __shared__ int sdec;
    const int tid = threadIdx.x, b = blockIdx.x, W = p.W;
    double *l = p.L + (long long)b * W, *r = p.R + (long long)b * W;
    double s_ll = 0, s_rr = 0, s_lr = 0, s_mix = 0;
    for (int n = tid; n < W; n += 256) {
        const double a = l[n], c = r[n], m = (a + c) / 2;
        s_ll += a * a; s_rr += c * c; s_lr += a * c; s_mix += m * m;
    }
    s_ll = bm_block_sum(s_ll, sred); s_rr = bm_block_sum(s_rr, sred); s_lr = bm_block_sum(s_lr, sred); s_mix = bm_block_sum(s_mix, sred);
    if (tid == 0) {
        const double dW = (double)W, P = s_mix / dW, mll = s_ll / dW, mrr = s_rr / dW;
        const double Q = p.Q[b] * p.lambda + p.one_minus_lambda * P;
        p.Q[b] = Q;
        const bool temp = P < Q;
        const double den = sqrt(mll) * sqrt(mrr);
        const double nc = den == 0 ? 1.0 : (s_lr / dW) / den;
        const bool spat = nc < p.thr[b];
        const int dec = spat ? 2 : (temp ? 1 : 0);
        double gL = 0, gR = 0;                                 // RELATIVE only
        if (dec != 0 && p.method == 1) {
            double fl = mll * p.rho, fr = mrr * p.rho;
            if (Q < 1e-10) { fl = p.rho; fr = p.rho; } else { fl /= Q; fr /= Q; }
            gL = sqrt(fl); gR = sqrt(fr);
        }
        sg[0] = gL; sg[1] = gR; sdec = dec;
        if (p.decisions) p.decisions[b] = dec;
    }
    __syncthreads();
    const int dec = sdec;
    const double gL = sg[0], gR = sg[1];
    for (int n = tid; n < W; n += 256) {
        if (dec == 0) { l[n] *= p.enhance; r[n] *= p.enhance; }
        else if (p.method == 3) { l[n] /= 1000.0; r[n] /= 1000.0; }
        else if (p.method == 0) { const double f = dec == 2 ? p.spatial : p.temporal; l[n] /= f; r[n] /= f; }
        else { l[n] *= gL; r[n] *= gR; }
    }
}

// frameSynthesis, the literal loop: slots 0, 1, ... while slot <= 45 and slot * W < analysis_length - W
__global__ __launch_bounds__(256) void k_bmask_hook_synth(double *out, const double *analysis, int W, int analysis_length)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= W) return;
    double acc = 0;
    long long offset = 0;
    for (int bin = 0; bin <= BM_BANDS && offset < (long long)analysis_length - W; ++bin, offset += W) acc += analysis[offset + n];
    out[n] = acc;
}

}  // namespace mca
