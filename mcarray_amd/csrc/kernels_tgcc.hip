// kernels_tgcc.hip -- TemporalGCCBinauralLocalisation (src/mcarray/BinauralLocalisation.cpp:134-314) for batches of frames
// (gfx950), all in double.
//
//   k_tgcc_frames  one workgroup per (array, frame): the frame's two channels in LDS (float, zero-padded), the nd delay
//                  pairs' 2nd+1-lag cross-correlations in closed form, the deviations, index[] (:156-167), + tri, max-min
//                  normalisation, first-max pick, DOA and log-likelihood (:169-174); the frame's logPower and the
//                  energies the power-floor estimation needs.  Nothing here depends on the array's state.
//   k_tgcc_gate    one thread per array: the floor estimation, the gate and the _currentDOA / _prob recursion
//                  (:141-191) over the call's frames in order.
//
// Closed form (DESIGN.md [BUILD-DEFINES]): pair i delays channel 0 by i and channel 1 by nd - i; with the IPP convention
// c_i[n] = sum_m L_i[m] R_i[m + n - nd] this is c_i[n] = sum_p L[p] R[p + tau], tau = n + 2i - 2nd in [-2nd, 2nd - 2],
// p over [max(0, -tau), min(W-1-i, W-1-nd+i-tau)].  So each of the 4nd - 1 lags has one body sum B(tau) over the full
// overlap [max(0, -tau), W-1-max(tau, 0)], and each (i, n) drops the tail past its own upper end (< 3 nd products).
//
// Fixed reduction order: per-thread partial sums over a p-partition that depends on TG_THREADS only, a fixed shuffle tree,
// the waves summed in order; tails and the per-pair abs-sums run sequentially in one thread.  A frame's bits depend on its
// samples only (not on the batch, the call split or the frame's position in the call).
#include "mca_internal.h"

namespace mca {

constexpr int TG_THREADS = 256, TG_WAVES = TG_THREADS / 64;
constexpr int TG_PB = 8;       // p values per tile
constexpr int TG_G = 16;       // lags per tile
constexpr int TG_RW = TG_PB + TG_G - 1;

// sum over the block of NV doubles per thread; returns the totals in red[0..NV-1] (valid after the trailing barrier)
template <int NV>
__device__ __forceinline__ void tg_block_sum(double (&v)[NV], double *red_waves, double *red)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        double x = v[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        v[j] = x;
    }
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < NV; ++j) red_waves[wave * NV + j] = v[j];
    __syncthreads();
    if (tid < NV) {
        double s = red_waves[tid];
        for (int w = 1; w < TG_WAVES; ++w) s += red_waves[w * NV + tid];
        red[tid] = s;
    }
    __syncthreads();
}

// one tile's operands, as doubles: l[k] = L[p0 + k], r[u] = R[r0 + u].  LDS floats: 16-byte reads (p0 is a multiple of 8, r0
// of 4; a lane's run of 32 bytes keeps the 64 banks free of conflicts); the hook's global doubles: plain loads.
__device__ __forceinline__ void tg_load_tile(const float *L, const float *R, int p0, int r0, double (&l)[TG_PB], double (&r)[TG_RW])
{
    const float4 *l4 = reinterpret_cast<const float4 *>(L + p0);
    const float4 *r4 = reinterpret_cast<const float4 *>(R + r0);
    float lf[8], rf[24];
#pragma unroll
    for (int q = 0; q < 2; ++q) { const float4 v = l4[q]; lf[4 * q] = v.x; lf[4 * q + 1] = v.y; lf[4 * q + 2] = v.z; lf[4 * q + 3] = v.w; }
#pragma unroll
    for (int q = 0; q < 6; ++q) { const float4 v = r4[q]; rf[4 * q] = v.x; rf[4 * q + 1] = v.y; rf[4 * q + 2] = v.z; rf[4 * q + 3] = v.w; }
#pragma unroll
    for (int k = 0; k < TG_PB; ++k) l[k] = (double)lf[k];
#pragma unroll
    for (int u = 0; u < TG_RW; ++u) r[u] = (double)rf[u];
}
__device__ __forceinline__ void tg_load_tile(const double *L, const double *R, int p0, int r0, double (&l)[TG_PB], double (&r)[TG_RW])
{
#pragma unroll
    for (int k = 0; k < TG_PB; ++k) l[k] = L[p0 + k];
#pragma unroll
    for (int u = 0; u < TG_RW; ++u) r[u] = R[r0 + u];
}

// A thread's partial channel statistics about the shifts sl, sr (m as in tgcc_frame_core), for the hook's global frame.
template <typename T>
__device__ void tg_stats_partial(const T *L, const T *R, int W, int rem, double sl, double sr, double (&m)[7])
{
    for (int p = threadIdx.x; p < W; p += TG_THREADS) {
        const double l = (double)L[p], r = (double)R[p], dl = l - sl, dr = r - sr;
        m[0] += dl; m[1] += dl * dl; m[2] += dr; m[3] += dr * dr; m[4] += l * l; m[5] += r * r;
        if (p < rem) m[6] += l * l + r * r;
    }
}

// The per-frame stage on padded channels: L[p] for p in [0, W8) (0 past W), R[j] for j in [-TGCC_RPAD_FRONT, W8 + TGCC_RPAD_BACK)
// (0 outside [0, W)).  T = float (LDS copy of the PCM) or double (the frame hook's global copy).  LDS scratch `ws` as laid out
// in tgcc_frame_ws_doubles.  m = this thread's partial sums sum (L - sl), sum (L - sl)^2, sum (R - sr), sum (R - sr)^2,
// sum L^2, sum R^2, sum_{p < rem} (L^2 + R^2): the deviations below are exact for any shift, and a sample of the frame as the
// shift keeps them clear of cancellation under a DC offset.  Writes res[TGCC_RES] and, if index_out, the normalised index[nd].
template <typename T>
__device__ void tgcc_frame_core(const T *__restrict__ L, const T *__restrict__ R, int W, int nd, int rem, double (&m)[7], double sl,
                                double sr, double *ws, double *res, double *index_out)
{
    const int tid = threadIdx.x;
    // the lag grid starts at -2nd - o (o = 2 for odd nd): every tile's first channel-1 sample is a multiple of 4
    const int o = (2 * nd) & 2, NL = 4 * nd - 1 + o, NG = (NL + TG_G - 1) / TG_G, W8 = (W + TG_PB - 1) / TG_PB * TG_PB, NB = W8 / TG_PB;
    const int NC = 2 * nd + 1;
    double *sB = ws;                               // [NG * TG_G] body sums B(tau), tau = -2nd - o + slot
    double *sRedW = sB + 8 * TG_G;                 // [TG_WAVES][TG_G]
    double *sRed = sRedW + TG_WAVES * TG_G;        // [TG_G]
    double *sScale = sRed + TG_G;                  // [nd]
    double *sIdx = sScale + TGCC_MAX_ND;           // [nd]
    double *sStat = sIdx + TGCC_MAX_ND;            // [8] block totals of m
    double *sC = sStat + 8;                        // [nd][2nd+1] |c_i[n]|, scaled

    // ---- channel statistics (the deviations of the delayed frames, the energies): reduced first, so that m is not live
    //      across the body loop
    tg_block_sum<7>(m, sRedW, sRed);
    if (tid < 7) sStat[tid] = sRed[tid];

    // ---- body sums, TG_G lags at a time
    for (int g = 0; g < NG; ++g) {
        const int tau0 = -2 * nd - o + g * TG_G;
        double acc[TG_G];
#pragma unroll
        for (int j = 0; j < TG_G; ++j) acc[j] = 0.0;
        for (int b = tid; b < NB; b += TG_THREADS) {
            const int p0 = b * TG_PB;
            double l[TG_PB], r[TG_RW];
            tg_load_tile(L, R, p0, p0 + tau0, l, r);
#pragma unroll
            for (int j = 0; j < TG_G; ++j)
#pragma unroll
                for (int k = 0; k < TG_PB; ++k) acc[j] = fma(l[k], r[k + j], acc[j]);
        }
        tg_block_sum<TG_G>(acc, sRedW, sRed);
        if (tid < TG_G) sB[g * TG_G + tid] = sRed[tid];
    }

    const double e_part = sStat[6];

    // ---- divisor of pair i: stddev(L delayed by i) * stddev(R delayed by nd - i), denominator W - 1 over all W samples
    if (tid < nd) {
        const int i = tid;
        double a1 = sStat[0], a2 = sStat[1];
#pragma unroll 4
        for (int p = W - i; p < W; ++p) { const double d = (double)L[p] - sl; a1 -= d; a2 -= d * d; }
        a1 -= (double)i * sl; a2 += (double)i * sl * sl;           // the i leading zeros
        double b1 = sStat[2], b2 = sStat[3];
#pragma unroll 4
        for (int p = W - (nd - i); p < W; ++p) { const double d = (double)R[p] - sr; b1 -= d; b2 -= d * d; }
        b1 -= (double)(nd - i) * sr; b2 += (double)(nd - i) * sr * sr;
        const double vl = fmax((a2 - a1 * a1 / (double)W) / (double)(W - 1), 0.0);
        const double vr = fmax((b2 - b1 * b1 / (double)W) / (double)(W - 1), 0.0);
        sScale[i] = sqrt(vl) * sqrt(vr);
    }
    const double e_full = sStat[4] + sStat[5];
    __syncthreads();

    // ---- c_i[n] = B(tau) - tail, / divisor, |.|
    for (int q = tid; q < nd * NC; q += TG_THREADS) {
        const int i = q / NC, n = q - i * NC, tau = n + 2 * i - 2 * nd;
        const int full_hi = W - 1 - max(tau, 0);
        const int hi = min(W - 1 - i, W - 1 - nd + i - tau);
        double t = 0.0;
#pragma unroll 4
        for (int p = hi + 1; p <= full_hi; ++p) t = fma((double)L[p], (double)R[p + tau], t);
        double c = sB[tau + 2 * nd + o] - t;
        const double s = sScale[i];
        if (s != 0.0) c = c / s;                   // ippsDivC refuses a zero divisor: the division is skipped
        sC[q] = fabs(c);
    }
    __syncthreads();
    if (tid < nd) {
        double s = 0.0;
        for (int n = 0; n < NC; ++n) s += sC[tid * NC + n];
        sIdx[tid] = s + 0.1 * (1.0 - fabs(2.0 * (double)tid - (double)nd) / (double)nd);   // index + tri (:169)
    }
    __syncthreads();
    if (tid == 0) {
        double mn = sIdx[0];
        for (int i = 1; i < nd; ++i) mn = fmin(mn, sIdx[i]);
        double mx = sIdx[0] + mn;
        for (int i = 0; i < nd; ++i) { sIdx[i] = sIdx[i] + mn; mx = fmax(mx, sIdx[i]); }   // maxminNormalisation adds the minimum
        int k = 0;
        double best = -1.0, sum_abs = 0.0;
        for (int i = 0; i < nd; ++i) {
            const double x = sIdx[i] / mx;
            sIdx[i] = x;
            if (x > best) { best = x; k = i; }                                 // first maximum
            sum_abs += fabs(x);
        }
        const double shift = (double)(nd - 1) / 2;
        const double doa = acos(2 * ((double)k - shift) / (nd - 1)) * 180 / M_PI - 90;   // samples2Degrees - 90 (:173, :277-284)
        const double prob = sIdx[k] != 0 ? log(sIdx[k] / (sum_abs + 0.000001)) : log(0.0000000001);   // :111-132
        res[0] = doa; res[1] = prob; res[2] = (double)k;
        res[3] = 10.0 * log10(e_full / (2.0 * (double)W));                   // logPower over both channels
        res[4] = e_full; res[5] = e_part;
    }
    __syncthreads();
    if (index_out)
        for (int i = tid; i < nd; i += TG_THREADS) index_out[i] = sIdx[i];
}

// grid (n_frames, n_arrays), TG_THREADS threads.  LDS: L [W8] float, R [RPAD_FRONT + W8 + RPAD_BACK] float, then the scratch.
__global__ __launch_bounds__(TG_THREADS) void k_tgcc_frames(TgccFrameArgs p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int W = p.W, W8 = (W + TG_PB - 1) / TG_PB * TG_PB, RL = TGCC_RPAD_FRONT + W8 + TGCC_RPAD_BACK;
    double *ws = reinterpret_cast<double *>(smem_raw);
    float *sL = reinterpret_cast<float *>(ws + tgcc_frame_ws_doubles(p.nd));
    float *sR = sL + W8;
    const int a = blockIdx.y, f = blockIdx.x, tid = threadIdx.x;
    const long long row = (long long)a * p.n_frames + f;
    const float *gl = p.pcm + (long long)a * p.array_stride + (long long)f * p.hop;
    const float *gr = gl + p.ch_stride;
    // 8 + 8 independent loads in flight per thread and pass (a load-then-store loop waits out the memory latency per sample);
    // the channel statistics on the way, about each channel's first sample
    const double sl = (double)gl[0], sr = (double)gr[0];
    double m[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    constexpr int U = 8;
    for (int j0 = 0; j0 < RL; j0 += U * TG_THREADS) {
        float vl[U], vr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * TG_THREADS + tid, q = j - TGCC_RPAD_FRONT;
            vl[u] = j < W ? gl[j] : 0.f;
            vr[u] = (q >= 0 && q < W) ? gr[q] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * TG_THREADS + tid, q = j - TGCC_RPAD_FRONT;
            if (j < W8) sL[j] = vl[u];
            if (j < RL) sR[j] = vr[u];
            if (j < W) {
                const double l = (double)vl[u], d = l - sl;
                m[0] += d; m[1] += d * d; m[4] += l * l;
                if (j < p.rem) m[6] += l * l;
            }
            if (q >= 0 && q < W) {
                const double r = (double)vr[u], d = r - sr;
                m[2] += d; m[3] += d * d; m[5] += r * r;
                if (q < p.rem) m[6] += r * r;
            }
        }
    }
    __syncthreads();
    tgcc_frame_core<float>(sL, sR + TGCC_RPAD_FRONT, W, p.nd, p.rem, m, sl, sr, ws, p.res + row * TGCC_RES,
                           p.index ? p.index + row * p.nd : nullptr);
}

// the frame hook: one frame already padded in global memory (double), grid 1
__global__ __launch_bounds__(TG_THREADS) void k_tgcc_frame_f64(const double *Lp, const double *Rp, int W, int nd, int rem, double *res,
                                                              double *index)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const double *R = Rp + TGCC_RPAD_FRONT, sl = Lp[0], sr = R[0];
    double m[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    tg_stats_partial(Lp, R, W, rem, sl, sr, m);
    tgcc_frame_core<double>(Lp, R, W, nd, rem, m, sl, sr, reinterpret_cast<double *>(smem_raw), res, index);
}

// grid ceil(n_arrays / 64), 64 threads: thread a walks array a's frames in order (BinauralLocalisation.cpp:141-191).
__global__ __launch_bounds__(64) void k_tgcc_gate(TgccGateArgs p)
{
    const int a = blockIdx.x * 64 + threadIdx.x;
    if (a >= p.n_arrays) return;
    double *st = p.state + (long long)a * TGCC_STATE;
    double cur = st[0], prob = st[1], floor_acc = st[2];
    long long consumed = (long long)st[3];
    bool est = st[4] != 0.0;
    for (int f = 0; f < p.n_frames; ++f) {
        const long long row = (long long)a * p.n_frames + f;
        const double *r = p.res + row * TGCC_RES;
        double power;
        if (p.use_floor && !est) {                                               // setPowerFloor (:286-314)
            const int n = (int)min((long long)p.needed - consumed, (long long)p.W);
            const double e = n == p.W ? r[4] : r[5];
            floor_acc += e / (2.0 * (double)n) * (double)n;                      // power(first n samples) * n
            consumed += n;
            if (consumed >= p.needed) {
                est = true;
                floor_acc /= (double)consumed;
                floor_acc = 0.15 * (100 - floor_acc) + floor_acc;
            }
            power = floor_acc;
        } else {
            power = r[3];
        }
        const bool voiced = !p.use_floor || power > floor_acc;
        if (voiced) {
            prob = r[1];
            cur = cur * 0.5 + (1 - 0.5) * r[0];                                  // _doaMemoryFactor (:175)
        } else {
            cur = cur * 0.5 + (1 - 0.8) * 0;                                     // :180-181
            prob = -100000;
        }
        if (p.doa_deg) p.doa_deg[row] = (float)cur;
        if (p.prob) p.prob[row] = (float)prob;
        if (p.power) p.power[row] = (float)power;
        if (p.voiced) p.voiced[row] = voiced ? 1 : 0;
        if (p.delay_idx) p.delay_idx[row] = voiced ? (int)r[2] : -1;
        if (p.out_f64) {                                                         // frame hook: {voiced, doa, prob, power, k}
            double *o = p.out_f64 + row * 5;
            o[0] = voiced ? 1.0 : 0.0; o[1] = cur; o[2] = prob; o[3] = power; o[4] = voiced ? r[2] : -1.0;
        }
    }
    st[0] = cur; st[1] = prob; st[2] = floor_acc; st[3] = (double)consumed; st[4] = est ? 1.0 : 0.0;
}

}  // namespace mca
