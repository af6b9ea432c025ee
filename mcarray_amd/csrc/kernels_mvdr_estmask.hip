// kernels_mvdr_estmask.hip -- the update mask and the target masks of an MVDR call, estimated from the call's own spectra (gfx950;
// include/mcarray_hip.h, mca_hip_mvdr_set_mask_estimator).  k_mvdr_estmask runs between the analysis and k_mvdr_rtf / the
// solve of mca_hip_mvdr_sources_frames_auto_*, which read the masks it writes the way they read a caller's.
//
// Per stream a, frame t and bin k, with x the frame's M spectra of the bin and g_s = cmul(T_hi, T_lo) the geometric steering vector of
// doa[a][t][s] (mvdr_steer_rows: the bits the solve forms), s = 0 ... S-1:
//     e   = sum_m |x_m|^2
//     c_s = |g_s^H x|^2 / (M e)                  0 for every s where e <= 1e-30
//     w   = the s with the largest c_s, searched upwards with a strict '>' (ties and NaNs stay with the lower index)
//     v   = fminf(fmaxf((c_w - lo) / (hi - lo), 0), 1)                                    (a NaN counts as 0)
//     target_mask[a][s][t][k] = s == w ? v : 0,      update_mask[a][t][k] = w < P ? 1 - v : 1
// and target 0, update 1 in every cell outside the band [bin_lo, bin_hi].
//
// The layout is the solve's: FOUR lanes per cell, lane l of a quad owns the microphones l, l + 4, ...; the two reductions (e and
// g_s^H x) are quad sums (DPP).  Consecutive quads take consecutive bins of a frame, so a wave reads 16 cells x M spectra that lie
// behind one another (2 KiB at 16 microphones) and, per look direction, 16 consecutive low-order phasors of each of its rows; the
// tables T of a frame (12.5 KB at 16 microphones, two directions, N = 1024) are read by the 513 cells of the frame and stay in the
// cache.  Lane s of the quad stores target mask s, lane 0 the update mask as well: (S + 1) floats per cell, 64 B runs per wave and
// mask.  No LDS, no atomics, no state: a cell is a function of its own spectra and of the frame's look directions, so where a
// stream sits in the batch and how it is cut into calls do not change bytes.  Every sum is written out (fmaf where one is meant)
// and the complex products are the helpers of fft512.h; the divisions are the correctly rounded ones.
#include "fft512.h"
#include "mca_internal.h"
#include "mvdr_solve.h"

namespace mca {

// grid (ceil(streams * n_frames * K / 64)), 256 threads
template <int Q>
__global__ __launch_bounds__(256) void k_mvdr_estmask(MvdrEstmaskArgs p)
{
    static_assert(MCA_MAX_SOURCES <= 4, "lane s of a quad stores target mask s");
    const int tid = threadIdx.x, l = tid & 3;
    const int M = p.M, K = p.K, F = p.n_frames, S = p.S;
    const long long total = (long long)p.n_streams * F * K;
    const long long pid = (long long)blockIdx.x * 64 + (tid >> 2);
    const bool pv = pid < total;
    const long long pc = pv ? pid : total - 1;    // surplus quads shadow the last cell and store nothing
    const long long at = pc / K;                   // a F + t
    const int k = (int)(pc - at * K), a = (int)(at / F), t = (int)(at - (long long)a * F);
    const bool band = k >= p.bin_lo && k <= p.bin_hi;

    int w = 0;
    float v = 0.f;
    if (band) {
        float2 x[Q];
        const float2 *X = p.X + pc * M + l;
#pragma unroll
        for (int q = 0; q < Q; ++q) x[q] = (4 * q + l < M) ? X[4 * q] : make_float2(0.f, 0.f);
        float e = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) e = fmaf(x[q].x, x[q].x, fmaf(x[q].y, x[q].y, e));
        e = quad_sum(e);
        const int nhi = ((K - 1) >> 5) + 1, nph = nhi + 32;
        const float2 *T = p.T + (long long)a * F * S * M * nph + (k >> 5);
        const int lo_off = nhi - (k >> 5) + (k & 31);
        const bool live = e > 1e-30f;
        const float den = (float)M * e;
        float best = 0.f;
        for (int s = 0; s < S; ++s) {
            float2 g[Q];
            mvdr_steer_rows<Q, false>(g, T, (long long)t * S + s, M, nph, lo_off, l);
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int q = 0; q < Q; ++q) acc = cmacc(acc, x[q], g[q]);          // + x_m conj(g_m): g^H x over the rows of this lane
            acc = make_float2(quad_sum(acc.x), quad_sum(acc.y));
            const float c = live ? fmaf(acc.x, acc.x, acc.y * acc.y) / den : 0.f;
            if (s == 0) best = c;
            else if (c > best) { best = c; w = s; }
        }
        v = fminf(fmaxf((best - p.coherence_lo) / p.coherence_span, 0.f), 1.f);      // NaN -> 0
    }
    if (pv) {
        if (l < S && p.target) p.target[(((long long)a * S + l) * F + t) * K + k] = l == w ? v : 0.f;
        if (l == 0) p.update[pc] = w < p.n_protected ? 1.f - v : 1.f;
    }
}

const void *mvdr_estmask_kernel(int Q)
{
    const void *k[4] = {(const void *)k_mvdr_estmask<1>, (const void *)k_mvdr_estmask<2>, (const void *)k_mvdr_estmask<3>, (const void *)k_mvdr_estmask<4>};
    return Q >= 1 && Q <= 4 ? k[Q - 1] : nullptr;
}

}  // namespace mca
