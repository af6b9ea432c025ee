// kernels_mvdr_postfilter.hip -- the decision-directed Wiener post-filter on the beamformed spectra (gfx950; include/mcarray_hip.h,
// mca_hip_mvdr_set_postfilter).  It runs between the solve (k_mvdr_solve_t<..., NOISE = true>, which leaves Y and the residual noise
// power 1 / (d^H PhiL^-1 d) of every output) and k_mvdr_synth, and rewrites Y in place.
//
// Per stream a, slot s, bin k and frame t, with p = noise_scale * pn (pn == 0: the bin is digitally silent so far):
//     N = smoothing A + (1 - smoothing) max(|Y|^2 - p, 0),   G = p == 0 ? 1 : fmaxf(gain_floor, N / (N + p)),   Z = G Y,   A <- |Z|^2
// One thread per (a, s, k), bins fastest: the loads of Y (8 B), pn (4 B) and A of a wave are contiguous.  The frames are a
// sequential recursion through A, so a thread runs them in order with the loads of the next PF_DEPTH frames in flight ahead of the
// dependent arithmetic.  20 B of traffic per cell and the state once each way; no LDS, no atomics: the result is a function of
// the input and the state alone, and does not depend on how a stream is cut into calls (A carries everything).
// Every product and sum is written out (fmaf where one is meant), so the compiler's contraction has nothing to decide; the
// division is the correctly rounded one.  gain_floor == 1 gives G == 1 exactly (N / (N + p) <= 1, a NaN loses against 1 in fmaxf)
// and 1 * Y is Y.
#include "mca_internal.h"

namespace mca {

constexpr int PF_DEPTH = 4;   // frames loaded ahead

__global__ __launch_bounds__(256) void k_mvdr_postfilter(MvdrPostfilterArgs p)
{
    const int K = p.K, F = p.n_frames, S = p.S;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)p.n_streams * S * K) return;
    const long long as = id / K;                                   // a S + s
    const int k = (int)(id - as * K);
    const int a = (int)(as / S), s = (int)(as - (long long)a * S);
    float2 *Y = p.Y + as * F * K + k;                              // + t K
    const float *pn = p.pn + as * F * K + k;
    float *Ap = p.A + ((long long)a * p.slots + s) * K + k;
    const float sm = p.smoothing, oms = p.one_minus_smoothing, fl = p.gain_floor, ns = p.noise_scale;

    float2 yb[PF_DEPTH];
    float pb[PF_DEPTH];
#pragma unroll
    for (int i = 0; i < PF_DEPTH; ++i) {
        const bool in = i < F;
        yb[i] = in ? Y[(long long)i * K] : make_float2(0.f, 0.f);
        pb[i] = in ? pn[(long long)i * K] : 0.f;
    }
    float A = *Ap;
    for (int t0 = 0; t0 < F; t0 += PF_DEPTH) {
#pragma unroll
        for (int i = 0; i < PF_DEPTH; ++i) {
            const int t = t0 + i;
            if (t < F) {
                const float2 y = yb[i];
                const float pw = ns * pb[i];
                if (t + PF_DEPTH < F) {
                    yb[i] = Y[(long long)(t + PF_DEPTH) * K];
                    pb[i] = pn[(long long)(t + PF_DEPTH) * K];
                }
                const float e = fmaf(y.x, y.x, y.y * y.y);
                const float N = fmaf(sm, A, oms * fmaxf(e - pw, 0.f));
                const float G = pw == 0.f ? 1.f : fmaxf(fl, N / (N + pw));
                const float2 z = make_float2(G * y.x, G * y.y);
                A = fmaf(z.x, z.x, z.y * z.y);
                Y[(long long)t * K] = z;
            }
        }
    }
    *Ap = A;
}

}  // namespace mca
