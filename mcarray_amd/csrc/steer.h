// steer.h -- delay-and-sum on the HALF spectrum of the separated channels (Beamformer.cpp:51-71), for the kernels that hold
// 2 X_a, 2 X_b of a channel pair per bin anyway (k_stft_phat_wave<..., FUSE> and its patch pass k_steer_patch).
//
//   Y[k] = (1/M) sum_c X_c[k] P_c[k],  k = 0..512;   y = IDFT of its Hermitian extension
//        = Re IDFT_1024(A),  A[0] = Y[0], A[k] = 2 Y[k] (0 < k < 512), A[512] = Y[512], A[k > 512] = 0.
// The table (k_steer_table) carries P_c[k] / (M N), so that the doubled spectra 2 X_c the mirror separation yields accumulate A
// directly (bin 0 is halved at the end); the Nyquist bin (real: Re Z = X_a, Im Z = X_b) is one real term per channel and
// enters after the transform as A[512] (-1)^n.  Both callers go through these two routines and nothing else, in one
// operation order: a hop's bits do not depend on which of them produced it.
#pragma once
#include "fft1024c.h"

namespace mca {

// The steering phasor of channel c at the lane's bin k = lam + 64 s factors into P_c[lam] P_c[64 s]: a per-lane base B (one 16-byte
// load per pair: B_a, B_b, with the 1 / (M N) in it) and a wave-uniform step Q_c[s] (eight per channel, Q_c[0] = 1) -- no per-bin
// steering loads behind the sample loads of the next pair, whose latency a wait on them would expose (loads return in order).
// steer_base: B at the channels' own scales -- un_a, un_b undo the balance of the pair's transform (pair_balance.h: powers of two; 1 on
// balanced input) and are 0 for a channel of exact zeros.
__device__ __forceinline__ float4 steer_base(float4 B, float un_a, float un_b)
{
    const float2 a = cscale(make_float2(B.x, B.y), un_a), b = cscale(make_float2(B.z, B.w), un_b);
    return make_float4(a.x, a.y, b.x, b.y);
}
// y + (a2 Q_a) B_a + (b2 Q_b) B_b at one bin; FIRST (s = 0): Q = 1
template <bool FIRST>
__device__ __forceinline__ float2 steer_mac(float2 y, float2 a2, float2 b2, float4 B, float2 qa, float2 qb)
{
    if (!FIRST) { a2 = cmul(a2, qa); b2 = cmul(b2, qb); }
    y = cmac(y, a2, make_float2(B.x, B.y));
    return cmac(y, b2, make_float2(B.z, B.w));
}
// A[0] = Y[0] while every other bin carries 2 Y[k] (the spectra arrive doubled): bin 0 is lane 0's first
__device__ __forceinline__ float2 steer_dc(float2 y0, int lane) { return cscale(y0, lane == 0 ? 0.5f : 1.f); }

// A[512]: zn[p] = (X_a[512], X_b[512]) of pair p at the channels' own scales (real numbers), pn = Re P_c[512] / (M N) per channel
template <int NP>
__device__ __forceinline__ float steer_nyquist(const float2 (&zn)[NP], const float *pn)
{
    float yn = 0.f;
#pragma unroll
    for (int pr = 0; pr < NP; ++pr) yn = fmaf(zn[pr].y, pn[2 * pr + 1], fmaf(zn[pr].x, pn[2 * pr], yn));
    return yn;
}

// yv[s] = A[lane + 64 s], s < 8 (natural lane order: register i = bin lane + 64 i, the upper half of the spectrum is zero), yn = A[512].
// mid(): as fft1024c's.  On return y[p].x = sample lane + 64 dr16(p) of the beamformed frame.
template <typename Mid = F1kNoMid>
__device__ __forceinline__ void steer_inverse(float2 (&y)[16], const float2 (&yv)[8], float yn, float2 *buf, int lane, const float2 *tab, const F1kLane &lc, Mid mid = Mid())
{
#pragma unroll
    for (int i = 0; i < 8; ++i) { y[i] = yv[i]; y[i + 8] = make_float2(0.f, 0.f); }
    fft1024c<true, 3>(y, buf, lane, tab, lc, mid);
    const float sn = (lane & 1) ? -yn : yn;                                        // A[512] e^(j pi n), n = lane + 64 i
#pragma unroll
    for (int i = 0; i < 16; ++i) y[i].x += sn;
}

}  // namespace mca
