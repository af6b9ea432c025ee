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
#include "mca_internal.h"
#include "pair_balance.h"

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

// (x_a, x_b) * w for two consecutive points whose window samples share a register pair: op_sel broadcasts the low / high half
__device__ __forceinline__ float2 win_lo(float a, float b, v2f w)
{
    v2f x = {a, b}, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(r) : "v"(x), "v"(w));
    return from_v2f(r);
}
__device__ __forceinline__ float2 win_hi(float a, float b, v2f w)
{
    v2f x = {a, b}, r;
    asm("v_pk_mul_f32 %0, %2, %1 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(r) : "v"(x), "v"(w));   // w in src0: its high half may feed the low result there (fft512.h, RULE)
    return from_v2f(r);
}

// The mirror separation of one bin: zk = Z[k], zm = Z[1024 - k] of a pair's transform give
//     a2 = 2 X_a = (zk.x + zm.x, zk.y - zm.y),   b2 = 2 X_b = (zk.y + zm.y, zm.x - zk.x)
// in one packed instruction each: the signs and the crossed halves ride on neg_hi and op_sel, so no register is re-paired first
// (written as scalar expressions this was three packed adds and two moves per bin).  x - y = x + (-y) and x * 1 + y = x + y are
// exact, so the bits are those of the scalar expressions.  b2 crosses halves through src0 and src2 of an fma with 1.0, as the
// transform's multiplications by j do: the low result may not take the high half of src1 (fft512.h, RULE).
__device__ __forceinline__ void mirror_split(float2 zk, float2 zm, float2 &a2, float2 &b2)
{
    const v2f k = to_v2f(zk), m = to_v2f(zm);
    v2f a, b;
    asm("v_pk_add_f32 %0, %1, %2 neg_hi:[0,1]" : "=v"(a) : "v"(k), "v"(m));
    asm("v_pk_fma_f32 %0, %1, 1.0, %2 op_sel:[1,0,1] op_sel_hi:[0,0,0] neg_hi:[1,0,0]" : "=v"(b) : "v"(k), "v"(m));
    a2 = from_v2f(a);
    b2 = from_v2f(b);
}

// One frame of one array at the bin of its final pick, by one wave: per pair the steps of k_stft_phat_wave up to the separated spectra
// 2 X_a, 2 X_b -- the same window, balance, transform and mirror exchange, hence the same bits -- and steer_mac / steer_nyquist on
// them in the same order; the row of Y is replaced.  The one patch routine: k_steer_patch and the patching second pick
// (k_scan_repick<PL, true>) both call it, so a hop's bits do not depend on which of them patched it.
// win: the lane's window samples {w[lane + 128 i], w[lane + 128 i + 64]}; buf: this wave's F1K_SCRATCH words; tab, lc: fft1024c's.
__device__ __forceinline__ void steer_patch_frame(const SteerPatchArgs &p, int a, int f, int bin, const v2f (&win)[8], float2 *buf, const float2 *tab,
                                                  const F1kLane &lc, int lane)
{
    constexpr int NP = 4, MT = 8;
    const int lam = lane <= 32 ? lane : 96 - lane;
    const bool self = (lane & 31) == 0;
    const float4 *srow = p.bf.rows + (long long)(bin + 1) * (NP * 64);
    const float2 *qrow = p.bf.q + (long long)(bin + 1) * (MT * 8);            // (wave-uniform)
    const float *base = p.pcm + (long long)a * p.array_stride + (long long)f * FFT_H;
    float2 *yrow = p.bf.Y + ((long long)a * p.y_frames + f - p.y_f0) * STEER_ROW;
    float xa[16], xb[16];
    auto load_pair = [&](int pr) {
        const float *pa = base + (long long)(2 * pr) * p.mic_stride, *pb = pa + p.mic_stride;
#pragma unroll
        for (int i = 0; i < 16; ++i) { xa[i] = pa[(unsigned)lane + 64 * i]; xb[i] = pb[(unsigned)lane + 64 * i]; }
    };
    load_pair(0);
    float2 Y[8], zn[NP];
#pragma unroll
    for (int pr = 0; pr < NP; ++pr) {
        float2 z[16];
        float4 B;
#pragma unroll
        for (int i = 0; i < 8; ++i) { z[2 * i] = win_lo(xa[2 * i], xb[2 * i], win[i]); z[2 * i + 1] = win_hi(xa[2 * i + 1], xb[2 * i + 1], win[i]); }
        float ma = max3abs(z[0].x, z[1].x, z[2].x), mb = max3abs(z[0].y, z[1].y, z[2].y);
#pragma unroll
        for (int i = 3; i < 15; i += 2) { ma = max3abs(ma, z[i].x, z[i + 1].x); mb = max3abs(mb, z[i].y, z[i + 1].y); }
        ma = max2abs(ma, z[15].x); mb = max2abs(mb, z[15].y);
        const PairBalance pb = pair_balance(ma, mb);
        if (pb.scaled()) {
            const float sa = pb.sa(), sb = pb.sb();
#pragma unroll
            for (int i = 0; i < 16; ++i) z[i] = make_float2(z[i].x * sa, z[i].y * sb);
        }
        fft1024c<false, 3>(z, buf, lane, tab, lc, [&]() {
            B = (srow + pr * 64)[(unsigned)lane];
            if (pr < NP - 1) load_pair(pr + 1);
        }, lam);
        const float un_a = pb.un_a(), un_b = pb.un_b();
        zn[pr] = make_float2(z[dr16(8)].x * un_a, z[dr16(8)].y * un_b);
        const float4 Bu = steer_base(B, un_a, un_b);
        // the mirror exchange of k_stft_phat_wave
        if (lane == 0) {
            float2 t[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) t[j] = z[dr16(j)];
#pragma unroll
            for (int j = 8; j < 16; ++j) z[dr16(j < 12 ? j + 4 : j - 4)] = t[(j + 1) & 15];
        } else if (self) {
#pragma unroll
            for (int j = 8; j < 12; ++j) { const float2 t = z[dr16(j)]; z[dr16(j)] = z[dr16(j + 4)]; z[dr16(j + 4)] = t; }
        } else {
#pragma unroll
            for (int j = 8; j < 12; ++j) {
                float2 &u = z[dr16(j)], &w = z[dr16(j + 4)];
                swap_rows32(u.x, w.x); swap_rows32(w.x, u.x);
                swap_rows32(u.y, w.y); swap_rows32(w.y, u.y);
            }
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const float2 zk = z[dr16(s)], zm = z[dr16(15 - s < 12 ? 15 - s + 4 : 15 - s - 4)];
            // (the values of mirror_split, bit for bit; as scalar expressions here: k_steer_patch holds 218 registers with them, 224 with it)
            const float2 a2 = make_float2(zk.x + zm.x, zk.y - zm.y);                               // 2 X_a
            const float2 b2 = make_float2(zk.y + zm.y, zm.x - zk.x);                               // 2 X_b
            const float2 y = pr == 0 ? make_float2(0.f, 0.f) : Y[s];
            if (s == 0) Y[s] = steer_mac<true>(y, a2, b2, Bu, a2, b2);
            else Y[s] = steer_mac<false>(y, a2, b2, Bu, qrow[(2 * pr) * 8 + s], qrow[(2 * pr + 1) * 8 + s]);
        }
        wave_lds_fence();
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) yrow[(unsigned)lam + 64 * s] = s == 0 ? steer_dc(Y[s], lane) : Y[s];
    if (lane == 0) yrow[FFT_H] = make_float2(steer_nyquist<NP>(zn, p.bf.nyq + (bin + 1) * MT), 0.f);
}

}  // namespace mca
