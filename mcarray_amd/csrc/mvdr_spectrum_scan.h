// mvdr_spectrum_scan.h -- the two halves of a Capon scan that k_mvdr_spectrum<Q> (kernels_mvdr_spectrum.hip, one row of angles) and
// k_mvdr_map_scan<Q> (kernels_mvdr_map.hip, azimuth x elevation) share: the factor of the 64 bins of a chunk, one quad per bin, and
// the forward-substitution scan with lanes as directions.  One text for both, so that the arithmetic per (bin, direction) and the
// (chunk, wave) order of the partial sums are the same in both units.
#pragma once
#include "mca_internal.h"
#include "mvdr_solve.h"

namespace mca {

// LDS of a workgroup of either kernel: Ls [64][tri] float2, L below the diagonal and (1 / L_jj, 0) on it; Ws [64] float, w' of the
// bin, 0 for a bin that contributes nothing.
// The factor of every bin of the chunk at kbase of stream a, one quad per bin (the column loop of k_mvdr_solve without right-hand
// sides); 256 threads, the caller synchronises behind it
template <int Q>
__device__ __forceinline__ void mvdr_spectrum_factor(const MvdrSpectrumArgs &p, int a, int kbase, float2 *Ls, float *Ws)
{
    constexpr int NE = 2 * Q * (Q + 1);          // row slot q holds 4 (q + 1) entries, starting at 2 q (q + 1)
    const int M = p.M, tri = M * (M + 1) / 2;
    const int tid = threadIdx.x, l = tid & 3, b = tid >> 2;
    const int k = kbase + b;
    const bool in = k >= p.bin_lo && k <= p.bin_hi;
    const long long pc = (long long)a * p.K + (in ? k : p.bin_lo);
    const float tr = p.trace[pc];
    const bool live = in && tr > 1e-30f;
    const float sc = live ? (float)M / tr : 0.f;
    const float2 *st = p.phi + pc * tri;
    float2 *Lb = Ls + b * tri;
    float2 P[NE], L[NE];
    float dsum[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = 4 * q + l;
        dsum[q] = 0.f;
#pragma unroll
        for (int m = 0; m < 4 * (q + 1); ++m) {
            const float2 v = (i < M && m <= i) ? st[i * (i + 1) / 2 + m] : make_float2(0.f, 0.f);
            P[2 * q * (q + 1) + m] = make_float2(v.x * sc, v.y * sc);
        }
    }
    mvdr_static_for<0, 4 * Q>([&](auto jc) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value, jq = j >> 2, jl = j & 3, jo = 2 * jq * (jq + 1);
        if (j < M) {
            const float pjj = P[jo + j].x + p.loading;
            const float inv = __builtin_amdgcn_rsqf(quad_bcast1<jl>(pjj - dsum[jq]));
            if (l == jl) Lb[j * (j + 1) / 2 + j] = make_float2(inv, 0.f);
            // L_ij = (Phi_ij - sum_{m<j} L_im conj(L_jm)) / L_jj for the rows below j (rows <= j compute dead values)
            float2 s_[Q];
#pragma unroll
            for (int q = jq; q < Q; ++q) s_[q] = P[2 * q * (q + 1) + j];
#pragma unroll
            for (int m = 0; m < j; ++m) {
                const float2 r = quad_bcast(L[jo + m], jl);
#pragma unroll
                for (int q = jq; q < Q; ++q) s_[q] = cnmacc(s_[q], L[2 * q * (q + 1) + m], r);
            }
#pragma unroll
            for (int q = jq; q < Q; ++q) {
                const float2 lq = make_float2(s_[q].x * inv, s_[q].y * inv);
                L[2 * q * (q + 1) + j] = lq;
                dsum[q] = fmaf(lq.x, lq.x, fmaf(lq.y, lq.y, dsum[q]));
                if (4 * q + l > j && 4 * q + l < M) Lb[(4 * q + l) * (4 * q + l + 1) / 2 + j] = lq;
            }
        }
    });
    if (l == 0) Ws[b] = live ? (p.power ? tr / (float)M : 1.f) : 0.f;
}

// NA angles of this lane (a0, a0 + 64) against the bins wv, wv + 4, ... of the chunk: forward substitution u = L^-1 d per bin, L read
// from LDS at an address all lanes share (broadcast), the steering phasors as the product of their two table factors
template <int Q, int NA>
__device__ __forceinline__ void mvdr_spectrum_scan(const MvdrSpectrumArgs &p, const float2 *Ls, const float *Ws, int tri, int kbase, int wv,
                                                   int a0, float *po)
{
    const int M = p.M;
    const long long Dpad = p.Dpad;
    float acc[NA];
#pragma unroll
    for (int n = 0; n < NA; ++n) acc[n] = 0.f;
#pragma unroll 1
    for (int bl = wv; bl < MVDR_SPEC_CHUNK; bl += 4) {
        const float w = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(Ws[bl])));
        if (w == 0.f) continue;                  // outside the band or digital silence (the same for the whole wave)
        const int k = kbase + bl;
        const float2 *th = p.T + (long long)(k >> 5) * Dpad + a0;
        const float2 *tl = p.T + (long long)(p.nhi + (k & 31)) * Dpad + a0;
        const float2 *Lb = Ls + bl * tri;
        float2 u[NA][4 * Q];
        float q[NA];
#pragma unroll
        for (int n = 0; n < NA; ++n) q[n] = 0.f;
        mvdr_static_for<0, 4 * Q>([&](auto jc) __attribute__((always_inline)) {
            constexpr int j = decltype(jc)::value;
            if (j < M) {
                const long long mo = (long long)j * p.nph * Dpad;
                float2 s[NA];
#pragma unroll
                for (int n = 0; n < NA; ++n) s[n] = cmul(th[mo + 64 * n], tl[mo + 64 * n]);
                const float2 *Lj = Lb + j * (j + 1) / 2;
#pragma unroll
                for (int m = 0; m < j; ++m) {
                    const float2 lv = Lj[m];
#pragma unroll
                    for (int n = 0; n < NA; ++n) s[n] = cnmac(s[n], lv, u[n][m]);
                }
                const float inv = Lj[j].x;           // 1 / L_jj
#pragma unroll
                for (int n = 0; n < NA; ++n) {
                    u[n][j] = make_float2(s[n].x * inv, s[n].y * inv);
                    q[n] = fmaf(u[n][j].x, u[n][j].x, fmaf(u[n][j].y, u[n][j].y, q[n]));
                }
            }
        });
#pragma unroll
        for (int n = 0; n < NA; ++n) acc[n] += w / q[n];
    }
#pragma unroll
    for (int n = 0; n < NA; ++n)
        if (a0 + 64 * n < p.D) po[a0 + 64 * n] = acc[n];
}

}  // namespace mca
