// mvdr_rtf.h -- the estimator of the relative transfer function on the rows a quad holds, shared by k_mvdr_rtf /
// k_mvdr_rtf_steering (kernels_mvdr_rtf.hip) and by k_mvdr_track_spectrum (kernels_mvdr_track.hip): one text, so the
// tracks read the steering vector the RTF calls steer with.
#pragma once
#include "fft512.h"
#include "mca_internal.h"
#include "mvdr_solve.h"

namespace mca {

// the lower-triangle rows of problem st (row-major packed triangle) of this lane
template <int Q>
__device__ __forceinline__ void rtf_load_rows(float2 (&P)[2 * Q * (Q + 1)], const float2 *st, int M, int l)
{
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = 4 * q + l;
#pragma unroll
        for (int m = 0; m < 4 * (q + 1); ++m)
            P[2 * q * (q + 1) + m] = (i < M && m <= i) ? st[i * (i + 1) / 2 + m] : make_float2(0.f, 0.f);
    }
}

// The estimator on the rows the quad holds: d and whether it is the estimate (the same in the four lanes: every decision is taken
// on quad sums and quad broadcasts).  Entries of a row slot right of the diagonal are not part of the triangle and are not read.
template <int Q>
__device__ __forceinline__ bool mvdr_rtf_estimate(float2 (&d)[Q], const float2 (&R)[2 * Q * (Q + 1)], const float2 (&P)[2 * Q * (Q + 1)], float cpsi,
                                                  float cphi, const float2 (&g0)[Q], int iterations, int ref_mic, float min_share, int M, int l)
{
    float e = 0.f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int o = 2 * q * (q + 1) + 4 * q;
        e += l == 0 ? R[o].x : l == 1 ? R[o + 1].x : l == 2 ? R[o + 2].x : R[o + 3].x;   // rows >= M hold zeros
    }
    const float tau = quad_sum(e) / cpsi;
    bool ok = cpsi > 0.f && tau > 1e-30f;
    const float sp = 1.f / (cpsi * tau), sn = cphi > 0.f ? 1.f / (cphi * tau) : 0.f;
    const float rm = 1.f / sqrtf((float)M);
    float2 v[Q];
    float2 (&g)[Q] = d;                          // g = Delta v lives in the output rows
#pragma unroll
    for (int q = 0; q < Q; ++q) { v[q] = make_float2(g0[q].x * rm, g0[q].y * rm); g[q] = make_float2(0.f, 0.f); }
    float n = 0.f, rho = 0.f;
#pragma unroll 1
    for (int it = 0; it < iterations; ++it) {
        // an element of Delta, formed where it is used.  The scales pass through a register of the iteration's own: as loop invariants
        // the 2 x NE elements would be formed once ahead of the loop and held, which the registers do not have room for
        float spi = sp, sni = sn;
        asm volatile("" : "+v"(spi), "+v"(sni));
        auto delta = [&](int idx) __attribute__((always_inline)) {
            return make_float2(fmaf(spi, R[idx].x, -(sni * P[idx].x)), fmaf(spi, R[idx].y, -(sni * P[idx].y)));
        };
        // the row part: columns left of the diagonal block, then the block up to the (real) diagonal
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int m = 0; m < 4 * q; ++m)
                if (m < M) {
                    acc = cmac(acc, delta(2 * q * (q + 1) + m), quad_bcast(v[m >> 2], m & 3));
                    if ((m & 3) == 3) __builtin_amdgcn_sched_barrier(0);    // four terms, a row, a column at a time: scheduled across them, the
                }                                                           // elements of Delta in flight cost scratch
#pragma unroll
            for (int ml = 0; ml < 4; ++ml)
                if (4 * q + ml < M) {
                    const float2 c = delta(2 * q * (q + 1) + 4 * q + ml);
                    acc = cmac(acc, make_float2(ml <= l ? c.x : 0.f, ml < l ? c.y : 0.f), quad_bcast(v[q], ml));
                }
            g[q] = acc;
            __builtin_amdgcn_sched_barrier(0);
        }
        // the column part: conj(Delta_ij) v_i over the rows i > j, summed over the quad, to the owner of row j.  (The scales anew: an
        // element is formed a second time here, not held from the row part.)
        asm volatile("" : "+v"(spi), "+v"(sni));
        mvdr_static_for<0, 4 * Q>([&](auto jc) __attribute__((always_inline)) {
            constexpr int j = decltype(jc)::value, jq = j >> 2, jl = j & 3;
            if (j < M) {
                float2 acc = make_float2(0.f, 0.f);
#pragma unroll
                for (int q = jq; q < Q; ++q) {
                    const bool below = q > jq || l > jl;
                    acc = cmacc(acc, below ? v[q] : make_float2(0.f, 0.f), delta(2 * q * (q + 1) + j));
                }
                acc = make_float2(quad_sum(acc.x), quad_sum(acc.y));
                if (l == jl) g[jq] = cadd(g[jq], acc);
                __builtin_amdgcn_sched_barrier(0);
            }
        });
        float nn = 0.f, rr = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            nn = fmaf(g[q].x, g[q].x, fmaf(g[q].y, g[q].y, nn));
            rr = fmaf(v[q].x, g[q].x, fmaf(v[q].y, g[q].y, rr));
        }
        n = quad_sum(nn); rho = quad_sum(rr);
        ok = ok && n > 1e-20f;
        const float rn = 1.f / sqrtf(n);
#pragma unroll
        for (int q = 0; q < Q; ++q) v[q] = make_float2(g[q].x * rn, g[q].y * rn);
    }
    ok = ok && rho > min_share;
    float2 sel = g[0];
#pragma unroll
    for (int q = 1; q < Q; ++q) sel = (ref_mic >> 2) == q ? g[q] : sel;
    const float2 gr = quad_bcast(sel, ref_mic & 3);
    const float pr = fmaf(gr.x, gr.x, gr.y * gr.y);
    ok = ok && pr > 1e-6f * n;
    const float ir = 1.f / pr;
    const float2 cg = make_float2(gr.x * ir, -(gr.y * ir));                  // 1 / g_ref
    float fin = 0.f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        d[q] = cmul(d[q], cg);
        if (4 * q + l == ref_mic) d[q] = make_float2(1.f, 0.f);
        fin = fmaf(d[q].x, d[q].x, fmaf(d[q].y, d[q].y, fin));
    }
    ok = ok && quad_sum(fin) < 3.0e38f;                                      // false for a NaN as well
    if (!ok) {
#pragma unroll
        for (int q = 0; q < Q; ++q) d[q] = g0[q];
    }
    return ok;
}

}  // namespace mca
