// mvdr_nulls.h -- the small per-direction solves of the MVDR solve with soft nulls (k_mvdr_solve_t<..., NULLS = true, ...>): the quad
// sums, the pair index of the Gram matrix and the (S-1) x (S-1) solve of one output.  Included by mvdr_solve.h, behind its helpers.
#pragma once
#include "mvdr_solve.h"

namespace mca {

template <int CTRL>
__device__ __forceinline__ float quad_perm_add(float v)     // v + v of the lane that quad_perm CTRL names
{
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float quad_sum(float v) { return quad_perm_add<0x4e>(quad_perm_add<0xb1>(v)); }   // [1,0,3,2] then [2,3,0,1]

constexpr int mvdr_pair(int S, int a, int b) { return a * (2 * S - a - 1) / 2 + (b - a - 1); }   // index of (a < b) among the S (S - 1) / 2 pairs

// c_ab from the stored upper triangle
template <int S, int A, int B>
__device__ __forceinline__ float2 mvdr_coh(const float2 (&c)[S * (S - 1) / 2])
{
    if constexpr (A < B) return c[mvdr_pair(S, A, B)];
    else return cconj(c[mvdr_pair(S, B, A)]);
}

// output SD of the S: (I + g C_RR) z = g c_Rs by an unpivoted L D L^H (Hermitian positive definite for every g >= 0: C_RR is a
// Gram matrix), then Y = rs_s (beta_s - z^H beta_R) / (1 - z^H c_Rs); rs_a = 1 / sqrt(G_aa)
template <int S, int SD>
__device__ __forceinline__ float2 mvdr_null_output(const float2 (&c)[S * (S - 1) / 2], const float2 (&beta)[S], const float (&rs)[S], float g)
{
    constexpr int n = S - 1;
    float2 A[n][n], z[n], bR[n], cs[n];         // A: the lower triangle, then the unit lower factor in its place
    float dg[n];
    mvdr_static_for<0, n>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value, ri = i < SD ? i : i + 1;
        cs[i] = mvdr_coh<S, ri, SD>(c);
        bR[i] = beta[ri];
        z[i] = make_float2(g * cs[i].x, g * cs[i].y);
        mvdr_static_for<0, i>([&](auto kc) __attribute__((always_inline)) {
            constexpr int k = decltype(kc)::value, rk = k < SD ? k : k + 1;
            const float2 e = mvdr_coh<S, ri, rk>(c);
            A[i][k] = make_float2(g * e.x, g * e.y);
        });
    });
#pragma unroll
    for (int i = 0; i < n; ++i) {
        float di = 1.0f + g;
#pragma unroll
        for (int k = 0; k < i; ++k) {
            // A[i][k] <- (A_ik - sum_{m<k} l_im d_m conj(l_km)) / d_k; the products l_im d_m wait in the upper triangle
            float2 e = A[i][k];
#pragma unroll
            for (int m = 0; m < k; ++m) e = cnmacc(e, A[m][i], A[k][m]);
            A[k][i] = e;                                                 // l_ik d_k
            const float rd = __builtin_amdgcn_rcpf(dg[k]);
            A[i][k] = make_float2(e.x * rd, e.y * rd);
            di = fmaf(-A[i][k].x, e.x, fmaf(-A[i][k].y, e.y, di));       // - |l_ik|^2 d_k
            z[i] = cnmac(z[i], A[i][k], z[k]);                           // forward substitution
        }
        dg[i] = di;
    }
#pragma unroll
    for (int i = 0; i < n; ++i) {
        const float rd = __builtin_amdgcn_rcpf(dg[i]);
        z[i] = make_float2(z[i].x * rd, z[i].y * rd);
    }
#pragma unroll
    for (int i = n - 2; i >= 0; --i) {
#pragma unroll
        for (int k = i + 1; k < n; ++k) z[i] = cnmacc(z[i], z[k], A[k][i]);   // z_i -= conj(l_ki) z_k
    }
    float2 nu = beta[SD];
    float de = 1.0f;
#pragma unroll
    for (int i = 0; i < n; ++i) {
        nu = cnmacc(nu, bR[i], z[i]);                                    // - conj(z_i) beta_i
        de = fmaf(-z[i].x, cs[i].x, fmaf(-z[i].y, cs[i].y, de));         // - Re(conj(z_i) c_is): z^H c_Rs is real
    }
    const float sc = rs[SD] * __builtin_amdgcn_rcpf(de);
    return make_float2(nu.x * sc, nu.y * sc);
}

}  // namespace mca
