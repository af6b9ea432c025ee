// kernels_mvdr_rtf.hip -- steering vectors estimated from a target covariance: the relative transfer function towards a reference
// microphone (gfx950; include/mcarray_hip.h, mca_hip_mvdr_set_rtf).  k_mvdr_rtf runs between the analysis and the solve
// (k_mvdr_solve_rtf_t of mvdr_solve.h, which reads the steering plane D this kernel writes the way it reads X).
//
// Per stream a, slot s, bin k and frame t, with x the frame's spectra, u the clamped update mask (the solve's WEIGHT = CELL), m the
// clamped target mask of the slot (a NaN counts as 0), g0 the geometric vector of doa[a][t][s]:
//     Phi_t, tr_t  the solve's recursion, with its operations, so that this kernel's Phi has the solve's bits (not written back)
//     cphi_t = a cphi + (1 - a)                                  a = 1 - (1 - alpha) u; untouched where u == 0
//     Psi_t  = b Psi + (1 - b) x x^H,  cpsi_t = b cpsi + (1 - b)   b = 1 - (1 - target_alpha) m; untouched, bit for bit, where m == 0
//     tau    = tr(Psi_t) / cpsi_t                                needs cpsi_t > 0 and tau > 1e-30
//     Delta  = Psi_t / (cpsi_t tau) - [cphi_t > 0] Phi_t / (cphi_t tau)
//     v = g0 / sqrt(M);  `iterations` times:  g = Delta v,  n = |g|^2 (needs n > 1e-20),  rho = Re(v^H g),  v = g / sqrt(n)
//     needs rho > min_share and |g[ref_mic]|^2 > 1e-6 n;   d = g / g[ref_mic]   (any need not met, or a non-finite value: d = g0)
// and D[a][s][t][k][.] = d, or g0 where the bin's noise trace is <= 1e-30 (the solve's silence branch reads the plane too).
//
// The layout is the solve's: FOUR lanes per (stream, slot, bin) problem, lane l of a quad owns the rows l, l + 4, ... of the lower
// triangles of Psi and of a private copy of Phi, both in registers across the frame loop (2 x 80 VGPRs at 13 ... 16 microphones; no
// factor L here).  The Hermitian product g = Delta v is formed from the lower-triangle rows: the row part g_i += Delta_im v_m (m <= i)
// with v_m by quad_bcast, and the column part g_j += sum_{i > j} conj(Delta_ij) v_i, whose terms sit with the owners of the rows i:
// a quad sum (DPP) per column, taken by the lane that owns row j.  Delta is not held: an element is sp Psi_im - sn Phi_im wherever it
// is used (twice per iteration).  No LDS, no atomics; a quad depends on its own problem only, so where a stream sits in the batch and
// how it is cut into calls do not change bytes.  A fallback cell is cmul(T_hi, T_lo) through mvdr_steer_rows: the bits of the vector
// the kernels without RTF form.  One instantiation per Q serves M = 4 Q and M < 4 Q: the branch-free M = 4 Q form, all in one basic block,
// is the one that does not fit the 256 registers of __launch_bounds__(256, 2) at Q = 4.
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

// P <- at P + bt x x^H on the rows of this lane (the recursion of mvdr_solve.h, operation for operation); returns |x|^2
template <int Q>
__device__ __forceinline__ float rtf_rank1(float2 (&P)[2 * Q * (Q + 1)], const float2 (&x)[Q], float at, float bt, int M)
{
    float e = 0.f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const float2 xs = make_float2(bt * x[q].x, bt * x[q].y);
#pragma unroll
        for (int m = 0; m < 4 * (q + 1); ++m)
            if (m < M) {
                const float2 xm = quad_bcast(x[m >> 2], m & 3);
                float2 &e_ = P[2 * q * (q + 1) + m];
                e_ = cmacc(make_float2(at * e_.x, at * e_.y), xs, xm);
                if (q == Q - 1) e = fmaf(xm.x, xm.x, fmaf(xm.y, xm.y, e));
            }
    }
    return e;
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

// grid (ceil(streams * S * K / 64)), 256 threads
template <int Q>
__global__ __launch_bounds__(256, 2) void k_mvdr_rtf(MvdrRtfArgs p)
{
    constexpr int NE = 2 * Q * (Q + 1);
    const int tid = threadIdx.x, l = tid & 3;
    const int M = p.M, K = p.K, F = p.n_frames, FL = p.n_loop, S = p.S;   // FL frames of a call of F (the strides of X, T and the masks)
    const long long total = (long long)p.n_streams * S * K;
    const long long pid = (long long)blockIdx.x * 64 + (tid >> 2);
    const bool pv = pid < total;
    const long long pc = pv ? pid : total - 1;   // surplus quads shadow the last problem and store nothing
    const long long as = pc / K;                  // a S + s
    const int k = (int)(pc - as * K), a = (int)(as / S), s = (int)(as - (long long)a * S);
    const int tri = M * (M + 1) / 2;
    const long long ak = (long long)a * K + k, ask = ((long long)a * p.slots + s) * K + k;

    float2 P[NE], R[NE];
    rtf_load_rows<Q>(P, p.phi + ak * tri, M, l);
    rtf_load_rows<Q>(R, p.psi + ask * tri, M, l);
    float tr = p.trace[ak], cphi = p.cphi_in[ak], cpsi = p.cpsi[ask];
    const int nhi = ((K - 1) >> 5) + 1, nph = nhi + 32;
    const float2 *T = p.T + (long long)a * F * S * M * nph + (k >> 5);
    const int lo_off = nhi - (k >> 5) + (k & 31);
    const long long fstride = (long long)K * M;
    const float2 *X = p.X + (long long)a * F * fstride + (long long)k * M + l;
    const float al = p.alpha, oma = p.one_minus_alpha, tal = p.talpha, omt = p.one_minus_talpha;
    const float *um = p.update ? p.update + ((long long)a * F * K + k) : nullptr;                  // + t K
    const float *tm = p.tmask ? p.tmask + (((long long)a * S + s) * F * K + k) : nullptr;          // + t K
    float2 *Dp = p.D + (((long long)a * S + s) * FL * K + k) * M + l;                              // + t K M + 4 q

    for (int t = 0; t < FL; ++t) {
        float2 x[Q], g0[Q], d[Q];
        float w = um ? um[(long long)t * K] : 1.f, m = tm ? tm[(long long)t * K] : 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) x[q] = (4 * q + l < M) ? X[(long long)t * fstride + 4 * q] : make_float2(0.f, 0.f);
        mvdr_steer_rows<Q, false>(g0, T, (long long)t * S + s, M, nph, lo_off, l);
        w = fminf(fmaxf(w, 0.f), 1.f);            // NaN -> 0
        m = fminf(fmaxf(m, 0.f), 1.f);
        if (w > 0.f) {
            const float bt = w == 1.f ? oma : oma * w, at = w == 1.f ? al : 1.f - oma * w;
            const float e = rtf_rank1<Q>(P, x, at, bt, M);
            tr = fmaf(at, tr, bt * e);
            cphi = fmaf(at, cphi, bt);
        }
        if (m > 0.f) {
            const float bt = m == 1.f ? omt : omt * m, at = m == 1.f ? tal : 1.f - omt * m;
            (void)rtf_rank1<Q>(R, x, at, bt, M);
            cpsi = fmaf(at, cpsi, bt);
        }
        (void)mvdr_rtf_estimate<Q>(d, R, P, cpsi, cphi, g0, p.iterations, p.ref_mic, p.min_share, M, l);
        const bool silent = !(tr > 1e-30f);
        if (pv) {
#pragma unroll
            for (int q = 0; q < Q; ++q)
                if (4 * q + l < M) Dp[(long long)t * fstride + 4 * q] = silent ? g0[q] : d[q];
        }
    }
    if (pv) {
        float2 *so = p.psi + ask * tri;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int i = 4 * q + l;
#pragma unroll
            for (int m = 0; m < 4 * (q + 1); ++m)
                if (i < M && m <= i) so[i * (i + 1) / 2 + m] = R[2 * q * (q + 1) + m];
        }
        if (l == 0) {
            p.cpsi[ask] = cpsi;
            if (s == 0) p.cphi_out[ak] = cphi;
        }
    }
}

// grid (ceil(K / 64)), 256 threads
template <int Q>
__global__ __launch_bounds__(256, 2) void k_mvdr_rtf_steering(MvdrRtfSteerArgs p)
{
    constexpr int NE = 2 * Q * (Q + 1);
    const int tid = threadIdx.x, l = tid & 3;
    const int M = p.M, K = p.K;
    const int kk = blockIdx.x * 64 + (tid >> 2);
    const bool pv = kk < K;
    const int k = pv ? kk : K - 1;
    const int tri = M * (M + 1) / 2;
    float2 P[NE], R[NE], g0[Q], d[Q];
    rtf_load_rows<Q>(P, p.phi + (long long)k * tri, M, l);
    rtf_load_rows<Q>(R, p.psi + (long long)k * tri, M, l);
    const int nhi = ((K - 1) >> 5) + 1, nph = nhi + 32;
    mvdr_steer_rows<Q, false>(g0, p.T + (k >> 5), 0, M, nph, nhi - (k >> 5) + (k & 31), l);
    const bool est = mvdr_rtf_estimate<Q>(d, R, P, p.cpsi[k], p.cphi[k], g0, p.iterations, p.ref_mic, p.min_share, M, l);
    if (pv) {
#pragma unroll
        for (int q = 0; q < Q; ++q)
            if (4 * q + l < M) p.out[(long long)k * M + 4 * q + l] = d[q];
        if (l == 0) p.estimated[k] = est ? 1 : 0;
    }
}

const void *mvdr_rtf_kernel(int Q, bool steering)
{
    const void *k[4][2] = {{(const void *)k_mvdr_rtf<1>, (const void *)k_mvdr_rtf_steering<1>}, {(const void *)k_mvdr_rtf<2>, (const void *)k_mvdr_rtf_steering<2>},
                           {(const void *)k_mvdr_rtf<3>, (const void *)k_mvdr_rtf_steering<3>}, {(const void *)k_mvdr_rtf<4>, (const void *)k_mvdr_rtf_steering<4>}};
    return Q >= 1 && Q <= 4 ? k[Q - 1][steering] : nullptr;
}

}  // namespace mca
