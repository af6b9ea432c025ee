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
#include "mvdr_rtf.h"

namespace mca {

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
