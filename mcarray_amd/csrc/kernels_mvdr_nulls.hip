// kernels_mvdr_nulls.hip -- the MVDR solve with soft nulls at the other look directions (gfx950).  A translation unit of its own:
// k_mvdr_solve and k_mvdr_solve_sources of kernels_mvdr.hip compile to the instruction streams they had before this kernel
// existed only if nothing is added to theirs (with this kernel beside them, three k_mvdr_solve_sources instantiations came out
// with other scalar registers and hoists).  What the kernels share is in mvdr_solve.h.
#include "fft_block.h"
#include "mca_internal.h"
#include "mvdr_nulls.h"
#include "mvdr_solve.h"

namespace mca {

// --------------------------------------------------------------------------------------
// k_mvdr_nulls<Q, S, S1, PF>: the solve for S look directions with a soft null of gain g = MvdrNullsArgs::null_gain > 0 at
// every other look direction of the frame (include/mcarray_hip.h, mca_hip_mvdr_set_null_gain):
//     p_r = 1 / (d_r^H PhiL^-1 d_r),  Phi_s = PhiL + g sum_{r != s} p_r d_r d_r^H,  Y_s = w_s^H x,  w_s = Phi_s^-1 d_s / (d_s^H Phi_s^-1 d_s)
// With U = L^-1 [d_0 ... d_{S-1}], v = L^-1 x, G = U^H U, b = U^H v and R the other directions of s (matrix inversion lemma):
//     (g G_RR + diag G_RR) q = g G_Rs,  Y_s = (b_s - q^H b_R) / (G_ss - q^H G_Rs)
// b_s and G_ss are num[s] and den[s] of k_mvdr_solve_sources; the kernel is that one (same loads, recursion, loading, column loop,
// passes, launch plan, state stores and silence branch: the covariance it leaves has the same bits) plus the off-diagonal G and
// one (S-1) x (S-1) Hermitian solve per direction, evaluated on the normalised quantities
//     c_ab = G_ab / sqrt(G_aa G_bb) (|c| <= 1),  beta_a = b_a / sqrt(G_aa):  (I + g C_RR) z = g c_Rs,
//     Y_s = (beta_s - z^H beta_R) / (sqrt(G_ss) (1 - z^H c_Rs))
// so that nothing of the order G^2 is formed (G ~ M / power reaches 1e31 at the silence threshold).
//
// Where the cross terms come from: the pairs of directions of different passes never meet in registers, and four row slots with
// three directions have no registers left for six more accumulators.  So the lane that owns row j parks the u_j[s] it has just
// scaled in LDS (words [q][s][thread]: conflict free, read back by the thread that wrote them, no synchronisation), a pass of a
// kernel with several passes parks its num and den the same way, and after the last pass -- L is dead by then -- every lane sums
// conj(u_j[a]) u_j[b] over its own rows, the quad adds the four partial sums (DPP), and every lane holds G.  The small solves are
// written out per direction with compile-time indices (every lane computes all S of them; lane s stores output s).
// LDS: 256 (Q S + 3/2 S [S1 < S]) float2 per workgroup, 44 KiB at Q = S = 4.
// --------------------------------------------------------------------------------------
template <int Q, int S, int S1, bool PF>
__global__ __launch_bounds__(256, 2) void k_mvdr_nulls(MvdrNullsArgs pa)
{
    const MvdrSolveArgs &p = pa.s;
    static_assert(S >= 2 && S <= MCA_MAX_SOURCES && S1 >= 1 && S % S1 == 0, "look directions per frame, in whole passes");
    constexpr int NE = 2 * Q * (Q + 1);          // row slot q holds 4 (q + 1) entries, starting at 2 q (q + 1)
    constexpr int NP = S * (S - 1) / 2;          // pairs of look directions
    constexpr bool PASSES = S1 < S;
    // dynamic LDS, sized by the launch (mvdr_nulls_lds_bytes)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *Us = reinterpret_cast<float2 *>(smem_raw);      // [q][s][thread]: u_{4q+l}[s] of the thread's problem, by the row's owner
    float2 *Ns = Us + Q * S * 256;                          // [s][thread]: num of every pass (PASSES only)
    float *Ds = reinterpret_cast<float *>(Ns + S * 256);    // [s][thread]: den
    const int tid = threadIdx.x, l = tid & 3;
    const int M = p.M, K = p.K, F = p.n_frames;
    const int piece = (int)(blockIdx.x % (unsigned)p.pieces);
    const int t_first = (int)((long long)piece * F / p.pieces), t_last = (int)((long long)(piece + 1) * F / p.pieces);   // frames this workgroup solves
    const long long total = p.pid0 + p.n_prob;
    const long long pid = p.pid0 + (long long)(blockIdx.x / (unsigned)p.pieces) * 64 + (tid >> 2);
    const bool pv = pid < total;
    const long long pc = pv ? pid : total - 1;   // surplus quads shadow the last problem and store nothing
    const int a = (int)(pc / K), k = (int)(pc - (long long)a * K);

    const int tri = M * (M + 1) / 2;
    float2 *st = p.phi + pc * tri;
    float2 P[NE], L[NE];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = 4 * q + l;
#pragma unroll
        for (int m = 0; m < 4 * (q + 1); ++m)
            P[2 * q * (q + 1) + m] = (i < M && m <= i) ? st[i * (i + 1) / 2 + m] : make_float2(0.f, 0.f);
    }
    float tr = p.trace[pc];
    const int nhi = ((K - 1) >> 5) + 1, nph = nhi + 32;
    const float2 *T = p.T + (long long)a * F * S * M * nph + (k >> 5);     // + ((t S + s) M + m) nph: hi factor; + lo_off: lo
    const int lo_off = nhi - (k >> 5) + (k & 31);
    const long long fstride = (long long)K * M;
    const float2 *X = p.X + (long long)a * F * fstride + (long long)k * M + l;
    const float al = p.alpha, oma = p.one_minus_alpha;
    float2 *yo = p.Y + (long long)a * S * F * K + k;                        // + (s F + t) K

    float2 xn[Q];                                 // the next frame's spectra, loaded a frame ahead (PF)
#pragma unroll
    for (int q = 0; q < Q; ++q) xn[q] = (PF && 4 * q + l < M) ? X[4 * q] : make_float2(0.f, 0.f);
    for (int t = 0; t < t_last; ++t) {
        float2 x[Q], rd[S1][Q], rx[Q];
        float dsum[Q];
        const long long tn = (long long)min(t + 1, t_last - 1) * fstride;
#pragma unroll
        for (int q = 0; q < Q; ++q) x[q] = PF ? xn[q] : (4 * q + l < M ? X[(long long)t * fstride + 4 * q] : make_float2(0.f, 0.f));
        if (t >= t_first) {
#pragma unroll
            for (int s = 0; s < S1; ++s) mvdr_steer_rows<Q, false>(rd[s], T, (long long)t * S + s, M, nph, lo_off, l);
        }
        if constexpr (PF) {
#pragma unroll
            for (int q = 0; q < Q; ++q) xn[q] = 4 * q + l < M ? X[tn + 4 * q] : make_float2(0.f, 0.f);
        }
        // Phi <- alpha Phi + (1 - alpha) x x^H (the rows of this lane), tr <- alpha tr + (1 - alpha) |x|^2
        float e = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float2 xs = make_float2(oma * x[q].x, oma * x[q].y);
#pragma unroll
            for (int m = 0; m < 4 * (q + 1); ++m)
                if (m < M) {
                    const float2 xm = quad_bcast(x[m >> 2], m & 3);
                    float2 &e_ = P[2 * q * (q + 1) + m];
                    e_ = cmacc(make_float2(al * e_.x, al * e_.y), xs, xm);
                    if (q == Q - 1) e = fmaf(xm.x, xm.x, fmaf(xm.y, xm.y, e));
                }
        }
        tr = fmaf(al, tr, oma * e);
        if (t < t_first) continue;               // (an earlier piece solves this frame)
        const float delta = p.loading_over_m * tr;
        const bool silent = !(tr > 1e-30f);       // the same in the four lanes of a quad
        // x does not ride the column loop: a further pass and the silence branch read the frame again (8 registers at Q = 4)
#pragma unroll
        for (int q = 0; q < Q; ++q) rx[q] = x[q];

        float2 bq[S];                             // b_s = num and G_ss = den of every direction
        float gd[S];
        // one pass per S1 look directions, s0 ... s0 + S1 - 1
#pragma unroll 1
        for (int s0 = 0;;) {
            float2 num[S1];
            float den[S1];
#pragma unroll
            for (int s = 0; s < S1; ++s) { num[s] = make_float2(0.f, 0.f); den[s] = 0.f; }
#pragma unroll
            for (int q = 0; q < Q; ++q) dsum[q] = 0.f;
            float2 *up = Us + s0 * 256 + tid;
            mvdr_static_for<0, 4 * Q>([&](auto jc) __attribute__((always_inline)) {
                constexpr int j = decltype(jc)::value, jq = j >> 2, jl = j & 3, jo = 2 * jq * (jq + 1);
                if (j < M) {
                    // pivot and the substitution values of row j, from its owner
                    const float pjj = P[jo + j].x + delta;
                    const float inv = __builtin_amdgcn_rsqf(quad_bcast1<jl>(pjj - dsum[jq]));
                    float2 uj[S1], vj = quad_bcast(rx[jq], jl);
                    vj = make_float2(vj.x * inv, vj.y * inv);
#pragma unroll
                    for (int s = 0; s < S1; ++s) {
                        uj[s] = quad_bcast(rd[s][jq], jl);
                        uj[s] = make_float2(uj[s].x * inv, uj[s].y * inv);
                        num[s] = cmacc(num[s], vj, uj[s]);                  // conj(u_j) v_j
                        den[s] = fmaf(uj[s].x, uj[s].x, fmaf(uj[s].y, uj[s].y, den[s]));
                    }
                    if (l == jl) {                                          // the row's owner parks u_j for the cross terms
#pragma unroll
                        for (int s = 0; s < S1; ++s) up[(jq * S + s) * 256] = uj[s];
                    }
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
#pragma unroll
                        for (int s = 0; s < S1; ++s) rd[s][q] = cnmac(rd[s][q], lq, uj[s]);
                        rx[q] = cnmac(rx[q], lq, vj);
                    }
                }
            });
            if (silent) {
                // digital silence so far: w = d/M per direction, the operations and the bits of k_mvdr_solve_sources
                float2 y[S1], xr[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) xr[q] = 4 * q + l < M ? X[(long long)t * fstride + 4 * q] : make_float2(0.f, 0.f);
#pragma unroll
                for (int s = 0; s < S1; ++s) {
                    float2 d[Q];
                    mvdr_steer_rows<Q, false>(d, T, (long long)t * S + s0 + s, M, nph, lo_off, l);
                    float2 acc = make_float2(0.f, 0.f);
#pragma unroll
                    for (int q = 0; q < Q; ++q) acc = cmacc(acc, xr[q], d[q]);   // conj(d_i) x_i
                    acc.x += __shfl_xor(acc.x, 1, 4); acc.y += __shfl_xor(acc.y, 1, 4);
                    acc.x += __shfl_xor(acc.x, 2, 4); acc.y += __shfl_xor(acc.y, 2, 4);
                    y[s] = make_float2(acc.x / (float)M, acc.y / (float)M);
                }
                float2 ys = y[0];
#pragma unroll
                for (int s = 1; s < S1; ++s) if (l == s) ys = y[s];
                if (l < S1 && pv) yo[((long long)(s0 + l) * F + t) * K] = ys;
            }
            if constexpr (PASSES) {
#pragma unroll
                for (int s = 0; s < S1; ++s) { Ns[(s0 + s) * 256 + tid] = num[s]; Ds[(s0 + s) * 256 + tid] = den[s]; }
            } else {
#pragma unroll
                for (int s = 0; s < S1; ++s) { bq[s] = num[s]; gd[s] = den[s]; }
            }
            s0 += S1;
            if (S1 == S || s0 >= S) break;
#pragma unroll
            for (int q = 0; q < Q; ++q) rx[q] = 4 * q + l < M ? X[(long long)t * fstride + 4 * q] : make_float2(0.f, 0.f);
#pragma unroll
            for (int s = 0; s < S1; ++s) mvdr_steer_rows<Q, false>(rd[s], T, (long long)t * S + s0 + s, M, nph, lo_off, l);
        }
        if (silent) continue;
        if constexpr (PASSES) {
#pragma unroll
            for (int s = 0; s < S; ++s) { bq[s] = Ns[s * 256 + tid]; gd[s] = Ds[s * 256 + tid]; }
        }
        // G_ab = sum_j conj(u_j[a]) u_j[b], a < b: the rows of this lane, then the quad
        float2 c[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) c[i] = make_float2(0.f, 0.f);
#pragma unroll
        for (int q = 0; q < Q; ++q)
            if (4 * q + l < M) {
                float2 u[S];
#pragma unroll
                for (int s = 0; s < S; ++s) u[s] = Us[(q * S + s) * 256 + tid];
#pragma unroll
                for (int sa = 0; sa < S; ++sa)
#pragma unroll
                    for (int sb = sa + 1; sb < S; ++sb) c[mvdr_pair(S, sa, sb)] = cmacc(c[mvdr_pair(S, sa, sb)], u[sb], u[sa]);
            }
        float rs[S];
        float2 beta[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            rs[s] = __builtin_amdgcn_rsqf(gd[s]);
            beta[s] = make_float2(bq[s].x * rs[s], bq[s].y * rs[s]);
        }
#pragma unroll
        for (int sa = 0; sa < S; ++sa)
#pragma unroll
            for (int sb = sa + 1; sb < S; ++sb) {
                float2 &e_ = c[mvdr_pair(S, sa, sb)];
                const float w = rs[sa] * rs[sb];
                e_ = make_float2(quad_sum(e_.x) * w, quad_sum(e_.y) * w);
            }
        const float g = pa.null_gain;
        float2 ys = make_float2(0.f, 0.f);
        mvdr_static_for<0, S>([&](auto sc) __attribute__((always_inline)) {
            constexpr int s = decltype(sc)::value;
            const float2 y = mvdr_null_output<S, s>(c, beta, rs, g);
            if (l == s) ys = y;
        });
        // every lane of the quad holds the S results: lane s stores direction s
        if (l < S && pv) yo[((long long)l * F + t) * K] = ys;
    }
    if (pv && t_last == F) {
        float2 *so = p.phi_out + (pc - p.out_base) * tri;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int i = 4 * q + l;
#pragma unroll
            for (int m = 0; m < 4 * (q + 1); ++m)
                if (i < M && m <= i) so[i * (i + 1) / 2 + m] = P[2 * q * (q + 1) + m];
        }
        if (l == 0) p.trace_out[pc - p.out_base] = tr;
    }
}

#define MCA_MVDR_NULLS_INST(Q, S, S1, PF) template __global__ void k_mvdr_nulls<Q, S, S1, PF>(MvdrNullsArgs);
MCA_MVDR_NULLS_TABLE(MCA_MVDR_NULLS_INST)
#undef MCA_MVDR_NULLS_INST

}  // namespace mca
