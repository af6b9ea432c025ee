// mvdr_solve.h -- k_mvdr_solve_t, the one template of the MVDR solve (gfx950), its arms k_mvdr_solve_rtf_t that takes the
// steering vectors from a plane (4.8) and k_mvdr_solve_rtf_nulls_t that puts soft nulls at those vectors (4.10), and the lookups that
// instantiate them.
// The translation units kernels_mvdr_solve_*.hip instantiate one (WEIGHT, NOISE) group each (build parallelism, nothing else); the
// hand-written single-look kernel k_mvdr_solve of kernels_mvdr.hip shares the helpers below.
//
// Per stream a, bin k and frame t (kernels_mvdr.hip has the definitions and the four-lanes-per-problem layout):
//     Phi_t = a_t Phi_{t-1} + (1 - a_t) x x^H,  tr_t = a_t tr_{t-1} + (1 - a_t) |x|^2,  PhiL = Phi_t + loading tr_t / M I = L L^H
//     u_s = L^-1 d_s,  v = L^-1 x,  Y_s = (u_s^H v) / (u_s^H u_s)          for the S look directions of the frame
// The recursion, the pivots, L and v do not depend on the look direction; a direction adds its own u (rd, num, den: about 11
// registers with four row slots).  S1 directions ride one pass of the column loop; with S1 < S a further pass repeats the
// factorisation.  The frame's loads and the recursion happen once in any case.  Every direction runs exactly the operations of
// k_mvdr_solve in its order (the complex helpers are inline asm), so output s has the bits of a single-look launch with that
// direction.  mvdr_solve_form (mca_internal.h) says which S1, PF and REUSE a row takes, and why.
//
// WEIGHT: a_t = 1 - (1 - alpha) u with u = fminf(fmaxf(w, 0), 1) (a NaN weight becomes 0), w = update[a][t]
// (FRAME) or update[(a F + t) K + k] (CELL).  u == 1 takes the context's own fp32 alpha and 1 - alpha, the operations of a kernel
// without weights; u == 0 does not touch Phi and tr at all.  NONE reads no weight and is the u == 1 arm at compile time.
// CELL: the four lanes of a quad read one address, the 64 quads of a workgroup 64 consecutive floats.  frozen is then the quad's
// own and the recursion a divergent branch; every quad_bcast / quad_sum / __shfl_xor(.., 4) stays inside a quad, whose four lanes
// take the branch together (the silence branch has always been per quad).
//
// REUSE (FRAME only): a frame with u == 0 that follows a frame this workgroup has solved finds PhiL, and with it L and the inverse
// pivots, as that frame left them.  L lives in registers across the frame loop anyway; the inverse pivot of row j is kept by the
// lane that owns the row (Q more registers).  Such a frame runs only the forward substitutions of its columns -- the same
// operations in the same order on the same L bits as a frame that factorises, so its output does not depend on which of the two
// it did.  The first solved frame of a launch or of a piece always factorises.
//
// NULLS (mvdr_nulls.h): a soft null of gain g = null_gain > 0 at every other look direction of the frame,
//     p_r = 1 / (d_r^H PhiL^-1 d_r),  Phi_s = PhiL + g sum_{r != s} p_r d_r d_r^H,  Y_s = w_s^H x,  w_s = Phi_s^-1 d_s / (d_s^H Phi_s^-1 d_s)
// With U = L^-1 [d_0 ... d_{S-1}], G = U^H U, b = U^H v and R the other directions of s (matrix inversion lemma):
//     (g G_RR + diag G_RR) q = g G_Rs,  Y_s = (b_s - q^H b_R) / (G_ss - q^H G_Rs)
// b_s and G_ss are num[s] and den[s]; the off-diagonal G and one (S-1) x (S-1) Hermitian solve per direction come on top, evaluated
// on the normalised quantities c_ab = G_ab / sqrt(G_aa G_bb) (|c| <= 1), beta_a = b_a / sqrt(G_aa):
//     (I + g C_RR) z = g c_Rs,  Y_s = (beta_s - z^H beta_R) / (sqrt(G_ss) (1 - z^H c_Rs))
// so that nothing of the order G^2 is formed (G ~ M / power reaches 1e31 at the silence threshold).  The pairs of directions of
// different passes never meet in registers, and four row slots with three directions have no registers left for six more
// accumulators.  So the lane that owns row j parks the u_j[s] it has just scaled in LDS (words [q][s][thread]: conflict free, read
// back by the thread that wrote them, no synchronisation), a pass of a kernel with several passes parks its num and den the same
// way, and after the last pass -- L is dead by then -- every lane sums conj(u_j[a]) u_j[b] over its own rows, the quad adds the four
// partial sums (DPP), and every lane holds G.  The small solves are written out per direction with compile-time indices (every
// lane computes all S of them; lane s stores output s).  LDS: mvdr_nulls_lds_bytes, 44 KiB at Q = S = 4.
//
// NOISE: the lane that stores Y[(s F + t) K + k] also stores the residual noise power of the plain estimate of that
// direction, 1 / (d_s^H PhiL_t^-1 d_s), to pn at the same index (fp32) -- the reciprocal of den[s] that the output divides by (the
// plain den[s] = G_ss also under the nulls) -- and 0 for a bin that is digitally silent so far.  Stored for t >= t_first only, like Y.
#pragma once
#include "fft512.h"
#include "fft_block.h"
#include "mca_internal.h"

#include <type_traits>

namespace mca {

template <int B>
__device__ __forceinline__ float quad_bcast1(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), B * 0x55, 0xf, 0xf, true));   // quad_perm:[B,B,B,B]
}
__device__ __forceinline__ float quad_bcast(float v, int b)
{
    switch (b) {
    case 0: return quad_bcast1<0>(v);
    case 1: return quad_bcast1<1>(v);
    case 2: return quad_bcast1<2>(v);
    default: return quad_bcast1<3>(v);
    }
}
__device__ __forceinline__ float2 quad_bcast(float2 v, int b) { return make_float2(quad_bcast(v.x, b), quad_bcast(v.y, b)); }

// f(integral_constant<int, J0>), ..., f(integral_constant<int, J1 - 1>): the column loop of the solve kernels written out at compile time.  As
// a "#pragma unroll" loop it passes the size up to which the compiler honours the pragma once a column carries three right-hand
// sides, and a loop left rolled puts L and P into scratch.
template <int J0, int J1, class Fn>
__host__ __device__ __forceinline__ void mvdr_static_for(Fn &&f)
{
    if constexpr (J0 < J1) {
        f(std::integral_constant<int, J0>{});
        mvdr_static_for<J0 + 1, J1>(f);
    }
}

// steering d_i of look direction s in frame t for the rows of this lane (T already offset to the stream and k >> 5)
template <int Q, bool FULL>
__device__ __forceinline__ void mvdr_steer_rows(float2 (&d)[Q], const float2 *T, long long ts, int M, int nph, int lo_off, int l)
{
    float2 th[Q], tl[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const float2 *tq = T + (ts * M + ((FULL || 4 * q + l < M) ? 4 * q + l : 0)) * nph;
        th[q] = tq[0]; tl[q] = tq[lo_off];
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) d[q] = (FULL || 4 * q + l < M) ? cmul(th[q], tl[q]) : make_float2(0.f, 0.f);
}

}  // namespace mca

#include "mvdr_nulls.h"   // the small solves of NULLS, on the helpers above

namespace mca {

// The body of the solve kernels.  RTF: the right-hand sides of the S look directions are not formed from the factored
// phasors T but read from the steering plane D [stream][slot][frame][bin][mic] that k_mvdr_rtf (kernels_mvdr_rtf.hip) wrote -- the
// way X is read -- and so is the vector of the silence branch (k_mvdr_rtf leaves the geometric vector in the cells of a silent bin).
// Nothing else differs: a plane that holds cmul(T_hi, T_lo) gives the bits of the kernel without RTF.
// RTF with NULLS (4.10): the nulls algebra needs only U = L^-1 [d_0 ... d_{S-1}] and p_r d_r d_r^H does not depend on the scale of d_r,
// so the vectors of the plane -- normalised to the reference microphone, or the geometric vector where the estimator fell back --
// enter it as they are.
template <int Q, bool FULL, int S, int S1, bool PF, bool NULLS, bool REUSE, MvdrWeight WEIGHT, bool NOISE, bool RTF>
__device__ __forceinline__ void mvdr_solve_body(const MvdrSolveArgs &p)
{
    static_assert(!RTF || WEIGHT == MvdrWeight::CELL, "the steering plane comes with the masks");
    constexpr bool WEIGHTED = WEIGHT != MvdrWeight::NONE, CELL = WEIGHT == MvdrWeight::CELL;
    static_assert(!REUSE || WEIGHT == MvdrWeight::FRAME, "no frame is frozen without weights; a wave of quads with weights of their own would run both column bodies");
    static_assert(S >= 1 && S <= MCA_MAX_SOURCES && S1 >= 1 && S % S1 == 0, "look directions per frame, in whole passes");
    static_assert(!NULLS || (S >= 2 && !FULL), "the nulls need another direction; their kernel has no branch-free M = 4Q form");
    static_assert(NULLS || PF || NOISE || WEIGHT == MvdrWeight::CELL, "only the nulls kernel, and a NOISE or CELL row that needs the registers, give up the load a frame ahead");
    constexpr int NE = 2 * Q * (Q + 1);          // row slot q holds 4 (q + 1) entries, starting at 2 q (q + 1)
    constexpr int NP = NULLS ? S * (S - 1) / 2 : 1;   // pairs of look directions
    constexpr bool PASSES = S1 < S;
    // dynamic LDS of the nulls, sized by the launch (mvdr_nulls_lds_bytes)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2 *Us = reinterpret_cast<float2 *>(smem_raw);      // [q][s][thread]: u_{4q+l}[s] of the thread's problem, by the row's owner
    float2 *Ns = Us + Q * S * 256;                          // [s][thread]: num of every pass (PASSES only)
    float *Ds = reinterpret_cast<float *>(Ns + S * 256);    // [s][thread]: den
    const int tid = threadIdx.x, l = tid & 3;
    const int M = p.M, K = p.K, F = p.n_frames;
    const int FL = RTF ? p.n_loop : F;          // frames of the launch (RTF: a chunk of the call, F stays the stride of X, update, Y, pn)
    const int piece = (int)(blockIdx.x % (unsigned)p.pieces);
    const int t_first = (int)((long long)piece * FL / p.pieces), t_last = (int)((long long)(piece + 1) * FL / p.pieces);   // frames this workgroup solves
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
    // each kernel forms its own address only: FRAME update[a F + t], CELL update[(a F + t) K + k]
    const int uw0 = CELL ? 0 : a * F;                                       // + t: the weight of the frame, the same for the four lanes (< 2^31: T is larger)
    const float *um = CELL ? p.update + ((long long)a * F * K + k) : nullptr;     // + t K: the weight of the cell (64-bit index), the same for the four lanes
    float2 *yo = p.Y + (long long)a * S * F * K + k;                        // + (s F + t) K
    const float2 *Dp = RTF ? p.D + ((long long)a * S * FL * K + k) * M + l : nullptr;   // RTF: + ((s FL + t) K) M + 4 q
    // the steering vector of look direction s in frame t, the rows of this lane
    auto steer = [&](float2 (&d)[Q], int t, int s) __attribute__((always_inline)) {
        if constexpr (RTF) {
            const float2 *dq = Dp + ((long long)s * FL + t) * fstride;
#pragma unroll
            for (int q = 0; q < Q; ++q) d[q] = (FULL || 4 * q + l < M) ? dq[4 * q] : make_float2(0.f, 0.f);
        } else mvdr_steer_rows<Q, FULL>(d, T, (long long)t * S + s, M, nph, lo_off, l);
    };
    float *pno = NOISE ? p.pn : nullptr;                                   // NOISE: the same index
    if constexpr (NOISE) pno += (long long)a * S * F * K + k;

    float hp[Q];                                  // REUSE: inverse pivots of the rows of this lane, of the last frame that factorised
    bool have_l = false;                          // REUSE: L and hp are those of PhiL as it stands
#pragma unroll
    for (int q = 0; q < Q; ++q) hp[q] = 0.f;
    float2 xn[Q];                                 // the next frame's spectra, loaded a frame ahead (PF)
#pragma unroll
    for (int q = 0; q < Q; ++q) xn[q] = (PF && (FULL || 4 * q + l < M)) ? X[4 * q] : make_float2(0.f, 0.f);
    for (int t = 0; t < t_last; ++t) {
        float2 x[Q], rd[S1][Q], rx[Q];
        float dsum[Q];
        // the loads of the frame first, the weight among them
        const long long tn = (long long)min(t + 1, t_last - 1) * fstride;
        float w = 1.f;
        if constexpr (WEIGHTED) w = CELL ? um[(long long)t * K] : p.update[uw0 + t];
#pragma unroll
        for (int q = 0; q < Q; ++q) x[q] = PF ? xn[q] : ((FULL || 4 * q + l < M) ? X[(long long)t * fstride + 4 * q] : make_float2(0.f, 0.f));
        if (t >= t_first) {
#pragma unroll
            for (int s = 0; s < S1; ++s) steer(rd[s], t, s);
        }
        if constexpr (PF) {
#pragma unroll
            for (int q = 0; q < Q; ++q) xn[q] = (FULL || 4 * q + l < M) ? X[tn + 4 * q] : make_float2(0.f, 0.f);
        }
        if constexpr (WEIGHTED) w = fminf(fmaxf(w, 0.f), 1.f);   // NaN -> 0
        const bool frozen = !(w > 0.f);             // NONE: never, and the recursion below is the w == 1 arm at compile time
        if (!frozen) {
            // Phi <- a Phi + b x x^H (the rows of this lane), tr <- a tr + b |x|^2; b = (1 - alpha) u, a = 1 - b, and at u == 1 the
            // context's own 1 - alpha and alpha
            const float bt = w == 1.f ? oma : oma * w, at = w == 1.f ? al : 1.f - oma * w;
            float e = 0.f;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float2 xs = make_float2(bt * x[q].x, bt * x[q].y);
#pragma unroll
                for (int m = 0; m < 4 * (q + 1); ++m)
                    if (FULL || m < M) {
                        const float2 xm = quad_bcast(x[m >> 2], m & 3);
                        float2 &e_ = P[2 * q * (q + 1) + m];
                        e_ = cmacc(make_float2(at * e_.x, at * e_.y), xs, xm);
                        if (q == Q - 1) e = fmaf(xm.x, xm.x, fmaf(xm.y, xm.y, e));
                    }
            }
            tr = fmaf(at, tr, bt * e);
        }
        if (t < t_first) continue;               // (an earlier piece solves this frame)
        const bool reuse = REUSE && frozen && have_l;
        have_l = true;
        // The loading as k_mvdr_solve applies it, which the compiler decides there and this kernel has to repeat to keep its bits:
        // with all columns in one basic block (FULL) the product is contracted into the pivot, fma(loading, tr, Phi_jj); behind
        // the "j < M" branches it is rounded on its own first.  Spelled out here, because the loop over the passes moves the
        // product out of the columns' block and would leave that choice to chance.
        float delta = p.loading_over_m * tr;
        asm volatile("" : "+v"(delta));
        const bool silent = !(tr > 1e-30f);       // the same in the four lanes of a quad
        if constexpr (NULLS) {
            // x does not ride the column loop: a further pass and the silence branch read the frame again (8 registers at Q = 4)
#pragma unroll
            for (int q = 0; q < Q; ++q) rx[q] = x[q];
        }

        float2 bq[S];                             // NULLS: b_s = num and G_ss = den of every direction
        float gd[S];
        // one pass per S1 look directions, s0 ... s0 + S1 - 1
#pragma unroll 1
        for (int s0 = 0;;) {
            float2 num[S1];
            float den[S1];
#pragma unroll
            for (int s = 0; s < S1; ++s) { num[s] = make_float2(0.f, 0.f); den[s] = 0.f; }
#pragma unroll
            for (int q = 0; q < Q; ++q) { if (!NULLS) rx[q] = x[q]; dsum[q] = 0.f; }
            float2 *up = Us + s0 * 256 + tid;
            // the columns; SUB: substitutions only, against the held L and inverse pivots
            auto columns = [&](auto subc) __attribute__((always_inline)) {
                constexpr bool SUB = decltype(subc)::value;
                mvdr_static_for<0, 4 * Q>([&](auto jc) __attribute__((always_inline)) {
                    constexpr int j = decltype(jc)::value, jq = j >> 2, jl = j & 3, jo = 2 * jq * (jq + 1);
                    if (FULL || j < M) {
                        // pivot and the substitution values of row j, from its owner
                        float inv;
                        if constexpr (SUB) inv = quad_bcast1<jl>(hp[jq]);
                        else {
                            // (NULLS: what the compiler chose for the kernel this one replaced -- contracted in column 0, and in every column of
                            // the two-pass instantiation, rounded on its own elsewhere)
                            const float pjj = (FULL || (NULLS && (PASSES || j == 0))) ? fmaf(p.loading_over_m, tr, P[jo + j].x) : P[jo + j].x + delta;
                            inv = __builtin_amdgcn_rsqf(quad_bcast1<jl>(pjj - dsum[jq]));
                            if constexpr (REUSE) hp[jq] = l == jl ? inv : hp[jq];
                        }
                        float2 uj[S1], vj = quad_bcast(rx[jq], jl);
                        vj = make_float2(vj.x * inv, vj.y * inv);
#pragma unroll
                        for (int s = 0; s < S1; ++s) {
                            uj[s] = quad_bcast(rd[s][jq], jl);
                            uj[s] = make_float2(uj[s].x * inv, uj[s].y * inv);
                            num[s] = cmacc(num[s], vj, uj[s]);                  // conj(u_j) v_j
                            den[s] = fmaf(uj[s].x, uj[s].x, fmaf(uj[s].y, uj[s].y, den[s]));
                        }
                        if constexpr (NULLS) {
                            if (l == jl) {                                      // the row's owner parks u_j for the cross terms
#pragma unroll
                                for (int s = 0; s < S1; ++s) up[(jq * S + s) * 256] = uj[s];
                            }
                        }
                        if constexpr (!SUB) {
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
                            }
                        }
#pragma unroll
                        for (int q = jq; q < Q; ++q) {
                            const float2 lq = L[2 * q * (q + 1) + j];
#pragma unroll
                            for (int s = 0; s < S1; ++s) rd[s][q] = cnmac(rd[s][q], lq, uj[s]);
                            rx[q] = cnmac(rx[q], lq, vj);
                        }
                    }
                });
            };
            if constexpr (REUSE) {
                if (reuse) columns(std::true_type{});
                else columns(std::false_type{});
            } else columns(std::false_type{});
            float2 y[S1];
            float pr = 0.f;                       // NOISE: 1 / den of the direction this lane stores
            if constexpr (!NULLS) {
#pragma unroll
                for (int s = 0; s < S1; ++s) {
                    const float rden = __builtin_amdgcn_rcpf(den[s]);
                    y[s] = make_float2(num[s].x * rden, num[s].y * rden);
                    if constexpr (NOISE) pr = (s == 0 || l == s) ? rden : pr;
                }
            }
            if (NULLS ? silent : !(tr > 1e-30f)) {
                // digital silence so far: w = d/M, the reference's delay-and-sum (Beamformer.cpp:51-71), per direction
                float2 xr[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) xr[q] = !NULLS ? x[q] : ((FULL || 4 * q + l < M) ? X[(long long)t * fstride + 4 * q] : make_float2(0.f, 0.f));
#pragma unroll
                for (int s = 0; s < S1; ++s) {
                    float2 d[Q];
                    steer(d, t, s0 + s);
                    float2 acc = make_float2(0.f, 0.f);
#pragma unroll
                    for (int q = 0; q < Q; ++q) acc = cmacc(acc, xr[q], d[q]);   // conj(d_i) x_i
                    acc.x += __shfl_xor(acc.x, 1, 4); acc.y += __shfl_xor(acc.y, 1, 4);
                    acc.x += __shfl_xor(acc.x, 2, 4); acc.y += __shfl_xor(acc.y, 2, 4);
                    y[s] = make_float2(acc.x / (float)M, acc.y / (float)M);
                }
                if constexpr (NOISE) pr = 0.f;
            }
            if (!NULLS || silent) {
                // every lane of the quad holds the S1 results: lane s stores direction s0 + s
                float2 ys = y[0];
#pragma unroll
                for (int s = 1; s < S1; ++s) if (l == s) ys = y[s];
                if (l < S1 && pv) {
                    yo[((long long)(s0 + l) * F + t) * K] = ys;
                    if constexpr (NOISE) pno[((long long)(s0 + l) * F + t) * K] = pr;
                }
            }
            if constexpr (NULLS) {
                if constexpr (PASSES) {
#pragma unroll
                    for (int s = 0; s < S1; ++s) { Ns[(s0 + s) * 256 + tid] = num[s]; Ds[(s0 + s) * 256 + tid] = den[s]; }
                } else {
#pragma unroll
                    for (int s = 0; s < S1; ++s) { bq[s] = num[s]; gd[s] = den[s]; }
                }
            }
            s0 += S1;
            if (S1 == S || s0 >= S) break;
            if constexpr (NULLS) {
#pragma unroll
                for (int q = 0; q < Q; ++q) rx[q] = (FULL || 4 * q + l < M) ? X[(long long)t * fstride + 4 * q] : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int s = 0; s < S1; ++s) steer(rd[s], t, s0 + s);
        }
        if constexpr (NULLS) {
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
                    const float ww = rs[sa] * rs[sb];
                    e_ = make_float2(quad_sum(e_.x) * ww, quad_sum(e_.y) * ww);
                }
            const float g = p.null_gain;
            float2 ys = make_float2(0.f, 0.f);
            mvdr_static_for<0, S>([&](auto sc) __attribute__((always_inline)) {
                constexpr int s = decltype(sc)::value;
                const float2 y = mvdr_null_output<S, s>(c, beta, rs, g);
                if (l == s) ys = y;
            });
            // every lane of the quad holds the S results: lane s stores direction s
            if (l < S && pv) {
                yo[((long long)l * F + t) * K] = ys;
                if constexpr (NOISE) {
                    float gs = gd[0];
#pragma unroll
                    for (int s = 1; s < S; ++s) gs = l == s ? gd[s] : gs;
                    pno[((long long)l * F + t) * K] = __builtin_amdgcn_rcpf(gs);
                }
            }
        }
    }
    if (pv && t_last == FL) {
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

// grid (ceil(problems / 64) * pieces), 256 threads, dynamic LDS mvdr_nulls_lds_bytes (NULLS) or none
template <int Q, bool FULL, int S, int S1, bool PF, bool NULLS, bool REUSE, MvdrWeight WEIGHT, bool NOISE>
__global__ __launch_bounds__(256, 2) void k_mvdr_solve_t(MvdrSolveArgs p)
{
    mvdr_solve_body<Q, FULL, S, S1, PF, NULLS, REUSE, WEIGHT, NOISE, false>(p);
}

// the same with the right-hand sides from the steering plane; a weight per frame and bin, no nulls (mca_hip_mvdr_sources_frames_rtf_*)
template <int Q, bool FULL, int S, int S1, bool PF, bool NOISE>
__global__ __launch_bounds__(256, 2) void k_mvdr_solve_rtf_t(MvdrSolveArgs p)
{
    mvdr_solve_body<Q, FULL, S, S1, PF, false, false, MvdrWeight::CELL, NOISE, true>(p);
}

// the nulls of k_mvdr_solve_t at the vectors of the steering plane (mca_hip_mvdr_set_rtf_nulls); dynamic LDS
// mvdr_nulls_lds_bytes.  One instantiation serves M = 4Q and M < 4Q, as in the nulls kernel without RTF
template <int Q, int S, int S1, bool PF, bool NOISE>
__global__ __launch_bounds__(256, 2) void k_mvdr_solve_rtf_nulls_t(MvdrSolveArgs p)
{
    mvdr_solve_body<Q, false, S, S1, PF, true, false, MvdrWeight::CELL, NOISE, true>(p);
}

// The instantiation of a call, or nullptr where the build has none, and the dynamic LDS of its workgroups.  The definition is the
// row list: it names every (Q, FULL, S, NULLS) of mvdr_solve_row with the form of mvdr_solve_form, once, and a translation unit
// that instantiates it for its (WEIGHT, NOISE) thereby instantiates those kernels.
template <MvdrWeight WEIGHT, bool NOISE>
const void *mvdr_solve_kernel_of(int Q, bool full, int S, bool nulls, int *lds_bytes)
{
    const void *kernel = nullptr;
    mvdr_static_for<0, 4 * 2 * MCA_MAX_SOURCES * 2>([&](auto rc) {
        constexpr int r = decltype(rc)::value, RQ = r / (4 * MCA_MAX_SOURCES) + 1, RS = r / 4 % MCA_MAX_SOURCES + 1;
        constexpr bool RFULL = r & 1, RNULLS = r & 2;
        if constexpr (mvdr_solve_row(RQ, RFULL, RS, RNULLS, WEIGHT, NOISE)) {
            constexpr MvdrSolveForm f = mvdr_solve_form(RQ, RFULL, RS, RNULLS, WEIGHT, NOISE);
            if (Q == RQ && full == RFULL && S == RS && nulls == RNULLS) {
                kernel = reinterpret_cast<const void *>(k_mvdr_solve_t<RQ, RFULL, RS, f.S1, f.PF, RNULLS, f.REUSE, WEIGHT, NOISE>);
                *lds_bytes = RNULLS ? mvdr_nulls_lds_bytes(RQ, RS, f.S1) : 0;
            }
        }
    });
    return kernel;
}

// The same for k_mvdr_solve_rtf_t: every (Q, FULL, S) row without NULLS, with the form of the CELL row.
template <bool NOISE>
const void *mvdr_solve_rtf_kernel_of(int Q, bool full, int S)
{
    const void *kernel = nullptr;
    mvdr_static_for<0, 4 * 2 * MCA_MAX_SOURCES>([&](auto rc) {
        constexpr int r = decltype(rc)::value, RQ = r / (2 * MCA_MAX_SOURCES) + 1, RS = r / 2 % MCA_MAX_SOURCES + 1;
        constexpr bool RFULL = r & 1;
        constexpr MvdrSolveForm f = mvdr_solve_form(RQ, RFULL, RS, false, MvdrWeight::CELL, NOISE);
        if (Q == RQ && full == RFULL && S == RS) kernel = reinterpret_cast<const void *>(k_mvdr_solve_rtf_t<RQ, RFULL, RS, f.S1, f.PF, NOISE>);
    });
    return kernel;
}

// The same for k_mvdr_solve_rtf_nulls_t: every (Q, S >= 2), with the form of the CELL nulls row, and the dynamic LDS of its workgroups.
template <bool NOISE>
const void *mvdr_solve_rtf_nulls_kernel_of(int Q, int S, int *lds_bytes)
{
    const void *kernel = nullptr;
    mvdr_static_for<0, 4 * (MCA_MAX_SOURCES - 1)>([&](auto rc) {
        constexpr int r = decltype(rc)::value, RQ = r / (MCA_MAX_SOURCES - 1) + 1, RS = r % (MCA_MAX_SOURCES - 1) + 2;
        constexpr MvdrSolveForm f = mvdr_solve_form(RQ, false, RS, true, MvdrWeight::CELL, NOISE);
        if (Q == RQ && S == RS) {
            kernel = reinterpret_cast<const void *>(k_mvdr_solve_rtf_nulls_t<RQ, RS, f.S1, f.PF, NOISE>);
            *lds_bytes = mvdr_nulls_lds_bytes(RQ, RS, f.S1);
        }
    });
    return kernel;
}

}  // namespace mca
