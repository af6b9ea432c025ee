// kernels_mvdr_spectrum.hip -- the Capon (minimum-variance) spatial spectrum of the covariance an MVDR context holds (gfx950;
// include/mcarray_hip.h, mca_hip_mvdr_spectrum_*).  A translation unit of its own:
// the solve kernels keep the instruction streams they have.  Read-only on the stream state.
//
//     PhiL[k] = Phi[k] + loading tr[k]/M I,   q[k][i] = d(theta_i,k)^H PhiL[k]^-1 d(theta_i,k),   P[i] = sum_k w[k] / q[k][i]
//
// Route: PhiL / (tr/M) = L L^H (the unit-trace-per-microphone matrix: its factor and q' = ||L^-1 d||^2 = q tr/M are dimensionless
// and lie between ~M/(1 + loading) and ~M/loading whatever the signal level), so w'/q' with w' = 1 (NORMALISED) or tr/M (POWER).
// q' is a sum of squares: only cond(L) enters its error, nothing cancels at a peak.
#include "mca_internal.h"
#include "mvdr_solve.h"

namespace mca {

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

template <int Q>
__global__ __launch_bounds__(256, 2) void k_mvdr_spectrum(MvdrSpectrumArgs p)
{
    constexpr int NE = 2 * Q * (Q + 1);          // row slot q holds 4 (q + 1) entries, starting at 2 q (q + 1)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int M = p.M, tri = M * (M + 1) / 2;
    float2 *Ls = reinterpret_cast<float2 *>(smem_raw);                 // [64][tri]: L below the diagonal, (1 / L_jj, 0) on it
    float *Ws = reinterpret_cast<float *>(Ls + MVDR_SPEC_CHUNK * tri); // [64]: w' of the bin, 0 for a bin that contributes nothing
    const int tid = threadIdx.x, l = tid & 3, b = tid >> 2;
    const int a = (int)(blockIdx.x / (unsigned)p.n_chunks), ci = (int)(blockIdx.x % (unsigned)p.n_chunks);
    const int kbase = MVDR_SPEC_CHUNK * (p.chunk0 + ci);

    // ---- the factor of every bin of the chunk, one quad per bin (the column loop of k_mvdr_solve without right-hand sides) ----
    {
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
    __syncthreads();

    // ---- the scan: wave wv takes the bins wv, wv + 4, ... of the chunk, its lanes the angles, two passes of 64 at a time ----
    const int wv = tid >> 6, lane = tid & 63;
    float *po = p.part + (((long long)a * p.n_chunks + ci) * 4 + wv) * p.Dpad;
    int a0 = lane;
    for (; a0 + 64 < p.Dpad; a0 += 128) mvdr_spectrum_scan<Q, 2>(p, Ls, Ws, tri, kbase, wv, a0, po);
    if (a0 < p.Dpad) mvdr_spectrum_scan<Q, 1>(p, Ls, Ws, tri, kbase, wv, a0, po);
}

template __global__ void k_mvdr_spectrum<1>(MvdrSpectrumArgs);
template __global__ void k_mvdr_spectrum<2>(MvdrSpectrumArgs);
template __global__ void k_mvdr_spectrum<3>(MvdrSpectrumArgs);
template __global__ void k_mvdr_spectrum<4>(MvdrSpectrumArgs);

// One workgroup per stream: P[i] = the partial sums of the stream in (chunk, wave) order -- no atomics, the same bytes on every
// run -- then the peaks (include/mcarray_hip.h: local maxima ranked by value, ties to the lower index; empty slots repeat slot 0
// with value 0).  At most 361 angles and 4 peaks: one lane walks the row.
__global__ __launch_bounds__(256) void k_mvdr_spectrum_pick(MvdrSpectrumPickArgs p)
{
    __shared__ float Ps[MVDR_SPEC_MAX_ANGLES + 1];
    const int a = blockIdx.x, D = p.D;
    const float *part = p.part + (long long)a * p.n_slices * p.Dpad;
    for (int i = threadIdx.x; i < D; i += 256) {
        float s = 0.f;
        for (int sl = 0; sl < p.n_slices; ++sl) s += part[(long long)sl * p.Dpad + i];
        Ps[i] = s;
        if (p.spectrum) p.spectrum[(long long)a * D + i] = s;
    }
    if (!p.peak_doa && !p.peak_val) return;
    __syncthreads();
    if (threadIdx.x != 0) return;
    float val[MCA_MAX_SOURCES];
    int idx[MCA_MAX_SOURCES];
#pragma unroll
    for (int r = 0; r < MCA_MAX_SOURCES; ++r) { val[r] = -1.f; idx[r] = -1; }
    for (int i = 0; i < D; ++i) {
        const float v = Ps[i];
        // on the periodic grid of XYZ mode the ends are neighbours: a row end is a peak only against the other end too
        const bool lo = i > 0 ? v > Ps[i - 1] : (!p.circular || v > Ps[D - 1]);
        const bool hi = i < D - 1 ? v >= Ps[i + 1] : (!p.circular || v >= Ps[0]);
        if (!(v > 0.f) || !lo || !hi) continue;
        float cv = v;
        int ci = i;
        bool ins = false;                        // once inserted, the displaced entries move down a slot each
#pragma unroll
        for (int r = 0; r < MCA_MAX_SOURCES; ++r)
            if (r < p.n_peaks && (ins || cv > val[r])) {
                const float tv = val[r]; const int ti = idx[r];
                val[r] = cv; idx[r] = ci; cv = tv; ci = ti; ins = true;
            }
    }
    const float first = idx[0] >= 0 ? p.grid[idx[0]] : 0.f;
#pragma unroll
    for (int r = 0; r < MCA_MAX_SOURCES; ++r)
        if (r < p.n_peaks) {
            const bool has = idx[r] >= 0;
            if (p.peak_doa) p.peak_doa[(long long)a * p.n_peaks + r] = has ? p.grid[idx[r]] : first;
            if (p.peak_val) p.peak_val[(long long)a * p.n_peaks + r] = has ? val[r] : 0.f;
        }
}

}  // namespace mca
