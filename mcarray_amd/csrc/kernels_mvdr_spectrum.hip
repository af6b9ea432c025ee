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
#include "mvdr_spectrum_scan.h"

namespace mca {

template <int Q>
__global__ __launch_bounds__(256, 2) void k_mvdr_spectrum(MvdrSpectrumArgs p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int M = p.M, tri = M * (M + 1) / 2;
    float2 *Ls = reinterpret_cast<float2 *>(smem_raw);                 // [64][tri]: L below the diagonal, (1 / L_jj, 0) on it
    float *Ws = reinterpret_cast<float *>(Ls + MVDR_SPEC_CHUNK * tri); // [64]: w' of the bin, 0 for a bin that contributes nothing
    const int tid = threadIdx.x;
    const int a = (int)(blockIdx.x / (unsigned)p.n_chunks), ci = (int)(blockIdx.x % (unsigned)p.n_chunks);
    const int kbase = MVDR_SPEC_CHUNK * (p.chunk0 + ci);

    // ---- the factor of every bin of the chunk, one quad per bin (mvdr_spectrum_scan.h) ----
    mvdr_spectrum_factor<Q>(p, a, kbase, Ls, Ws);
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

const void *mvdr_spectrum_kernel(int Q)
{
    return Q == 1 ? reinterpret_cast<const void *>(k_mvdr_spectrum<1>) : Q == 2 ? reinterpret_cast<const void *>(k_mvdr_spectrum<2>)
         : Q == 3 ? reinterpret_cast<const void *>(k_mvdr_spectrum<3>) : reinterpret_cast<const void *>(k_mvdr_spectrum<4>);
}

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
