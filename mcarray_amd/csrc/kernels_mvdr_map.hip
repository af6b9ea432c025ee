// kernels_mvdr_map.hip -- the Capon spatial spectrum of the covariance an MVDR context holds on a grid of azimuths x elevations
// (gfx950; include/mcarray_hip.h, mca_hip_mvdr_map_*).  The quantity, the factor-and-substitute route and the
// arithmetic per (bin, direction) are those of kernels_mvdr_spectrum.hip (mvdr_spectrum_scan.h); new here are the cut of the flat
// list of directions into tiles and the peak rule on the grid.  Read-only on the stream state.
#include "mca_internal.h"
#include "mvdr_solve.h"
#include "mvdr_spectrum_scan.h"

namespace mca {

// One (stream, chunk of 64 bins, tile of MVDR_MAP_TILE directions) per workgroup.  k_mvdr_spectrum<Q> gives a workgroup every angle of
// its chunk; at 2048 directions that would leave a stream on N/128 + 1 workgroups, each with 16 passes of the scan.  The tile is 128
// directions, one <Q, 2> pass per wave (two directions per lane): the register shape the sibling holds at two workgroups per CU,
// and 16 times the workgroups.  Every tile factors its chunk again: 64 factors of M^3/6 multiply-adds against 64 x 128
// substitutions of M^2/2, 1/24 of the tile's work at 16 microphones.
template <int Q>
__global__ __launch_bounds__(256, 2) void k_mvdr_map_scan(MvdrMapScanArgs pa)
{
    const MvdrSpectrumArgs &p = pa.s;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int M = p.M, tri = M * (M + 1) / 2;
    float2 *Ls = reinterpret_cast<float2 *>(smem_raw);                 // [64][tri]: L below the diagonal, (1 / L_jj, 0) on it
    float *Ws = reinterpret_cast<float *>(Ls + MVDR_SPEC_CHUNK * tri); // [64]: w' of the bin, 0 for a bin that contributes nothing
    const int tid = threadIdx.x;
    // the stream runs fastest over the grid: the workgroups resident at one time share a few (chunk, tile) slices of the phasor
    // table (34 rows x M x 128 directions, 544 KiB at M = 16) in L2 and differ in the 68 KiB of covariance they factor
    const unsigned ct = blockIdx.x / (unsigned)pa.n_streams;
    const int a = (int)(blockIdx.x % (unsigned)pa.n_streams);
    const int t = (int)(ct % (unsigned)pa.n_tiles), ci = (int)(ct / (unsigned)pa.n_tiles);
    const int kbase = MVDR_SPEC_CHUNK * (p.chunk0 + ci);

    mvdr_spectrum_factor<Q>(p, a, kbase, Ls, Ws);
    __syncthreads();

    // wave wv takes the bins wv, wv + 4, ... of the chunk; the last tile may hold one block of 64 directions only (Dpad is whole waves)
    const int wv = tid >> 6, lane = tid & 63;
    float *po = p.part + (((long long)a * p.n_chunks + ci) * 4 + wv) * p.Dpad;
    const int a0 = t * MVDR_MAP_TILE + lane;
    if (a0 + 64 < p.Dpad) mvdr_spectrum_scan<Q, 2>(p, Ls, Ws, tri, kbase, wv, a0, po);
    else if (a0 < p.Dpad) mvdr_spectrum_scan<Q, 1>(p, Ls, Ws, tri, kbase, wv, a0, po);
}

template __global__ void k_mvdr_map_scan<1>(MvdrMapScanArgs);
template __global__ void k_mvdr_map_scan<2>(MvdrMapScanArgs);
template __global__ void k_mvdr_map_scan<3>(MvdrMapScanArgs);
template __global__ void k_mvdr_map_scan<4>(MvdrMapScanArgs);

const void *mvdr_map_scan_kernel(int Q)
{
    return Q == 1 ? reinterpret_cast<const void *>(k_mvdr_map_scan<1>) : Q == 2 ? reinterpret_cast<const void *>(k_mvdr_map_scan<2>)
         : Q == 3 ? reinterpret_cast<const void *>(k_mvdr_map_scan<3>) : reinterpret_cast<const void *>(k_mvdr_map_scan<4>);
}

// the better of two candidates: the larger value, then the lower flat index
__device__ __forceinline__ void map_better(float &v, int &i, float ov, int oi)
{
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// One workgroup per stream: P = the partial sums of the stream in (chunk, wave) order -- no atomics, the same bytes on every run --
// then the peaks (include/mcarray_hip.h).  Thread t owns the cells t, t + 256, ... (8 at most): it tests them against their 8
// neighbours, keeps a bit per local maximum, and n_peaks rounds of a workgroup arg-max take the maxima out in rank order.
__global__ __launch_bounds__(256) void k_mvdr_map_pick(MvdrMapPickArgs p)
{
    constexpr int CPT = MVDR_MAP_MAX_DIRS / 256;
    __shared__ float Ps[MVDR_MAP_MAX_DIRS];
    __shared__ float wval[2][4];
    __shared__ int widx[2][4];
    const int a = blockIdx.x, tid = threadIdx.x, n_az = p.n_az, n_el = p.n_el, D = n_az * n_el;
    const float *part = p.part + (long long)a * p.n_slices * p.Dpad;
    for (int c = tid; c < D; c += 256) {
        float s = 0.f;
        for (int sl = 0; sl < p.n_slices; ++sl) s += part[(long long)sl * p.Dpad + c];
        Ps[c] = s;
        if (p.map) p.map[(long long)a * D + c] = s;
    }
    if (!p.peak_az && !p.peak_el && !p.peak_val) return;
    __syncthreads();
    // strictly greater than the cell before in the row and the row below, >= the cell behind and the row above: a plateau counts once
    unsigned mine = 0;
#pragma unroll
    for (int r = 0; r < CPT; ++r) {
        const int c = tid + 256 * r;
        if (c >= D) continue;
        const int j = c / n_az, i = c - j * n_az, im = i > 0 ? i - 1 : n_az - 1, ip = i + 1 < n_az ? i + 1 : 0;
        const float v = Ps[c];
        const float *row = Ps + j * n_az;
        bool ok = v > 0.f && v > row[im] && v >= row[ip];
        if (j > 0) ok = ok && v > row[im - n_az] && v > row[i - n_az] && v > row[ip - n_az];
        if (j < n_el - 1) ok = ok && v >= row[im + n_az] && v >= row[i + n_az] && v >= row[ip + n_az];
        if (ok) mine |= 1u << r;
    }
    const int wv = tid >> 6, lane = tid & 63;
    float val[MCA_MAX_SOURCES];
    int idx[MCA_MAX_SOURCES];
#pragma unroll
    for (int r = 0; r < MCA_MAX_SOURCES; ++r) {
        val[r] = 0.f; idx[r] = -1;
        if (r >= p.n_peaks) continue;            // (the same for every thread)
        float bv = 0.f;
        int bi = MVDR_MAP_MAX_DIRS;              // no candidate: behind every cell
#pragma unroll
        for (int q = 0; q < CPT; ++q)
            if (mine & (1u << q)) map_better(bv, bi, Ps[tid + 256 * q], tid + 256 * q);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            map_better(bv, bi, ov, oi);
        }
        if (lane == 0) { wval[r & 1][wv] = bv; widx[r & 1][wv] = bi; }
        __syncthreads();                         // (the buffer of round r - 2 was read before the barrier of round r - 1)
        bv = wval[r & 1][0]; bi = widx[r & 1][0];
#pragma unroll
        for (int w = 1; w < 4; ++w) map_better(bv, bi, wval[r & 1][w], widx[r & 1][w]);
        if (bi < MVDR_MAP_MAX_DIRS) {
            val[r] = bv; idx[r] = bi;
            if ((bi & 255) == tid) mine &= ~(1u << (bi >> 8));
        }
    }
    if (tid != 0) return;
    const bool any = idx[0] >= 0;
    const float az0 = any ? p.az[idx[0] % n_az] : 0.f, el0 = any ? p.el[idx[0] / n_az] : p.ctx_el;
#pragma unroll
    for (int r = 0; r < MCA_MAX_SOURCES; ++r)
        if (r < p.n_peaks) {
            const bool has = idx[r] >= 0;
            const long long o = (long long)a * p.n_peaks + r;
            if (p.peak_az) p.peak_az[o] = has ? p.az[idx[r] % n_az] : az0;
            if (p.peak_el) p.peak_el[o] = has ? p.el[idx[r] / n_az] : el0;
            if (p.peak_val) p.peak_val[o] = has ? val[r] : 0.f;
        }
}

// The (cos eps, sin eps) pairs of the look-direction slots from angles on the device (mca_hip_mvdr_set_elevations_dev): a NaN takes the
// context's pair, bit for bit; anything else is clamped to [-pi/2, pi/2] in double (an infinity goes to its end).  One thread per entry.
__global__ __launch_bounds__(256) void k_mvdr_elevations(MvdrElevationsArgs p)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= p.n) return;
    const int a = e / p.max_sources, s = e - a * p.max_sources;
    const float v = p.elev[e];
    const long long o = (long long)a * MCA_MAX_SOURCES + s;
    if (v != v) {
        p.slot_el[o] = make_double2(p.ce, p.se);
        p.slot_val[o] = v;
        return;
    }
    const double eps = fmin(fmax((double)v, -1.57079632679489661923), 1.57079632679489661923);
    p.slot_el[o] = make_double2(cos(eps), sin(eps));
    p.slot_val[o] = (float)eps;
}

}  // namespace mca
