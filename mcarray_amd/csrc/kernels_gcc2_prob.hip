// kernels_gcc2_prob.hip -- FreqGCCBinauralLocalisation::setProbability at caller-given angles (BinauralLocalisation.cpp:569-631)
// and the per-frame hook processParametrisation (:406-567) of the 2-microphone localiser.
//
// k_gcc2_prob evaluates the smoothed correlation of up to n_arrays arrays at n angles each: the weights the particle filter's
// observation model asks for (SoundLocalisationParticleFilter.cpp:51, 500 particles per frame).  k_frame_gcc2 finishes one
// frame of the frame hook after k_frame_srp (P = 1) has smoothed the correlation: first-max argmax, setProbability of the
// previous DOA (:454) and the DOA recursion (:502-504).  Both are latency / launch bound: a row is at most a few hundred values.
#include "kernels.h"
#include "gcc2_prob.h"

namespace mca {

// grid (ceil(n / 256), n_arrays), 256 threads: thread = particle.  corr: [n_arrays][corr_stride] (row a at a * corr_stride);
// doas / probs: [n_arrays][n].  A row whose sum - min * D is not positive (a fresh or reset state) gives zeros.
template <typename TC, typename TA>
__global__ __launch_bounds__(256) void k_gcc2_prob(const TC *corr, long long corr_stride, int D, float step, const float *grid,
                                                   const TA *doas, TA *probs, int n)
{
    const int a = blockIdx.y, lane = threadIdx.x & 63;
    const TC *row = corr + (long long)a * corr_stride;
    double mn, sm;
    gcc2_row_min_sum<TC>(row, D, lane, &mn, &sm);       // every wave of the block the same way (no LDS, no barrier)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double sum_adj;
    {
#pragma clang fp contract(off)
        sum_adj = sm - mn * (double)D;
    }
    const long long o = (long long)a * n + i;
    probs[o] = (TA)gcc2_prob_at<TC>(row, D, mn, sum_adj, step, grid, (double)doas[o]);
}

// one frame of the frame hook after the smoothing: one wave.  corr: the new smoothed row [D]; doa_prev = _currentDOA before the
// frame; doa_mem / one_minus = _doaMemoryFactor and 1 - it (float arithmetic, widened).  res[0] = argmax (first max, as a
// double), res[1] = setProbability(doa_prev) on the new row (:454), res[2] = the DOA after the frame (:502-504).
template <typename T>
__global__ __launch_bounds__(64) void k_frame_gcc2(const T *corr, int D, float step, const float *grid, double doa_prev,
                                                   double doa_mem, double one_minus_doa_mem, double *res)
{
    const int lane = threadIdx.x;
    T bv = -INFINITY; int bi = 0x7fffffff;
    for (int d = lane; d < D; d += 64) {
        const T v = corr[d];
        if (v > bv) { bv = v; bi = d; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T ov = __shfl_xor(bv, off); const int oi = __shfl_xor(bi, off);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (bi >= D) bi = 0;                 // (a row of NaNs has no maximum: the reference's maxidx keeps index 0)
    double mn, sm;
    gcc2_row_min_sum<T>(corr, D, lane, &mn, &sm);
    if (lane == 0) {
#pragma clang fp contract(off)
        const double pr = gcc2_prob_at<T>(corr, D, mn, sm - mn * (double)D, step, grid, doa_prev);
        const double doa = doa_mem * doa_prev + one_minus_doa_mem * (double)grid[bi];
        res[0] = (double)bi; res[1] = pr; res[2] = doa;
    }
}

template __global__ void k_gcc2_prob<float, float>(const float *, long long, int, float, const float *, const float *, float *, int);
template __global__ void k_gcc2_prob<float, double>(const float *, long long, int, float, const float *, const double *, double *, int);
template __global__ void k_gcc2_prob<double, double>(const double *, long long, int, float, const float *, const double *, double *, int);
template __global__ void k_frame_gcc2<double>(const double *, int, float, const float *, double, double, double, double *);

}  // namespace mca
