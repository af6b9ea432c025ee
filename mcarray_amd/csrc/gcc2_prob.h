// gcc2_prob.h -- the two device functions of FreqGCCBinauralLocalisation::setProbability (BinauralLocalisation.cpp:569-631)
// that kernels_gcc2_prob.hip (angles given by the caller, the frame hook) and kernels_gcc2_track.hip (the particles of the
// DOA tracker) share, so that a weight is the same bits whoever asks for it.
#pragma once
#include "kernels.h"

namespace mca {

// min and sum of a correlation row in double, one wave, in a fixed order: lane l folds d = l, l + 64, ... in turn, then a xor
// butterfly (a + b and b + a are the same bits, so every lane ends with the same values).  What a particle gets therefore does not
// depend on how many particles there are, where it sits in the list or the launch shape.
template <typename TC>
__device__ __forceinline__ void gcc2_row_min_sum(const TC *row, int D, int lane, double *mn, double *sm)
{
    double m = INFINITY, s = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = (double)row[d];
        m = fmin(m, v);
        s += v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        m = fmin(m, __shfl_xor(m, off));
        s += __shfl_xor(s, off);
    }
    *mn = m; *sm = s;
}

// setProbability for one angle (BinauralLocalisation.cpp:590-630) in the reference's mixed arithmetic: angle2DOAidx takes a
// FLOAT argument, clamps it in double and stores the result back into that float, then divides (angle + pi/2) by the float
// step in double (microhponeArrayHelpers.cpp:110-115); the grid angles are the float doaIdx2angle values; the interpolation
// uses the unrounded double angle; the two edge cells take corr[idx] as it is.  sum_adj = sum - min * D (:588).
template <typename TC>
__device__ __forceinline__ double gcc2_prob_at(const TC *corr, int D, double mn, double sum_adj, float step, const float *grid, double doa)
{
#pragma clang fp contract(off)
    const double halfpi = 1.57079632679489661923;
    double a = (double)(float)doa;
    a = (double)(float)fmax(a, -halfpi);
    a = (double)(float)fmin(a, halfpi);
    int idx = (int)((a + halfpi) / (double)step);
    idx = min(max(idx, 0), D - 1);      // (the reference's steps never leave the grid; this only keeps a NaN angle in bounds)
    const double angle = (double)grid[idx];
    double p;
    if (0 < idx && idx < D - 1) {
        double pc, nc, pd, nd;
        if (angle > doa) { pc = (double)corr[idx - 1]; pd = (double)grid[idx - 1]; nc = (double)corr[idx]; nd = angle; }
        else { pc = (double)corr[idx]; pd = angle; nc = (double)corr[idx + 1]; nd = (double)grid[idx + 1]; }
        const double slope = (nc - pc) / (nd - pd);
        p = slope * (doa - pd) + pc;
    } else {
        p = (double)corr[idx];
    }
    double pb = 0.0;
    if (sum_adj > 0.0) pb = (p - mn) / sum_adj;
    return pb < 0.01 ? 0.0 : pb;
}

}  // namespace mca
