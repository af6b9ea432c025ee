// mvdr_track_scan.h -- what the tracks on one angle (kernels_mvdr_track.hip) and the tracks on the azimuth x
// elevation map (kernels_mvdr_trk2.hip) share: the scan of a chunk's normalised steering vectors against a phasor
// table, and the angle helpers of the association.  One text, so that both follow the same steered spectrum; moved here from
// kernels_mvdr_track.hip without a change, and that unit's kernels keep their instruction streams.
#pragma once
#include "fft512.h"
#include "mca_internal.h"

namespace mca {

// NA angles of this lane (a0, a0 + 64) against the bins wv, wv + 4, ... of the chunk: c = sum_j u_j conj(d_j(theta)), u read from LDS at
// an address all lanes share (broadcast), the phasors as the product of their two table factors (mvdr_spectrum_scan)
template <int NA>
__device__ __forceinline__ void mvdr_track_scan(const MvdrTrackSpectrumArgs &p, const float2 *Us, const int *Fs, int kbase, int wv, int a0, float *po)
{
    const int M = p.M;
    const long long Dpad = p.Dpad;
    const float im = 1.f / (float)M;
    float acc[NA];
#pragma unroll
    for (int n = 0; n < NA; ++n) acc[n] = 0.f;
#pragma unroll 1
    for (int bl = wv; bl < MVDR_SPEC_CHUNK; bl += 4) {
        if (__builtin_amdgcn_readfirstlane(Fs[bl]) == 0) continue;     // not used (the same for the whole wave)
        const int k = kbase + bl;
        const float2 *th = p.T + (long long)(k >> 5) * Dpad + a0;
        const float2 *tl = p.T + (long long)(p.nhi + (k & 31)) * Dpad + a0;
        const float2 *ub = Us + bl * M;
        float2 c[NA];
#pragma unroll
        for (int n = 0; n < NA; ++n) c[n] = make_float2(0.f, 0.f);
        for (int j = 0; j < M; ++j) {
            const long long mo = (long long)j * p.nph * Dpad;
            const float2 uv = ub[j];
#pragma unroll
            for (int n = 0; n < NA; ++n) c[n] = cmacc(c[n], uv, cmul(th[mo + 64 * n], tl[mo + 64 * n]));
        }
#pragma unroll
        for (int n = 0; n < NA; ++n) acc[n] = fmaf(fmaf(c[n].x, c[n].x, c[n].y * c[n].y), im, acc[n]);
    }
#pragma unroll
    for (int n = 0; n < NA; ++n)
        if (a0 + 64 * n < p.D) po[a0 + 64 * n] = acc[n];
}

// XYZ mode (circular != 0): a finite angle that enters is reduced to [-pi, pi] (a NaN or an infinity stays what it is), a difference
// takes the shorter way round.  Otherwise the plain value and the plain difference.
__device__ __forceinline__ float mvdr_track_angle(float v, int circular) { return circular && fabsf(v) < __int_as_float(0x7f800000) ? mvdr_reduce(v) : v; }
__device__ __forceinline__ float mvdr_track_diff(float x, float y, int circular)
{
    const float d = x - y;
    return circular ? mvdr_wrap(d) : d;
}

}  // namespace mca
