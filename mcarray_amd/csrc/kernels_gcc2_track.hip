// kernels_gcc2_track.hip -- the particle-filter DOA tracker of FreqGCCBinauralLocalisation (BinauralLocalisation.cpp:429-561
// as the reference is compiled, USE_PARTICLE_FILTER): a sequential-importance-resampling filter per array whose observation
// model is setProbability on the smoothed correlation (SoundLocalisationParticleFilter.cpp:47-53).  DSPONE's filter engine is
// not available, so everything the reference does not pin is defined in DESIGN.md ("The DOA tracker", [BUILD-DEFINES]) and
// restated in tests/gcc2_tracker_twin.py, which this kernel matches bit for bit: counter-based integer random numbers, integer
// weights and prefix sums, and single IEEE double operations (no contraction anywhere in this file) in one fixed order.
//
// The work is a strict chain over the frames of an array and parallel over arrays and particles: ONE WAVE PER ARRAY, particle i
// in lane i % 64, register slot i / 64.  The wave keeps the current row and the grid in its own LDS slice (the weights read
// two neighbouring cells at a data-dependent index) and stages the prefix sums and the particles there for the ancestor search
// and the gather of the resampling.  No workgroup barrier: the waves of a workgroup never meet.
#include "kernels.h"
#include "gcc2_prob.h"

#pragma clang fp contract(off)

namespace mca {

namespace {

typedef unsigned long long u64;

// LDS instructions of one wave execute in order: only the compiler has to be kept from moving them across an exchange point
__device__ __forceinline__ void track_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr u64 TRK_G = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ u64 trk_mix(u64 z)          // the splitmix64 finaliser
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ u64 trk_draw(u64 key, u64 c) { return trk_mix(key + TRK_G * (c + 1)); }
__device__ __forceinline__ u64 trk_key(u64 seed, u64 a, u64 track, u64 upd)
{
    u64 k = trk_mix(seed + TRK_G);
    k = trk_mix((k ^ a) + TRK_G);
    k = trk_mix((k ^ track) + TRK_G);
    return trk_mix((k ^ upd) + TRK_G);
}
// the twelve 16-bit fields of three draws, centred: an integer below 2^21 times 2^-17, exact
__device__ __forceinline__ double trk_gauss(u64 key, u64 i)
{
    long long s = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const u64 d = trk_draw(key, 3 * i + j);
        s += (long long)((d & 0xFFFF) + ((d >> 16) & 0xFFFF) + ((d >> 32) & 0xFFFF) + (d >> 48));
    }
    return (double)(2 * s - 12 * 65535) / 131072.0;
}
__device__ __forceinline__ double trk_unif(u64 key, u64 c) { return (double)(trk_draw(key, c) >> 11) * 0x1p-53; }
__device__ __forceinline__ double trk_clamp(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

}  // namespace

// grid (ceil(arrays / GCC2_TRACK_WAVES)), 64 * GCC2_TRACK_WAVES threads, p.slice_bytes of LDS per wave.
template <typename TC, int SLOTS>
__global__ __launch_bounds__(64 * GCC2_TRACK_WAVES) void k_gcc2_track(Gcc2TrackArgs p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int a = blockIdx.x * GCC2_TRACK_WAVES + wave;
    if (a >= p.n_arrays) return;                                         // (a whole wave; there is no barrier below)
    const int N = p.N, D = p.D, F = p.n_frames, Dl = (D + 1) & ~1;
    constexpr int NP = SLOTS * 64;
    unsigned char *slice = smem_raw + (size_t)wave * p.slice_bytes;
    u64 *sC = reinterpret_cast<u64 *>(slice);                            // [NP] inclusive prefix sums of the weights
    double *sX = reinterpret_cast<double *>(sC + NP);                    // [NP] particles before the resampling
    TC *sRow = reinterpret_cast<TC *>(sX + NP);                          // [Dl] the current smoothed correlation
    float *sGrid = reinterpret_cast<float *>(sRow + Dl);                 // [Dl]
    const double halfpi = 1.57079632679489661923, pi = 3.14159265358979323846;

    const int slot = p.state0 + a;
    double *gx = p.x + (size_t)slot * N;
    double x[SLOTS];
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) { const int i = k * 64 + lane; x[k] = i < N ? gx[i] : 0.0; }
    double doa = p.sd[slot * 2], prob = p.sd[slot * 2 + 1];
    int alive = p.si[slot * 4], track = p.si[slot * 4 + 1], upd = p.si[slot * 4 + 2];
    const u64 key_a = p.key_a >= 0 ? (u64)p.key_a : (u64)a;

    for (int d = lane; d < D; d += 64) sGrid[d] = p.grid[d];
    double mn = 0.0, sum_adj = 0.0;
    auto stage_row = [&](const TC *src) {
        track_lds_fence();                                               // (the reads of the row it replaces are done)
        for (int d = lane; d < D; d += 64) sRow[d] = src[d];
        track_lds_fence();
        double sm;
        gcc2_row_min_sum<TC>(sRow, D, lane, &mn, &sm);
        sum_adj = sm - mn * (double)D;                                   // :588
    };
    stage_row(static_cast<const TC *>(p.corr_state) + (size_t)a * D);

    // updateFilter(): predict, weigh, estimate, resample, inject -> the estimate
    auto update = [&]() -> double {
        upd += 1;
        const u64 key = trk_key(p.seed, key_a, (u64)track, (u64)upd);
        u64 q[SLOTS], c[SLOTS], carry = 0;
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) {
            const int i = k * 64 + lane;
            q[k] = 0;
            if (i < N) {
                x[k] = trk_clamp(x[k] + p.sigma_step * trk_gauss(key, (u64)i), -halfpi, halfpi);
                const double w = gcc2_prob_at<TC>(sRow, D, mn, sum_adj, p.step, sGrid, x[k]);
                q[k] = (u64)floor(w * 0x1p40);
            }
        }
        // inclusive prefix sums in particle order (slot after slot, lane after lane): integers, so any order gives these values
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) {
            u64 incl = q[k];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const u64 t = __shfl_up(incl, off);
                if (lane >= off) incl += t;
            }
            c[k] = carry + incl;
            carry += __shfl(incl, 63);
        }
        const u64 Q = carry;
        // the estimate, in the order of gcc2_row_min_sum: every lane folds its particles in turn, then the xor butterfly
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < SLOTS; ++k)
            if (k * 64 + lane < N) acc += Q > 0 ? (double)q[k] * x[k] : x[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        const double e = acc / (Q > 0 ? (double)Q : (double)N);
        if (Q > 0) {                                                     // systematic resampling on the integer weights
            const double u = trk_unif(key, 3ull * N), qn = (double)Q / (double)N;
            track_lds_fence();
#pragma unroll
            for (int k = 0; k < SLOTS; ++k) {
                const int i = k * 64 + lane;
                if (i < N) { sC[i] = c[k]; sX[i] = x[k]; }
            }
            track_lds_fence();
#pragma unroll
            for (int k = 0; k < SLOTS; ++k) {
                const int j = k * 64 + lane;
                if (j < N) {
                    const u64 T = (u64)floor(((double)j + u) * qn);
                    int lo = 0, hi = N;                                  // the number of i with C_i <= T
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (sC[mid] <= T) lo = mid + 1; else hi = mid;
                    }
                    x[k] = sX[min(lo, N - 1)];
                }
            }
        }
        if (p.n_inject > 0) {                                            // a few particles anywhere in the range: what finds a source that jumped
            const int first = N - p.n_inject;
#pragma unroll
            for (int k = 0; k < SLOTS; ++k) {
                const int i = k * 64 + lane;
                if (i >= first && i < N) x[k] = (trk_unif(key, 3ull * N + 1 + (u64)(i - first)) - 0.5) * pi;
            }
        }
        return e;
    };

    int sil = p.one_kind >= 0 ? p.one_sil : (p.voiced ? p.sil_in[a] : 0);
    const int p0 = p.voiced ? p.post0[a] : 0;
    const unsigned char *vc = p.voiced ? p.voiced + (size_t)a * F : nullptr;
    for (int t = 0; t < F; ++t) {
        const size_t o = (size_t)a * F + t;
        int kind;                                                        // 1 fired; 2 gated out, floor known; 0 nothing happens
        if (p.one_kind >= 0) kind = p.one_kind;
        else if (!vc || vc[t]) kind = 1;
        else kind = t >= p0 ? 2 : 0;
        int fired = 0;
        if (kind == 1) {
            stage_row(static_cast<const TC *>(p.corr) + o * D);
            prob = gcc2_prob_at<TC>(sRow, D, mn, sum_adj, p.step, sGrid, doa);        // setProbability of the DOA before the frame (:454)
            if (!alive) {                                                // :457-465
                track += 1; upd = 0; alive = 1;
                const u64 key = trk_key(p.seed, key_a, (u64)track, 0);
                int am = p.one_kind >= 0 ? p.one_argmax : p.argmax[o];
                am = min(max(am, 0), D - 1);
                const double centre = (double)sGrid[am];
#pragma unroll
                for (int k = 0; k < SLOTS; ++k) {
                    const int i = k * 64 + lane;
                    if (i < N) x[k] = trk_clamp(centre + p.sigma_init * trk_gauss(key, (u64)i), -pi, pi);
                }
            }
            doa = update();                                              // :473
            fired = 1; sil = 0;
        } else if (kind == 2) {
            if (sil < p.windows_to_decay) {                              // :536-548 the track coasts on the unchanged row
                if (alive) { doa = update(); fired = 2; }
            } else {
                alive = 0;                                               // :551-558
            }
            sil += 1;
        }
        if (lane == 0) {
            static_cast<TC *>(p.doa_out)[o] = (TC)doa;
            if (p.prob_out) static_cast<TC *>(p.prob_out)[o] = (TC)prob;
            if (p.fired) p.fired[o] = (unsigned char)fired;
            if (p.track) p.track[o] = track;
        }
    }
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) { const int i = k * 64 + lane; if (i < N) gx[i] = x[k]; }
    if (lane == 0) {
        p.sd[slot * 2] = doa; p.sd[slot * 2 + 1] = prob;
        p.si[slot * 4] = alive; p.si[slot * 4 + 1] = track; p.si[slot * 4 + 2] = upd;
    }
}

template __global__ void k_gcc2_track<float, 8>(Gcc2TrackArgs);
template __global__ void k_gcc2_track<float, 16>(Gcc2TrackArgs);
template __global__ void k_gcc2_track<double, 8>(Gcc2TrackArgs);
template __global__ void k_gcc2_track<double, 16>(Gcc2TrackArgs);

}  // namespace mca
