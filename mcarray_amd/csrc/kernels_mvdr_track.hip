// kernels_mvdr_track.hip -- tracks of the look directions of an MVDR context, updated on the device between chunks (gfx950;
// include/mcarray_hip.h, mca_hip_mvdr_tracks_*).  A translation unit of its own: the kernels of the frames calls and of
// the Capon spectrum keep the instruction streams they have.  Read-only on the stream state, but for Psi and cpsi of a slot at its birth.
//
// An own track (slot s < n_own) follows the talker's own cells: with d_k the steering vector the estimator of mvdr_rtf.h reads from
// (Psi_s, cpsi_s, Phi, cphi) at g0 = the geometric vector of theta_s, u_k = d_k / |d_k|, and d(theta_i, k) the grid vectors of the Capon
// spectrum (its phasor table),
//     T_s[i] = sum over the used bins k of |d(theta_i,k)^H u_k|^2 / M          used: the estimator did not fall back and tr[k] > 1e-30
// and the track moves to the grid angle that maximises T_s within max_step of theta_s.  The other tracks follow the Capon peaks,
// associated by angle.  No atomics: partial sums per (chunk, wave), added in that order, so the result is a pure function of state and
// configuration and does not depend on where a stream sits in the batch.
#include "fft512.h"
#include "mca_internal.h"
#include "mvdr_solve.h"
#include "mvdr_rtf.h"
#include "mvdr_track_scan.h"   // the scan and the angle helpers, shared with kernels_mvdr_trk2.hip

namespace mca {

// grid (streams * n_own), 256 threads: the table of mvdr_steering_tables (kernels_mvdr.hip), operation for operation, at doa = theta_s
__global__ __launch_bounds__(256) void k_mvdr_track_tables(MvdrTrackTablesArgs p)
{
    const int nhi = (p.N >> 6) + 1, nph = nhi + 32;
    const int a = (int)(blockIdx.x / (unsigned)p.n_own), s = (int)(blockIdx.x % (unsigned)p.n_own);
    const double cd = cos((double)p.theta[a * MCA_MAX_SOURCES + s] + 1.57079632679489661923);
    const double cy = p.geo.xyz ? -cos((double)p.theta[a * MCA_MAX_SOURCES + s]) : 0.0;
    float2 *T = p.T0 + (long long)blockIdx.x * p.M * nph;
    for (int e = threadIdx.x; e < p.M * nph; e += 256) {
        const int m = e / nph, i = e - m * nph;
        const int kk = i < nhi ? (i << 5) : i - nhi;
        double turns = (double)kk * (p.geo.xyz ? mvdr_projection(p.geo, p.M, m, cd, cy) : p.unit * p.mic_x[m] * cd);
        turns -= rint(turns);
        float sn, cs;
        sincospif(2.0f * (float)turns, &sn, &cs);
        T[e] = make_float2(cs, -sn);
    }
}

// grid (streams * n_own * n_chunks), 256 threads
template <int Q>
__global__ __launch_bounds__(256, 2) void k_mvdr_track_spectrum(MvdrTrackSpectrumArgs p)
{
    constexpr int NE = 2 * Q * (Q + 1);
    __shared__ float2 Us[MVDR_SPEC_CHUNK * 4 * Q];   // [64][M]: u of the bin, zero where the bin is not used
    __shared__ int Fs[MVDR_SPEC_CHUNK];              // [64]: used
    const int M = p.M, K = p.K, tri = M * (M + 1) / 2;
    const int tid = threadIdx.x, l = tid & 3, b = tid >> 2;
    const int ci = (int)(blockIdx.x % (unsigned)p.n_chunks), as = (int)(blockIdx.x / (unsigned)p.n_chunks);    // as = a n_own + s
    const int a = as / p.n_own, s = as - a * p.n_own;
    const int kbase = MVDR_SPEC_CHUNK * (p.chunk0 + ci);
    if (p.alive[a * MCA_MAX_SOURCES + s] == 0) {             // a dead slot uses no bin (the same for the whole workgroup): zero partial rows,
        float *pz = p.part + ((long long)as * p.n_chunks + ci) * 4 * p.Dpad;                    // and its flags stay as the caller cleared them
        for (int i = tid; i < 4 * p.Dpad; i += 256) pz[i] = 0.f;
        return;
    }

    // ---- the estimator on every bin of the chunk, one quad per bin (k_mvdr_rtf_steering), u = d / |d| to LDS ----
    {
        const int kk = kbase + b;
        const bool in = kk >= p.bin_lo && kk <= p.bin_hi;
        const int k = in ? kk : p.bin_lo;
        const long long ak = (long long)a * K + k, ask = ((long long)a * p.slots + s) * K + k;
        float2 P[NE], R[NE], g0[Q], d[Q];
        rtf_load_rows<Q>(P, p.phi + ak * tri, M, l);
        rtf_load_rows<Q>(R, p.psi + ask * tri, M, l);
        mvdr_steer_rows<Q, false>(g0, p.T0 + (long long)as * M * p.nph + (k >> 5), 0, M, p.nph, p.nhi - (k >> 5) + (k & 31), l);
        const bool est = mvdr_rtf_estimate<Q>(d, R, P, p.cpsi[ask], p.cphi[ak], g0, p.iterations, p.ref_mic, p.min_share, M, l);
        const bool used = est && in && p.trace[ak] > 1e-30f;
        float e = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) e = fmaf(d[q].x, d[q].x, fmaf(d[q].y, d[q].y, e));
        const float rn = used ? 1.f / sqrtf(quad_sum(e)) : 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q)
            if (4 * q + l < M) Us[b * M + 4 * q + l] = used ? make_float2(d[q].x * rn, d[q].y * rn) : make_float2(0.f, 0.f);
        if (l == 0) {
            Fs[b] = used ? 1 : 0;
            if (p.used && in) p.used[(long long)as * K + k] = used ? 1 : 0;
        }
    }
    __syncthreads();

    // ---- the scan: wave wv takes the bins wv, wv + 4, ... of the chunk, its lanes the angles, two passes of 64 at a time ----
    const int wv = tid >> 6, lane = tid & 63;
    float *po = p.part + (((long long)as * p.n_chunks + ci) * 4 + wv) * p.Dpad;
    int a0 = lane;
    for (; a0 + 64 < p.Dpad; a0 += 128) mvdr_track_scan<2>(p, Us, Fs, kbase, wv, a0, po);
    if (a0 < p.Dpad) mvdr_track_scan<1>(p, Us, Fs, kbase, wv, a0, po);
}

template __global__ void k_mvdr_track_spectrum<1>(MvdrTrackSpectrumArgs);
template __global__ void k_mvdr_track_spectrum<2>(MvdrTrackSpectrumArgs);
template __global__ void k_mvdr_track_spectrum<3>(MvdrTrackSpectrumArgs);
template __global__ void k_mvdr_track_spectrum<4>(MvdrTrackSpectrumArgs);

const void *mvdr_track_spectrum_kernel(int Q)
{
    const void *k[4] = {(const void *)k_mvdr_track_spectrum<1>, (const void *)k_mvdr_track_spectrum<2>, (const void *)k_mvdr_track_spectrum<3>,
                        (const void *)k_mvdr_track_spectrum<4>};
    return Q >= 1 && Q <= 4 ? k[Q - 1] : nullptr;
}

// The association of one stream (include/mcarray_hip.h, mca_hip_mvdr_tracks_configure: the normative text; tests/mvdr_tracks_twin.py
// restates it operation by operation).  All in float; returns the mask of the slots born.
__device__ __forceinline__ int mvdr_track_associate(const MvdrTrackPickArgs &p, float *theta, int *alive, int *miss, int *gen, const float *own_doa,
                                                    float *birth, const float *cand_doa, const float *cand_val)
{
    constexpr int MAXC = MVDR_TRACK_MAX_CAND;
    const float inf = __int_as_float(0x7f800000);
    // 1. own slots
    for (int s = 0; s < p.n_own; ++s) {
        if (!alive[s]) continue;
        const float o = mvdr_track_angle(own_doa[s], p.circular);
        if (fabsf(o) < inf) {                                   // finite (false for a NaN)
            const float dl = mvdr_track_diff(o, theta[s], p.circular);
            const float th = theta[s] + fminf(fmaxf(dl, -p.max_step), p.max_step);
            theta[s] = p.circular ? mvdr_wrap(th) : th;
            miss[s] = 0;
        } else miss[s] += 1;
    }
    // 2. candidates in the order given
    int matched = 0, n_birth = 0;
    for (int c = 0; c < p.n_cand && c < MAXC; ++c) {
        const float psi = mvdr_track_angle(cand_doa[c], p.circular);
        if (!(cand_val[c] > 0.f) || !(fabsf(psi) < inf)) continue;
        bool own = false;
        for (int s = 0; s < p.n_own; ++s) own = own || (alive[s] && fabsf(mvdr_track_diff(psi, theta[s], p.circular)) <= p.min_sep);
        if (own) continue;
        int best = -1;
        float bd = 0.f;
        for (int s = p.n_own; s < p.n_tracks; ++s) {
            if (!alive[s] || (matched >> s & 1)) continue;
            const float ds = fabsf(mvdr_track_diff(psi, theta[s], p.circular));
            if (ds <= p.max_step && (best < 0 || ds < bd)) { best = s; bd = ds; }
        }
        if (best >= 0) { theta[best] = psi; miss[best] = 0; matched |= 1 << best; }
        else birth[n_birth++] = psi;
    }
    // 3. unmatched alive interferer slots
    for (int s = p.n_own; s < p.n_tracks; ++s)
        if (alive[s] && !(matched >> s & 1)) {
            miss[s] += 1;
            if (miss[s] > p.hold) alive[s] = 0;
        }
    // 4. births in candidate order
    int born = 0;
    for (int c = 0; c < n_birth; ++c) {
        int f = -1;
        for (int s = p.n_tracks - 1; s >= p.n_own; --s) f = alive[s] ? f : s;
        if (f < 0) break;
        theta[f] = birth[c]; alive[f] = 1; miss[f] = 0; gen[f] += 1; born |= 1 << f;
    }
    return born;
}

// grid (streams), 256 threads
__global__ __launch_bounds__(256) void k_mvdr_track_pick(MvdrTrackPickArgs p)
{
    __shared__ float Ts[MCA_MAX_SOURCES][MVDR_SPEC_MAX_ANGLES + 1];
    // the state of the stream under the one lane that associates: in LDS, where a slot chosen at run time is an address, not a register
    __shared__ float st_f[2 * MCA_MAX_SOURCES + MVDR_TRACK_MAX_CAND];   // theta, own_doa, the births
    __shared__ int st_i[3 * MCA_MAX_SOURCES];                           // alive, miss, gen
    __shared__ int born_s;
    const int a = blockIdx.x, D = p.D;
    if (p.part) {
        for (int e = threadIdx.x; e < p.n_own * D; e += 256) {
            const int s = e / D, i = e - s * D;
            const float *part = p.part + ((long long)a * p.n_own + s) * p.n_slices * p.Dpad;
            float t = 0.f;
            for (int sl = 0; sl < p.n_slices; ++sl) t += part[(long long)sl * p.Dpad + i];
            Ts[s][i] = t;
            if (p.own_spectrum) p.own_spectrum[((long long)a * p.n_own + s) * D + i] = t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float *theta = st_f, *own = st_f + MCA_MAX_SOURCES;
        int *alive = st_i, *miss = st_i + MCA_MAX_SOURCES, *gen = st_i + 2 * MCA_MAX_SOURCES;
        for (int s = 0; s < MCA_MAX_SOURCES; ++s) {
            const int o = a * MCA_MAX_SOURCES + s;
            theta[s] = p.st.theta[o]; alive[s] = p.st.alive[o]; miss[s] = p.st.miss[o]; gen[s] = p.st.gen[o];
            own[s] = __int_as_float(0x7fc00000);
        }
        if (p.part) {
            // the window argmax of every own slot: comparison in float, the lower index wins ties
            for (int s = 0; s < p.n_own; ++s) {
                float bv = 0.f;
                int bi = -1;
                for (int i = 0; i < D; ++i)
                    if (fabsf(mvdr_track_diff(p.grid[i], theta[s], p.circular)) <= p.max_step && Ts[s][i] > bv) { bv = Ts[s][i]; bi = i; }
                if (bi >= 0 && alive[s]) own[s] = p.grid[bi];
            }
        } else if (p.own_doa) {
            for (int s = 0; s < p.n_own; ++s) own[s] = p.own_doa[(long long)a * p.n_own + s];
        }
        born_s = mvdr_track_associate(p, theta, alive, miss, gen, own, st_f + 2 * MCA_MAX_SOURCES, p.cand_doa + (long long)a * p.n_cand,
                                      p.cand_val + (long long)a * p.n_cand);
        for (int s = 0; s < MCA_MAX_SOURCES; ++s) {
            const int o = a * MCA_MAX_SOURCES + s;
            p.st.theta[o] = theta[s]; p.st.alive[o] = alive[s]; p.st.miss[o] = miss[s]; p.st.gen[o] = gen[s];
        }
    }
    __syncthreads();
    // Psi and cpsi of a slot born belong to whoever held the slot before
    const int born = born_s;
    if (!p.psi || !born) return;
    for (int s = 0; s < p.n_tracks; ++s) {
        if (!(born >> s & 1)) continue;
        const long long slot = (long long)a * p.slots + s;
        float2 *ps = p.psi + slot * p.K * p.tri;
        float *cp = p.cpsi + slot * p.K;
        for (long long e = threadIdx.x; e < (long long)p.K * p.tri; e += 256) ps[e] = make_float2(0.f, 0.f);
        for (int e = threadIdx.x; e < p.K; e += 256) cp[e] = 0.f;
    }
}

// grid (ceil(streams * n_frames / 256)), 256 threads: theta of every alive slot for every frame; a dead slot reports the lowest alive
// slot's, or 0 rad
__global__ __launch_bounds__(256) void k_mvdr_track_fill(MvdrTrackFillArgs p)
{
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)p.n_streams * p.n_frames) return;
    const int a = (int)(id / p.n_frames);
    float first = 0.f;
    for (int s = p.n_tracks - 1; s >= 0; --s) first = p.st.alive[a * MCA_MAX_SOURCES + s] ? p.st.theta[a * MCA_MAX_SOURCES + s] : first;
    for (int s = 0; s < p.n_tracks; ++s)
        p.doa_rad[id * p.n_tracks + s] = p.st.alive[a * MCA_MAX_SOURCES + s] ? p.st.theta[a * MCA_MAX_SOURCES + s] : first;
}

// grid (ceil(streams * n_tracks / 256)), 256 threads
__global__ __launch_bounds__(256) void k_mvdr_track_seed(MvdrTrackSeedArgs p)
{
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= p.n_streams * p.n_tracks) return;
    const int a = id / p.n_tracks, s = id - a * p.n_tracks, o = a * MCA_MAX_SOURCES + s;
    const float v = p.doa[id];
    if (!(fabsf(v) < __int_as_float(0x7f800000))) return;       // NaN (or an infinity): leave the slot
    p.st.theta[o] = mvdr_track_angle(v, p.circular); p.st.alive[o] = 1; p.st.miss[o] = 0; p.st.gen[o] += 1;
}

}  // namespace mca
