// kernels_mvdr_trk2.hip -- tracks of the look directions in azimuth and elevation, fed by the Capon map of an MVDR context (gfx950;
// include/mcarray_hip.h, mca_hip_mvdr_tracks_*_map).  A translation unit of its own: the kernels of the tracks on one
// angle (kernels_mvdr_track.hip), of the map and of the frames calls keep the instruction streams they have.  Read-only on the stream
// state, but for Psi and cpsi of a slot at its birth.
//
// An own track (slot s < n_own) holds (theta_s, eps_s).  With d_k the steering vector the estimator of mvdr_rtf.h reads from
// (Psi_s, cpsi_s, Phi, cphi) at g0 = the geometric vector of (theta_s, eps_s), u_k = d_k / |d_k|, and d(theta_i, eps_j, k) the vectors
// of the map's phasor table,
//     T_s[j][i] = sum over the used bins k of |d(theta_i, eps_j, k)^H u_k|^2 / M
// and the track moves towards the cell that maximises T_s within (max_step, max_step_el) of (theta_s, eps_s).  The estimator runs once
// per (stream, own slot, bin) and leaves u in workspace (k_mvdr_trk2_vectors); the scan is cut into tiles of 128 directions of the flat
// list as k_mvdr_map_scan cuts it (k_mvdr_trk2_scan), and a tile that holds no cell of the window is not scanned at all unless the
// caller asks for the whole map.  No atomics: partial sums per (chunk, wave), added in that order.
#include "fft512.h"
#include "mca_internal.h"
#include "mvdr_solve.h"
#include "mvdr_rtf.h"
#include "mvdr_track_scan.h"

namespace mca {

__device__ __forceinline__ bool trk2_finite(float v) { return fabsf(v) < __int_as_float(0x7f800000); }
// an elevation as the tracks hold it: within +-(float) pi/2
__device__ __forceinline__ float trk2_clamp_el(float v) { return fminf(fmaxf(v, -MVDR_HALF_PI_F), MVDR_HALF_PI_F); }
// a cell (az, el) of the grid lies in the box (da, de) round (th, ep): the search window of an own track, the gate and the own box of the
// association.  Float differences, the azimuth the shorter way round
__device__ __forceinline__ bool trk2_in_box(float az, float el, float th, float ep, float da, float de)
{
    return fabsf(mvdr_track_diff(az, th, 1)) <= da && fabsf(el - ep) <= de;
}
// the better of two cells: the larger value, then the lower flat index
__device__ __forceinline__ void trk2_better(float &v, int &i, float ov, int oi)
{
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// grid (streams * n_own), 256 threads: the table of k_mvdr_track_tables (XYZ arm), operation for operation, with the pair of eps_s
// where that one reads the context's
__global__ __launch_bounds__(256) void k_mvdr_trk2_tables(MvdrTrk2TablesArgs p)
{
    const int nhi = (p.N >> 6) + 1, nph = nhi + 32;
    const int a = (int)(blockIdx.x / (unsigned)p.n_own), s = (int)(blockIdx.x % (unsigned)p.n_own);
    const int o = a * MCA_MAX_SOURCES + s;
    if (p.alive[o] == 0) return;                                   // (the vectors of a dead slot are not formed)
    const double cd = cos((double)p.theta[o] + 1.57079632679489661923);
    const double cy = -cos((double)p.theta[o]);
    const double ce = cos((double)p.eps[o]), se = sin((double)p.eps[o]);
    float2 *T = p.T0 + (long long)blockIdx.x * p.M * nph;
    for (int e = threadIdx.x; e < p.M * nph; e += 256) {
        const int m = e / nph, i = e - m * nph;
        const int kk = i < nhi ? (i << 5) : i - nhi;
        double turns = (double)kk * mvdr_projection(p.geo, p.M, m, cd, cy, ce, se);
        turns -= rint(turns);
        float sn, cs;
        sincospif(2.0f * (float)turns, &sn, &cs);
        T[e] = make_float2(cs, -sn);
    }
}

// grid (streams * n_own * n_chunks), 256 threads: the estimator on every bin of the chunk, one quad per bin (phase 1 of
// k_mvdr_track_spectrum<Q>), u = d / |d| and the used flag to workspace.  Once per bin, whatever the number of tiles
template <int Q>
__global__ __launch_bounds__(256, 2) void k_mvdr_trk2_vectors(MvdrTrk2ScanArgs pa)
{
    const MvdrTrackSpectrumArgs &p = pa.s;
    constexpr int NE = 2 * Q * (Q + 1);
    const int M = p.M, K = p.K, tri = M * (M + 1) / 2;
    const int tid = threadIdx.x, l = tid & 3, b = tid >> 2;
    const int ci = (int)(blockIdx.x % (unsigned)p.n_chunks), as = (int)(blockIdx.x / (unsigned)p.n_chunks);    // as = a n_own + s
    const int a = as / p.n_own, s = as - a * p.n_own;
    if (p.alive[a * MCA_MAX_SOURCES + s] == 0) return;       // a dead slot: nothing is read or written, the scan and the pick skip it too
    const int kbase = MVDR_SPEC_CHUNK * (p.chunk0 + ci);
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
    const long long cb = (long long)as * p.n_chunks + ci;
    float2 *U = pa.U + (cb * MVDR_SPEC_CHUNK + b) * M;
#pragma unroll
    for (int q = 0; q < Q; ++q)
        if (4 * q + l < M) U[4 * q + l] = used ? make_float2(d[q].x * rn, d[q].y * rn) : make_float2(0.f, 0.f);
    if (l == 0) {
        pa.F[cb * MVDR_SPEC_CHUNK + b] = used ? 1 : 0;
        if (p.used && in) p.used[(long long)as * K + k] = used ? 1 : 0;
    }
}

template __global__ void k_mvdr_trk2_vectors<1>(MvdrTrk2ScanArgs);
template __global__ void k_mvdr_trk2_vectors<2>(MvdrTrk2ScanArgs);
template __global__ void k_mvdr_trk2_vectors<3>(MvdrTrk2ScanArgs);
template __global__ void k_mvdr_trk2_vectors<4>(MvdrTrk2ScanArgs);

const void *mvdr_trk2_vectors_kernel(int Q)
{
    const void *k[4] = {(const void *)k_mvdr_trk2_vectors<1>, (const void *)k_mvdr_trk2_vectors<2>, (const void *)k_mvdr_trk2_vectors<3>,
                        (const void *)k_mvdr_trk2_vectors<4>};
    return Q >= 1 && Q <= 4 ? k[Q - 1] : nullptr;
}

// grid (((chunk n_tiles + tile) n_own + slot) n_streams + stream), 256 threads: the stream runs fastest, so that the workgroups
// resident at one time share a few (chunk, tile) slices of the map's phasor table in L2 and differ in the 8 KiB of u
// they load.  One partial row per wave; the scan text is that of the tracks on one angle (mvdr_track_scan.h)
__global__ __launch_bounds__(256, 2) void k_mvdr_trk2_scan(MvdrTrk2ScanArgs pa)
{
    const MvdrTrackSpectrumArgs &p = pa.s;
    __shared__ float2 Us[MVDR_SPEC_CHUNK * 16];      // [64][M]: u of the bin, zero where the bin is not used
    __shared__ int Fs[MVDR_SPEC_CHUNK];              // [64]: used
    const int tid = threadIdx.x, M = p.M;
    unsigned r = blockIdx.x;
    const int a = (int)(r % (unsigned)pa.n_streams); r /= (unsigned)pa.n_streams;
    const int s = (int)(r % (unsigned)p.n_own); r /= (unsigned)p.n_own;
    const int t = (int)(r % (unsigned)pa.n_tiles), ci = (int)(r / (unsigned)pa.n_tiles);
    const int o = a * MCA_MAX_SOURCES + s;
    if (p.alive[o] == 0) return;                     // a dead slot costs no loads (the same for the whole workgroup)
    if (pa.skip) {
        // the caller takes no map: a tile without a cell of the slot's search window is never read by the pick
        const int c = t * MVDR_MAP_TILE + (tid & (MVDR_MAP_TILE - 1));
        int hit = 0;
        if (tid < MVDR_MAP_TILE && c < p.D) {
            const int j = c / pa.n_az, i = c - j * pa.n_az;
            hit = trk2_in_box(pa.az[i], pa.el[j], pa.theta[o], pa.eps[o], pa.max_step, pa.max_step_el) ? 1 : 0;
        }
        if (!__syncthreads_or(hit)) return;
    }
    const long long cb = ((long long)a * p.n_own + s) * p.n_chunks + ci;
    const float2 *U = pa.U + cb * MVDR_SPEC_CHUNK * M;
    for (int e = tid; e < MVDR_SPEC_CHUNK * M; e += 256) Us[e] = U[e];
    if (tid < MVDR_SPEC_CHUNK) Fs[tid] = pa.F[cb * MVDR_SPEC_CHUNK + tid];
    __syncthreads();
    // wave wv takes the bins wv, wv + 4, ... of the chunk; the last tile may hold one block of 64 directions only (Dpad is whole waves)
    const int wv = tid >> 6, lane = tid & 63;
    const int kbase = MVDR_SPEC_CHUNK * (p.chunk0 + ci);
    float *po = p.part + (cb * 4 + wv) * p.Dpad;
    const int a0 = t * MVDR_MAP_TILE + lane;
    if (a0 + 64 < p.Dpad) mvdr_track_scan<2>(p, Us, Fs, kbase, wv, a0, po);
    else if (a0 < p.Dpad) mvdr_track_scan<1>(p, Us, Fs, kbase, wv, a0, po);
}

// The association of one stream in two angles (include/mcarray_hip.h, mca_hip_mvdr_tracks_set_map: the normative text;
// tests/mvdr_tracks_map_twin.py restates it operation by operation).  All in float, every step one rounded operation; with every
// elevation equal it is mvdr_track_associate on the circle bit for bit.  Returns the mask of the slots born.
__device__ __forceinline__ int trk2_associate(const MvdrTrk2PickArgs &p, float *theta, float *eps, int *alive, int *miss, int *gen, const float *own_az,
                                              const float *own_el, float *birth_az, float *birth_el, const float *cand_az, const float *cand_el,
                                              const float *cand_val)
{
    constexpr int MAXC = MVDR_TRACK_MAX_CAND;
    // 1. own slots
    for (int s = 0; s < p.n_own; ++s) {
        if (!alive[s]) continue;
        const float oa = mvdr_track_angle(own_az[s], 1), oe = own_el[s];
        if (trk2_finite(oa) && trk2_finite(oe)) {
            const float dl = mvdr_track_diff(oa, theta[s], 1);
            const float th = theta[s] + fminf(fmaxf(dl, -p.max_step), p.max_step);
            theta[s] = mvdr_wrap(th);
            const float de = trk2_clamp_el(oe) - eps[s];
            const float ep = eps[s] + fminf(fmaxf(de, -p.max_step_el), p.max_step_el);
            eps[s] = trk2_clamp_el(ep);
            miss[s] = 0;
        } else miss[s] += 1;
    }
    // 2. candidates in the order given
    int matched = 0, n_birth = 0;
    for (int c = 0; c < p.n_cand && c < MAXC; ++c) {
        const float psi = mvdr_track_angle(cand_az[c], 1);
        if (!(cand_val[c] > 0.f) || !trk2_finite(psi) || !trk2_finite(cand_el[c])) continue;
        const float eta = trk2_clamp_el(cand_el[c]);
        bool own = false;
        for (int s = 0; s < p.n_own; ++s) own = own || (alive[s] && trk2_in_box(psi, eta, theta[s], eps[s], p.min_sep, p.min_sep_el));
        if (own) continue;
        int best = -1;
        float bd = 0.f;
        for (int s = p.n_own; s < p.n_tracks; ++s) {
            if (!alive[s] || (matched >> s & 1)) continue;
            const float da = fabsf(mvdr_track_diff(psi, theta[s], 1)), de = fabsf(eta - eps[s]);
            const float ds = da + de;
            if (da <= p.max_step && de <= p.max_step_el && (best < 0 || ds < bd)) { best = s; bd = ds; }
        }
        if (best >= 0) { theta[best] = psi; eps[best] = eta; miss[best] = 0; matched |= 1 << best; }
        else { birth_az[n_birth] = psi; birth_el[n_birth++] = eta; }
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
        theta[f] = birth_az[c]; eps[f] = birth_el[c]; alive[f] = 1; miss[f] = 0; gen[f] += 1; born |= 1 << f;
    }
    return born;
}

// grid (streams), 256 threads.  With part: T_s of every alive own slot summed in (chunk, wave) order -- the whole map when the caller
// takes it, else the cells of the search window alone, the only ones whose tiles were scanned -- and its window argmax by a workgroup
// arg-max; then one lane runs the association on the state in LDS, where a slot chosen at run time is an address, not a register
// (DESIGN.md 4.11), and the workgroup clears Psi and cpsi of the slots born
__global__ __launch_bounds__(256) void k_mvdr_trk2_pick(MvdrTrk2PickArgs p)
{
    __shared__ float st_f[4 * MCA_MAX_SOURCES + 2 * MVDR_TRACK_MAX_CAND];   // theta, eps, own az, own el, the births (az, el)
    __shared__ int st_i[3 * MCA_MAX_SOURCES];                               // alive, miss, gen
    __shared__ int born_s;
    __shared__ float wval[4];
    __shared__ int widx[4];
    const int a = blockIdx.x, tid = threadIdx.x, n_az = p.n_az, D = p.n_az * p.n_el;
    float *own_az = st_f + 2 * MCA_MAX_SOURCES, *own_el = st_f + 3 * MCA_MAX_SOURCES;
    if (tid < MCA_MAX_SOURCES) { own_az[tid] = __int_as_float(0x7fc00000); own_el[tid] = __int_as_float(0x7fc00000); }
    __syncthreads();
    if (p.part) {
        const int wv = tid >> 6, lane = tid & 63;
        for (int s = 0; s < p.n_own; ++s) {
            const int o = a * MCA_MAX_SOURCES + s;
            const bool live = p.st.alive[o] != 0;
            const float th = p.st.theta[o], ep = p.st.eps[o];
            const float *part = p.part + ((long long)a * p.n_own + s) * p.n_slices * p.Dpad;
            float bv = 0.f;
            int bi = MVDR_MAP_MAX_DIRS;              // no cell: behind every cell
            for (int c = tid; c < D; c += 256) {
                const int j = c / n_az, i = c - j * n_az;
                const bool win = live && trk2_in_box(p.az[i], p.el[j], th, ep, p.max_step, p.max_step_el);
                float t = 0.f;
                if (live && (p.own_map || win))
                    for (int sl = 0; sl < p.n_slices; ++sl) t += part[(long long)sl * p.Dpad + c];
                if (p.own_map) p.own_map[((long long)a * p.n_own + s) * D + c] = t;
                if (win && t > 0.f) trk2_better(bv, bi, t, c);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float ov = __shfl_xor(bv, off);
                const int oi = __shfl_xor(bi, off);
                trk2_better(bv, bi, ov, oi);
            }
            if (lane == 0) { wval[wv] = bv; widx[wv] = bi; }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < 4; ++w) trk2_better(bv, bi, wval[w], widx[w]);
                if (bi < MVDR_MAP_MAX_DIRS) { own_az[s] = p.az[bi % n_az]; own_el[s] = p.el[bi / n_az]; }
            }
            __syncthreads();
        }
    } else if (p.own_az) {
        if (tid < p.n_own) { own_az[tid] = p.own_az[(long long)a * p.n_own + tid]; own_el[tid] = p.own_el[(long long)a * p.n_own + tid]; }
        __syncthreads();
    }
    if (tid == 0) {
        float *theta = st_f, *eps = st_f + MCA_MAX_SOURCES, *birth = st_f + 4 * MCA_MAX_SOURCES;
        int *alive = st_i, *miss = st_i + MCA_MAX_SOURCES, *gen = st_i + 2 * MCA_MAX_SOURCES;
        for (int s = 0; s < MCA_MAX_SOURCES; ++s) {
            const int o = a * MCA_MAX_SOURCES + s;
            theta[s] = p.st.theta[o]; eps[s] = p.st.eps[o]; alive[s] = p.st.alive[o]; miss[s] = p.st.miss[o]; gen[s] = p.st.gen[o];
        }
        born_s = trk2_associate(p, theta, eps, alive, miss, gen, own_az, own_el, birth, birth + MVDR_TRACK_MAX_CAND, p.cand_az + (long long)a * p.n_cand,
                                p.cand_el + (long long)a * p.n_cand, p.cand_val + (long long)a * p.n_cand);
        for (int s = 0; s < MCA_MAX_SOURCES; ++s) {
            const int o = a * MCA_MAX_SOURCES + s;
            p.st.theta[o] = theta[s]; p.st.eps[o] = eps[s]; p.st.alive[o] = alive[s]; p.st.miss[o] = miss[s]; p.st.gen[o] = gen[s];
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
        for (long long e = tid; e < (long long)p.K * p.tri; e += 256) ps[e] = make_float2(0.f, 0.f);
        for (int e = tid; e < p.K; e += 256) cp[e] = 0.f;
    }
}

// grid (ceil(streams * n_frames / 256)), 256 threads: theta of every alive slot for every frame, as k_mvdr_track_fill writes it, and --
// by the thread of a stream's first frame -- the (cos eps, sin eps) pair and the reported angle of every slot s < n_tracks: the clamp in
// double and the double cos / sin of k_mvdr_elevations (kernels_mvdr_map.hip), so the bytes mca_hip_mvdr_set_elevations_dev leaves for the
// same angles.  A dead slot takes (theta, eps) of the lowest alive slot; a stream without an alive slot 0 rad and the context's pair
__global__ __launch_bounds__(256) void k_mvdr_trk2_fill(MvdrTrk2FillArgs p)
{
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)p.n_streams * p.n_frames) return;
    const int a = (int)(id / p.n_frames);
    float first = 0.f, first_el = __int_as_float(0x7fc00000);
    for (int s = p.n_tracks - 1; s >= 0; --s)
        if (p.st.alive[a * MCA_MAX_SOURCES + s]) { first = p.st.theta[a * MCA_MAX_SOURCES + s]; first_el = p.st.eps[a * MCA_MAX_SOURCES + s]; }
    for (int s = 0; s < p.n_tracks; ++s)
        p.doa_rad[id * p.n_tracks + s] = p.st.alive[a * MCA_MAX_SOURCES + s] ? p.st.theta[a * MCA_MAX_SOURCES + s] : first;
    if (id - (long long)a * p.n_frames != 0) return;
    for (int s = 0; s < p.n_tracks; ++s) {
        const int o = a * MCA_MAX_SOURCES + s;
        const float v = p.st.alive[o] ? p.st.eps[o] : first_el;
        if (v != v) {
            p.slot_el[o] = make_double2(p.ce, p.se);
            p.slot_val[o] = v;
            continue;
        }
        const double eps = fmin(fmax((double)v, -1.57079632679489661923), 1.57079632679489661923);
        p.slot_el[o] = make_double2(cos(eps), sin(eps));
        p.slot_val[o] = (float)eps;
    }
}

// grid (ceil(streams * n_tracks / 256)), 256 threads: a slot whose azimuth or elevation is not finite is left as it is
__global__ __launch_bounds__(256) void k_mvdr_trk2_seed(MvdrTrk2SeedArgs p)
{
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= p.n_streams * p.n_tracks) return;
    const int a = id / p.n_tracks, s = id - a * p.n_tracks, o = a * MCA_MAX_SOURCES + s;
    const float v = p.az[id], w = p.el[id];
    if (!trk2_finite(v) || !trk2_finite(w)) return;
    p.st.theta[o] = mvdr_track_angle(v, 1); p.st.eps[o] = trk2_clamp_el(w); p.st.alive[o] = 1; p.st.miss[o] = 0; p.st.gen[o] += 1;
}

}  // namespace mca
