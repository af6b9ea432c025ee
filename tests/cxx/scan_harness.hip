// scan_harness.hip -- TEST-ONLY, libscan_harness.so (tests/test_gpu_scan_kernels.py): csrc/kernels_stream.hip included unchanged and
// compiled with the product's line for it (-fno-slp-vectorize), behind one launcher per kernel of the group that turns the correlation map
// into DOA bins: k_scan_partial, k_scan_carry, k_scan_pick<PL, MODE>, k_scan_repick<PL, false>, k_gate, k_doa_fill, k_hist_list and
// k_hist_settle.  A library of its own: a second translation unit with the same kernels cannot link into libgemm_harness.so.
// Same rules as gemm_harness_stream.hip: host pointers and counts in, every argument validated before anything is launched -- every entry
// of clist, chunk_from, list and nvoiced a kernel will index is checked against the buffer it addresses --, exactly sized device buffers,
// the hipError_t out as an int, no abort and no print; in / out buffers go back whole.  Launch shapes are the product's (api.hip,
// localise_impl).
// Out of scope: k_scan_repick<PL, true> -- its transform-and-patch half is tests/test_gpu_steer_tail.py's.
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../mcarray_amd/csrc/kernels_stream.hip"
#include "gemm_harness.h"

using namespace mca;

namespace {
constexpr int BAD = (int)hipErrorInvalidValue;
constexpr float MAG = 1.2676506e30f;                    // 2^100: every float a recursion reads is finite and at most this (no overflow in 512 steps)

inline int round_up_i(int x, int m) { return (x + m - 1) / m * m; }

// every float of [rows][ld], columns 0 .. cols - 1, finite and at most MAG (the pad columns may hold anything)
bool bounded(const float *x, long long rows, int ld, int cols)
{
    for (long long r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            const float v = x[r * ld + c];
            if (!(std::fabs(v) <= MAG)) return false;
        }
    return true;
}

// a device buffer that may be absent (host == NULL): p stays NULL
struct OBuf {
    gh::DBuf b;
    bool on = false;
    hipError_t up(const void *host, size_t n) { on = host != nullptr; return on ? b.up(host, n) : hipSuccess; }
    hipError_t down(void *host) const { return on ? b.down(host) : hipSuccess; }
    template <typename T> T *ptr() const { return on ? (T *)b.p : nullptr; }
};
}  // namespace

extern "C" {

// the shape every scan launcher shares
struct ShDims {
    int arrays, n_frames, D, Dp, S, P, c_planes, chunk;
    float mu, omu, inv_norm;
};

// what k_scan_pick takes beyond the shape.  Pointers are host pointers; "io" buffers are copied in, and copied back whole.
struct ShPick {
    int PL, mode, lookback;
    const float *C;                 // [c_planes][arrays][n_frames][Dp]
    const unsigned char *voiced;    // [arrays][n_frames] or NULL
    const float *part; int part_planes;          // [part_planes][arrays][n_chunks][D] (lookback > 0)
    const float *state_in;          // [arrays][D] (lookback > 0)
    float *e_start;                 // io [arrays][n_chunks][D]: read without the look-back, written with it
    float *state_out;               // io [arrays][D]
    const float *grid;              // [D]
    int *doa_bin; float *doa_rad; float *prob;   // io [arrays][n_frames][S]; doa_rad / prob may be NULL
    float *energy;                  // io [arrays][n_frames][D] or NULL
    // mode 1
    float tau;
    unsigned char *flags;           // io [arrays][n_frames]
    int gpa;                        // repair units per array = ceil(n_frames / REPAIR_GROUP)
    int *need, *list; int list_len; // io [list_len] each, list_len >= arrays * gpa + arrays * HIST_UNITS
    int *n_list;                    // io [1]
    int *chunk_from;                // io [arrays][n_chunks], every entry >= n_chunks at entry
    int *clist; int clist_len;      // io [clist_len], clist_len >= arrays * n_chunks
    int *n_clist;                   // io [2]
    int *last_vchunk;               // io [arrays]: read without the look-back, written with it
    unsigned long long *stats;      // io [4]
    const unsigned char *dead, *unsure;          // [arrays][n_frames] or NULL
    int lazy, hist_valid, hist_base;
    float *hist_C_out, *e_hist_out; // io [arrays][HIST_FRAMES][Dp], [arrays][D] (lazy)
    unsigned *umask; int umask_words;            // io [list_len][umask_words] or NULL (whole rows)
    int *n_miss;                    // io [1 + arrays * n_frames] or NULL
    const int *pred;                // [arrays] (with n_miss): SteerPatchArgs::bf.pred, the only member of it that is set
};

struct ShRepick {
    int PL, grid_x;
    const float *C;                 // [c_planes][arrays][n_frames][Dp], the listed rows already exact
    const unsigned char *voiced;    // [arrays][n_frames] or NULL
    const float *e_start;           // [arrays][n_chunks][D], the coarse pass's
    const unsigned char *flags;     // [arrays][n_frames]
    int *clist; int clist_len;      // io
    int *n_clist;                   // io [2]; [1] is zero at entry
    int *chunk_from;                // io [arrays][n_chunks]
    const int *last_vchunk;         // [arrays]
    int *n_list;                    // io [1]
    float *state_out;               // io [arrays][D]
    const float *grid;              // [D]
    int *doa_bin; float *doa_rad; float *prob;   // io [arrays][n_frames][S]
    float *energy;                  // io [arrays][n_frames][D] or NULL
    const float *hist_C_in, *e_hist_in;          // [arrays][HIST_FRAMES][Dp], [arrays][D] or NULL
};

void sh_constants(int *out)
{
    out[0] = SCAN_CHUNK; out[1] = SCAN_SUB; out[2] = REPAIR_WARM; out[3] = REPAIR_GROUP; out[4] = HIST_FRAMES; out[5] = HIST_UNITS;
    out[6] = CAND_WORDS_MAX; out[7] = MCA_MAX_SOURCES;
}

// The product's choice of the positions per lane of the peak pick -- RESTATED from api.hip (localise_impl: `ppl`), not shared with it.
int sh_product_pl(int D) { return D - 2 <= 128 ? 2 : D - 2 <= 384 ? 6 : 8; }

}  // extern "C"

namespace {
bool dims_ok(const ShDims *d)
{
    return d && d->arrays >= 1 && d->arrays <= 8 && d->n_frames >= 1 && d->n_frames <= 512 && d->D >= 3 && d->D <= 514 && d->Dp >= d->D && d->Dp <= 576 &&
           d->Dp % 64 == 0 && d->S >= 1 && d->S <= MCA_MAX_SOURCES && d->P >= 1 && d->P <= 1024 && d->c_planes >= 1 && d->c_planes <= 8 && d->chunk == SCAN_CHUNK &&
           d->mu >= 0.f && d->mu <= 1.f && d->omu >= 0.f && d->omu <= 1.f && std::isfinite(d->inv_norm);
}
inline int n_chunks_of(const ShDims *d) { return (d->n_frames + d->chunk - 1) / d->chunk; }
inline long long map_rows(const ShDims *d) { return (long long)d->arrays * d->n_frames; }
inline size_t map_bytes(const ShDims *d) { return (size_t)d->c_planes * map_rows(d) * d->Dp * 4; }
bool bytes01(const unsigned char *x, long long n)
{
    for (long long i = 0; i < n; ++i) if (x[i] > 1) return false;
    return true;
}
void fill_common(ScanPickArgs &pa, const ShDims *d)
{
    pa.c_planes = d->c_planes; pa.c_plane_stride = map_rows(d) * d->Dp; pa.n_frames = d->n_frames; pa.Dp = d->Dp; pa.D = d->D; pa.P = d->P; pa.S = d->S;
    pa.chunk = d->chunk; pa.n_chunks = n_chunks_of(d); pa.mu = d->mu; pa.one_minus_mu = d->omu; pa.inv_norm = d->inv_norm;
}

// The product's block, max(round_up(D, 64), 512), is 576 threads for D = 513, 514.  k_scan_pick<8, MODE> is bound to 576; k_scan_repick is
// bound to 512 (at 576 it would spill a hundred registers), and a launch above a kernel's bound is turned down by the runtime: asked before
// the launch, not tried.  (The product itself refuses D > 512 when a context is made.)
bool block_fits(const void *kernel, int block)
{
    hipFuncAttributes fa;
    return hipFuncGetAttributes(&fa, kernel) == hipSuccess && block <= fa.maxThreadsPerBlock;
}

template <int PL, int MODE>
hipError_t launch_pick(const ScanPickArgs &pa, int arrays)
{
    const size_t smem = (size_t)SCAN_SUB * (pa.Dp + 8) * sizeof(float);
    if (smem > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_scan_pick<PL, MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
    }
    const int block = std::max(round_up_i(pa.D, 64), 512);
    if (!block_fits(reinterpret_cast<const void *>(k_scan_pick<PL, MODE>), block)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL((k_scan_pick<PL, MODE>), dim3(pa.n_chunks, arrays), dim3(block), smem, 0, pa);
    return gh::finish();
}
template <int PL>
hipError_t launch_repick(const ScanPickArgs &pa, int grid_x)
{
    const size_t smem = (size_t)32 * (pa.Dp + 8) * sizeof(float);
    if (smem > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_scan_repick<PL, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
    }
    const int block = std::max(round_up_i(pa.D, 64), 512);
    if (!block_fits(reinterpret_cast<const void *>(&k_scan_repick<PL, false>), block)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL((k_scan_repick<PL, false>), dim3(grid_x), dim3(block), smem, 0, pa);
    return gh::finish();
}
}  // namespace

extern "C" {

// k_scan_partial.  part: io [arrays][n_chunks][D], nvoiced: io [arrays][n_chunks]
int sh_partial(const ShDims *d, const float *C, const unsigned char *voiced, float *part, int *nvoiced)
{
    if (!dims_ok(d) || !C || !part || !nvoiced) return BAD;
    if (!bounded(C, (long long)d->c_planes * map_rows(d), d->Dp, d->D) || (voiced && !bytes01(voiced, map_rows(d)))) return BAD;
    const int nc = n_chunks_of(d);
    gh::DBuf dC, dP, dN; OBuf dV;
    hipError_t e;
    if ((e = dC.up(C, map_bytes(d))) != hipSuccess) return (int)e;
    if ((e = dV.up(voiced, (size_t)map_rows(d))) != hipSuccess) return (int)e;
    if ((e = dP.up(part, (size_t)d->arrays * nc * d->D * 4)) != hipSuccess) return (int)e;
    if ((e = dN.up(nvoiced, (size_t)d->arrays * nc * 4)) != hipSuccess) return (int)e;
    ScanPickArgs pa{};
    fill_common(pa, d);
    pa.C = (const float *)dC.p; pa.voiced = dV.ptr<const unsigned char>(); pa.part = (float *)dP.p; pa.nvoiced = (int *)dN.p;
    hipLaunchKernelGGL(k_scan_partial, dim3(nc, d->arrays), dim3(round_up_i(d->Dp / 4, 64)), 0, 0, pa);
    if ((e = gh::finish()) != hipSuccess) return (int)e;
    if ((e = dP.down(part)) != hipSuccess) return (int)e;
    return (int)dN.down(nvoiced);
}

// k_scan_carry.  part: [part_planes][arrays][n_chunks][D]; e_start io [arrays][n_chunks][D]; state_out io [arrays][D];
// mode 1: n_list io [1], n_clist io [2], last_vchunk io [arrays]
int sh_carry(const ShDims *d, int mode, const float *part, int part_planes, const int *nvoiced, const float *state_in, float *e_start, float *state_out,
             int *n_list, int *n_clist, int *last_vchunk)
{
    if (!dims_ok(d) || (mode != 0 && mode != 1) || !part || (part_planes != 1 && part_planes != 2) || !nvoiced || !state_in || !e_start || !state_out) return BAD;
    if (mode == 1 && (!n_list || !n_clist || !last_vchunk)) return BAD;
    const int nc = n_chunks_of(d);
    const long long pn = (long long)d->arrays * nc;
    for (long long i = 0; i < pn; ++i) if (nvoiced[i] < 0 || nvoiced[i] > SCAN_CHUNK) return BAD;      // the index of the table of powers
    if (!bounded(part, part_planes * pn, d->D, d->D) || !bounded(state_in, d->arrays, d->D, d->D)) return BAD;
    gh::DBuf dP, dN, dS, dE, dO; OBuf dL, dCl, dLv;
    hipError_t e;
    if ((e = dP.up(part, (size_t)part_planes * pn * d->D * 4)) != hipSuccess) return (int)e;
    if ((e = dN.up(nvoiced, (size_t)pn * 4)) != hipSuccess) return (int)e;
    if ((e = dS.up(state_in, (size_t)d->arrays * d->D * 4)) != hipSuccess) return (int)e;
    if ((e = dE.up(e_start, (size_t)pn * d->D * 4)) != hipSuccess) return (int)e;
    if ((e = dO.up(state_out, (size_t)d->arrays * d->D * 4)) != hipSuccess) return (int)e;
    if (mode == 1) {
        if ((e = dL.up(n_list, 4)) != hipSuccess) return (int)e;
        if ((e = dCl.up(n_clist, 8)) != hipSuccess) return (int)e;
        if ((e = dLv.up(last_vchunk, (size_t)d->arrays * 4)) != hipSuccess) return (int)e;
    }
    ScanPickArgs pa{};
    fill_common(pa, d);
    pa.mode = mode; pa.part = (float *)dP.p; pa.part_planes = part_planes; pa.part_plane_stride = pn * d->D; pa.nvoiced = (int *)dN.p;
    pa.state_in = (const float *)dS.p; pa.e_start = (float *)dE.p; pa.state_out = (float *)dO.p;
    pa.n_list = dL.ptr<int>(); pa.n_clist = dCl.ptr<int>(); pa.last_vchunk = dLv.ptr<int>();
    hipLaunchKernelGGL(k_scan_carry, dim3(d->arrays, round_up_i(d->D, 64) / 64), dim3(64), 0, 0, pa);
    if ((e = gh::finish()) != hipSuccess) return (int)e;
    if ((e = dE.down(e_start)) != hipSuccess) return (int)e;
    if ((e = dO.down(state_out)) != hipSuccess) return (int)e;
    if ((e = dL.down(n_list)) != hipSuccess) return (int)e;
    if ((e = dCl.down(n_clist)) != hipSuccess) return (int)e;
    return (int)dLv.down(last_vchunk);
}

// k_scan_pick<PL, mode>
int sh_pick(const ShDims *d, const ShPick *q)
{
    if (!dims_ok(d) || !q) return BAD;
    const int PL = q->PL, D = d->D, nc = n_chunks_of(d), arrays = d->arrays;
    const long long rows = map_rows(d), pn = (long long)arrays * nc;
    if ((PL != 2 && PL != 6 && PL != 8) || PL * 64 < D - 2 || (q->mode != 0 && q->mode != 1) || (q->lookback != 0 && q->lookback != 4)) return BAD;
    if (!q->C || !q->e_start || !q->grid || !q->doa_bin || !q->state_out) return BAD;
    if (!bounded(q->C, (long long)d->c_planes * rows, d->Dp, D) || (q->voiced && !bytes01(q->voiced, rows))) return BAD;
    if (q->lookback) {
        if (!q->part || (q->part_planes != 1 && q->part_planes != 2) || !q->state_in) return BAD;
        if (!bounded(q->part, q->part_planes * pn, D, D) || !bounded(q->state_in, arrays, D, D)) return BAD;
    } else if (!bounded(q->e_start, pn, D, D)) return BAD;
    const bool m1 = q->mode == 1;
    const bool cand = m1 && q->umask != nullptr;
    if (m1) {
        const int gpa = (d->n_frames + REPAIR_GROUP - 1) / REPAIR_GROUP;
        if (!q->flags || !q->need || !q->list || !q->n_list || !q->chunk_from || !q->clist || !q->n_clist || !q->last_vchunk || !q->stats) return BAD;
        if (!(q->tau >= 0.f) || !std::isfinite(q->tau) || q->gpa != gpa || q->hist_base != arrays * gpa) return BAD;
        if ((long long)q->list_len < (long long)arrays * gpa + (long long)arrays * HIST_UNITS || q->list_len > (1 << 20)) return BAD;
        // every unit whose test-and-set word is free may be appended once: the list has room behind its length at entry
        int free_units = 0;
        for (int i = 0; i < q->list_len; ++i) {
            if (q->need[i] != 0 && q->need[i] != 1) return BAD;
            free_units += q->need[i] == 0;
        }
        if (q->n_list[0] < 0 || (long long)q->n_list[0] + free_units > q->list_len) return BAD;
        for (long long i = 0; i < pn; ++i) if (q->chunk_from[i] < nc) return BAD;                       // "no flagged frame" at entry
        if (q->clist_len < pn || q->n_clist[0] < 0 || (long long)q->n_clist[0] + pn > q->clist_len) return BAD;
        if (!q->lookback) for (int a = 0; a < arrays; ++a) if (q->last_vchunk[a] < -1 || q->last_vchunk[a] >= nc) return BAD;
        if ((q->lazy != 0 && q->lazy != 1) || (q->hist_valid != 0 && q->hist_valid != 1)) return BAD;
        if (q->lazy && (!q->hist_C_out || !q->e_hist_out)) return BAD;
        if ((q->dead && !bytes01(q->dead, rows)) || (q->unsure && !bytes01(q->unsure, rows))) return BAD;
        if (cand && (q->umask_words != d->Dp / 32 || q->umask_words > CAND_WORDS_MAX)) return BAD;
        if (q->n_miss && (!q->pred || q->n_miss[0] != 0 || SCAN_SUB != SCAN_CHUNK)) return BAD;          // the list holds every frame of the call once
    }
    gh::DBuf dC, dE, dO, dG, dB;
    OBuf dV, dP, dS, dR, dPr, dEn, dF, dNeed, dL, dNl, dCf, dCl, dNc, dLv, dSt, dDead, dUn, dHc, dEh, dUm, dNm, dPred;
    hipError_t e;
    const size_t out_n = (size_t)rows * d->S;
#define UP(buf, host, bytes) if ((e = (buf).up((host), (bytes))) != hipSuccess) return (int)e
    UP(dC, q->C, map_bytes(d));
    UP(dV, q->voiced, (size_t)rows);
    UP(dP, q->lookback ? q->part : nullptr, (size_t)(q->lookback ? q->part_planes : 0) * pn * D * 4);
    UP(dS, q->lookback ? q->state_in : nullptr, (size_t)arrays * D * 4);
    UP(dE, q->e_start, (size_t)pn * D * 4);
    UP(dO, q->state_out, (size_t)arrays * D * 4);
    UP(dG, q->grid, (size_t)D * 4);
    UP(dB, q->doa_bin, out_n * 4);
    UP(dR, q->doa_rad, out_n * 4);
    UP(dPr, q->prob, out_n * 4);
    UP(dEn, q->energy, (size_t)rows * D * 4);
    if (m1) {
        UP(dF, q->flags, (size_t)rows);
        UP(dNeed, q->need, (size_t)q->list_len * 4);
        UP(dL, q->list, (size_t)q->list_len * 4);
        UP(dNl, q->n_list, 4);
        UP(dCf, q->chunk_from, (size_t)pn * 4);
        UP(dCl, q->clist, (size_t)q->clist_len * 4);
        UP(dNc, q->n_clist, 8);
        UP(dLv, q->last_vchunk, (size_t)arrays * 4);
        UP(dSt, q->stats, 32);
        UP(dDead, q->dead, (size_t)rows);
        UP(dUn, q->unsure, (size_t)rows);
        UP(dHc, q->lazy ? q->hist_C_out : nullptr, (size_t)arrays * HIST_FRAMES * d->Dp * 4);
        UP(dEh, q->lazy ? q->e_hist_out : nullptr, (size_t)arrays * D * 4);
        UP(dUm, q->umask, (size_t)q->list_len * (cand ? q->umask_words : 0) * 4);
        UP(dNm, q->n_miss, (size_t)(1 + rows) * 4);
        UP(dPred, q->n_miss ? q->pred : nullptr, (size_t)arrays * 4);
    }
    ScanPickArgs pa{};
    fill_common(pa, d);
    pa.C = (const float *)dC.p; pa.voiced = dV.ptr<const unsigned char>(); pa.part = dP.ptr<float>(); pa.part_planes = q->lookback ? q->part_planes : 1;
    pa.part_plane_stride = pn * D; pa.state_in = dS.ptr<const float>(); pa.e_start = (float *)dE.p; pa.state_out = (float *)dO.p; pa.grid = (const float *)dG.p;
    pa.doa_bin = (int *)dB.p; pa.doa_rad = dR.ptr<float>(); pa.prob = dPr.ptr<float>(); pa.energy = dEn.ptr<float>(); pa.mode = q->mode; pa.lookback = q->lookback;
    if (m1) {
        pa.tau = q->tau; pa.flags = dF.ptr<unsigned char>(); pa.groups_per_array = q->gpa; pa.need = dNeed.ptr<int>(); pa.list = dL.ptr<int>(); pa.n_list = dNl.ptr<int>();
        pa.chunk_from = dCf.ptr<int>(); pa.clist = dCl.ptr<int>(); pa.n_clist = dNc.ptr<int>(); pa.last_vchunk = dLv.ptr<int>(); pa.stats = dSt.ptr<unsigned long long>();
        pa.dead = dDead.ptr<const unsigned char>(); pa.unsure = dUn.ptr<const unsigned char>(); pa.lazy = q->lazy; pa.hist_valid = q->hist_valid; pa.hist_base = q->hist_base;
        pa.hist_C_out = dHc.ptr<float>(); pa.e_hist_out = dEh.ptr<float>(); pa.umask = dUm.ptr<unsigned>(); pa.umask_words = cand ? q->umask_words : 0;
        pa.n_miss = dNm.ptr<int>(); pa.miss_cap = (int)rows; pa.sp.bf.pred = dPred.ptr<const int>();
    }
    if (m1) e = PL == 2 ? launch_pick<2, 1>(pa, arrays) : PL == 6 ? launch_pick<6, 1>(pa, arrays) : launch_pick<8, 1>(pa, arrays);
    else e = PL == 2 ? launch_pick<2, 0>(pa, arrays) : PL == 6 ? launch_pick<6, 0>(pa, arrays) : launch_pick<8, 0>(pa, arrays);
    if (e != hipSuccess) return (int)e;
#define DOWN(buf, host) if ((e = (buf).down((void *)(host))) != hipSuccess) return (int)e
    DOWN(dE, q->e_start); DOWN(dO, q->state_out); DOWN(dB, q->doa_bin); DOWN(dR, q->doa_rad); DOWN(dPr, q->prob); DOWN(dEn, q->energy);
    if (m1) {
        DOWN(dF, q->flags); DOWN(dNeed, q->need); DOWN(dL, q->list); DOWN(dNl, q->n_list); DOWN(dCf, q->chunk_from); DOWN(dCl, q->clist); DOWN(dNc, q->n_clist);
        DOWN(dLv, q->last_vchunk); DOWN(dSt, q->stats); DOWN(dHc, q->hist_C_out); DOWN(dEh, q->e_hist_out); DOWN(dUm, q->umask); DOWN(dNm, q->n_miss);
    }
    return (int)hipSuccess;
}

// k_scan_repick<PL, false> on grid_x workgroups
int sh_repick(const ShDims *d, const ShRepick *q)
{
    if (!dims_ok(d) || !q) return BAD;
    const int PL = q->PL, D = d->D, nc = n_chunks_of(d), arrays = d->arrays;
    const long long rows = map_rows(d), pn = (long long)arrays * nc;
    if ((PL != 2 && PL != 6 && PL != 8) || PL * 64 < D - 2 || q->grid_x < 1 || q->grid_x > 256) return BAD;
    if (!q->C || !q->e_start || !q->flags || !q->clist || !q->n_clist || !q->chunk_from || !q->last_vchunk || !q->n_list || !q->state_out || !q->grid || !q->doa_bin) return BAD;
    if ((q->hist_C_in == nullptr) != (q->e_hist_in == nullptr)) return BAD;
    // without the gate the kernel requests the 32 rows of chunk max(chunk - 1, 0) unclamped (the product runs it on calls of 64 frames and more)
    if (!q->voiced && d->n_frames < SCAN_CHUNK) return BAD;
    if (!bounded(q->C, (long long)d->c_planes * rows, d->Dp, D) || !bounded(q->e_start, pn, D, D) || !bytes01(q->flags, rows) || (q->voiced && !bytes01(q->voiced, rows))) return BAD;
    if (q->hist_C_in && (!bounded(q->hist_C_in, (long long)arrays * HIST_FRAMES, d->Dp, D) || !bounded(q->e_hist_in, arrays, D, D))) return BAD;
    if (q->clist_len < pn || q->n_clist[0] < 0 || q->n_clist[0] > q->clist_len || q->n_clist[1] != 0) return BAD;
    for (int i = 0; i < q->n_clist[0]; ++i) {
        const int ci = q->clist[i];
        if (ci < 0 || ci >= pn) return BAD;
        const int chunk = ci % nc, cf = q->chunk_from[ci];
        // the walk starts at a chunk of the same array, not behind this one; -1 (the history) only without the gate and with a history
        if (cf > chunk || cf < -1 || (cf == -1 && (q->voiced || !q->hist_C_in))) return BAD;
        if (!q->voiced && cf >= 0 && cf < chunk - 1) return BAD;            // (without the gate: this chunk or the one before it, REPAIR_WARM < chunk)
    }
    for (int a = 0; a < arrays; ++a) if (q->last_vchunk[a] < -1 || q->last_vchunk[a] >= nc) return BAD;
    gh::DBuf dC, dE, dF, dCl, dNc, dCf, dLv, dNl, dO, dG, dB;
    OBuf dV, dR, dPr, dEn, dHc, dEh;
    hipError_t e;
    const size_t out_n = (size_t)rows * d->S;
    UP(dC, q->C, map_bytes(d)); UP(dV, q->voiced, (size_t)rows); UP(dE, q->e_start, (size_t)pn * D * 4); UP(dF, q->flags, (size_t)rows);
    UP(dCl, q->clist, (size_t)q->clist_len * 4); UP(dNc, q->n_clist, 8); UP(dCf, q->chunk_from, (size_t)pn * 4); UP(dLv, q->last_vchunk, (size_t)arrays * 4);
    UP(dNl, q->n_list, 4); UP(dO, q->state_out, (size_t)arrays * D * 4); UP(dG, q->grid, (size_t)D * 4); UP(dB, q->doa_bin, out_n * 4);
    UP(dR, q->doa_rad, out_n * 4); UP(dPr, q->prob, out_n * 4); UP(dEn, q->energy, (size_t)rows * D * 4);
    UP(dHc, q->hist_C_in, (size_t)arrays * HIST_FRAMES * d->Dp * 4); UP(dEh, q->e_hist_in, (size_t)arrays * D * 4);
    ScanPickArgs pa{};
    fill_common(pa, d);
    pa.mode = 1; pa.C = (const float *)dC.p; pa.voiced = dV.ptr<const unsigned char>(); pa.e_start = (float *)dE.p; pa.flags = (unsigned char *)dF.p;
    pa.clist = (int *)dCl.p; pa.n_clist = (int *)dNc.p; pa.chunk_from = (int *)dCf.p; pa.last_vchunk = (int *)dLv.p; pa.n_list = (int *)dNl.p;
    pa.state_out = (float *)dO.p; pa.grid = (const float *)dG.p; pa.doa_bin = (int *)dB.p; pa.doa_rad = dR.ptr<float>(); pa.prob = dPr.ptr<float>();
    pa.energy = dEn.ptr<float>(); pa.hist_C_in = dHc.ptr<const float>(); pa.e_hist_in = dEh.ptr<const float>();
    e = PL == 2 ? launch_repick<2>(pa, q->grid_x) : PL == 6 ? launch_repick<6>(pa, q->grid_x) : launch_repick<8>(pa, q->grid_x);
    if (e != hipSuccess) return (int)e;
    DOWN(dCl, q->clist); DOWN(dNc, q->n_clist); DOWN(dCf, q->chunk_from); DOWN(dNl, q->n_list); DOWN(dO, q->state_out); DOWN(dB, q->doa_bin);
    DOWN(dR, q->doa_rad); DOWN(dPr, q->prob); DOWN(dEn, q->energy);
    return (int)hipSuccess;
}

// k_gate.  state io [arrays][4] double; voiced io [arrays][n_frames]; power_out io or NULL; post0 io [arrays] or NULL
int sh_gate(const float *power_lin, int arrays, int n_frames, int fft_n, int needed_samples, float margin_db, double eps, double *state, unsigned char *voiced,
            float *power_out, int *post0)
{
    if (!power_lin || !state || !voiced || arrays < 1 || arrays > 8 || n_frames < 1 || n_frames > 4096 || fft_n < 1 || needed_samples < 0) return BAD;
    const size_t n = (size_t)arrays * n_frames;
    gh::DBuf dP, dS, dV; OBuf dO, dP0;
    hipError_t e;
    UP(dP, power_lin, n * 4); UP(dS, state, (size_t)arrays * 32); UP(dV, voiced, n); UP(dO, power_out, n * 4); UP(dP0, post0, (size_t)arrays * 4);
    GateArgs g{};
    g.power_lin = (const float *)dP.p; g.n_frames = n_frames; g.fft_n = fft_n; g.needed_samples = needed_samples; g.margin_db = margin_db; g.eps = eps;
    g.state = (double *)dS.p; g.voiced = (unsigned char *)dV.p; g.power_out = dO.ptr<float>(); g.post0 = dP0.ptr<int>();
    hipLaunchKernelGGL(k_gate, dim3(arrays), dim3(256), 0, 0, g);
    if ((e = gh::finish()) != hipSuccess) return (int)e;
    DOWN(dS, state); DOWN(dV, voiced); DOWN(dO, power_out); DOWN(dP0, post0);
    return (int)hipSuccess;
}

// k_doa_fill (n_frames up to 4096 for this launcher: more than 1 024 frames give a thread a segment of several)
int sh_doa_fill(const unsigned char *voiced, int arrays, int n_frames, int S, int *doa_bin, float *doa_rad, float *prob, int *last_bin, float *last_rad, float *last_prob)
{
    if (!voiced || !doa_bin || !last_bin || arrays < 1 || arrays > 8 || n_frames < 1 || n_frames > 4096 || S < 1 || S > MCA_MAX_SOURCES) return BAD;
    if ((doa_rad && !last_rad) || (prob && !last_prob) || !bytes01(voiced, (long long)arrays * n_frames)) return BAD;
    const size_t n = (size_t)arrays * n_frames * S;
    gh::DBuf dV, dB, dLb; OBuf dR, dPr, dLr, dLp;
    hipError_t e;
    UP(dV, voiced, (size_t)arrays * n_frames); UP(dB, doa_bin, n * 4); UP(dLb, last_bin, (size_t)arrays * S * 4); UP(dR, doa_rad, n * 4); UP(dPr, prob, n * 4);
    UP(dLr, doa_rad ? last_rad : nullptr, (size_t)arrays * S * 4); UP(dLp, prob ? last_prob : nullptr, (size_t)arrays * S * 4);
    DoaFillArgs f{};
    f.voiced = (const unsigned char *)dV.p; f.n_frames = n_frames; f.S = S; f.doa_bin = (int *)dB.p; f.doa_rad = dR.ptr<float>(); f.prob = dPr.ptr<float>();
    f.last_bin = (int *)dLb.p; f.last_rad = dLr.ptr<float>(); f.last_prob = dLp.ptr<float>();
    hipLaunchKernelGGL(k_doa_fill, dim3(arrays), dim3(1024), 0, 0, f);
    if ((e = gh::finish()) != hipSuccess) return (int)e;
    DOWN(dB, doa_bin); DOWN(dR, doa_rad); DOWN(dPr, prob); DOWN(dLb, last_bin); DOWN(dLr, last_rad); DOWN(dLp, last_prob);
    return (int)hipSuccess;
}

// k_hist_list: list / need io [len], n_list io [1]
int sh_hist_list(int *list, int *need, int len, int *n_list, int n_units)
{
    if (!list || !need || !n_list || len < 1 || len > (1 << 20) || n_units < 0 || n_units > len) return BAD;
    gh::DBuf dL, dN, dC;
    hipError_t e;
    UP(dL, list, (size_t)len * 4); UP(dN, need, (size_t)len * 4); UP(dC, n_list, 4);
    hipLaunchKernelGGL(k_hist_list, dim3(std::max((n_units + 255) / 256, 1)), dim3(256), 0, 0, (int *)dL.p, (int *)dC.p, (int *)dN.p, n_units);
    if ((e = gh::finish()) != hipSuccess) return (int)e;
    DOWN(dL, list); DOWN(dN, need); DOWN(dC, n_list);
    return (int)hipSuccess;
}

// k_hist_settle: e_hist [arrays][D], hist_C [arrays][HIST_FRAMES][Dp], state io [arrays][D], n_list io [1]
int sh_hist_settle(const float *e_hist, const float *hist_C, float *state, int *n_list, int arrays, int D, int Dp, float mu, float omu)
{
    if (!e_hist || !hist_C || !state || !n_list || arrays < 1 || arrays > 8 || D < 3 || D > 512 || Dp < D || Dp > 576 || Dp % 64 != 0) return BAD;
    gh::DBuf dE, dH, dS, dN;
    hipError_t e;
    UP(dE, e_hist, (size_t)arrays * D * 4); UP(dH, hist_C, (size_t)arrays * HIST_FRAMES * Dp * 4); UP(dS, state, (size_t)arrays * D * 4); UP(dN, n_list, 4);
    hipLaunchKernelGGL(k_hist_settle, dim3(arrays), dim3(std::max(round_up_i(D, 64), 64)), 0, 0, (const float *)dE.p, (const float *)dH.p, (float *)dS.p, (int *)dN.p, D, Dp, mu, omu);
    if ((e = gh::finish()) != hipSuccess) return (int)e;
    DOWN(dS, state); DOWN(dN, n_list);
    return (int)hipSuccess;
}
#undef UP
#undef DOWN

}  // extern "C"
