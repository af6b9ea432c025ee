// xform_harness.hip -- TEST-ONLY kernels (tests/test_gpu_xform.py): every wave-level transform and packed complex product of
// csrc/fft512.h, fft1024c.h, fft_block.h and pair_balance.h behind a kernel that does nothing but load, call and store.  The headers
// are included unchanged and compiled with the product's line for them (-fno-slp-vectorize: what runs is the headers' own assembly).
// Launch shape: one wave per transform, four waves per workgroup; LDS: the twiddle table first, then wave w's scratch at
// w * FFT_SCRATCH / w * F1K_SCRATCH, as the product lays them out.  Device tables come from the product's initialisers, the host
// tables exp(-j 2 pi i / N) are built in double and rounded to float like d_tw of csrc/api.hip.
// Entry points: extern "C", host pointers and counts in, the hipError_t out as an int; they never abort or print.
// build: tests/cxx/Makefile (nothing of the product links this library)
#include <hip/hip_runtime.h>
#include <cmath>
#include <vector>
#include "fft512.h"
#include "fft1024c.h"
#include "fft_block.h"
#include "pair_balance.h"

using namespace mca;

namespace {

constexpr int WPB = 4, NT = 64 * WPB;        // waves per workgroup, threads

// ---- complex arithmetic: thread = element; in: (acc, a, b) as 6 floats; out: 2 floats --------------------------------------------
__global__ __launch_bounds__(NT) void k_carith(int op, const float2 *in, float2 *out, int n)
{
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const float2 c = in[3 * i], a = in[3 * i + 1], b = in[3 * i + 2];
    float2 r = make_float2(0.f, 0.f);
    switch (op) {
    case 0: r = cmul(a, b); break;
    case 1: r = cmulc(a, b); break;
    case 2: r = cmac(c, a, b); break;
    case 3: r = cmacc(c, a, b); break;
    case 4: r = cnmac(c, a, b); break;
    case 5: r = cnmacc(c, a, b); break;
    case 6: r = csub_jb(a, b); break;
    case 7: r = cadd_jb(a, b); break;
    case 8: r = cscale(a, b.x); break;
    case 9: r = cmul_mj(a); break;
    case 10: r = cmul_pj(a); break;
    }
    out[i] = r;
}

// ---- the in-register DFTs: thread = transform, natural order out (br3 / dr16 undone) --------------------------------------------
template <int P, bool INV>
__global__ __launch_bounds__(NT) void k_small_dft(const float2 *in, float2 *out, int n)
{
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    if constexpr (P == 4) {
        float2 a0 = in[4 * i], a1 = in[4 * i + 1], a2 = in[4 * i + 2], a3 = in[4 * i + 3];
        bfly4<INV>(a0, a1, a2, a3);
        out[4 * i] = a0; out[4 * i + 1] = a1; out[4 * i + 2] = a2; out[4 * i + 3] = a3;
    } else if constexpr (P == 8) {
        float2 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = in[8 * i + r];
        fft8<INV>(v);
#pragma unroll
        for (int r = 0; r < 8; ++r) out[8 * i + br3(r)] = v[r];
    } else {
        float2 v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = in[16 * i + r];
        fft16<INV>(v);
#pragma unroll
        for (int r = 0; r < 16; ++r) out[16 * i + dr16(r)] = v[r];
    }
}

// ---- pair_balance.h ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_maxabs(int three, const float *in, float *out, int n)
{
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    out[i] = three ? max3abs(in[3 * i], in[3 * i + 1], in[3 * i + 2]) : max2abs(in[3 * i], in[3 * i + 1]);
}

// wave = case: in [n][2][64], out [n][2][64] (every lane's view of the two maxima)
__global__ __launch_bounds__(NT) void k_wave_max64_2(const float *in, float *out, int n)
{
    const int lane = threadIdx.x & 63, idx = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (idx >= n) return;
    float a = in[(2 * idx) * 64 + lane], b = in[(2 * idx + 1) * 64 + lane];
    wave_max64_2(a, b);
    out[(2 * idx) * 64 + lane] = a; out[(2 * idx + 1) * 64 + lane] = b;
}

// wave = case: in [n][2][64] (ma, mb per lane), out [n][4] (na, nb, alive_a, alive_b)
__global__ __launch_bounds__(NT) void k_pair_balance(const float *in, int *out, int n)
{
    const int lane = threadIdx.x & 63, idx = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (idx >= n) return;
    const PairBalance pb = pair_balance(in[(2 * idx) * 64 + lane], in[(2 * idx + 1) * 64 + lane]);
    if (lane == 0) { out[4 * idx] = pb.na; out[4 * idx + 1] = pb.nb; out[4 * idx + 2] = pb.alive_a ? 1 : 0; out[4 * idx + 3] = pb.alive_b ? 1 : 0; }
}

// ---- the tables as the initialisers leave them ------------------------------------------------------------------------------------
// which 0: fft_table_init without a window (TW_WIN words), 1: with one (TW_WORDS), 2: f1k_table_init (F1K_TWORDS; the two pad words of
// a row read back as the zeros written here), 3: F1kLane::wb[1..3] of the 64 lanes (3 words per lane)
__global__ __launch_bounds__(NT) void k_tables(int which, const float *window, float2 *out)
{
    __shared__ __attribute__((aligned(16))) float2 tab[TW_WORDS];
    const int tid = threadIdx.x;
    for (int e = tid; e < TW_WORDS; e += NT) tab[e] = make_float2(0.f, 0.f);
    __syncthreads();
    if (which == 0) fft_table_init(tab, nullptr, tid, NT);
    else if (which == 1) fft_table_init(tab, window, tid, NT);
    else if (which == 2) f1k_table_init(tab, tid, NT);
    __syncthreads();
    if (which == 3) {
        if (tid < 64) {
            F1kLane lc;
            lc.init(tid);
            for (int q = 1; q < 4; ++q) out[3 * tid + q - 1] = lc.wb[q];
        }
        return;
    }
    const int words = which == 0 ? TW_WIN : which == 1 ? TW_WORDS : F1K_TWORDS;
    for (int e = tid; e < words; e += NT) out[e] = tab[e];
}

// ---- fft512.h: the 512-point complex transform and the real transforms on it -----------------------------------------------------
// in [n][512], out [n][512] natural order
template <bool INV, bool AHEAD>
__global__ __launch_bounds__(NT) void k_cfft512(const float2 *in, float2 *out, int n)
{
    __shared__ __attribute__((aligned(16))) float2 smem[TW_WIN + WPB * FFT_SCRATCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, idx = blockIdx.x * WPB + wave;
    fft_table_init(smem, nullptr, tid, NT);
    __syncthreads();
    if (idx >= n) return;
    const FftTw tw{smem};
    float2 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = in[(long long)idx * 512 + lane + 64 * r];
    cfft512_regs<INV, AHEAD>(v, smem + TW_WIN + wave * FFT_SCRATCH, lane, tw);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[(long long)idx * 512 + lane + 64 * br3(i)] = v[i];
}

// in [n][1024] real, out [n][513]; the kernel passes (x[2m], x[2m+1]) / 2 as the header asks of its caller
template <bool AHEAD>
__global__ __launch_bounds__(NT) void k_rfft1024(const float2 *in, float2 *out, int n)
{
    __shared__ __attribute__((aligned(16))) float2 smem[TW_WIN + WPB * FFT_SCRATCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, idx = blockIdx.x * WPB + wave;
    fft_table_init(smem, nullptr, tid, NT);
    __syncthreads();
    if (idx >= n) return;
    const FftTw tw{smem};
    float2 *buf = smem + TW_WIN + wave * FFT_SCRATCH;
    float2 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const float2 x = in[(long long)idx * 512 + lane + 64 * r];
        v[r] = make_float2(0.5f * x.x, 0.5f * x.y);
    }
    rfft1024<AHEAD>(v, buf, lane, tw);
    for (int k = lane; k < FFT_K; k += 64) out[(long long)idx * FFT_K + k] = buf[k];
}

// in [n][513], out [n][1024] real
__global__ __launch_bounds__(NT) void k_irfft1024(const float2 *in, float2 *out, int n)
{
    __shared__ __attribute__((aligned(16))) float2 smem[TW_WIN + WPB * FFT_SCRATCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, idx = blockIdx.x * WPB + wave;
    fft_table_init(smem, nullptr, tid, NT);
    __syncthreads();
    if (idx >= n) return;
    const FftTw tw{smem};
    float2 *buf = smem + TW_WIN + wave * FFT_SCRATCH;
    for (int k = lane; k < FFT_K; k += 64) buf[k] = in[(long long)idx * FFT_K + k];
    wave_lds_fence();
    irfft1024(buf, lane, tw);
    for (int m = lane; m < 512; m += 64) out[(long long)idx * 512 + m] = buf[m];
}

// in [n][2][512] real (channels a, b), out [n][2][257].  balance: pair_balance_512 -> rfft512_pair -> pair_restore_512 as the
// 512-sample analysis chains them
__global__ __launch_bounds__(NT) void k_rfft512_pair(int balance, const float *in, float2 *out, int n)
{
    __shared__ __attribute__((aligned(16))) float2 smem[TW_WIN + WPB * FFT_SCRATCH + WPB * 2 * N512_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, idx = blockIdx.x * WPB + wave;
    fft_table_init(smem, nullptr, tid, NT);
    __syncthreads();
    if (idx >= n) return;
    const FftTw tw{smem};
    float2 *buf = smem + TW_WIN + wave * FFT_SCRATCH;
    float2 *specA = smem + TW_WIN + WPB * FFT_SCRATCH + (2 * wave) * N512_ROW, *specB = specA + N512_ROW;
    const float *a = in + (long long)idx * 1024, *b = a + 512;
    float2 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = make_float2(0.5f * a[lane + 64 * r], 0.5f * b[lane + 64 * r]);
    if (balance) {
        const PairBalance pb = pair_balance_512(v);
        rfft512_pair(v, buf, specA, specB, lane, tw);
        pair_restore_512(pb, specA, specB, lane);
    } else {
        rfft512_pair(v, buf, specA, specB, lane, tw);
    }
    for (int k = lane; k < N512_K; k += 64) {
        out[((long long)idx * 2) * N512_K + k] = specA[k];
        out[((long long)idx * 2 + 1) * N512_K + k] = specB[k];
    }
}

// in [n][2][257], out [n][2][512] real
__global__ __launch_bounds__(NT) void k_irfft512_pair(const float2 *in, float *out, int n)
{
    __shared__ __attribute__((aligned(16))) float2 smem[TW_WIN + WPB * FFT_SCRATCH + WPB * 2 * N512_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, idx = blockIdx.x * WPB + wave;
    fft_table_init(smem, nullptr, tid, NT);
    __syncthreads();
    if (idx >= n) return;
    const FftTw tw{smem};
    float2 *buf = smem + TW_WIN + wave * FFT_SCRATCH;
    float2 *Ya = smem + TW_WIN + WPB * FFT_SCRATCH + (2 * wave) * N512_ROW, *Yb = Ya + N512_ROW;
    for (int k = lane; k < N512_K; k += 64) {
        Ya[k] = in[((long long)idx * 2) * N512_K + k];
        Yb[k] = in[((long long)idx * 2 + 1) * N512_K + k];
    }
    wave_lds_fence();
    float2 v[8];
    irfft512_pair(Ya, Yb, buf, v, lane, tw);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int m = lane + 64 * br3(i);
        out[(long long)idx * 1024 + m] = v[i].x;
        out[(long long)idx * 1024 + 512 + m] = v[i].y;
    }
}

// ---- 2048 / 4096-sample frames: R sub-sequences x[R n + r], two per wave, then one butterfly per m ------------------------------
// in [n][512 R] real, out [n][256 R + 1]; a workgroup holds 8 / R frames
template <int R>
__global__ __launch_bounds__(NT) void k_rfft_sub(const float2 *in, const float2 *twN, float2 *out, int n)
{
    constexpr int H = 256 * R, K = H + 1, XR = H + 2, FPB = 8 / R;
    __shared__ __attribute__((aligned(16))) float2 smem[TW_WIN + WPB * FFT_SCRATCH + 8 * N512_ROW + FPB * XR];
    float2 *sub = smem + TW_WIN + WPB * FFT_SCRATCH, *X = sub + 8 * N512_ROW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = wave / (R / 2), pr = wave % (R / 2), idx = blockIdx.x * FPB + slot;
    fft_table_init(smem, nullptr, tid, NT);
    __syncthreads();
    const FftTw tw{smem};
    if (idx < n) {
        const float2 *src = in + (long long)idx * H;
        float2 v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float2 x = src[(R / 2) * (lane + 64 * r) + pr];            // x[R m + 2 pr], x[R m + 2 pr + 1]
            v[r] = make_float2(0.5f * x.x, 0.5f * x.y);
        }
        float2 *S = sub + (slot * R + 2 * pr) * N512_ROW;
        rfft512_pair(v, smem + TW_WIN + wave * FFT_SCRATCH, S, S + N512_ROW, lane, tw);
    }
    __syncthreads();
    for (int e = tid; e < FPB * 512; e += NT) {
        const int j = e >> 9, m = e & 511;
        if (blockIdx.x * FPB + j >= n) continue;
        if constexpr (R == 8) combine4096_m(sub + j * R * N512_ROW, m, twN, X + j * XR);
        else combine2048_m(sub + j * R * N512_ROW, m, twN, X + j * XR);
    }
    __syncthreads();
    for (int e = tid; e < FPB * K; e += NT) {
        const int j = e / K, k = e - j * K;
        if (blockIdx.x * FPB + j < n) out[(long long)(blockIdx.x * FPB + j) * K + k] = X[j * XR + k];
    }
}

// in [n][1025], out [n][2048] real: split2048_inv -> irfft512_pair; a workgroup holds 2 frames
__global__ __launch_bounds__(NT) void k_irfft2048(const float2 *in, const float2 *tw2048, float2 *out, int n)
{
    constexpr int K = 1025, XR = 1026;
    __shared__ __attribute__((aligned(16))) float2 smem[TW_WIN + WPB * FFT_SCRATCH + 8 * N512_ROW + 2 * XR];
    float2 *sub = smem + TW_WIN + WPB * FFT_SCRATCH, *Y = sub + 8 * N512_ROW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = wave >> 1, pr = wave & 1, idx = blockIdx.x * 2 + slot;
    fft_table_init(smem, nullptr, tid, NT);
    for (int e = tid; e < 2 * K; e += NT) {
        const int j = e / K, k = e - j * K;
        if (blockIdx.x * 2 + j < n) Y[j * XR + k] = in[(long long)(blockIdx.x * 2 + j) * K + k];
    }
    __syncthreads();
    for (int e = tid; e < 2 * N512_K; e += NT) {
        const int j = e / N512_K, m = e - j * N512_K;
        if (blockIdx.x * 2 + j >= n) continue;
        float2 o4[4];
        split2048_inv(Y + j * XR, m, tw2048, o4);
#pragma unroll
        for (int r = 0; r < 4; ++r) sub[(j * 4 + r) * N512_ROW + m] = o4[r];
    }
    __syncthreads();
    if (idx >= n) return;
    const FftTw tw{smem};
    const float2 *Ya = sub + (slot * 4 + 2 * pr) * N512_ROW;
    float2 v[8];
    irfft512_pair(Ya, Ya + N512_ROW, smem + TW_WIN + wave * FFT_SCRATCH, v, lane, tw);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[(long long)idx * 1024 + 2 * (lane + 64 * br3(i)) + pr] = v[i];   // y[4 m + 2 pr], y[4 m + 2 pr + 1]
}

// ---- fft1024c.h -------------------------------------------------------------------------------------------------------------------
// in [n][1024], out [n][1024] natural order.  perm: row = lam (lam = l for l <= 32, 96 - l above), the permutation of the analysis kernels
template <bool INV, int OPT>
__global__ __launch_bounds__(NT) void k_fft1024c(int perm, const float2 *in, float2 *out, int n)
{
    __shared__ __attribute__((aligned(16))) float2 smem[F1K_TWORDS + WPB * F1K_SCRATCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, idx = blockIdx.x * WPB + wave;
    f1k_table_init(smem, tid, NT);
    __syncthreads();
    if (idx >= n) return;
    F1kLane lc;
    lc.init(lane);
    if (OPT & 4) lc.load_t1(smem, lane);
    float2 v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = in[(long long)idx * 1024 + lane + 64 * i];
    const int lam = lane <= 32 ? lane : 96 - lane;
    fft1024c<INV, OPT>(v, smem + F1K_TWORDS + wave * F1K_SCRATCH, lane, smem, lc, F1kNoMid(), perm ? lam : -1);
    const int res = perm ? lam : lane;
#pragma unroll
    for (int p = 0; p < 16; ++p) out[(long long)idx * 1024 + res + 64 * dr16(p)] = v[p];
}

// ---- fft_block.h: workgroup = frame of nch channels ---------------------------------------------------------------------------------
constexpr int BLK_MAXH = 2048, BLK_MAXCH = 3;

// in [n][nch][2 H] real, window [2 H], out [n][nch][H + 1]: load_frames -> block_fft_dit -> split_forward
__global__ __launch_bounds__(NT) void k_block_rfft(int logH, int nch, const float *in, const float *window, const float2 *tw, float2 *out)
{
    __shared__ __attribute__((aligned(16))) float2 z[BLK_MAXCH * (BLK_MAXH + 1)];
    const int H = 1 << logH, N = 2 * H, zs = H + 1, tid = threadIdx.x;
    load_frames(z, zs, nch, logH, in + (long long)blockIdx.x * nch * N, N, 0, window, tid, NT);
    block_fft_dit(z, zs, nch, logH, tw, N, tid, NT);
    split_forward(z, zs, nch, logH, tw, tid, NT);
    for (int e = tid; e < nch * zs; e += NT) out[(long long)blockIdx.x * nch * zs + e] = z[e];
}

// in [n][nch][H] natural order, out [n][nch][H] as block_ifft_dif leaves it (bit-reversed)
__global__ __launch_bounds__(NT) void k_block_ifft(int logH, int nch, const float2 *in, const float2 *tw, float2 *out)
{
    __shared__ __attribute__((aligned(16))) float2 z[BLK_MAXCH * (BLK_MAXH + 1)];
    const int H = 1 << logH, N = 2 * H, zs = H + 1, tid = threadIdx.x;
    for (int e = tid; e < nch * H; e += NT) z[(e >> logH) * zs + (e & (H - 1))] = in[(long long)blockIdx.x * nch * H + e];
    __syncthreads();
    block_ifft_dif(z, zs, nch, logH, tw, N, tid, NT);
    for (int e = tid; e < nch * H; e += NT) out[(long long)blockIdx.x * nch * H + e] = z[(e >> logH) * zs + (e & (H - 1))];
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
struct DBuf {
    void *p = nullptr;
    ~DBuf() { if (p) (void)hipFree(p); }
    hipError_t up(const void *host, size_t bytes)
    {
        hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
        if (e == hipSuccess && bytes && host) e = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
        return e;
    }
    hipError_t zeros(size_t bytes)
    {
        hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
        if (e == hipSuccess && bytes) e = hipMemset(p, 0, bytes);
        return e;
    }
};

// exp(-j 2 pi i / N), i < N / 2: double precision, rounded to float (d_tw of csrc/api.hip)
std::vector<float2> host_tw(int N)
{
    std::vector<float2> t((size_t)N / 2);
    for (int i = 0; i < N / 2; ++i) t[(size_t)i] = make_float2((float)std::cos(2.0 * M_PI * i / N), (float)(-std::sin(2.0 * M_PI * i / N)));
    return t;
}

// allocate, copy, launch, synchronise, copy back, free
template <class Launch>
int run(const void *in, size_t in_bytes, void *out, size_t out_bytes, const void *aux, size_t aux_bytes, Launch launch)
{
    if (out_bytes == 0) return (int)hipSuccess;
    DBuf din, dout, daux;
    hipError_t e;
    if ((e = din.up(in, in_bytes)) != hipSuccess) return (int)e;
    if ((e = dout.zeros(out_bytes)) != hipSuccess) return (int)e;
    if ((e = daux.up(aux, aux_bytes)) != hipSuccess) return (int)e;
    launch(din.p, dout.p, daux.p);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = hipDeviceSynchronize()) != hipSuccess) return (int)e;
    return (int)hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost);
}

inline unsigned blocks(int n, int per) { return (unsigned)((n + per - 1) / per); }
constexpr int ERR_ARG = (int)hipErrorInvalidValue;

}  // namespace

#define XH_LAUNCH(kernel, grid, ...) hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), 0, 0, __VA_ARGS__)

extern "C" {

// op: 0 cmul 1 cmulc 2 cmac 3 cmacc 4 cnmac 5 cnmacc 6 csub_jb 7 cadd_jb 8 cscale(a, b.x) 9 cmul_mj 10 cmul_pj
int xh_carith(int op, const float *in, float *out, int n)
{
    if (op < 0 || op > 10 || n < 0) return ERR_ARG;
    return run(in, (size_t)n * 24, out, (size_t)n * 8, nullptr, 0, [&](void *i, void *o, void *) {
        XH_LAUNCH(k_carith, blocks(n, NT), op, (const float2 *)i, (float2 *)o, n);
    });
}

// points: 4 (bfly4), 8 (fft8), 16 (fft16)
int xh_small_dft(int points, int inv, const float *in, float *out, int n)
{
    if ((points != 4 && points != 8 && points != 16) || n < 0) return ERR_ARG;
    const size_t bytes = (size_t)n * points * 8;
    return run(in, bytes, out, bytes, nullptr, 0, [&](void *i, void *o, void *) {
        const float2 *pi = (const float2 *)i; float2 *po = (float2 *)o; const unsigned g = blocks(n, NT);
        if (points == 4) { if (inv) XH_LAUNCH((k_small_dft<4, true>), g, pi, po, n); else XH_LAUNCH((k_small_dft<4, false>), g, pi, po, n); }
        else if (points == 8) { if (inv) XH_LAUNCH((k_small_dft<8, true>), g, pi, po, n); else XH_LAUNCH((k_small_dft<8, false>), g, pi, po, n); }
        else { if (inv) XH_LAUNCH((k_small_dft<16, true>), g, pi, po, n); else XH_LAUNCH((k_small_dft<16, false>), g, pi, po, n); }
    });
}

// in [n][3]; three != 0: max3abs of the three, else max2abs of the first two
int xh_maxabs(int three, const float *in, float *out, int n)
{
    if (n < 0) return ERR_ARG;
    return run(in, (size_t)n * 12, out, (size_t)n * 4, nullptr, 0, [&](void *i, void *o, void *) {
        XH_LAUNCH(k_maxabs, blocks(n, NT), three, (const float *)i, (float *)o, n);
    });
}

int xh_wave_max64_2(const float *in, float *out, int n)
{
    if (n < 0) return ERR_ARG;
    return run(in, (size_t)n * 512, out, (size_t)n * 512, nullptr, 0, [&](void *i, void *o, void *) {
        XH_LAUNCH(k_wave_max64_2, blocks(n, WPB), (const float *)i, (float *)o, n);
    });
}

int xh_pair_balance(const float *in, int *out, int n)
{
    if (n < 0) return ERR_ARG;
    return run(in, (size_t)n * 512, out, (size_t)n * 16, nullptr, 0, [&](void *i, void *o, void *) {
        XH_LAUNCH(k_pair_balance, blocks(n, WPB), (const float *)i, (int *)o, n);
    });
}

// which: see k_tables; window: 1024 floats for which == 1; out: xh_table_words(which) complex words
int xh_table_words(int which) { return which == 0 ? TW_WIN : which == 1 ? TW_WORDS : which == 2 ? F1K_TWORDS : which == 3 ? 192 : 0; }
int xh_tables(int which, const float *window, float *out)
{
    if (which < 0 || which > 3 || (which == 1 && !window)) return ERR_ARG;
    return run(window, which == 1 ? 4096 : 0, out, (size_t)xh_table_words(which) * 8, nullptr, 0, [&](void *w, void *o, void *) {
        XH_LAUNCH(k_tables, 1, which, (const float *)w, (float2 *)o);
    });
}

// variant: 0 forward, 1 forward AHEAD, 2 inverse
int xh_cfft512(int variant, const float *in, float *out, int n)
{
    if (variant < 0 || variant > 2 || n < 0) return ERR_ARG;
    return run(in, (size_t)n * 4096, out, (size_t)n * 4096, nullptr, 0, [&](void *i, void *o, void *) {
        const float2 *pi = (const float2 *)i; float2 *po = (float2 *)o; const unsigned g = blocks(n, WPB);
        if (variant == 0) XH_LAUNCH((k_cfft512<false, false>), g, pi, po, n);
        else if (variant == 1) XH_LAUNCH((k_cfft512<false, true>), g, pi, po, n);
        else XH_LAUNCH((k_cfft512<true, false>), g, pi, po, n);
    });
}

int xh_rfft1024(int ahead, const float *in, float *out, int n)
{
    if (n < 0) return ERR_ARG;
    return run(in, (size_t)n * 4096, out, (size_t)n * FFT_K * 8, nullptr, 0, [&](void *i, void *o, void *) {
        if (ahead) XH_LAUNCH(k_rfft1024<true>, blocks(n, WPB), (const float2 *)i, (float2 *)o, n);
        else XH_LAUNCH(k_rfft1024<false>, blocks(n, WPB), (const float2 *)i, (float2 *)o, n);
    });
}

int xh_irfft1024(const float *in, float *out, int n)
{
    if (n < 0) return ERR_ARG;
    return run(in, (size_t)n * FFT_K * 8, out, (size_t)n * 4096, nullptr, 0, [&](void *i, void *o, void *) {
        XH_LAUNCH(k_irfft1024, blocks(n, WPB), (const float2 *)i, (float2 *)o, n);
    });
}

int xh_rfft512_pair(int balance, const float *in, float *out, int n)
{
    if (n < 0) return ERR_ARG;
    return run(in, (size_t)n * 4096, out, (size_t)n * 2 * N512_K * 8, nullptr, 0, [&](void *i, void *o, void *) {
        XH_LAUNCH(k_rfft512_pair, blocks(n, WPB), balance, (const float *)i, (float2 *)o, n);
    });
}

int xh_irfft512_pair(const float *in, float *out, int n)
{
    if (n < 0) return ERR_ARG;
    return run(in, (size_t)n * 2 * N512_K * 8, out, (size_t)n * 4096, nullptr, 0, [&](void *i, void *o, void *) {
        XH_LAUNCH(k_irfft512_pair, blocks(n, WPB), (const float2 *)i, (float *)o, n);
    });
}

// N: 2048 or 4096
int xh_rfft_sub(int N, const float *in, float *out, int n)
{
    if ((N != 2048 && N != 4096) || n < 0) return ERR_ARG;
    const std::vector<float2> tw = host_tw(N);
    return run(in, (size_t)n * N * 4, out, (size_t)n * (N / 2 + 1) * 8, tw.data(), tw.size() * 8, [&](void *i, void *o, void *t) {
        if (N == 2048) XH_LAUNCH(k_rfft_sub<4>, blocks(n, 2), (const float2 *)i, (const float2 *)t, (float2 *)o, n);
        else XH_LAUNCH(k_rfft_sub<8>, blocks(n, 1), (const float2 *)i, (const float2 *)t, (float2 *)o, n);
    });
}

int xh_irfft2048(const float *in, float *out, int n)
{
    if (n < 0) return ERR_ARG;
    const std::vector<float2> tw = host_tw(2048);
    return run(in, (size_t)n * 1025 * 8, out, (size_t)n * 2048 * 4, tw.data(), tw.size() * 8, [&](void *i, void *o, void *t) {
        XH_LAUNCH(k_irfft2048, blocks(n, 2), (const float2 *)i, (const float2 *)t, (float2 *)o, n);
    });
}

// opt: 3 or 7
int xh_fft1024c(int inv, int opt, int perm, const float *in, float *out, int n)
{
    if ((opt != 3 && opt != 7) || n < 0) return ERR_ARG;
    return run(in, (size_t)n * 8192, out, (size_t)n * 8192, nullptr, 0, [&](void *i, void *o, void *) {
        const float2 *pi = (const float2 *)i; float2 *po = (float2 *)o; const unsigned g = blocks(n, WPB);
        if (!inv && opt == 3) XH_LAUNCH((k_fft1024c<false, 3>), g, perm, pi, po, n);
        else if (!inv) XH_LAUNCH((k_fft1024c<false, 7>), g, perm, pi, po, n);
        else if (opt == 3) XH_LAUNCH((k_fft1024c<true, 3>), g, perm, pi, po, n);
        else XH_LAUNCH((k_fft1024c<true, 7>), g, perm, pi, po, n);
    });
}

// in [n][nch][2 H] real, window [2 H], out [n][nch][H + 1]
int xh_block_rfft(int logH, int nch, const float *in, const float *window, float *out, int n)
{
    if (logH < 2 || logH > 11 || nch < 1 || nch > BLK_MAXCH || n < 0 || !window) return ERR_ARG;
    if (n == 0) return (int)hipSuccess;
    const int H = 1 << logH, N = 2 * H;
    const std::vector<float2> tw = host_tw(N);
    DBuf dwin;
    hipError_t e = dwin.up(window, (size_t)N * 4);
    if (e != hipSuccess) return (int)e;
    return run(in, (size_t)n * nch * N * 4, out, (size_t)n * nch * (H + 1) * 8, tw.data(), tw.size() * 8, [&](void *i, void *o, void *t) {
        XH_LAUNCH(k_block_rfft, (unsigned)n, logH, nch, (const float *)i, (const float *)dwin.p, (const float2 *)t, (float2 *)o);
    });
}

// in [n][nch][H] natural order, out [n][nch][H] in the bit-reversed order block_ifft_dif leaves
int xh_block_ifft(int logH, int nch, const float *in, float *out, int n)
{
    if (logH < 2 || logH > 11 || nch < 1 || nch > BLK_MAXCH || n < 0) return ERR_ARG;
    if (n == 0) return (int)hipSuccess;
    const int H = 1 << logH;
    const std::vector<float2> tw = host_tw(2 * H);
    return run(in, (size_t)n * nch * H * 8, out, (size_t)n * nch * H * 8, tw.data(), tw.size() * 8, [&](void *i, void *o, void *t) {
        XH_LAUNCH(k_block_ifft, (unsigned)n, logH, nch, (const float2 *)i, (const float2 *)t, (float2 *)o);
    });
}

}  // extern "C"
