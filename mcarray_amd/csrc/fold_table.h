// fold_table.h -- the mirror fold of the merged steering table (host side, plain C++: no HIP, so a CPU program can call it;
// tests/cxx/fold_table_cli.cpp does).
//
// The angle grid of a linear array is mirror-symmetric about broadside: with c = (D - 1) / 2 the delay of column c - j is minus
// that of column c + j.  With the merged PHAT sums S[m] = R[m] + j I[m] and the phase phi_j[m] = 2 pi m t_j / N
//
//     E(c +- j) = sum_m R[m] cos phi_j[m]  -+  sum_m I[m] sin phi_j[m]  =  Ec(j) -+ Es(j)
//
// (table rows cos, -sin as in build_merged_tables), so the D columns over 2 n reals are two products over n reals each: an "even"
// table cos phi_j against the R half of a row and an "odd" table -sin phi_j against its I half, 192 columns each
// (k_srp_gemm_f16_fold).  The symmetry holds up to the rounding of the reference's float chain (measured: 9.5e-7 samples, 2.1e-5
// rad at m = 3 584, the size of the approximation the merged index already makes); it is checked here, else no fold.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace mca {

constexpr int FOLD_DP = 384, FOLD_COLS = 192;      // the padded grid width that folds, column pairs per folded table
// |delay[c + j] + delay[c - j]| at most, in samples: four times the 9.5e-7 measured on the 361-angle grid of the reference's float
// chain (0.04 m, 48 kHz, 0.5 degrees)
constexpr double FOLD_MAX_ASYM = 4e-6;

// float -> IEEE binary16 bits, round to nearest even: what (_Float16)(float) gives on the device compiler
inline uint16_t f16_bits(float f)
{
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
    x &= 0x7fffffffu;
    if (x > 0x7f800000u) return sign | 0x7e00u;
    if (x >= 0x477ff000u) return sign | 0x7c00u;               // >= 65 520 rounds to infinity
    if (x < 0x38800000u) {                                      // below 2^-14: a binary16 subnormal (the float adder rounds it)
        float a;
        std::memcpy(&a, &x, 4);
        a += 0.5f;
        std::memcpy(&x, &a, 4);
        return sign | (uint16_t)(x - 0x3f000000u);
    }
    const uint32_t odd = (x >> 13) & 1u;
    x += ((uint32_t)(15 - 127) << 23) + 0xfffu + odd;
    return sign | (uint16_t)(x >> 13);
}

// The products m = k g (bin k < K, spacing g <= G) in rising order, and each product's rank among them (0xffff: not a product).
inline void merged_products(int G, int K, std::vector<unsigned short> &rank, std::vector<int> &ms)
{
    rank.assign((size_t)G * (K - 1) + 1, 0xffff);
    ms.clear();
    for (int g = 1; g <= G; ++g)
        for (int k = 0; k < K; ++k) rank[(size_t)k * g] = 0;
    for (size_t m = 0; m < rank.size(); ++m)
        if (rank[m] == 0) { rank[m] = (unsigned short)ms.size(); ms.push_back((int)m); }
}

// Does a merged context fold?  delay: the D delays (samples) of the unit spacing.  n_frame: its frame length, fft_n: the 1024 of the
// wave-level analysis (the merged kernel of 2048-sample frames keeps the interleaved rows).
inline bool fold_applies(bool merged, int n_frame, int fft_n, int D, int Dp, const float *delay)
{
    if (!merged || n_frame != fft_n || Dp != FOLD_DP || D < 3 || (D & 1) == 0) return false;
    const int c = (D - 1) / 2;
    if (c >= FOLD_COLS) return false;
    for (int j = 0; j <= c; ++j)
        if (!(std::fabs((double)delay[c + j] + (double)delay[c - j]) <= FOLD_MAX_ASYM)) return false;      // (j = 0: twice the centre's own delay)
    return true;
}

// The delay column pair j steers with: (delay[c + j] - delay[c - j]) / 2; j = 0 keeps the centre's own delay, so the entries of
// column c stay what the unfolded table holds, bit for bit.
inline double fold_delay(const float *delay, int c, int j) { return j == 0 ? (double)delay[c] : 0.5 * ((double)delay[c + j] - (double)delay[c - j]); }

struct FoldTables {
    int c = 0, half = 0;                 // centre column; reals per half row = Kp / 2
    std::vector<uint16_t> even, odd;     // [half / 32][192][32] fp16: cos phi_j[m] / -sin phi_j[m] for column c + j, zero from j > c, tiled per 32-deep stage
    std::vector<uint16_t> full;          // [Dp][Kp] fp16, planar K order (all cos rows, then all -sin rows): the same values at full width
    std::vector<uint16_t> full_tiled;    // [Kp / 32][Dp][32]: `full` tiled per stage like d_Btm
};

// ms: the n_merged products; Kp: the padded depth of a merged row (both halves, a multiple of 64); n_frame: 2 (K - 1)
inline void build_fold_tables(const float *delay, int D, int Dp, const int *ms, int n_merged, int Kp, int n_frame, FoldTables &t)
{
    const int c = (D - 1) / 2, half = Kp / 2, ns = half / 32;
    t.c = c; t.half = half;
    t.even.assign((size_t)ns * FOLD_COLS * 32, 0); t.odd.assign((size_t)ns * FOLD_COLS * 32, 0);
    t.full.assign((size_t)Dp * Kp, 0); t.full_tiled.assign((size_t)Dp * Kp, 0);
    for (int j = 0; j <= c; ++j) {
        const double tj = fold_delay(delay, c, j);
        for (int r = 0; r < n_merged; ++r) {
            const double ph = 2.0 * M_PI * (double)ms[r] * tj / (double)n_frame;
            const uint16_t cs = f16_bits((float)std::cos(ph)), sn = f16_bits((float)(-std::sin(ph)));
            const size_t e = ((size_t)(r >> 5) * FOLD_COLS + j) * 32 + (r & 31);
            t.even[e] = cs; t.odd[e] = sn;
            t.full[(size_t)(c + j) * Kp + r] = cs; t.full[(size_t)(c + j) * Kp + half + r] = sn;
            if (j > 0) { t.full[(size_t)(c - j) * Kp + r] = cs; t.full[(size_t)(c - j) * Kp + half + r] = (sn & 0x7fffu) ? (uint16_t)(sn ^ 0x8000u) : sn; }
        }
    }
    for (int sl = 0; sl < Kp / 32; ++sl)
        for (int d = 0; d < Dp; ++d)
            std::memcpy(&t.full_tiled[((size_t)sl * Dp + d) * 32], &t.full[(size_t)d * Kp + (size_t)sl * 32], 32 * sizeof(uint16_t));
}

}  // namespace mca
