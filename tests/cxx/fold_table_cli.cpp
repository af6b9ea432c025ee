// fold_table_cli.cpp -- a stand-alone CPU program over csrc/fold_table.h (plain C++, no HIP) for tests/test_fold_table.py.
//   fold_table_cli <delays.f32> <D> <Dp> <G> <K> <out.bin>
// delays.f32: the D float delays (samples) of the unit spacing.  Prints "fold=<0|1> n_merged=<n> Kp=<Kp> c=<c>"; when the grid
// folds, out.bin receives the fp16 bits of the even table, the odd table ([Kp / 64][192][32] each) and the full-width planar table
// ([Dp][Kp]), in that order.
#include "fold_table.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc != 7) { std::fprintf(stderr, "usage: %s delays.f32 D Dp G K out.bin\n", argv[0]); return 2; }
    const int D = std::atoi(argv[2]), Dp = std::atoi(argv[3]), G = std::atoi(argv[4]), K = std::atoi(argv[5]);
    if (D < 1 || Dp < D || G < 1 || K < 2) { std::fprintf(stderr, "bad sizes\n"); return 2; }
    std::vector<float> delay((size_t)D);
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(delay.data(), sizeof(float), (size_t)D, f) != (size_t)D) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::fclose(f);
    std::vector<unsigned short> rank;
    std::vector<int> ms;
    mca::merged_products(G, K, rank, ms);
    const int n_merged = (int)ms.size(), Kp = 2 * ((n_merged + 63) & ~63), n_frame = 2 * (K - 1);
    const bool fold = mca::fold_applies(true, n_frame, n_frame, D, Dp, delay.data());
    std::printf("fold=%d n_merged=%d Kp=%d c=%d\n", fold ? 1 : 0, n_merged, Kp, (D - 1) / 2);
    if (!fold) return 0;
    mca::FoldTables t;
    mca::build_fold_tables(delay.data(), D, Dp, ms.data(), n_merged, Kp, n_frame, t);
    f = std::fopen(argv[6], "wb");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", argv[6]); return 2; }
    bool ok = std::fwrite(t.even.data(), 2, t.even.size(), f) == t.even.size() && std::fwrite(t.odd.data(), 2, t.odd.size(), f) == t.odd.size() &&
              std::fwrite(t.full.data(), 2, t.full.size(), f) == t.full.size();
    ok = std::fclose(f) == 0 && ok;
    return ok ? 0 : 2;
}
