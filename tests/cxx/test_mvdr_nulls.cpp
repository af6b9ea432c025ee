// mca::MvdrBeamformer with soft nulls at the other look directions: setMaxSources / setNullGain / setDOAs /
// process(in, n, {out_0, ..., out_S-1}, size) over chunks that are no multiple of the hop, with the gain changed once on the way.
// The outputs go to a file that tests/test_gpu_mvdr_nulls.py compares, bit for bit, with the Python class's output for the same calls.
//   test_mvdr_nulls pcm.f32 out.f32 fs N M S g0 g1   (pcm.f32: [M][L] float; out.f32: [S][F hop] float)
// prints "switch_frame K": frames 0 .. K-1 ran under the gain g0, the others under g1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mcarray/micarray.h"

using namespace mca;

static const double FIRST[4] = {0.35, -0.6, 1.1, -0.1};

int main(int argc, char **argv)
{
    if (argc != 9) { std::fprintf(stderr, "usage: %s pcm.f32 out.f32 fs N M S g0 g1\n", argv[0]); return 2; }
    const double g0 = std::atof(argv[7]), g1 = std::atof(argv[8]);
    const int fs = std::atoi(argv[3]), N = std::atoi(argv[4]), M = std::atoi(argv[5]), S = std::atoi(argv[6]), hop = N / 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::fseek(f, 0, SEEK_END);
    const long L = std::ftell(f) / static_cast<long>(sizeof(float)) / M;
    std::fseek(f, 0, SEEK_SET);
    std::vector<float> pcm(static_cast<size_t>(L) * static_cast<size_t>(M));
    if (std::fread(pcm.data(), sizeof(float), pcm.size(), f) != pcm.size()) { std::fprintf(stderr, "short read\n"); return 2; }
    std::fclose(f);
    const int F = static_cast<int>(L / hop) - 1;
    int failures = 0;
    try {
        std::vector<double> xs(static_cast<size_t>(M));
        for (int m = 0; m < M; ++m) xs[static_cast<size_t>(m)] = 0.035 * m;
        MvdrBeamformer bf(fs, ArrayDescription::make_linear_array_description(xs), N);
        if (bf.getNullGain() != 0.0) { std::printf("FAIL: the default gain is %g\n", bf.getNullGain()); ++failures; }
        bf.setMaxSources(S);
        bf.setNullGain(g0);
        // a gain outside [0, 1000] is refused and leaves the one set before
        const double bad[3] = {-1.0, 1001.0, std::nan("")};
        for (int i = 0; i < 3; ++i) {
            bool refused = false;
            try { bf.setNullGain(bad[i]); } catch (const MCArrayException &) { refused = true; }
            if (!refused) { std::printf("FAIL: setNullGain(%g) accepted\n", bad[i]); ++failures; }
        }
        if (bf.getNullGain() != g0) { std::printf("FAIL: getNullGain() gives %g after setNullGain(%g)\n", bf.getNullGain(), g0); ++failures; }
        bf.setDOAs(std::vector<double>(FIRST, FIRST + S));
        std::vector<std::vector<float> > out(static_cast<size_t>(S), std::vector<float>(static_cast<size_t>(F) * static_cast<size_t>(hop)));
        std::vector<float *> in(static_cast<size_t>(M)), o(static_cast<size_t>(S));
        const int chunk = 700;                              // no multiple of the hop
        int written = 0, switch_frame = -1;
        for (long pos = 0; pos < L; pos += chunk) {
            const int n = static_cast<int>(std::min<long>(chunk, L - pos));
            if (switch_frame < 0 && pos >= L / 2) {
                bf.setNullGain(g1);
                switch_frame = written / hop;
            }
            for (int m = 0; m < M; ++m) in[static_cast<size_t>(m)] = pcm.data() + static_cast<size_t>(m) * static_cast<size_t>(L) + pos;
            for (int s = 0; s < S; ++s) o[static_cast<size_t>(s)] = out[static_cast<size_t>(s)].data() + written;
            written += bf.process(in, n, o, F * hop - written);
        }
        if (written != F * hop) { std::printf("FAIL: %d samples written, %d expected\n", written, F * hop); ++failures; }
        std::printf("switch_frame %d\n", switch_frame);
        f = std::fopen(argv[2], "wb");
        if (!f) { std::perror(argv[2]); return 2; }
        for (int s = 0; s < S; ++s) std::fwrite(out[static_cast<size_t>(s)].data(), sizeof(float), out[static_cast<size_t>(s)].size(), f);
        std::fclose(f);
    } catch (const MCArrayException &e) {
        std::printf("FAIL: exception: %s\n", e.what());
        ++failures;
    }
    std::printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
