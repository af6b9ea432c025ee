// mca::MvdrBeamformer with several look directions per frame: setMaxSources / setDOAs / process(in, n, {out_0, ..., out_S-1}, size)
// over chunks that are no multiple of the hop, with the directions changed once on the way.  The outputs go to a file that
// tests/test_gpu_mvdr_sources.py compares, bit for bit, with the C-ABI call on the whole stream.
//   test_mvdr_sources pcm.f32 out.f32 fs N M S   (pcm.f32: [M][L] float; out.f32: [S][F hop] float)
// prints "switch_frame K": frames 0 .. K-1 were steered to the first set of directions, the others to the second.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mcarray/micarray.h"

using namespace mca;

static const double FIRST[4] = {0.35, -0.6, 1.1, -0.1}, SECOND[4] = {0.30, -0.7, 0.9, 0.2};

int main(int argc, char **argv)
{
    if (argc != 7) { std::fprintf(stderr, "usage: %s pcm.f32 out.f32 fs N M S\n", argv[0]); return 2; }
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
        // the multi-output form needs the maximum raised first
        bool refused = false;
        try { bf.setDOAs(std::vector<double>(FIRST, FIRST + 2)); } catch (const MCArrayException &) { refused = true; }
        if (!refused) { std::printf("FAIL: setDOAs with two directions accepted before setMaxSources\n"); ++failures; }
        refused = false;
        try { bf.setMaxSources(5); } catch (const MCArrayException &) { refused = true; }
        if (!refused) { std::printf("FAIL: setMaxSources(5) accepted\n"); ++failures; }
        bf.setMaxSources(S);
        bf.setDOAs(std::vector<double>(FIRST, FIRST + S));
        std::vector<std::vector<float> > out(static_cast<size_t>(S), std::vector<float>(static_cast<size_t>(F) * static_cast<size_t>(hop)));
        std::vector<float *> in(static_cast<size_t>(M)), o(static_cast<size_t>(S));
        const int chunk = 700;                              // no multiple of the hop
        int written = 0, switch_frame = -1;
        for (long pos = 0; pos < L; pos += chunk) {
            const int n = static_cast<int>(std::min<long>(chunk, L - pos));
            if (switch_frame < 0 && pos >= L / 2) {
                bf.setDOAs(std::vector<double>(SECOND, SECOND + S));
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
