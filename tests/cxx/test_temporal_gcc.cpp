// TemporalGCCBinauralLocalisation end to end through the C++ module API: the reference's testBinauralLocalisation
// (test/test_mcarray.cpp:305-339) on five two-channel int16 recordings at 44.1 kHz, d = 0.086 m.  Built and run by
// tests/test_gpu_temporal_gcc.py, which writes the recordings.
//
//   test_temporal_gcc <dir>
//   in:  dir/<name>.raw  interleaved int16, 2 channels, for name in right90 right45 front left45 left90
//
// Per file: process(SignalVector16s) in 4096-sample chunks; every setDOA must lie in the reference's accepted range and
// there must be at least 40 of them.  A second object fed the same frames as doubles through processParametrisation must
// fire as many callbacks, with DOAs within 1e-4 degrees (the stream path's values pass through float).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "mcarray/BinauralLocalisation.h"

using namespace mca;

namespace {

int failures = 0;
#define EXPECT(cond)                                                                             \
    do {                                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

struct RangeCallback : LocalisationCallback {
    double lo, hi;
    std::vector<double> doas;
    int out_of_range = 0;
    RangeCallback(double l, double h) : lo(l), hi(h) {}
    void setDOA(SignalPtr doa, SignalPtr prob, double power, int numOfSources) override
    {
        (void)prob; (void)power;
        if (numOfSources != 1) ++failures;
        doas.push_back(doa[0]);
        if (doa[0] < lo || doa[0] > hi) {
            ++out_of_range;
            std::printf("  DOA %.4f outside [%g, %g]\n", doa[0], lo, hi);
        }
    }
};

std::vector<short> read_raw(const std::string &path)
{
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { std::printf("cannot read %s\n", path.c_str()); std::exit(2); }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<short> v(static_cast<size_t>(bytes) / sizeof(short));
    if (std::fread(v.data(), sizeof(short), v.size(), f) != v.size()) { std::printf("short read %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
    return v;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) { std::printf("usage: %s <dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const char *names[5] = {"right90", "right45", "front", "left45", "left90"};
    const double ranges[5][2] = {{-90, -30}, {-90, 0}, {-20, 20}, {0, 90}, {30, 90}};   // test_mcarray.cpp:313-322
    const int sampleRate = 44100, chunk = 4096;
    const double microDistance = 0.086;

    ArrayDescription adesc;
    adesc.pushPosition(0, 0, 0);
    adesc.pushPosition(microDistance, 0, 0);

    for (int fi = 0; fi < 5; ++fi) {
        const std::vector<short> raw = read_raw(dir + "/" + names[fi] + ".raw");
        const int n = static_cast<int>(raw.size() / 2);

        TemporalGCCBinauralLocalisation tbl(sampleRate, adesc);
        RangeCallback cb(ranges[fi][0], ranges[fi][1]);
        tbl.setCallback(&cb);
        EXPECT(tbl.getWindowSize() == 6615 && tbl.getAnalysisLength() == 6615);
        for (int s0 = 0; s0 < n; s0 += chunk) {
            const int len = std::min(chunk, n - s0);
            SignalVector16s in;
            for (int c = 0; c < 2; ++c) {
                SignalPtr16s p(new BaseType16s[static_cast<size_t>(len)]);
                for (int i = 0; i < len; ++i) p[i] = raw[2 * static_cast<size_t>(s0 + i) + static_cast<size_t>(c)];
                in.push_back(p);
            }
            tbl.process(in, len);
        }
        std::printf("%s: %d callbacks in [%g, %g], %d outside\n", names[fi], static_cast<int>(cb.doas.size()), cb.lo, cb.hi, cb.out_of_range);
        EXPECT(cb.doas.size() >= 40);
        EXPECT(cb.out_of_range == 0);

        // the per-frame hook on the same frames, as doubles
        TemporalGCCBinauralLocalisation hook(sampleRate, adesc);
        RangeCallback cb2(ranges[fi][0], ranges[fi][1]);
        hook.setCallback(cb2);
        const int W = hook.getAnalysisLength(), hop = W / 2;
        std::vector<double> l(static_cast<size_t>(W)), r(static_cast<size_t>(W));
        std::vector<double *> frames = {l.data(), r.data()}, data;
        for (int f0 = 0; f0 + W <= n; f0 += hop) {
            for (int i = 0; i < W; ++i) {
                l[static_cast<size_t>(i)] = raw[2 * static_cast<size_t>(f0 + i)];
                r[static_cast<size_t>(i)] = raw[2 * static_cast<size_t>(f0 + i) + 1];
            }
            hook.processParametrisation(frames, W, data, 0);
        }
        EXPECT(cb2.doas.size() == cb.doas.size());
        double worst = 0;
        for (size_t i = 0; i < std::min(cb.doas.size(), cb2.doas.size()); ++i) worst = std::max(worst, std::fabs(cb.doas[i] - cb2.doas[i]));
        std::printf("%s: frame hook %d callbacks, max |DOA difference| %.3g deg\n", names[fi], static_cast<int>(cb2.doas.size()), worst);
        EXPECT(worst <= 1e-4);
    }
    if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
    std::printf("ALL PASSED\n");
    return 0;
}
