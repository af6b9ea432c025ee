// mca::BinauralMaskingImpl through the C++ class: process() with SignalVector16s on the reference's spatial-masking signal
// (test/test_mcarray.cpp:892-958; the caller checks the band-power windows on the output file), the three hooks once, and
// the two-channel rule.  usage: test_binaural_masking_impl <interleaved int16 stereo in> <interleaved int16 stereo out>
#include <cmath>
#include <cstdio>
#include <vector>

#include "mcarray/micarray.h"

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 3) { std::printf("usage: %s in.raw out.raw\n", argv[0]); return 2; }
    std::vector<short> raw;
    {
        std::FILE *f = std::fopen(argv[1], "rb");
        if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
        short buf[4096];
        size_t n;
        while ((n = std::fread(buf, sizeof(short), 4096, f)) > 0) raw.insert(raw.end(), buf, buf + n);
        std::fclose(f);
    }
    const int n = static_cast<int>(raw.size() / 2);

    mca::BinauralMaskingImpl masking(16000, 0.086, 500, 5000, mca::BinauralMaskingImpl::FULL);
    CHECK(masking.getWindowSize() == 1024);
    CHECK(masking.getFrameSize() == 512);
    CHECK(masking.getAnalysisLength() == 46 * 1024);
    CHECK(masking.getNumberOfChannels() == 2);
    CHECK(masking.getNonMaskingAngle() == 10);
    CHECK(std::fabs(masking.getMicroPhoneDistance() - 0.086f) < 1e-7f);
    CHECK(masking.getSpatialMaskingFactor() == 1.f && masking.getTemporalMaskingFactor() == 1.f);

    // process() as testSpatialMaskingCore calls it
    const int outSize = n + masking.getMaxLatency();
    mca::SignalVector16s in, out;
    for (int c = 0; c < 2; ++c) {
        in.push_back(mca::SignalPtr16s(new mca::BaseType16s[n]));
        out.push_back(mca::SignalPtr16s(new mca::BaseType16s[outSize]));
        for (int i = 0; i < n; ++i) in[c][i] = raw[2 * i + c];
    }
    const int done = masking.process(in, n, out, outSize);
    CHECK(done == (n / 512 - 1) * 512);
    {
        std::FILE *f = std::fopen(argv[2], "wb");
        if (!f) { std::printf("cannot open %s\n", argv[2]); return 2; }
        for (int i = 0; i < done; ++i) { const short s[2] = {out[0][i], out[1][i]}; std::fwrite(s, sizeof(short), 2, f); }
        std::fclose(f);
    }

    // the three hooks once: bands + residual give the frame back, the synthesis of 46 W sums the 45 bands
    const int W = masking.getWindowSize(), A = masking.getAnalysisLength();
    std::vector<double> frame[2], ana[2], y(W);
    for (int c = 0; c < 2; ++c) {
        frame[c].resize(W); ana[c].assign(A, 0.0);
        for (int i = 0; i < W; ++i) frame[c][i] = raw[2 * (i + 1024) + c] * (0.5 - 0.5 * std::cos(2.0 * M_PI * i / W));
        masking.frameAnalysis(frame[c].data(), ana[c].data(), W, A, c);
        double worst = 0, peak = 0;
        for (int i = 0; i < W; ++i) {
            double s = 0;
            for (int b = 0; b <= 45; ++b) s += ana[c][b * W + i];
            worst = std::fmax(worst, std::fabs(s - frame[c][i]));
            peak = std::fmax(peak, std::fabs(frame[c][i]));
        }
        CHECK(worst <= 1e-10 * peak);
    }
    std::vector<double> before(ana[0]);
    std::vector<double *> frames, data;
    frames.push_back(ana[0].data()); frames.push_back(ana[1].data());
    masking.processParametrisation(frames, A, data, 0);
    int scaled = 0;                                         // FULL: a masked band is its input / 1000
    for (int b = 0; b < 45; ++b) {
        double pb = 0, pa = 0;
        for (int i = 0; i < W; ++i) { pb += before[b * W + i] * before[b * W + i]; pa += ana[0][b * W + i] * ana[0][b * W + i]; }
        if (pb > 0 && std::fabs(pa / pb - 1e-6) < 1e-9) ++scaled;
        else CHECK(pa == pb);
    }
    CHECK(scaled > 0);                                      // the 4800 Hz interferer's bands are masked
    masking.frameSynthesis(y.data(), ana[0].data(), W, A, 0);
    {
        double worst = 0, peak = 0;
        for (int i = 0; i < W; ++i) {
            double s = 0;
            for (int b = 0; b < 45; ++b) s += ana[0][b * W + i];
            worst = std::fmax(worst, std::fabs(s - y[i]));
            peak = std::fmax(peak, std::fabs(y[i]));
        }
        CHECK(worst <= 1e-10 * peak);
    }

    // three channels are refused
    bool thrown = false;
    try {
        std::vector<double *> three(frames);
        three.push_back(ana[0].data());
        masking.processParametrisation(three, A, data, 0);
    } catch (const mca::MCArrayException &) { thrown = true; }
    CHECK(thrown);
    thrown = false;
    try { masking.frameAnalysis(frame[0].data(), ana[0].data(), W, A, 2); } catch (const mca::MCArrayException &) { thrown = true; }
    CHECK(thrown);

    std::printf(g_fail ? "%d CHECKS FAILED\n" : "ALL PASSED\n", g_fail);
    return g_fail ? 1 : 0;
}
