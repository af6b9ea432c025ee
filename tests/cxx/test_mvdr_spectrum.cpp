// mca::MvdrBeamformer::configureSpectrum / spectrumGrid / spectrum / peaks on the 16-microphone line array (0.02 m pitch), and their
// exceptions.  The grid, the spectrum and the peaks go to a file that tests/test_gpu_mvdr_spectrum.py compares, bit for bit, with
// the Python class's results on the same input.
//   test_mvdr_spectrum pcm.f32 out.f32 fs N D binLo binHi P   (pcm.f32: [16][L] float; out.f32: grid [D], spectrum [D], doa [P], value [P])
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mcarray/micarray.h"

using namespace mca;

template <class Fn>
static bool throws(Fn f)
{
    try { f(); } catch (const MCArrayException &) { return true; }
    return false;
}

int main(int argc, char **argv)
{
    if (argc != 9) { std::fprintf(stderr, "usage: %s pcm.f32 out.f32 fs N D binLo binHi P\n", argv[0]); return 2; }
    const int fs = std::atoi(argv[3]), N = std::atoi(argv[4]), D = std::atoi(argv[5]), lo = std::atoi(argv[6]), hi = std::atoi(argv[7]),
              P = std::atoi(argv[8]), M = 16;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::fseek(f, 0, SEEK_END);
    const long L = std::ftell(f) / static_cast<long>(sizeof(float)) / M;
    std::fseek(f, 0, SEEK_SET);
    std::vector<float> pcm(static_cast<size_t>(L) * static_cast<size_t>(M));
    if (std::fread(pcm.data(), sizeof(float), pcm.size(), f) != pcm.size()) { std::fprintf(stderr, "short read\n"); return 2; }
    std::fclose(f);
    int failures = 0;
    try {
        std::vector<double> xs(static_cast<size_t>(M));
        for (int m = 0; m < M; ++m) xs[static_cast<size_t>(m)] = 0.02 * m;
        MvdrBeamformer bf(fs, ArrayDescription::make_linear_array_description(xs), N);
        std::vector<double> grid, spec, doa, val;
        // nothing is configured yet
        if (!throws([&] { bf.spectrum(spec); })) { std::printf("FAIL: spectrum() before configureSpectrum() accepted\n"); ++failures; }
        if (!throws([&] { bf.peaks(doa, val); })) { std::printf("FAIL: peaks() before configureSpectrum() accepted\n"); ++failures; }
        if (!throws([&] { bf.spectrumGrid(); })) { std::printf("FAIL: spectrumGrid() before configureSpectrum() accepted\n"); ++failures; }
        // a fresh stream: the zero row, no peak
        bf.configureSpectrum(D, lo, hi, MCA_HIP_MVDR_SPECTRUM_NORMALISED, P);
        bf.spectrum(spec);
        bf.peaks(doa, val);
        for (int i = 0; i < D; ++i)
            if (spec[static_cast<size_t>(i)] != 0.0) { std::printf("FAIL: a fresh stream has spectrum[%d] = %g\n", i, spec[static_cast<size_t>(i)]); ++failures; break; }
        for (int r = 0; r < P; ++r)
            if (doa[static_cast<size_t>(r)] != 0.0 || val[static_cast<size_t>(r)] != 0.0) { std::printf("FAIL: a fresh stream has a peak in slot %d\n", r); ++failures; }
        // one chunk of audio towards 0 rad
        std::vector<float *> in(static_cast<size_t>(M));
        for (int m = 0; m < M; ++m) in[static_cast<size_t>(m)] = pcm.data() + static_cast<size_t>(m) * static_cast<size_t>(L);
        std::vector<float> out(static_cast<size_t>(L));
        bf.setDOA(0.0);
        const int written = bf.process(in, static_cast<int>(L), out.data(), static_cast<int>(L));
        if (written != (static_cast<int>(L) / (N / 2) - 1) * (N / 2)) { std::printf("FAIL: %d samples written\n", written); ++failures; }
        // refused configurations leave the one set before
        if (!throws([&] { bf.configureSpectrum(1, lo, hi); })) { std::printf("FAIL: 1 angle accepted\n"); ++failures; }
        if (!throws([&] { bf.configureSpectrum(362, lo, hi); })) { std::printf("FAIL: 362 angles accepted\n"); ++failures; }
        if (!throws([&] { bf.configureSpectrum(D, hi + 1, hi); })) { std::printf("FAIL: binLo > binHi accepted\n"); ++failures; }
        if (!throws([&] { bf.configureSpectrum(D, lo, N / 2 + 1); })) { std::printf("FAIL: binHi > N/2 accepted\n"); ++failures; }
        if (!throws([&] { bf.configureSpectrum(D, lo, hi, 2); })) { std::printf("FAIL: weighting 2 accepted\n"); ++failures; }
        if (!throws([&] { bf.configureSpectrum(D, lo, hi, MCA_HIP_MVDR_SPECTRUM_POWER, 5); })) { std::printf("FAIL: 5 peaks accepted\n"); ++failures; }
        grid = bf.spectrumGrid();
        bf.spectrum(spec);
        bf.peaks(doa, val);
        if (static_cast<int>(grid.size()) != D || static_cast<int>(spec.size()) != D || static_cast<int>(doa.size()) != P || static_cast<int>(val.size()) != P) {
            std::printf("FAIL: sizes %zu %zu %zu %zu\n", grid.size(), spec.size(), doa.size(), val.size()); ++failures;
        }
        const double PI = 3.14159265358979323846;
        if (std::fabs(grid.front() + PI / 2) > 1e-6 || std::fabs(grid.back() - PI / 2) > 1e-6) { std::printf("FAIL: the grid runs from %g to %g\n", grid.front(), grid.back()); ++failures; }
        // the first peak is the row's maximum, at its grid point; the values descend
        int imax = 0;
        for (int i = 1; i < D; ++i) if (spec[static_cast<size_t>(i)] > spec[static_cast<size_t>(imax)]) imax = i;
        if (!(spec[static_cast<size_t>(imax)] > 0.0) || val[0] != spec[static_cast<size_t>(imax)] || doa[0] != grid[static_cast<size_t>(imax)]) {
            std::printf("FAIL: slot 0 is (%g, %g), the maximum (%g, %g)\n", doa[0], val[0], grid[static_cast<size_t>(imax)], spec[static_cast<size_t>(imax)]); ++failures;
        }
        for (int r = 1; r < P; ++r)
            if (val[static_cast<size_t>(r)] > val[static_cast<size_t>(r - 1)]) { std::printf("FAIL: the peak values do not descend at slot %d\n", r); ++failures; }
        for (int r = 0; r < P; ++r) std::printf("peak %d: %.3f degrees, %g\n", r, doa[static_cast<size_t>(r)] * 180.0 / PI, val[static_cast<size_t>(r)]);
        // the peaks as the look directions of the next chunk
        if (P >= 2) {
            bf.setMaxSources(2);
            bf.setDOAs(std::vector<double>(doa.begin(), doa.begin() + 2));
        }
        f = std::fopen(argv[2], "wb");
        if (!f) { std::perror(argv[2]); return 2; }
        const std::vector<double> *parts[4] = {&grid, &spec, &doa, &val};
        for (int p = 0; p < 4; ++p) {
            std::vector<float> v(parts[p]->begin(), parts[p]->end());
            std::fwrite(v.data(), sizeof(float), v.size(), f);
        }
        std::fclose(f);
    } catch (const MCArrayException &e) {
        std::printf("FAIL: exception: %s\n", e.what());
        ++failures;
    }
    std::printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
