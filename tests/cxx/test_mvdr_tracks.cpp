// mca::MvdrBeamformer: configureTracks() / seedTracks() / updateTracks() / tracks() / followTracks(), over chunks that are no multiple
// of the hop.  The loop is processAuto() with one protected talker, then updateTracks() per chunk:
//   - with followTracks(true) the outputs and the covariance are those of the loop that reads tracks() and hands them to setDOAs(),
//     byte for byte;
//   - the own track stays alive, the interferer's slot is born from the Capon peaks;
//   - the calls before configureTracks() throw, and so does a configuration the library refuses.
// The stream is synthetic (two tones from two directions plus a deterministic noise per channel); no input files.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mcarray/micarray.h"

using namespace mca;

namespace {

const int FS = 16000, N = 256, M = 6, HOP = N / 2, CHUNK = 300;      // CHUNK: no multiple of the hop
const int TOTAL = 14 * CHUNK;
const int S = 2;

ArrayDescription array()
{
    std::vector<double> xs(static_cast<size_t>(M));
    for (int m = 0; m < M; ++m) xs[static_cast<size_t>(m)] = 0.035 * m;
    return ArrayDescription::make_linear_array_description(xs);
}

std::vector<float> channel(int m, int n)
{
    std::vector<float> x(static_cast<size_t>(n));
    unsigned s = 12345u + 977u * static_cast<unsigned>(m);
    for (int i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        const double noise = (static_cast<double>(s >> 8) / 8388608.0 - 1.0) * 0.05;
        x[static_cast<size_t>(i)] = static_cast<float>(0.2 * std::sin(2.0 * M_PI * 440.0 * (i - 3 * m) / FS) + 0.1 * std::sin(2.0 * M_PI * 1900.0 * (i + 2 * m) / FS) + noise);
    }
    return x;
}

struct Run {
    std::vector<float> out;               // [S][samples written]
    std::vector<double> cov, doas;        // the covariance at the end; the tracks after every chunk
    std::vector<int> alive;
    int written = 0;
};

Run run(bool follow)
{
    std::vector<std::vector<float> > ch;
    for (int m = 0; m < M; ++m) ch.push_back(channel(m, TOTAL));
    MvdrBeamformer bf(FS, array(), N);
    bf.setMaxSources(S);
    bf.setRtf(true, 0.9, 2, 1);
    bf.setMaskEstimator(true, 2, -1, 0.3, 0.8, 1);
    bf.configureSpectrum(91, 4, 100, MCA_HIP_MVDR_SPECTRUM_NORMALISED, S);
    bf.configureTracks(S, 1, 0.1, 0.1, 2);
    std::vector<double> seed(static_cast<size_t>(S), std::nan(""));
    seed[0] = 0.3;
    bf.seedTracks(seed);
    bf.followTracks(follow);
    Run r;
    std::vector<std::vector<float> > out(static_cast<size_t>(S), std::vector<float>(static_cast<size_t>(TOTAL)));
    std::vector<float *> in(static_cast<size_t>(M)), o(static_cast<size_t>(S));
    for (int pos = 0; pos < TOTAL; pos += CHUNK) {
        for (int m = 0; m < M; ++m) in[static_cast<size_t>(m)] = ch[static_cast<size_t>(m)].data() + pos;
        for (int s = 0; s < S; ++s) o[static_cast<size_t>(s)] = out[static_cast<size_t>(s)].data() + r.written;
        std::vector<double> d;
        std::vector<int> alive;
        if (!follow) {
            bf.tracks(d, alive);
            bf.setDOAs(d);
        }
        r.written += bf.processAuto(in, CHUNK, o, TOTAL - r.written);
        bf.updateTracks();
        bf.tracks(d, alive);
        r.doas.insert(r.doas.end(), d.begin(), d.end());
        r.alive.insert(r.alive.end(), alive.begin(), alive.end());
    }
    bf.covariance(r.cov);
    for (int s = 0; s < S; ++s) r.out.insert(r.out.end(), out[static_cast<size_t>(s)].begin(), out[static_cast<size_t>(s)].begin() + r.written);
    return r;
}

template <typename T>
bool same(const std::vector<T> &a, const std::vector<T> &b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

}  // namespace

int main()
{
    int failures = 0;
    try {
        const Run f = run(true), h = run(false);
        if (!same(f.out, h.out) || !same(f.cov, h.cov)) { std::printf("FAIL: followTracks(true) differs from setDOAs(tracks())\n"); ++failures; }
        if (!same(f.doas, h.doas) || !same(f.alive, h.alive)) { std::printf("FAIL: the tracks of the two loops differ\n"); ++failures; }
        if (f.written < 20 * HOP) { std::printf("FAIL: %d samples written\n", f.written); ++failures; }
        bool own = true, finite = true;
        for (size_t c = 0; c < f.alive.size(); c += S) own = own && f.alive[c] == 1;
        for (float v : f.out) finite = finite && std::isfinite(v);
        if (!own) { std::printf("FAIL: the own track was released\n"); ++failures; }
        if (!finite) { std::printf("FAIL: an output sample is not finite\n"); ++failures; }
        if (f.alive[f.alive.size() - 1] != 1) { std::printf("FAIL: no interferer track was born from the Capon peaks\n"); ++failures; }
        std::printf("followTracks(true) == setDOAs(tracks()): %d samples; tracks at the end %.1f and %.1f degrees\n", f.written,
                    f.doas[f.doas.size() - 2] * 180.0 / M_PI, f.doas[f.doas.size() - 1] * 180.0 / M_PI);
        // before configureTracks(): refused; a configuration the library refuses throws
        MvdrBeamformer p(FS, array(), N);
        std::vector<double> d;
        std::vector<int> alive;
        int threw = 0;
        try { p.updateTracks(); } catch (const MCArrayException &) { ++threw; }
        try { p.tracks(d, alive); } catch (const MCArrayException &) { ++threw; }
        try { p.followTracks(true); } catch (const MCArrayException &) { ++threw; }
        try { p.seedTracks(std::vector<double>(1, 0.1)); } catch (const MCArrayException &) { ++threw; }
        try { p.configureTracks(1); } catch (const MCArrayException &) { ++threw; }                      // the spectrum first
        p.configureSpectrum(61, 1, 100);
        try { p.configureTracks(1, 1); } catch (const MCArrayException &) { ++threw; }                   // own tracks need setRtf(true)
        try { p.configureTracks(2); } catch (const MCArrayException &) { ++threw; }                      // more tracks than sources
        if (threw != 7) { std::printf("FAIL: %d of 7 refusals threw\n", threw); ++failures; }
        p.configureTracks(1);
        p.updateTracks();
        p.tracks(d, alive);
        if (d.size() != 1 || alive.size() != 1 || alive[0] != 0 || d[0] != 0.0) { std::printf("FAIL: the tracks of a silent stream\n"); ++failures; }
    } catch (const MCArrayException &e) {
        std::printf("FAIL: exception: %s\n", e.what());
        ++failures;
    }
    std::printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
