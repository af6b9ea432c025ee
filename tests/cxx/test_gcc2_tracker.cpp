// FreqGCCBinauralLocalisation with useParticleFilter() end to end through the C++ module API: which frames fire the callback
// (voiced ones and the ones a track coasts through) and with what, through process() on chunked PCM and through
// processParametrisation() on CCS frames.  Built and run by tests/test_gpu_gcc2_tracker.py, which writes the inputs and compares
// the outputs with tests/gcc2_tracker_twin.py.
//
//   test_gcc2_tracker <dir> <n_samples> <n_frames> <seed>
//   in:  dir/pcm.bin  double [2][n_samples]      dir/ccs.bin  double [n_frames][2][N + 2]
//   out: dir/cb_stream.bin, dir/cb_hook.bin double [calls][4] (frame, degrees, prob, power);
//        dir/tracks_stream.bin, dir/tracks_hook.bin double [n_frames] getSourceCounter() after every frame
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "mcarray/BinauralLocalisation.h"

using namespace mca;

namespace {

int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

struct Recorder : LocalisationCallback {
    std::vector<double> rows;
    int frame = 0;
    void setDOA(SignalPtr doa, SignalPtr prob, double power, int numOfSources) override
    {
        if (numOfSources != 1) ++failures;
        rows.push_back(frame); rows.push_back(doa[0]); rows.push_back(prob[0]); rows.push_back(power);
    }
};

std::vector<double> read_doubles(const std::string &path, size_t n)
{
    std::vector<double> v(n);
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f || std::fread(v.data(), sizeof(double), n, f) != n) { std::printf("cannot read %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
    return v;
}

void write_doubles(const std::string &path, const std::vector<double> &v)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(double), v.size(), f) != v.size()) { std::printf("cannot write %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 5) { std::printf("usage: %s <dir> <n_samples> <n_frames> <seed>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const int n = std::atoi(argv[2]), F = std::atoi(argv[3]);
    const unsigned long long seed = std::strtoull(argv[4], nullptr, 10);
    const int fs = 16000;
    ArrayDescription mics = ArrayDescription::make_linear_array_description(std::vector<double>{0.0, 0.086});
    std::vector<double> pcm = read_doubles(dir + "/pcm.bin", 2 * static_cast<size_t>(n));

    // 1. process(), one hop per call: every call after the first completes exactly one frame
    FreqGCCBinauralLocalisation stream(fs, mics, true);
    EXPECT(!stream.usesParticleFilter() && stream.getSourceCounter() == 0);
    stream.useParticleFilter(seed);
    EXPECT(stream.usesParticleFilter());
    bool threw = false;
    try { stream.useParticleFilter(seed); } catch (const MCArrayException &) { threw = true; }      // once
    EXPECT(threw);
    Recorder rec;
    stream.setCallback(rec);
    const int L = stream.getAnalysisLength(), hop = stream.getFrameSize();
    std::vector<double> tracks;
    int frames = 0;
    for (int s0 = 0; s0 + hop <= n; s0 += hop) {
        std::vector<double *> in = {pcm.data() + s0, pcm.data() + n + s0};
        rec.frame = frames;
        const int done = stream.process(in, hop);
        EXPECT(done == (s0 == 0 ? 0 : 1));
        frames += done;
        if (done) tracks.push_back(stream.getSourceCounter());
    }
    EXPECT(frames == F);
    write_doubles(dir + "/cb_stream.bin", rec.rows);
    write_doubles(dir + "/tracks_stream.bin", tracks);

    // 2. processParametrisation, frame by frame
    std::vector<double> ccs = read_doubles(dir + "/ccs.bin", static_cast<size_t>(F) * 2 * L);
    std::vector<double *> none;
    FreqGCCBinauralLocalisation hook(fs, mics, true);
    hook.useParticleFilter(seed);
    Recorder rec_h;
    hook.setCallback(rec_h);
    tracks.clear();
    for (int t = 0; t < F; ++t) {
        std::vector<double *> fr = {ccs.data() + static_cast<size_t>(t) * 2 * L, ccs.data() + (static_cast<size_t>(t) * 2 + 1) * L};
        rec_h.frame = t;
        hook.processParametrisation(fr, L, none, 0);
        tracks.push_back(hook.getSourceCounter());
    }
    write_doubles(dir + "/cb_hook.bin", rec_h.rows);
    write_doubles(dir + "/tracks_hook.bin", tracks);

    std::printf(failures ? "FAILURES: %d\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
