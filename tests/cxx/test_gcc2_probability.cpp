// FreqGCCBinauralLocalisation end to end through the C++ module API: setProbability at 500 particle angles through a
// SoundLocalisationImpl& (what SoundLocalisationObservationModel::getWeights does, SoundLocalisationParticleFilter.cpp:51),
// after process() on chunked PCM and after processParametrisation() on CCS frames.  Built and run by
// tests/test_gpu_gcc2_probability.py, which writes the inputs and compares the outputs with the restated reference.
//
//   test_gcc2_probability <dir> <n_samples> <n_frames>
//   in:  dir/pcm.bin  double [2][n_samples]      dir/ccs.bin  double [n_frames][2][N + 2]      dir/doas.bin double [500]
//   out: dir/probs_stream.bin, dir/probs_frame.bin double [500]; dir/callbacks.bin double [calls][3] (degrees, prob, power)
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
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

struct Recorder : LocalisationCallback {
    std::vector<double> rows;
    void setDOA(SignalPtr doa, SignalPtr prob, double power, int numOfSources) override
    {
        if (numOfSources != 1) ++failures;
        rows.push_back(doa[0]); rows.push_back(prob[0]); rows.push_back(power);
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
    if (argc != 4) { std::printf("usage: %s <dir> <n_samples> <n_frames>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const int n = std::atoi(argv[2]), F = std::atoi(argv[3]);
    const int fs = 16000, P = 500;
    ArrayDescription mics = ArrayDescription::make_linear_array_description(std::vector<double>{0.0, 0.086});
    std::vector<double> pcm = read_doubles(dir + "/pcm.bin", 2 * static_cast<size_t>(n));
    std::vector<double> doas = read_doubles(dir + "/doas.bin", P);

    // 1. process() in chunks of 1 000 samples, then setProbability on the stream state
    FreqGCCBinauralLocalisation stream(fs, mics, false);
    const int L = stream.getAnalysisLength();
    int frames = 0;
    for (int s0 = 0; s0 < n; s0 += 1000) {
        const int len = std::min(1000, n - s0);
        std::vector<double *> in = {pcm.data() + s0, pcm.data() + n + s0};
        frames += stream.process(in, len);
    }
    EXPECT(frames == F);
    std::vector<double> probs(P, -1.0);
    SoundLocalisationImpl &impl_s = stream;
    impl_s.setProbability(doas.data(), probs.data(), P);
    write_doubles(dir + "/probs_stream.bin", probs);

    // 2. processParametrisation with a callback, frame by frame
    std::vector<double> ccs = read_doubles(dir + "/ccs.bin", static_cast<size_t>(F) * 2 * L);
    std::vector<double *> none;
    FreqGCCBinauralLocalisation hook(fs, mics, false);
    Recorder rec;
    hook.setCallback(rec);
    SoundLocalisationImpl &impl_h = hook;
    impl_h.setProbability(doas.data(), probs.data(), P);                    // nothing has fired yet: zeros
    for (int i = 0; i < P; ++i) EXPECT(probs[static_cast<size_t>(i)] == 0.0);
    std::vector<double> copy(ccs);
    for (int t = 0; t < F; ++t) {
        std::vector<double *> fr = {copy.data() + static_cast<size_t>(t) * 2 * L, copy.data() + (static_cast<size_t>(t) * 2 + 1) * L};
        hook.processParametrisation(fr, L, none, 0);
    }
    EXPECT(rec.rows.size() == 3 * static_cast<size_t>(F));
    EXPECT(copy == ccs);                                                     // the frames are not modified
    impl_h.setProbability(doas.data(), probs.data(), P);
    write_doubles(dir + "/probs_frame.bin", probs);
    write_doubles(dir + "/callbacks.bin", rec.rows);

    // 3. no callback: nothing is computed (BinauralLocalisation.cpp:410-414), so the object does not advance
    FreqGCCBinauralLocalisation idle(fs, mics, false);
    for (int t = 0; t < F; ++t) {
        std::vector<double *> fr = {copy.data() + static_cast<size_t>(t) * 2 * L, copy.data() + (static_cast<size_t>(t) * 2 + 1) * L};
        idle.processParametrisation(fr, L, none, 0);
    }
    idle.setProbability(doas.data(), probs.data(), P);
    for (int i = 0; i < P; ++i) EXPECT(probs[static_cast<size_t>(i)] == 0.0);
    Recorder rec2;
    idle.setCallback(&rec2);
    std::vector<double *> fr0 = {copy.data(), copy.data() + L};
    idle.processParametrisation(fr0, L, none, 0);                              // acts as the first frame
    EXPECT(rec2.rows.size() == 3 && rec2.rows[0] == rec.rows[0] && rec2.rows[1] == rec.rows[1] && rec2.rows[2] == rec.rows[2]);
    bool threw = false;
    try { idle.processParametrisation(fr0, L - 2, none, 0); } catch (const MCArrayException &) { threw = true; }
    EXPECT(threw);

    std::printf(failures ? "FAILURES: %d\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
