// mca::MvdrBeamformer::setPostFilter: the decision-directed Wiener post-filter behind both process() overloads (one output / one
// output per look direction of setDOAs()), over chunks that are no multiple of the hop.
//   - setPostFilter(true, ..., gainFloor 1.0, ...) reproduces a run that never enabled it, byte for byte, audio and covariance;
//   - a filtered run (the defaults) lowers the power of an interferer that a noise-only covariance has learnt, and leaves the
//     covariance of the unfiltered run;
//   - getPostFilter round-trips, and a refused value leaves what was set.
// The stream is synthetic: a white interferer that reaches microphone m one sample later than microphone m - 1, plus a little
// independent noise per channel; the look direction is broadside.  No input files.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mcarray/micarray.h"

using namespace mca;

namespace {

const int FS = 16000, N = 256, M = 6, HOP = N / 2, CHUNK = 300;      // CHUNK: no multiple of the hop
const int LEAD = 20 * CHUNK, REST = 12 * CHUNK;

ArrayDescription array()
{
    std::vector<double> xs(static_cast<size_t>(M));
    for (int m = 0; m < M; ++m) xs[static_cast<size_t>(m)] = 0.04 * m;
    return ArrayDescription::make_linear_array_description(xs);
}

double uniform(unsigned &s)
{
    s = s * 1664525u + 1013904223u;
    return static_cast<double>(s >> 8) / 8388608.0 - 1.0;
}

std::vector<std::vector<float> > channels(int n)
{
    std::vector<double> src(static_cast<size_t>(n + M));
    unsigned s = 4711u;
    for (size_t i = 0; i < src.size(); ++i) src[i] = 0.3 * uniform(s);
    std::vector<std::vector<float> > ch(static_cast<size_t>(M), std::vector<float>(static_cast<size_t>(n)));
    for (int m = 0; m < M; ++m) {
        unsigned sm = 12345u + 977u * static_cast<unsigned>(m);
        for (int i = 0; i < n; ++i) ch[static_cast<size_t>(m)][static_cast<size_t>(i)] = static_cast<float>(src[static_cast<size_t>(i + M - m)] + 0.01 * uniform(sm));
    }
    return ch;
}

struct Run {
    std::vector<float> out;               // [S][samples written]
    std::vector<double> cov;
    int written = 0;
};

// S == 0: the single-output overload; S >= 1: one output per look direction.  mode 0: never enabled; 1: gainFloor 1; 2: the defaults.
// The covariance learns during the lead-in and is frozen behind it (a noise-only covariance).
Run run(int S, int mode)
{
    const int total = LEAD + REST, outs = S ? S : 1;
    const std::vector<std::vector<float> > ch = channels(total);
    MvdrBeamformer bf(FS, array(), N);
    const double doas[3] = {0.0, -0.9, 1.1};
    if (S) { bf.setMaxSources(S); bf.setDOAs(std::vector<double>(doas, doas + S)); }
    else bf.setDOA(0.0);
    if (mode == 1) bf.setPostFilter(true, 0.7, 1.0, 3.0);
    if (mode == 2) bf.setPostFilter(true);
    Run r;
    std::vector<std::vector<float> > out(static_cast<size_t>(outs), std::vector<float>(static_cast<size_t>(total)));
    std::vector<const float *> in(static_cast<size_t>(M));
    std::vector<float *> o(static_cast<size_t>(outs));
    for (int pos = 0; pos < total; pos += CHUNK) {
        if (pos == LEAD) bf.setUpdateWeight(0.0);
        for (int m = 0; m < M; ++m) in[static_cast<size_t>(m)] = ch[static_cast<size_t>(m)].data() + pos;
        for (int s = 0; s < outs; ++s) o[static_cast<size_t>(s)] = out[static_cast<size_t>(s)].data() + r.written;
        r.written += S ? bf.process(in, CHUNK, o, total - r.written) : bf.process(in, CHUNK, o[0], total - r.written);
    }
    bf.covariance(r.cov);
    for (int s = 0; s < outs; ++s) r.out.insert(r.out.end(), out[static_cast<size_t>(s)].begin(), out[static_cast<size_t>(s)].begin() + r.written);
    return r;
}

template <typename T>
bool same(const std::vector<T> &a, const std::vector<T> &b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

double power(const Run &r, int s, int from)
{
    double p = 0.0;
    const float *x = r.out.data() + static_cast<size_t>(s) * static_cast<size_t>(r.written);
    for (int i = from; i < r.written; ++i) p += static_cast<double>(x[i]) * x[i];
    return p;
}

}  // namespace

int main()
{
    int failures = 0;
    try {
        for (int S = 0; S <= 3; S += 3) {
            const char *form = S ? "process(in, n, {out_s}, size)" : "process(in, n, out, size)";
            const Run never = run(S, 0), one = run(S, 1), filt = run(S, 2);
            if (never.written <= LEAD) { std::printf("FAIL: %s: nothing written behind the lead-in\n", form); ++failures; }
            if (!same(one.out, never.out) || !same(one.cov, never.cov)) { std::printf("FAIL: %s: gainFloor 1 differs from a run that never enabled the filter\n", form); ++failures; }
            if (!same(filt.cov, never.cov)) { std::printf("FAIL: %s: the filter moved the covariance\n", form); ++failures; }
            if (same(filt.out, never.out)) { std::printf("FAIL: %s: the filter did nothing\n", form); ++failures; }
            // the interferer alone behind the lead-in, towards broadside (output 0): the floor of 0.1 allows -20 dB, the float64 twin
            // of the Python tests measures -18 dB on its scene; -6 dB is asked here
            const double pu = power(never, 0, LEAD + 4 * HOP), pf = power(filt, 0, LEAD + 4 * HOP);
            std::printf("%s: %d samples; interferer alone: unfiltered %.4g filtered %.4g ratio %.4f\n", form, never.written, pu, pf, pf / pu);
            if (!(pu > 0.0) || !(pf > 0.0) || !(pf < 0.25 * pu)) { std::printf("FAIL: %s: the filter did not lower the interferer by 6 dB\n", form); ++failures; }
            for (size_t i = 0; i < filt.out.size(); ++i)
                if (!std::isfinite(filt.out[i])) { std::printf("FAIL: %s: non-finite output\n", form); ++failures; break; }
        }
        MvdrBeamformer p(FS, array(), N);
        bool en = true; double sm = 0.0, fl = 0.0, ns = 0.0;
        p.getPostFilter(en, sm, fl, ns);
        if (en || sm != 0.98 || fl != 0.1 || ns != 1.0) { std::printf("FAIL: the defaults are %d %g %g %g\n", en, sm, fl, ns); ++failures; }
        p.setPostFilter(true, 0.5, 0.25, 2.0);
        p.getPostFilter(en, sm, fl, ns);
        if (!en || sm != 0.5 || fl != 0.25 || ns != 2.0) { std::printf("FAIL: getPostFilter gives %d %g %g %g\n", en, sm, fl, ns); ++failures; }
        bool thrown = false;
        try { p.setPostFilter(false, 1.0); } catch (const MCArrayException &) { thrown = true; }
        p.getPostFilter(en, sm, fl, ns);
        if (!thrown || !en || sm != 0.5 || fl != 0.25 || ns != 2.0) { std::printf("FAIL: a refused value: thrown %d, then %d %g %g %g\n", thrown, en, sm, fl, ns); ++failures; }
        p.setPostFilter(false);
        p.getPostFilter(en, sm, fl, ns);
        if (en || sm != 0.98 || fl != 0.1 || ns != 1.0) { std::printf("FAIL: after disabling: %d %g %g %g\n", en, sm, fl, ns); ++failures; }
    } catch (const MCArrayException &e) {
        std::printf("FAIL: exception: %s\n", e.what());
        ++failures;
    }
    std::printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
