// mca::MvdrBeamformer: setMaskEstimator() / getMaskEstimator() and both processAuto() overloads (one output / one output per look
// direction of setDOAs()), over chunks that are no multiple of the hop.
//   - with setRtf(true), processAuto() reproduces processRtf() fed the masks it returned, byte for byte, covariance included;
//   - without RTF it reproduces process() fed the update mask it returned;
//   - the masks lie in [0, 1], take values inside, and with one protected direction the update mask is 1 - target mask 0;
//   - processAuto() without setMaskEstimator(true) throws, and a refused configuration leaves the former one readable.
// The stream is synthetic (two tones from two directions plus a deterministic noise per channel); no input files.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mcarray/micarray.h"

using namespace mca;

namespace {

const int FS = 16000, N = 256, M = 6, HOP = N / 2, K = N / 2 + 1, CHUNK = 300;      // CHUNK: no multiple of the hop
const int TOTAL = 14 * CHUNK;
const double DOAS[2] = {0.35, -0.6};

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
    std::vector<float> um, tm;            // per chunk, behind one another: [F][K] and [S][F][K]
    std::vector<int> frames;              // F of every chunk
    std::vector<double> cov;
    int written = 0;
};

enum Mode { AUTO, FED };

// S == 0: the single-output overloads; S >= 1: one output per look direction.  FED: processRtf() / process() under the masks of `from`.
Run run(int S, bool rtf, Mode mode, const Run *from)
{
    const int outs = S ? S : 1;
    std::vector<std::vector<float> > ch;
    for (int m = 0; m < M; ++m) ch.push_back(channel(m, TOTAL));
    MvdrBeamformer bf(FS, array(), N);
    if (S) { bf.setMaxSources(S); bf.setDOAs(std::vector<double>(DOAS, DOAS + S)); }
    else bf.setDOA(DOAS[0]);
    if (rtf) bf.setRtf(true, 0.9, 2, 1);
    if (mode == AUTO) {
        if (S) bf.setMaskEstimator(true, 2, -1, 0.3, 0.8, 1);
        else bf.setMaskEstimator(true, 2, K - 3, 0.2, 0.4);
    }
    Run r;
    std::vector<std::vector<float> > out(static_cast<size_t>(outs), std::vector<float>(static_cast<size_t>(TOTAL)));
    std::vector<float *> in(static_cast<size_t>(M)), o(static_cast<size_t>(outs));
    size_t uo = 0, to = 0;
    int chunk = 0;
    for (int pos = 0; pos < TOTAL; pos += CHUNK, ++chunk) {
        const int F = bf.framesCompletedBy(CHUNK);
        for (int m = 0; m < M; ++m) in[static_cast<size_t>(m)] = ch[static_cast<size_t>(m)].data() + pos;
        for (int s = 0; s < outs; ++s) o[static_cast<size_t>(s)] = out[static_cast<size_t>(s)].data() + r.written;
        int w = 0;
        if (mode == AUTO) {
            std::vector<float> um(static_cast<size_t>(F) * K + 1, -7.f), tm(static_cast<size_t>(outs) * F * K + 1, -7.f);
            w = S ? bf.processAuto(in, CHUNK, o, TOTAL - r.written, um.data(), tm.data()) : bf.processAuto(in, CHUNK, o[0], TOTAL - r.written, um.data(), tm.data());
            r.um.insert(r.um.end(), um.begin(), um.end() - 1);
            r.tm.insert(r.tm.end(), tm.begin(), tm.end() - 1);
            r.frames.push_back(F);
        } else {
            const float *um = from->um.data() + uo, *tm = from->tm.data() + to;
            if (F != from->frames[static_cast<size_t>(chunk)]) throw MCArrayException("the chunks of the two runs differ");
            if (rtf) w = S ? bf.processRtf(in, CHUNK, o, TOTAL - r.written, um, tm) : bf.processRtf(in, CHUNK, o[0], TOTAL - r.written, um, tm);
            else w = S ? bf.process(in, CHUNK, o, TOTAL - r.written, um) : bf.process(in, CHUNK, o[0], TOTAL - r.written, um);
            uo += static_cast<size_t>(F) * K;
            to += static_cast<size_t>(outs) * F * K;
        }
        if (w != F * HOP) throw MCArrayException("framesCompletedBy() is not the frames of the chunk");
        r.written += w;
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

}  // namespace

int main()
{
    int failures = 0;
    try {
        for (int S = 0; S <= 2; S += 2) {
            for (int rtf = 1; rtf >= 0; --rtf) {
                const char *form = S ? "processAuto(in, n, {out_s}, size, um, tm)" : "processAuto(in, n, out, size, um, tm)";
                const char *under = rtf ? "processRtf()" : "process()";
                const Run a = run(S, rtf != 0, AUTO, nullptr), f = run(S, rtf != 0, FED, &a);
                if (!same(a.out, f.out) || !same(a.cov, f.cov)) { std::printf("FAIL: %s differs from %s fed its masks\n", form, under); ++failures; }
                size_t inside = 0, closed = 0;
                bool range = true, relation = true;
                for (float v : a.tm) { range = range && v >= 0.f && v <= 1.f; inside += v > 0.f && v < 1.f; }
                for (float v : a.um) { range = range && v >= 0.f && v <= 1.f; closed += v < 1.f; }
                // one protected direction (or one direction): update = 1 - target mask 0, chunk by chunk
                size_t uo = 0, to = 0;
                const int outs = S ? S : 1;
                for (size_t c = 0; c < a.frames.size(); ++c) {
                    const size_t n = static_cast<size_t>(a.frames[c]) * K;
                    for (size_t i = 0; i < n; ++i) relation = relation && a.um[uo + i] == 1.f - a.tm[to + i];
                    uo += n; to += n * static_cast<size_t>(outs);
                }
                if (!range) { std::printf("FAIL: %s: a mask value outside [0, 1] (or a cell not written)\n", form); ++failures; }
                if (!relation) { std::printf("FAIL: %s: the update mask is not 1 - target mask 0\n", form); ++failures; }
                if (!inside || !closed) { std::printf("FAIL: %s: the masks are trivial\n", form); ++failures; }
                for (size_t i = 0; i < a.out.size(); ++i)
                    if (!std::isfinite(a.out[i])) { std::printf("FAIL: %s: output %zu is not finite\n", form, i); ++failures; break; }
                std::printf("%s == %s under the returned masks: %d samples, %zu of %zu target cells inside (0, 1), %zu of %zu update cells below 1\n",
                            form, under, a.written, inside, a.tm.size(), closed, a.um.size());
            }
        }
        // not enabled: refused; a refused configuration leaves the former one
        MvdrBeamformer p(FS, array(), N);
        std::vector<std::vector<float> > ch;
        for (int m = 0; m < M; ++m) ch.push_back(channel(m, 2 * N));
        std::vector<float *> in(static_cast<size_t>(M));
        for (int m = 0; m < M; ++m) in[static_cast<size_t>(m)] = ch[static_cast<size_t>(m)].data();
        std::vector<float> o(static_cast<size_t>(2 * N));
        bool threw = false;
        try { p.processAuto(in, 2 * N, o.data(), 2 * N); } catch (const MCArrayException &) { threw = true; }
        if (!threw) { std::printf("FAIL: processAuto() without setMaskEstimator(true) did not throw\n"); ++failures; }
        p.reset();
        p.setMaskEstimator(true, 3, 100, 0.1, 0.7, 1);
        threw = false;
        try { p.setMaskEstimator(true, 3, 100, 0.5, 0.5, 1); } catch (const MCArrayException &) { threw = true; }
        bool en = false; int lo = 0, hi = 0, np = 0; double cl = 0, chh = 0;
        p.getMaskEstimator(en, lo, hi, cl, chh, np);
        if (!threw || !en || lo != 3 || hi != 100 || cl != 0.1 || chh != 0.7 || np != 1) { std::printf("FAIL: a refused configuration changed the held one\n"); ++failures; }
        p.setMaskEstimator(true);
        p.getMaskEstimator(en, lo, hi, cl, chh, np);
        if (lo != 0 || hi != N / 2 || cl != 0.0 || chh != 0.05 || np != 0) { std::printf("FAIL: the defaults of setMaskEstimator()\n"); ++failures; }
        if (p.processAuto(in, 2 * N, o.data(), 2 * N) != 3 * HOP) { std::printf("FAIL: processAuto() without mask outputs\n"); ++failures; }
    } catch (const MCArrayException &e) {
        std::printf("FAIL: exception: %s\n", e.what());
        ++failures;
    }
    std::printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
