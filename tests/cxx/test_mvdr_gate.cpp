// mca::MvdrBeamformer::setUpdateWeight: the covariance update weight of the frames completed from now on, through both process()
// overloads (one output / one output per look direction of setDOAs()), over chunks that are no multiple of the hop.
//   - setUpdateWeight(0) after a lead-in keeps mca_hip_mvdr_get_covariance unchanged over further process() calls, and the frames
//     are still beamformed;
//   - setUpdateWeight(1) reproduces a run that never called it, byte for byte;
//   - a weight between moves the covariance, and differently from weight 1.
// The stream is synthetic (a tone plus a deterministic noise per channel); no input files.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mcarray/micarray.h"

using namespace mca;

namespace {

const int FS = 16000, N = 256, M = 6, HOP = N / 2, CHUNK = 300;      // CHUNK: no multiple of the hop
const int LEAD = 10 * CHUNK, REST = 8 * CHUNK;

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
        x[static_cast<size_t>(i)] = static_cast<float>(0.2 * std::sin(2.0 * M_PI * 440.0 * (i - 3 * m) / FS) + noise);
    }
    return x;
}

struct Run {
    std::vector<float> out;               // [S][samples written]
    std::vector<double> cov_lead, cov;    // covariance (mca_hip_mvdr_get_covariance, through the class) after the lead-in and at the end
    int written = 0;
};

// S == 0: the single-output overload; S >= 1: the overload with one output per look direction.  weight < 0: never call setUpdateWeight.
Run run(int S, double weight)
{
    const int total = LEAD + REST, outs = S ? S : 1;
    std::vector<std::vector<float> > ch;
    for (int m = 0; m < M; ++m) ch.push_back(channel(m, total));
    MvdrBeamformer bf(FS, array(), N);
    const double doas[3] = {0.35, -0.6, 1.1};
    if (S) { bf.setMaxSources(S); bf.setDOAs(std::vector<double>(doas, doas + S)); }
    else bf.setDOA(0.35);
    Run r;
    const size_t cap = static_cast<size_t>(total);
    std::vector<std::vector<float> > out(static_cast<size_t>(outs), std::vector<float>(cap));
    std::vector<float *> in(static_cast<size_t>(M)), o(static_cast<size_t>(outs));
    for (int pos = 0; pos < total; pos += CHUNK) {
        if (pos == LEAD) {
            bf.covariance(r.cov_lead);
            if (weight >= 0.0) bf.setUpdateWeight(weight);
        }
        for (int m = 0; m < M; ++m) in[static_cast<size_t>(m)] = ch[static_cast<size_t>(m)].data() + pos;
        for (int s = 0; s < outs; ++s) o[static_cast<size_t>(s)] = out[static_cast<size_t>(s)].data() + r.written;
        r.written += S ? bf.process(in, CHUNK, o, total - r.written) : bf.process(in, CHUNK, o[0], total - r.written);
    }
    bf.covariance(r.cov);
    if (r.cov.size() != static_cast<size_t>(N / 2 + 1) * M * M * 2) throw MCArrayException("covariance(): [K][M][M][2] expected");
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
        for (int S = 0; S <= 3; S += 3) {
            const char *form = S ? "process(in, n, {out_s}, size)" : "process(in, n, out, size)";
            const Run never = run(S, -1.0), one = run(S, 1.0), zero = run(S, 0.0), half = run(S, 0.5);
            const int lead_out = (LEAD - N) / HOP * HOP + HOP;      // samples written when the weight changes
            if (never.written <= lead_out) { std::printf("FAIL: %s: nothing written behind the lead-in\n", form); ++failures; }
            if (!same(one.out, never.out) || !same(one.cov, never.cov)) { std::printf("FAIL: %s: setUpdateWeight(1) differs from a run that never called it\n", form); ++failures; }
            if (!same(zero.cov, zero.cov_lead)) { std::printf("FAIL: %s: setUpdateWeight(0) changed the covariance\n", form); ++failures; }
            if (!same(zero.cov_lead, never.cov_lead)) { std::printf("FAIL: %s: the lead-in differs between runs\n", form); ++failures; }
            if (same(never.cov, never.cov_lead)) { std::printf("FAIL: %s: the covariance did not move at weight 1\n", form); ++failures; }
            if (same(half.cov, never.cov) || same(half.cov, zero.cov)) { std::printf("FAIL: %s: weight 0.5 equals weight 1 or 0\n", form); ++failures; }
            // frozen frames are still beamformed: audio behind the lead-in, and not the unfrozen run's
            const int outs = S ? S : 1;
            for (int s = 0; s < outs; ++s) {
                const float *z = zero.out.data() + static_cast<size_t>(s) * static_cast<size_t>(zero.written);
                const float *n = never.out.data() + static_cast<size_t>(s) * static_cast<size_t>(never.written);
                double pz = 0.0; bool differs = false, finite = true;
                for (int i = lead_out + HOP; i < zero.written; ++i) { pz += static_cast<double>(z[i]) * z[i]; differs |= z[i] != n[i]; finite &= std::isfinite(z[i]) != 0; }
                if (!(pz > 0.0) || !differs || !finite) { std::printf("FAIL: %s: output %d of the frozen frames: power %g, differs %d, finite %d\n", form, s, pz, differs, finite); ++failures; }
                if (std::memcmp(z, n, static_cast<size_t>(lead_out) * sizeof(float)) != 0) { std::printf("FAIL: %s: output %d of the lead-in differs\n", form, s); ++failures; }
            }
            std::printf("%s: %d samples, weight 1 == never, weight 0 keeps the covariance\n", form, never.written);
        }
        MvdrBeamformer p(FS, array(), N);
        if (p.getUpdateWeight() != 1.0) { std::printf("FAIL: the default weight is %g\n", p.getUpdateWeight()); ++failures; }
    } catch (const MCArrayException &e) {
        std::printf("FAIL: exception: %s\n", e.what());
        ++failures;
    }
    std::printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
