// mca::MvdrBeamformer: framesCompletedBy() and the updateMask argument of both process() overloads (one output / one output per look
// direction of setDOAs()), over chunks that are no multiple of the hop.
//   - framesCompletedBy(n) is the number of frames the next process() chunk of n samples completes (its return value / hop);
//   - a mask of ones reproduces a run that never passed one, byte for byte;
//   - a mask that holds 0.5 in every cell reproduces setUpdateWeight(0.5), and overrides another setUpdateWeight() for its call;
//   - a mask with closed bins keeps those bins of mca_hip_mvdr_get_covariance unchanged while the others move.
// The stream is synthetic (a tone plus a deterministic noise per channel); no input files.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mcarray/micarray.h"

using namespace mca;

namespace {

const int FS = 16000, N = 256, M = 6, HOP = N / 2, K = N / 2 + 1, CHUNK = 300;      // CHUNK: no multiple of the hop
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

bool closedBin(int k) { return k % 3 == 1; }

struct Run {
    std::vector<float> out;               // [S][samples written]
    std::vector<double> cov_lead, cov;    // covariance after the lead-in and at the end
    int written = 0;
    bool frames_ok = true;                // framesCompletedBy() named the frames of every chunk
};

enum Mode { NEVER, WEIGHT_HALF, MASK_ONES, MASK_HALF, MASK_HALF_OVER_WEIGHT_ZERO, MASK_CLOSED_BINS };

// S == 0: the single-output overload; S >= 1: the overload with one output per look direction.  The mode applies behind the lead-in.
Run run(int S, Mode mode)
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
    std::vector<float> mask;
    for (int pos = 0; pos < total; pos += CHUNK) {
        const bool behind = pos >= LEAD;
        if (pos == LEAD) {
            bf.covariance(r.cov_lead);
            if (mode == WEIGHT_HALF) bf.setUpdateWeight(0.5);
            if (mode == MASK_HALF_OVER_WEIGHT_ZERO) bf.setUpdateWeight(0.0);
        }
        const int F = bf.framesCompletedBy(CHUNK);
        const float *mp = nullptr;
        if (behind && mode >= MASK_ONES) {
            mask.assign(static_cast<size_t>(F) * K, mode == MASK_ONES ? 1.f : 0.5f);
            if (mode == MASK_CLOSED_BINS)
                for (int t = 0; t < F; ++t)
                    for (int k = 0; k < K; ++k) mask[static_cast<size_t>(t) * K + static_cast<size_t>(k)] = closedBin(k) ? 0.f : 1.f;
            mask.push_back(0.f);          // (a frame count of 0 still has a pointer)
            mp = mask.data();
        }
        for (int m = 0; m < M; ++m) in[static_cast<size_t>(m)] = ch[static_cast<size_t>(m)].data() + pos;
        for (int s = 0; s < outs; ++s) o[static_cast<size_t>(s)] = out[static_cast<size_t>(s)].data() + r.written;
        const int w = S ? bf.process(in, CHUNK, o, total - r.written, mp) : bf.process(in, CHUNK, o[0], total - r.written, mp);
        if (w != F * HOP) r.frames_ok = false;
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
        for (int S = 0; S <= 3; S += 3) {
            const char *form = S ? "process(in, n, {out_s}, size, mask)" : "process(in, n, out, size, mask)";
            const Run never = run(S, NEVER), half = run(S, WEIGHT_HALF), ones = run(S, MASK_ONES), mhalf = run(S, MASK_HALF),
                      over = run(S, MASK_HALF_OVER_WEIGHT_ZERO), closed = run(S, MASK_CLOSED_BINS);
            if (!never.frames_ok || !closed.frames_ok) { std::printf("FAIL: %s: framesCompletedBy() is not the frames of the chunk\n", form); ++failures; }
            if (!same(ones.out, never.out) || !same(ones.cov, never.cov)) { std::printf("FAIL: %s: a mask of ones differs from a run without a mask\n", form); ++failures; }
            if (!same(mhalf.out, half.out) || !same(mhalf.cov, half.cov)) { std::printf("FAIL: %s: a mask of 0.5 differs from setUpdateWeight(0.5)\n", form); ++failures; }
            if (!same(over.out, half.out) || !same(over.cov, half.cov)) { std::printf("FAIL: %s: the mask does not override setUpdateWeight(0)\n", form); ++failures; }
            if (same(half.cov, never.cov)) { std::printf("FAIL: %s: weight 0.5 equals weight 1\n", form); ++failures; }
            // closed bins keep the covariance of the lead-in, the others are those of the run without a mask
            const size_t per = static_cast<size_t>(M) * M * 2;
            for (int k = 0; k < K; ++k) {
                const double *c = closed.cov.data() + static_cast<size_t>(k) * per;
                const double *ref = (closedBin(k) ? closed.cov_lead.data() : never.cov.data()) + static_cast<size_t>(k) * per;
                if (std::memcmp(c, ref, per * sizeof(double)) != 0) { std::printf("FAIL: %s: bin %d (%s) of the covariance\n", form, k, closedBin(k) ? "closed" : "open"); ++failures; break; }
            }
            if (same(closed.cov, closed.cov_lead) || same(closed.cov, never.cov)) { std::printf("FAIL: %s: the closed-bin mask equals all 0 or all 1\n", form); ++failures; }
            for (size_t i = 0; i < closed.out.size(); ++i)
                if (!std::isfinite(closed.out[i])) { std::printf("FAIL: %s: output %zu is not finite\n", form, i); ++failures; break; }
            std::printf("%s: %d samples; ones == no mask, 0.5 == setUpdateWeight(0.5), closed bins keep their covariance\n", form, never.written);
        }
        MvdrBeamformer p(FS, array(), N);
        if (p.framesCompletedBy(N - 1) != 0 || p.framesCompletedBy(N) != 1 || p.framesCompletedBy(N + HOP - 1) != 1 || p.framesCompletedBy(N + 3 * HOP) != 4
            || p.framesCompletedBy(0) != 0) { std::printf("FAIL: framesCompletedBy() of a fresh stream\n"); ++failures; }
    } catch (const MCArrayException &e) {
        std::printf("FAIL: exception: %s\n", e.what());
        ++failures;
    }
    std::printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
