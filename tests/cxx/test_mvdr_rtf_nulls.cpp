// mca::MvdrBeamformer: setRtfNulls() / getRtfNulls() with processRtf() on two look directions, over chunks that are no multiple of
// the hop.
//   - setRtfNulls(true) + setNullGain(g) + processRtf() changes output 0 (and output 1) of the call and leaves the covariance's bytes;
//   - setRtfNulls(true) with gain 0 gives the bytes of the call without the switch;
//   - setRtfNulls(false) restores the refusal of a non-zero null gain, and the getter follows.
// The stream is synthetic (two tones from two directions plus a deterministic noise per channel); no input files.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mcarray/micarray.h"

using namespace mca;

namespace {

const int FS = 16000, N = 256, M = 6, HOP = N / 2, K = N / 2 + 1, CHUNK = 300, S = 2;      // CHUNK: no multiple of the hop
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
    std::vector<float> out[S];
    std::vector<double> cov;
    bool threw = false;
};

// the target masks: direction 0 owns the bins below 40, direction 1 those from 40 to 79; the update mask is open above
Run run(bool nulls, double gain)
{
    std::vector<std::vector<float> > ch;
    for (int m = 0; m < M; ++m) ch.push_back(channel(m, TOTAL));
    MvdrBeamformer bf(FS, array(), N);
    bf.setMaxSources(S);
    bf.setDOAs(std::vector<double>(DOAS, DOAS + S));
    bf.setRtf(true, 0.9, 2, 1);
    bf.setNullGain(gain);
    bf.setRtfNulls(nulls);
    Run r;
    std::vector<std::vector<float> > out(static_cast<size_t>(S), std::vector<float>(static_cast<size_t>(TOTAL)));
    std::vector<float *> in(static_cast<size_t>(M)), o(static_cast<size_t>(S));
    int written = 0;
    try {
        for (int pos = 0; pos < TOTAL; pos += CHUNK) {
            const int F = bf.framesCompletedBy(CHUNK);
            for (int m = 0; m < M; ++m) in[static_cast<size_t>(m)] = ch[static_cast<size_t>(m)].data() + pos;
            for (int s = 0; s < S; ++s) o[static_cast<size_t>(s)] = out[static_cast<size_t>(s)].data() + written;
            std::vector<float> um(static_cast<size_t>(F) * K, 0.f), tm(static_cast<size_t>(S) * F * K, 0.f);
            for (int t = 0; t < F; ++t)
                for (int k = 0; k < K; ++k) {
                    um[static_cast<size_t>(t * K + k)] = k >= 80 ? 1.f : 0.f;
                    tm[static_cast<size_t>((0 * F + t) * K + k)] = k < 40 ? 1.f : 0.f;
                    tm[static_cast<size_t>((1 * F + t) * K + k)] = k >= 40 && k < 80 ? 1.f : 0.f;
                }
            const int w = bf.processRtf(in, CHUNK, o, TOTAL - written, um.data(), tm.data());
            if (w != F * HOP) throw MCArrayException("framesCompletedBy() is not the frames of the chunk");
            written += w;
        }
    } catch (const MCArrayException &) {
        r.threw = true;
        return r;
    }
    bf.covariance(r.cov);
    for (int s = 0; s < S; ++s) r.out[s].assign(out[static_cast<size_t>(s)].begin(), out[static_cast<size_t>(s)].begin() + written);
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
        const Run plain = run(false, 0.0), armed = run(true, 0.0), nulled = run(true, 50.0), refused = run(false, 50.0);
        if (plain.threw || armed.threw || nulled.threw) { std::printf("FAIL: a call that should run threw\n"); ++failures; }
        else {
            if (!same(plain.out[0], armed.out[0]) || !same(plain.out[1], armed.out[1]) || !same(plain.cov, armed.cov)) {
                std::printf("FAIL: setRtfNulls(true) with gain 0 moved bytes\n"); ++failures;
            }
            for (int s = 0; s < S; ++s) {
                double diff = 0.0, peak = 0.0;
                bool finite = true;
                for (size_t i = 0; i < nulled.out[s].size(); ++i) {
                    finite = finite && std::isfinite(nulled.out[s][i]);
                    diff = std::fmax(diff, std::fabs(static_cast<double>(nulled.out[s][i]) - plain.out[s][i]));
                    peak = std::fmax(peak, std::fabs(static_cast<double>(plain.out[s][i])));
                }
                std::printf("output %d: the nulls move it by %.3g of its peak %.3g over %zu samples\n", s, diff / peak, peak, nulled.out[s].size());
                if (!finite) { std::printf("FAIL: output %d under nulls is not finite\n", s); ++failures; }
                if (!(diff > 1e-3 * peak)) { std::printf("FAIL: setRtfNulls(true) + setNullGain(50) did not change output %d\n", s); ++failures; }
            }
            if (!same(plain.cov, nulled.cov)) { std::printf("FAIL: the null gain entered the covariance\n"); ++failures; }
        }
        if (!refused.threw) { std::printf("FAIL: processRtf() under a null gain without setRtfNulls(true) did not throw\n"); ++failures; }

        // the switch on one object: on, a call runs; off, the same call is refused; the getter follows; bad values never reach it
        MvdrBeamformer p(FS, array(), N);
        p.setMaxSources(S);
        p.setDOAs(std::vector<double>(DOAS, DOAS + S));
        p.setRtf(true);
        if (p.getRtfNulls()) { std::printf("FAIL: the switch is not off by default\n"); ++failures; }
        p.setNullGain(10.0);
        p.setRtfNulls(true);
        if (!p.getRtfNulls() || p.getNullGain() != 10.0) { std::printf("FAIL: getRtfNulls() after setRtfNulls(true)\n"); ++failures; }
        std::vector<std::vector<float> > ch;
        for (int m = 0; m < M; ++m) ch.push_back(channel(m, 2 * N));
        std::vector<float *> in(static_cast<size_t>(M));
        for (int m = 0; m < M; ++m) in[static_cast<size_t>(m)] = ch[static_cast<size_t>(m)].data();
        std::vector<float> o0(static_cast<size_t>(2 * N)), o1(static_cast<size_t>(2 * N));
        std::vector<float *> o(2);
        o[0] = o0.data(); o[1] = o1.data();
        if (p.processRtf(in, 2 * N, o, 2 * N, static_cast<const float *>(nullptr), static_cast<const float *>(nullptr)) != 3 * HOP) {
            std::printf("FAIL: processRtf() under nulls\n"); ++failures;
        }
        p.setRtfNulls(false);
        bool threw = false;
        try { p.processRtf(in, N, o, 2 * N, static_cast<const float *>(nullptr), static_cast<const float *>(nullptr)); } catch (const MCArrayException &) { threw = true; }
        if (!threw || p.getRtfNulls()) { std::printf("FAIL: setRtfNulls(false) did not restore the refusal\n"); ++failures; }
    } catch (const MCArrayException &e) {
        std::printf("FAIL: exception: %s\n", e.what());
        ++failures;
    }
    std::printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
