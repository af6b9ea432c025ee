// mca::MvdrBeamformer: setGeometry() / getGeometry() on a planar array.
//   - the round trip, and LINEAR_X keeping the elevation at 0;
//   - process() with two look directions, one of them behind the array, gives the bytes of the C ABI
//     (mca_hip_mvdr_set_geometry + mca_hip_mvdr_sources_frames_host) on the same stream;
//   - a change un-configures the spectrum: spectrumGrid() throws until configureSpectrum(), then reports the periodic grid;
//   - what the library refuses throws MCArrayException and leaves the geometry as it was.
// The stream is synthetic (two tones plus a deterministic noise per channel); no input files.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mcarray/micarray.h"

using namespace mca;

namespace {

const int FS = 16000, N = 256, M = 6, HOP = N / 2, F = 8, S = 2;
const int TOTAL = (F + 1) * HOP;
const double LOOK[S] = {2.8, -1.0}, ELEVATION = 0.2;

ArrayDescription array()
{
    ArrayDescription d;
    for (int m = 0; m < M; ++m) d.pushPosition(0.045 * std::cos(2.0 * M_PI * m / M), 0.045 * std::sin(2.0 * M_PI * m / M), 0.01 * (m % 2));
    return d;
}

std::vector<float> channel(int m, int n)
{
    std::vector<float> x(static_cast<size_t>(n));
    unsigned s = 4321u + 977u * static_cast<unsigned>(m);
    for (int i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        const double noise = (static_cast<double>(s >> 8) / 8388608.0 - 1.0) * 0.05;
        x[static_cast<size_t>(i)] = static_cast<float>(0.2 * std::sin(2.0 * M_PI * 440.0 * (i - 2 * m) / FS) + 0.1 * std::sin(2.0 * M_PI * 1900.0 * (i + m) / FS) + noise);
    }
    return x;
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
        std::vector<std::vector<float> > ch;
        for (int m = 0; m < M; ++m) ch.push_back(channel(m, TOTAL));
        // ---- the class ----
        MvdrBeamformer bf(FS, array(), N);
        int mode = -1;
        double el = -1.0;
        bf.getGeometry(mode, el);
        if (mode != MCA_HIP_MVDR_GEOMETRY_LINEAR_X || el != 0.0) { std::printf("FAIL: the default geometry\n"); ++failures; }
        bf.setGeometry(MCA_HIP_MVDR_GEOMETRY_LINEAR_X, 0.7);
        bf.getGeometry(mode, el);
        if (mode != MCA_HIP_MVDR_GEOMETRY_LINEAR_X || el != 0.0) { std::printf("FAIL: LINEAR_X keeps the elevation at 0\n"); ++failures; }
        bf.setMaxSources(S);
        bf.configureSpectrum(61, 1, 100);
        bf.setGeometry(MCA_HIP_MVDR_GEOMETRY_XYZ, ELEVATION);
        bf.getGeometry(mode, el);
        if (mode != MCA_HIP_MVDR_GEOMETRY_XYZ || el != ELEVATION) { std::printf("FAIL: the round trip\n"); ++failures; }
        int threw = 0;
        try { bf.spectrumGrid(); } catch (const MCArrayException &) { ++threw; }                          // un-configured by the change
        try { bf.setGeometry(2); } catch (const MCArrayException &) { ++threw; }
        try { bf.setGeometry(MCA_HIP_MVDR_GEOMETRY_XYZ, std::nan("")); } catch (const MCArrayException &) { ++threw; }
        try { bf.setGeometry(MCA_HIP_MVDR_GEOMETRY_XYZ, 1.6); } catch (const MCArrayException &) { ++threw; }
        try { bf.setGeometry(MCA_HIP_MVDR_GEOMETRY_XYZ, -INFINITY); } catch (const MCArrayException &) { ++threw; }
        if (threw != 5) { std::printf("FAIL: %d of 5 refusals threw\n", threw); ++failures; }
        bf.getGeometry(mode, el);
        if (mode != MCA_HIP_MVDR_GEOMETRY_XYZ || el != ELEVATION) { std::printf("FAIL: a refusal changed the geometry\n"); ++failures; }
        bf.configureSpectrum(72, 1, 100);
        const std::vector<double> grid = bf.spectrumGrid();
        if (grid.size() != 72 || grid[0] != static_cast<double>(static_cast<float>(-M_PI)) || !(grid[71] < M_PI) || !(grid[71] > 3.0)) {
            std::printf("FAIL: the periodic grid\n"); ++failures;
        }
        bf.setDOAs(std::vector<double>(LOOK, LOOK + S));
        std::vector<std::vector<float> > out(static_cast<size_t>(S), std::vector<float>(static_cast<size_t>(TOTAL)));
        std::vector<float *> in(static_cast<size_t>(M)), o(static_cast<size_t>(S));
        for (int m = 0; m < M; ++m) in[static_cast<size_t>(m)] = ch[static_cast<size_t>(m)].data();
        for (int s = 0; s < S; ++s) o[static_cast<size_t>(s)] = out[static_cast<size_t>(s)].data();
        const int written = bf.process(in, TOTAL, o, TOTAL);
        if (written != F * HOP) { std::printf("FAIL: %d samples written\n", written); ++failures; }
        std::vector<double> cov;
        bf.covariance(cov);

        // ---- the C ABI on the same stream ----
        const std::vector<double> xyz = array().xyz();
        mca_hip_mvdr_config cfg;
        cfg.struct_size = static_cast<int>(sizeof(cfg));
        cfg.device = 0; cfg.sample_rate = FS; cfg.fft_size = N; cfg.n_mics = M; cfg.mic_xyz = xyz.data();
        cfg.alpha = 0.95; cfg.loading = 1e-3; cfg.max_streams = 1;
        mca_hip_mvdr_ctx *ctx = nullptr;
        mca_hip_mvdr_geometry_config geo;
        geo.struct_size = static_cast<int>(sizeof(geo));
        geo.mode = MCA_HIP_MVDR_GEOMETRY_XYZ;
        geo.elevation_rad = ELEVATION;
        std::vector<float> pcm(static_cast<size_t>(M) * TOTAL), doa(static_cast<size_t>(F) * S), ref(static_cast<size_t>(S) * F * HOP);
        for (int m = 0; m < M; ++m) std::memcpy(pcm.data() + static_cast<size_t>(m) * TOTAL, ch[static_cast<size_t>(m)].data(), sizeof(float) * TOTAL);
        for (int t = 0; t < F; ++t)
            for (int s = 0; s < S; ++s) doa[static_cast<size_t>(t * S + s)] = static_cast<float>(LOOK[s]);
        std::vector<double> cov_c(cov.size());
        if (mca_hip_mvdr_create(&cfg, &ctx) != MCA_HIP_OK || mca_hip_mvdr_set_max_sources(ctx, S) != MCA_HIP_OK ||
            mca_hip_mvdr_set_geometry(ctx, &geo) != MCA_HIP_OK ||
            mca_hip_mvdr_sources_frames_host(ctx, pcm.data(), 1, F, S, doa.data(), ref.data(), nullptr) != MCA_HIP_OK ||
            mca_hip_mvdr_get_covariance(ctx, 0, cov_c.data()) != MCA_HIP_OK) {
            std::printf("FAIL: the C ABI run: %s\n", mca_hip_mvdr_last_error(ctx));
            ++failures;
        }
        bool eq = same(cov, cov_c), finite = true, loud = false;
        for (int s = 0; s < S; ++s) {
            eq = eq && std::memcmp(out[static_cast<size_t>(s)].data(), ref.data() + static_cast<size_t>(s) * F * HOP, sizeof(float) * F * HOP) == 0;
            for (int i = 0; i < F * HOP; ++i) { finite = finite && std::isfinite(out[static_cast<size_t>(s)][static_cast<size_t>(i)]); loud = loud || out[static_cast<size_t>(s)][static_cast<size_t>(i)] != 0.f; }
        }
        if (!eq) { std::printf("FAIL: the class and the C ABI differ\n"); ++failures; }
        if (!finite || !loud) { std::printf("FAIL: the output is silent or not finite\n"); ++failures; }
        // and the geometry matters on this array: LINEAR_X gives other bytes
        geo.mode = MCA_HIP_MVDR_GEOMETRY_LINEAR_X;
        std::vector<float> lin(ref.size());
        if (mca_hip_mvdr_reset(ctx, nullptr) != MCA_HIP_OK || mca_hip_mvdr_set_geometry(ctx, &geo) != MCA_HIP_OK ||
            mca_hip_mvdr_sources_frames_host(ctx, pcm.data(), 1, F, S, doa.data(), lin.data(), nullptr) != MCA_HIP_OK) {
            std::printf("FAIL: the LINEAR_X run: %s\n", mca_hip_mvdr_last_error(ctx));
            ++failures;
        }
        if (same(lin, ref)) { std::printf("FAIL: XYZ and LINEAR_X agree on a planar array\n"); ++failures; }
        mca_hip_mvdr_destroy(ctx);
        std::printf("setGeometry(XYZ, %.1f): %d samples per look direction equal to the C ABI's, 5 refusals threw\n", ELEVATION, written);
    } catch (const MCArrayException &e) {
        std::printf("FAIL: exception: %s\n", e.what());
        ++failures;
    }
    std::printf(failures ? "%d FAILED\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
