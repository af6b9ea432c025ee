// mca::MvdrBeamformer -- frequency-domain beamformer with a per-bin spatial covariance (BASELINE.json configs[3]).
// NOT in the reference (its only beamformer is the delay-and-sum of Beamformer.h:39,49 / Beamformer.cpp:51-71); the
// class follows the shape of the reference's stream modules (constructor = whole configuration, process() over chunks
// of PCM with one pointer per channel, SourceSeparationAndLocalisation.h:47) and Beamformer's steering convention
// (Beamformer.cpp:59).  Definition: SURVEY A.9 / include/mcarray_hip.h (mca_hip_mvdr_*).
#ifndef MCA_HIP_MVDRBEAMFORMER_H
#define MCA_HIP_MVDRBEAMFORMER_H
#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "../mcarray_hip.h"
#include "ArrayDescription.h"
#include "mcarray_exception.h"

namespace mca {

class MvdrBeamformer {
public:
    MvdrBeamformer(int sampleRate, ArrayDescription microphonePositions, int fftSize = 1024, double alpha = 0.95,
                   double loading = 1e-3, int device = 0)
        : _nchannels(static_cast<int>(microphonePositions.size())), _N(fftSize)
    {
        std::vector<double> xyz = microphonePositions.xyz();
        mca_hip_mvdr_config cfg;
        cfg.struct_size = static_cast<int>(sizeof(cfg));
        cfg.device = device;
        cfg.sample_rate = sampleRate;
        cfg.fft_size = fftSize;
        cfg.n_mics = _nchannels;
        cfg.mic_xyz = xyz.data();
        cfg.alpha = alpha;
        cfg.loading = loading;
        cfg.max_streams = 1;
        const int rc = mca_hip_mvdr_create(&cfg, &_ctx);
        if (rc != MCA_HIP_OK) throw MCArrayException(std::string("mca_hip_mvdr_create: ") + mca_hip_mvdr_last_error(nullptr));
        _pending.assign(static_cast<size_t>(_nchannels), std::vector<float>());
    }
    virtual ~MvdrBeamformer() { mca_hip_mvdr_destroy(_ctx); }
    MvdrBeamformer(const MvdrBeamformer &) = delete;
    MvdrBeamformer &operator=(const MvdrBeamformer &) = delete;

    int getWindowSize() const { return _N; }
    int getFrameSize() const { return _N / 2; }
    int getMaxLatency() const { return _N; }
    int getNumberOfChannels() const { return _nchannels; }
    void setDOA(double doaRadians) { _doa = doaRadians; }      // look direction of the frames completed from now on
    // Several look directions per frame from the one covariance (mca_hip_mvdr_sources_frames_*): setMaxSources(1 ... 4) once,
    // then setDOAs() with up to that many directions and the process() overload with one output pointer per direction.
    void setMaxSources(int maxSources)
    {
        check(mca_hip_mvdr_set_max_sources(_ctx, maxSources));
        _maxSources = maxSources;
        if (static_cast<int>(_doas.size()) > maxSources) _doas.resize(static_cast<size_t>(maxSources));   // the directions that still fit
    }
    void setDOAs(const std::vector<double> &doasRadians)
    {
        if (doasRadians.empty() || static_cast<int>(doasRadians.size()) > _maxSources)
            throw MCArrayException("setDOAs: between 1 and the setMaxSources() maximum of look directions");
        _doas = doasRadians;
    }
    // Soft nulls at the other look directions of setDOAs() (mca_hip_mvdr_set_null_gain: finite, 0 ... 1000; 0, the default, is
    // the plain MVDR output).  Applies to the frames completed from now on; no part of the stream's state.
    void setNullGain(double nullGain) { check(mca_hip_mvdr_set_null_gain(_ctx, nullGain)); }
    // Covariance update weight of the frames completed from now on (mca_hip_mvdr_sources_frames_weighted_*): 1, the default,
    // learns as usual; 0 leaves the covariance as it is and beamforms with it (e.g. while a voice-activity decision says that the
    // target talks: a noise-only covariance); values between scale the step 1 - alpha.  Clamped to [0, 1], NaN counts as 0.
    // Both process() overloads honour it; no part of the stream's state.
    void setUpdateWeight(double updateWeight) { _update = updateWeight; }
    double getUpdateWeight() const { return _update; }
    // The frames the next process() chunk of nSamples samples per channel will complete: the rows of the updateMask it may carry.
    int framesCompletedBy(int nSamples) const
    {
        const long have = static_cast<long>(_pending[0].size()) + (nSamples > 0 ? nSamples : 0);
        return have >= _N ? static_cast<int>((have - _N) / (_N / 2) + 1) : 0;
    }
    double getNullGain() const
    {
        double g = 0.0;
        check(mca_hip_mvdr_get_null_gain(_ctx, &g));
        return g;
    }
    // Soft nulls at ESTIMATED steering vectors (mca_hip_mvdr_set_rtf_nulls): processRtf(), and processAuto() with setRtf() enabled,
    // honour setNullGain() with the nulls at the vectors the frame itself uses for the other look directions.  Off by default, and
    // then those calls refuse a non-zero null gain.  May change between chunks; no part of the stream's state.
    void setRtfNulls(bool enable) { check(mca_hip_mvdr_set_rtf_nulls(_ctx, enable ? 1 : 0)); }
    bool getRtfNulls() const
    {
        int e = 0;
        check(mca_hip_mvdr_get_rtf_nulls(_ctx, &e));
        return e != 0;
    }
    // The geometry of the steering vectors (mca_hip_mvdr_set_geometry).  MCA_HIP_MVDR_GEOMETRY_LINEAR_X, the default: the x coordinates
    // of the ArrayDescription alone (Beamformer.cpp:59).  MCA_HIP_MVDR_GEOMETRY_XYZ: all three coordinates; every look direction is an
    // azimuth round the whole circle (0: +y, +pi/2: +x) at the one elevation given here, in [-pi/2, pi/2].  A call that changes mode or
    // elevation un-configures the spectrum, the map and the tracks: configureSpectrum(), configureMap() and configureTracks() anew.  No part of the stream's state.
    void setGeometry(int mode, double elevationRad = 0.0)
    {
        mca_hip_mvdr_geometry_config before, cfg;
        check(mca_hip_mvdr_get_geometry(_ctx, &before));
        cfg.struct_size = static_cast<int>(sizeof(cfg));
        cfg.mode = mode;
        cfg.elevation_rad = elevationRad;
        check(mca_hip_mvdr_set_geometry(_ctx, &cfg));
        check(mca_hip_mvdr_get_geometry(_ctx, &cfg));
        if (cfg.mode != before.mode || cfg.elevation_rad != before.elevation_rad) { _nAngles = 0; _nPeaks = 0; _nAz = 0; _nEl = 0; _nMapPeaks = 0; _nTracks = 0; _follow = false; }
    }
    void getGeometry(int &mode, double &elevationRad) const
    {
        mca_hip_mvdr_geometry_config cfg;
        check(mca_hip_mvdr_get_geometry(_ctx, &cfg));
        mode = cfg.mode;
        elevationRad = cfg.elevation_rad;
    }
    // The decision-directed Wiener post-filter on the outputs of both process() overloads (mca_hip_mvdr_set_postfilter): smoothing in
    // [0, 1), gainFloor in [0, 1], noiseScale in (0, 100].  Enabling starts the filter's state from zero, disabling frees it; the three
    // values may change between chunks without touching that state.
    void setPostFilter(bool enable, double smoothing = 0.98, double gainFloor = 0.1, double noiseScale = 1.0)
    {
        mca_hip_mvdr_postfilter_config cfg;
        cfg.struct_size = static_cast<int>(sizeof(cfg));
        cfg.enable = enable ? 1 : 0;
        cfg.smoothing = smoothing;
        cfg.gain_floor = gainFloor;
        cfg.noise_scale = noiseScale;
        check(mca_hip_mvdr_set_postfilter(_ctx, &cfg));
    }
    void getPostFilter(bool &enable, double &smoothing, double &gainFloor, double &noiseScale) const
    {
        mca_hip_mvdr_postfilter_config cfg;
        check(mca_hip_mvdr_get_postfilter(_ctx, &cfg));
        enable = cfg.enable != 0;
        smoothing = cfg.smoothing;
        gainFloor = cfg.gain_floor;
        noiseScale = cfg.noise_scale;
    }
    // Steering vectors estimated from the data (mca_hip_mvdr_set_rtf): a second covariance over the cells of a target mask, and its
    // dominant direction beside the noise covariance as the relative transfer function towards microphone refMic.  targetAlpha in
    // [0, 1) (negative: keep the value the context holds, its alpha at first), iterations 1 ... 4, refMic 0 ... M - 1, minShare in
    // [0, 1).  Enabling allocates the target covariances (zero), disabling frees them.  The processRtf() calls use it.
    void setRtf(bool enable, double targetAlpha = -1.0, int iterations = 2, int refMic = 0, double minShare = 0.05)
    {
        mca_hip_mvdr_rtf_config cfg;
        check(mca_hip_mvdr_get_rtf(_ctx, &cfg));
        cfg.struct_size = static_cast<int>(sizeof(cfg));
        cfg.enable = enable ? 1 : 0;
        if (targetAlpha >= 0.0) cfg.target_alpha = targetAlpha;
        cfg.iterations = iterations;
        cfg.ref_mic = refMic;
        cfg.min_share = minShare;
        check(mca_hip_mvdr_set_rtf(_ctx, &cfg));
    }
    // the steering vectors a frame with look direction doaRadians would take from the held state (mca_hip_mvdr_get_steering):
    // d [N/2+1][M] complex as (re, im) pairs of doubles, estimated [N/2+1] (1: the RTF, 0: the geometric vector)
    void steering(double doaRadians, std::vector<double> &d, std::vector<unsigned char> &estimated, int source = 0)
    {
        d.resize(static_cast<size_t>(_N / 2 + 1) * static_cast<size_t>(_nchannels) * 2);
        estimated.resize(static_cast<size_t>(_N / 2 + 1));
        check(mca_hip_mvdr_get_steering(_ctx, 0, source, doaRadians, d.data(), estimated.data()));
    }
    // Masks estimated on the device from the chunk's own spectra (mca_hip_mvdr_set_mask_estimator): every cell goes to the look
    // direction of setDOA() / setDOAs() whose steering vector explains it best, and the winner's steered coherence between
    // coherenceLo and coherenceHi becomes its target mask; the first nProtected directions (0: all) close the noise covariance where
    // they win, the others are competitors.  The band of bins [binLo, binHi] (-1: N/2); outside it the plain recursion.  A single
    // look direction needs absolute thresholds such as 0.2 / 0.4.  The processAuto() calls use it; it holds no state.
    void setMaskEstimator(bool enable, int binLo = 0, int binHi = -1, double coherenceLo = 0.0, double coherenceHi = 0.05, int nProtected = 0)
    {
        mca_hip_mvdr_estmask_config cfg;
        cfg.struct_size = static_cast<int>(sizeof(cfg));
        cfg.enable = enable ? 1 : 0;
        cfg.bin_lo = binLo;
        cfg.bin_hi = binHi < 0 ? _N / 2 : binHi;
        cfg.coherence_lo = coherenceLo;
        cfg.coherence_hi = coherenceHi;
        cfg.n_protected = nProtected;
        check(mca_hip_mvdr_set_mask_estimator(_ctx, &cfg));
    }
    void getMaskEstimator(bool &enable, int &binLo, int &binHi, double &coherenceLo, double &coherenceHi, int &nProtected) const
    {
        mca_hip_mvdr_estmask_config cfg;
        check(mca_hip_mvdr_get_mask_estimator(_ctx, &cfg));
        enable = cfg.enable != 0;
        binLo = cfg.bin_lo;
        binHi = cfg.bin_hi;
        coherenceLo = cfg.coherence_lo;
        coherenceHi = cfg.coherence_hi;
        nProtected = cfg.n_protected;
    }
    // The Capon spatial spectrum of the covariance the stream holds, and its peaks (mca_hip_mvdr_spectrum_*): nAngles 2 ... 361 from
    // -pi/2 to pi/2, the band of bins [binLo, binHi], weighting MCA_HIP_MVDR_SPECTRUM_POWER / _NORMALISED, nPeaks 1 ... 4.  The peak
    // angles are look directions as setDOAs() takes them: process a chunk, read peaks(), setDOAs() for the next chunk.
    void configureSpectrum(int nAngles, int binLo, int binHi, int weighting = MCA_HIP_MVDR_SPECTRUM_NORMALISED, int nPeaks = 1)
    {
        mca_hip_mvdr_spectrum_config cfg;
        cfg.struct_size = static_cast<int>(sizeof(cfg));
        cfg.n_angles = nAngles;
        cfg.bin_lo = binLo;
        cfg.bin_hi = binHi;
        cfg.weighting = weighting;
        cfg.n_peaks = nPeaks;
        check(mca_hip_mvdr_spectrum_configure(_ctx, &cfg));
        _nAngles = nAngles;
        _nPeaks = nPeaks;
    }
    std::vector<double> spectrumGrid() const                   // the grid's angles (radians)
    {
        if (_nAngles == 0) throw MCArrayException("spectrumGrid: configureSpectrum() first");
        std::vector<float> g(static_cast<size_t>(_nAngles));
        check(mca_hip_mvdr_spectrum_get_grid(_ctx, g.data()));
        return std::vector<double>(g.begin(), g.end());
    }
    void spectrum(std::vector<double> &values)                 // [nAngles]
    {
        if (_nAngles == 0) throw MCArrayException("spectrum: configureSpectrum() first");
        std::vector<float> s(static_cast<size_t>(_nAngles));
        check(mca_hip_mvdr_spectrum_host(_ctx, 1, s.data(), nullptr, nullptr));
        values.assign(s.begin(), s.end());
    }
    void peaks(std::vector<double> &doaRadians, std::vector<double> &values)   // [nPeaks] each, ranked by value
    {
        if (_nAngles == 0) throw MCArrayException("peaks: configureSpectrum() first");
        std::vector<float> d(static_cast<size_t>(_nPeaks)), v(static_cast<size_t>(_nPeaks));
        check(mca_hip_mvdr_spectrum_host(_ctx, 1, nullptr, d.data(), v.data()));
        doaRadians.assign(d.begin(), d.end());
        values.assign(v.begin(), v.end());
    }
    // The Capon spectrum on a grid of azimuths x elevations and its peaks (mca_hip_mvdr_map_*; XYZ geometry only): nAz 3 ... 360
    // azimuths round the circle, nEl 1 ... 91 elevations from elLoRad to elHiRad (nEl == 1: both equal), nAz nEl <= 2048; band,
    // weighting and nPeaks as configureSpectrum().  mapPeaks(): azimuths as setDOAs() takes them, and the elevation of each.
    void configureMap(int nAz, int nEl, double elLoRad, double elHiRad, int binLo, int binHi, int weighting = MCA_HIP_MVDR_SPECTRUM_NORMALISED,
                      int nPeaks = 1)
    {
        mca_hip_mvdr_map_config cfg;
        cfg.struct_size = static_cast<int>(sizeof(cfg));
        cfg.n_az = nAz;
        cfg.n_el = nEl;
        cfg.el_lo_rad = elLoRad;
        cfg.el_hi_rad = elHiRad;
        cfg.bin_lo = binLo;
        cfg.bin_hi = binHi;
        cfg.weighting = weighting;
        cfg.n_peaks = nPeaks;
        check(mca_hip_mvdr_map_configure(_ctx, &cfg));
        _nAz = nAz;
        _nEl = nEl;
        _nMapPeaks = nPeaks;
    }
    void mapGrid(std::vector<double> &azRadians, std::vector<double> &elRadians) const   // [nAz], [nEl]
    {
        if (_nAz == 0) throw MCArrayException("mapGrid: configureMap() first");
        std::vector<float> a(static_cast<size_t>(_nAz)), e(static_cast<size_t>(_nEl));
        check(mca_hip_mvdr_map_get_grid(_ctx, a.data(), e.data()));
        azRadians.assign(a.begin(), a.end());
        elRadians.assign(e.begin(), e.end());
    }
    void map(std::vector<double> &values)                      // [nEl][nAz]
    {
        if (_nAz == 0) throw MCArrayException("map: configureMap() first");
        std::vector<float> m(static_cast<size_t>(_nAz) * static_cast<size_t>(_nEl));
        check(mca_hip_mvdr_map_host(_ctx, 1, m.data(), nullptr, nullptr, nullptr));
        values.assign(m.begin(), m.end());
    }
    void mapPeaks(std::vector<double> &azRadians, std::vector<double> &elRadians, std::vector<double> &values)   // [nPeaks] each, ranked by value
    {
        if (_nAz == 0) throw MCArrayException("mapPeaks: configureMap() first");
        const size_t n = static_cast<size_t>(_nMapPeaks);
        std::vector<float> a(n), e(n), v(n);
        check(mca_hip_mvdr_map_host(_ctx, 1, nullptr, a.data(), e.data(), v.data()));
        azRadians.assign(a.begin(), a.end());
        elRadians.assign(e.begin(), e.end());
        values.assign(v.begin(), v.end());
    }
    // An elevation per look direction (mca_hip_mvdr_set_elevations_host; XYZ geometry): one value per slot of setDOAs(), radians within
    // +-pi/2, NaN for the elevation of setGeometry(); slots beyond the vector are NaN.  mapPeaks() gives the values: setDOAs(az),
    // setElevations(el).  Kept across reset(); a geometry change and configureTracks() reset it, and setting it disables the tracks.
    void setElevations(const std::vector<double> &elevationsRadians)
    {
        if (static_cast<int>(elevationsRadians.size()) > _maxSources) throw MCArrayException("setElevations: more values than maxSources");
        std::vector<float> e(static_cast<size_t>(_maxSources), std::numeric_limits<float>::quiet_NaN());
        for (size_t i = 0; i < elevationsRadians.size(); ++i) e[i] = static_cast<float>(elevationsRadians[i]);
        check(mca_hip_mvdr_set_elevations_host(_ctx, 1, e.data()));
        _nTracks = 0;
        _follow = false;
    }
    // Tracks of the look directions, kept on the device between chunks (mca_hip_mvdr_tracks_*): nTracks 1 ... maxSources slots, of which
    // the first nOwn follow their own target covariance (setRtf(true) first) and the others the Capon peaks (configureSpectrum()
    // first), associated by angle with birth and release.  seedTracks(): one direction per slot, NaN leaves the slot.  Per chunk:
    // process, updateTracks().  tracks(): the look directions as the next chunk would take them (a dead slot repeats the lowest alive
    // one) and which slots are alive.  followTracks(true): the overloads of process(), processRtf() and processAuto() with several
    // outputs take their look directions from the tracks (mca_hip_mvdr_tracks_fill_*) instead of from setDOAs(), one output per slot.
    void configureTracks(int nTracks, int nOwn = 0, double maxStepRadians = 0.2, double minSepRadians = 0.1, int hold = 3)
    {
        mca_hip_mvdr_tracks_config cfg;
        cfg.struct_size = static_cast<int>(sizeof(cfg));
        cfg.enable = 1;
        cfg.n_tracks = nTracks;
        cfg.n_own = nOwn;
        cfg.max_step_rad = maxStepRadians;
        cfg.min_sep_rad = minSepRadians;
        cfg.hold = hold;
        check(mca_hip_mvdr_tracks_configure(_ctx, &cfg));
        _nTracks = nTracks;
    }
    void seedTracks(const std::vector<double> &doasRadians)
    {
        if (static_cast<int>(doasRadians.size()) != _nTracks || _nTracks == 0) throw MCArrayException("seedTracks: one direction per slot of configureTracks()");
        std::vector<float> d(doasRadians.begin(), doasRadians.end());
        check(mca_hip_mvdr_tracks_seed_host(_ctx, 1, d.data()));
    }
    void updateTracks() { check(mca_hip_mvdr_tracks_update_host(_ctx, 1, nullptr, nullptr)); }
    void tracks(std::vector<double> &doasRadians, std::vector<int> &alive)
    {
        if (_nTracks == 0) throw MCArrayException("tracks: configureTracks() first");
        std::vector<float> d(static_cast<size_t>(_nTracks));
        alive.assign(static_cast<size_t>(_nTracks), 0);
        check(mca_hip_mvdr_tracks_fill_host(_ctx, 1, 1, d.data()));
        check(mca_hip_mvdr_tracks_get(_ctx, 1, nullptr, alive.data(), nullptr, nullptr));
        doasRadians.assign(d.begin(), d.end());
    }
    void followTracks(bool follow)
    {
        if (follow && _nTracks == 0) throw MCArrayException("followTracks: configureTracks() first");
        _follow = follow;
    }
    // Map mode of the tracks (mca_hip_mvdr_tracks_set_map; XYZ geometry, configureTracks() and configureMap() first): every slot holds
    // an azimuth and an elevation, the own tracks search a patch of the Capon map and the others follow its peaks, associated in both
    // angles.  seedTracksMap(): one (azimuth, elevation) per slot, NaN leaves the slot.  Per chunk: process, updateTracksMap().
    // tracksMap(): the directions as the next chunk would take them.  followTracks(true) works as above: in map mode the fill writes the
    // elevation of every slot beside its azimuth.  configureTracks() leaves map mode.
    void configureTracksMap(double maxStepElRadians, double minSepElRadians, bool enable = true)
    {
        mca_hip_mvdr_tracks_map_config cfg;
        cfg.struct_size = static_cast<int>(sizeof(cfg));
        cfg.enable = enable ? 1 : 0;
        cfg.max_step_el_rad = maxStepElRadians;
        cfg.min_sep_el_rad = minSepElRadians;
        check(mca_hip_mvdr_tracks_set_map(_ctx, &cfg));
    }
    void seedTracksMap(const std::vector<double> &azRadians, const std::vector<double> &elRadians)
    {
        if (static_cast<int>(azRadians.size()) != _nTracks || azRadians.size() != elRadians.size() || _nTracks == 0)
            throw MCArrayException("seedTracksMap: one azimuth and one elevation per slot of configureTracks()");
        std::vector<float> a(azRadians.begin(), azRadians.end()), e(elRadians.begin(), elRadians.end());
        check(mca_hip_mvdr_tracks_seed_map_host(_ctx, 1, a.data(), e.data()));
    }
    void updateTracksMap() { check(mca_hip_mvdr_tracks_update_map_host(_ctx, 1, nullptr, nullptr)); }
    void tracksMap(std::vector<double> &azRadians, std::vector<double> &elRadians, std::vector<int> &alive)
    {
        if (_nTracks == 0) throw MCArrayException("tracksMap: configureTracks() first");
        std::vector<float> a(static_cast<size_t>(_nTracks)), e(static_cast<size_t>(_nTracks));
        alive.assign(static_cast<size_t>(_nTracks), 0);
        check(mca_hip_mvdr_tracks_get_map(_ctx, 1, a.data(), e.data(), alive.data(), nullptr, nullptr));
        // a dead slot repeats the lowest alive one, as the fill does
        int first = -1;
        for (int s = _nTracks - 1; s >= 0; --s) first = alive[static_cast<size_t>(s)] ? s : first;
        azRadians.assign(static_cast<size_t>(_nTracks), 0.0);
        elRadians.assign(static_cast<size_t>(_nTracks), 0.0);
        for (int s = 0; s < _nTracks; ++s) {
            const int src = alive[static_cast<size_t>(s)] ? s : first;
            if (src >= 0) { azRadians[static_cast<size_t>(s)] = a[static_cast<size_t>(src)]; elRadians[static_cast<size_t>(s)] = e[static_cast<size_t>(src)]; }
        }
    }
    // the covariance the stream holds (mca_hip_mvdr_get_covariance): [N/2+1][M][M] complex as (re, im) pairs of doubles
    void covariance(std::vector<double> &phi)
    {
        phi.resize(static_cast<size_t>(_N / 2 + 1) * static_cast<size_t>(_nchannels) * static_cast<size_t>(_nchannels) * 2);
        check(mca_hip_mvdr_get_covariance(_ctx, 0, phi.data()));
    }
    void reset()
    {
        check(mca_hip_mvdr_reset(_ctx, nullptr));
        for (std::vector<float> &b : _pending) b.clear();
    }

    // chunked PCM in (one pointer per channel), beamformed PCM out; returns the samples written (a multiple of the hop).
    // updateMask: covariance update weights per frame and bin, [framesCompletedBy(nSamples)][N/2 + 1]
    // (mca_hip_mvdr_sources_frames_masked_*); it overrides setUpdateWeight() for this call.
    template <typename Tin, typename Tout>
    int process(const std::vector<Tin *> &in, int nSamples, Tout *out, int outSize, const float *updateMask = nullptr)
    {
        const int hop = _N / 2;
        const int F = pend(in, nSamples);
        if (F == 0) return 0;
        if (F * hop > outSize) throw MCArrayException("output buffer too small for the frames completed by this chunk");
        std::vector<float> pcm = frames(F);
        std::vector<float> doa(static_cast<size_t>(F), static_cast<float>(_doa)), audio(static_cast<size_t>(F) * static_cast<size_t>(hop));
        const std::vector<float> upd = weights(F);
        if (updateMask) check(mca_hip_mvdr_sources_frames_masked_host(_ctx, pcm.data(), 1, F, 1, doa.data(), updateMask, audio.data(), nullptr));
        else check(mca_hip_mvdr_sources_frames_weighted_host(_ctx, pcm.data(), 1, F, 1, doa.data(), upd.empty() ? nullptr : upd.data(), audio.data(), nullptr));
        for (int i = 0; i < F * hop; ++i) out[i] = static_cast<Tout>(audio[static_cast<size_t>(i)]);
        consume(F);
        return F * hop;
    }

    // the same for the look directions of setDOAs(): out[s] receives the output of direction s; returns the samples written per output.
    // A direction that a call leaves out (fewer directions than in the call before) restarts from silence.  updateMask as above (one
    // mask for all directions: they share the covariance).
    template <typename Tin, typename Tout>
    int process(const std::vector<Tin *> &in, int nSamples, const std::vector<Tout *> &out, int outSize, const float *updateMask = nullptr)
    {
        const int hop = _N / 2, S = _follow ? _nTracks : static_cast<int>(_doas.size());
        if (S == 0) throw MCArrayException("process: setDOAs() first");
        if (static_cast<int>(out.size()) < S) throw MCArrayException("process: one output pointer per look direction of setDOAs()");
        const int F = pend(in, nSamples);
        if (F == 0) return 0;
        if (F * hop > outSize) throw MCArrayException("output buffer too small for the frames completed by this chunk");
        std::vector<float> pcm = frames(F);
        std::vector<float> doa(static_cast<size_t>(F) * static_cast<size_t>(S)), audio(doa.size() * static_cast<size_t>(hop));
        lookDirections(F, S, doa);
        const std::vector<float> upd = weights(F);
        if (updateMask) check(mca_hip_mvdr_sources_frames_masked_host(_ctx, pcm.data(), 1, F, S, doa.data(), updateMask, audio.data(), nullptr));
        else check(mca_hip_mvdr_sources_frames_weighted_host(_ctx, pcm.data(), 1, F, S, doa.data(), upd.empty() ? nullptr : upd.data(), audio.data(), nullptr));
        for (int s = 0; s < S; ++s)
            for (int i = 0; i < F * hop; ++i) out[static_cast<size_t>(s)][i] = static_cast<Tout>(audio[static_cast<size_t>(s) * static_cast<size_t>(F * hop) + static_cast<size_t>(i)]);
        consume(F);
        return F * hop;
    }

    // process() with estimated steering vectors (setRtf(true) first; mca_hip_mvdr_sources_frames_rtf_*): targetMask
    // [look directions][framesCompletedBy(nSamples)][N/2 + 1], 1 where the cell holds that direction's target (nullptr: nothing is
    // learned, the held target covariance steers); updateMask as above (nullptr: all 1), usually 1 - max over the directions of
    // targetMask.  The output is the target as microphone refMic records it.
    template <typename Tin, typename Tout>
    int processRtf(const std::vector<Tin *> &in, int nSamples, Tout *out, int outSize, const float *updateMask, const float *targetMask)
    {
        const int hop = _N / 2;
        const int F = pend(in, nSamples);
        if (F == 0) return 0;
        if (F * hop > outSize) throw MCArrayException("output buffer too small for the frames completed by this chunk");
        std::vector<float> pcm = frames(F);
        std::vector<float> doa(static_cast<size_t>(F), static_cast<float>(_doa)), audio(static_cast<size_t>(F) * static_cast<size_t>(hop));
        check(mca_hip_mvdr_sources_frames_rtf_host(_ctx, pcm.data(), 1, F, 1, doa.data(), updateMask, targetMask, audio.data(), nullptr));
        for (int i = 0; i < F * hop; ++i) out[i] = static_cast<Tout>(audio[static_cast<size_t>(i)]);
        consume(F);
        return F * hop;
    }
    template <typename Tin, typename Tout>
    int processRtf(const std::vector<Tin *> &in, int nSamples, const std::vector<Tout *> &out, int outSize, const float *updateMask, const float *targetMask)
    {
        const int hop = _N / 2, S = _follow ? _nTracks : static_cast<int>(_doas.size());
        if (S == 0) throw MCArrayException("processRtf: setDOAs() first");
        if (static_cast<int>(out.size()) < S) throw MCArrayException("processRtf: one output pointer per look direction of setDOAs()");
        const int F = pend(in, nSamples);
        if (F == 0) return 0;
        if (F * hop > outSize) throw MCArrayException("output buffer too small for the frames completed by this chunk");
        std::vector<float> pcm = frames(F);
        std::vector<float> doa(static_cast<size_t>(F) * static_cast<size_t>(S)), audio(doa.size() * static_cast<size_t>(hop));
        lookDirections(F, S, doa);
        check(mca_hip_mvdr_sources_frames_rtf_host(_ctx, pcm.data(), 1, F, S, doa.data(), updateMask, targetMask, audio.data(), nullptr));
        for (int s = 0; s < S; ++s)
            for (int i = 0; i < F * hop; ++i) out[static_cast<size_t>(s)][i] = static_cast<Tout>(audio[static_cast<size_t>(s) * static_cast<size_t>(F * hop) + static_cast<size_t>(i)]);
        consume(F);
        return F * hop;
    }

    // process() with masks estimated from the chunk's spectra (setMaskEstimator(true) first; mca_hip_mvdr_sources_frames_auto_*): with
    // setRtf(true) the call continues as processRtf() does with the two masks, else as process() does with the update mask.
    // updateMaskOut [framesCompletedBy(nSamples)][N/2 + 1] and targetMaskOut [look directions][framesCompletedBy(nSamples)][N/2 + 1]
    // receive the masks; either may be nullptr.
    template <typename Tin, typename Tout>
    int processAuto(const std::vector<Tin *> &in, int nSamples, Tout *out, int outSize, float *updateMaskOut = nullptr, float *targetMaskOut = nullptr)
    {
        const int hop = _N / 2;
        const int F = pend(in, nSamples);
        if (F == 0) return 0;
        if (F * hop > outSize) throw MCArrayException("output buffer too small for the frames completed by this chunk");
        std::vector<float> pcm = frames(F);
        std::vector<float> doa(static_cast<size_t>(F), static_cast<float>(_doa)), audio(static_cast<size_t>(F) * static_cast<size_t>(hop));
        check(mca_hip_mvdr_sources_frames_auto_host(_ctx, pcm.data(), 1, F, 1, doa.data(), updateMaskOut, targetMaskOut, audio.data(), nullptr));
        for (int i = 0; i < F * hop; ++i) out[i] = static_cast<Tout>(audio[static_cast<size_t>(i)]);
        consume(F);
        return F * hop;
    }
    template <typename Tin, typename Tout>
    int processAuto(const std::vector<Tin *> &in, int nSamples, const std::vector<Tout *> &out, int outSize, float *updateMaskOut = nullptr, float *targetMaskOut = nullptr)
    {
        const int hop = _N / 2, S = _follow ? _nTracks : static_cast<int>(_doas.size());
        if (S == 0) throw MCArrayException("processAuto: setDOAs() first");
        if (static_cast<int>(out.size()) < S) throw MCArrayException("processAuto: one output pointer per look direction of setDOAs()");
        const int F = pend(in, nSamples);
        if (F == 0) return 0;
        if (F * hop > outSize) throw MCArrayException("output buffer too small for the frames completed by this chunk");
        std::vector<float> pcm = frames(F);
        std::vector<float> doa(static_cast<size_t>(F) * static_cast<size_t>(S)), audio(doa.size() * static_cast<size_t>(hop));
        lookDirections(F, S, doa);
        check(mca_hip_mvdr_sources_frames_auto_host(_ctx, pcm.data(), 1, F, S, doa.data(), updateMaskOut, targetMaskOut, audio.data(), nullptr));
        for (int s = 0; s < S; ++s)
            for (int i = 0; i < F * hop; ++i) out[static_cast<size_t>(s)][i] = static_cast<Tout>(audio[static_cast<size_t>(s) * static_cast<size_t>(F * hop) + static_cast<size_t>(i)]);
        consume(F);
        return F * hop;
    }

private:
    // appends a chunk to the pending samples; returns the frames they complete
    template <typename Tin>
    int pend(const std::vector<Tin *> &in, int nSamples)
    {
        for (int c = 0; c < _nchannels; ++c) {
            std::vector<float> &buf = _pending[static_cast<size_t>(c)];
            const size_t old = buf.size();
            buf.resize(old + static_cast<size_t>(nSamples));
            for (int i = 0; i < nSamples; ++i) buf[old + static_cast<size_t>(i)] = static_cast<float>(in[static_cast<size_t>(c)][i]);
        }
        const int have = static_cast<int>(_pending[0].size());
        return have >= _N ? (have - _N) / (_N / 2) + 1 : 0;
    }
    std::vector<float> frames(int F) const      // [channel][(F + 1) hop]
    {
        const size_t L = static_cast<size_t>(F + 1) * static_cast<size_t>(_N / 2);
        std::vector<float> pcm(L * static_cast<size_t>(_nchannels));
        for (int c = 0; c < _nchannels; ++c)
            std::copy(_pending[static_cast<size_t>(c)].begin(), _pending[static_cast<size_t>(c)].begin() + static_cast<long>(L), pcm.begin() + static_cast<long>(L * static_cast<size_t>(c)));
        return pcm;
    }
    std::vector<float> weights(int F) const     // [F] update weights of a call, empty for the default (all 1: no weights passed)
    {
        return _update == 1.0 ? std::vector<float>() : std::vector<float>(static_cast<size_t>(F), static_cast<float>(_update));
    }
    // [F][S]: the directions of setDOAs(), or with followTracks(true) those of the tracks
    void lookDirections(int F, int S, std::vector<float> &doa)
    {
        if (_follow) { check(mca_hip_mvdr_tracks_fill_host(_ctx, 1, F, doa.data())); return; }
        for (int t = 0; t < F; ++t)
            for (int s = 0; s < S; ++s) doa[static_cast<size_t>(t * S + s)] = static_cast<float>(_doas[static_cast<size_t>(s)]);
    }
    void consume(int F)
    {
        for (int c = 0; c < _nchannels; ++c)
            _pending[static_cast<size_t>(c)].erase(_pending[static_cast<size_t>(c)].begin(), _pending[static_cast<size_t>(c)].begin() + static_cast<long>(F) * (_N / 2));
    }
    void check(int rc) const
    {
        if (rc != MCA_HIP_OK) throw MCArrayException(std::string("libmcarray_hip: ") + mca_hip_mvdr_last_error(_ctx));
    }
    int _nchannels, _N;
    double _doa = 0.0, _update = 1.0;
    int _maxSources = 1;
    int _nAngles = 0, _nPeaks = 0;
    int _nAz = 0, _nEl = 0, _nMapPeaks = 0;
    int _nTracks = 0;
    bool _follow = false;
    std::vector<double> _doas;
    mca_hip_mvdr_ctx *_ctx = nullptr;
    std::vector<std::vector<float> > _pending;
};

}  // namespace mca
#endif
