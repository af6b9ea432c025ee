// mca::FreqGCCBinauralLocalisation -- 2-microphone GCC-PHAT localiser, deterministic part of the reference class
// (include/mcarray/BinauralLocalisation.h:188-247; src/mcarray/BinauralLocalisation.cpp:320-631): smoothed
// correlation, first-max argmax, the author's DOA smoothing (#else branch :502-504), the per-frame DSPONE hook
// processParametrisation (:406-567) and setProbability at caller-given angles (:569-631, the weights of the particle
// filter's observation model).  The particle filter the reference is compiled with (:38, :456-473, :536-558) is opt-in:
// useParticleFilter() attaches the DOA tracker of mcarray_hip.h (mca_hip_gcc2_tracker_attach; DSPONE's filter engine is
// not available, DESIGN.md "The DOA tracker" defines ours), and then _currentDOA is the filter's estimate, the callback also
// fires while a track coasts through a pause, and getSourceCounter() counts the tracks.  Without it the class is unchanged.
//
// Two ways in, each with its own state on the GPU: process() (chunked PCM, the batched stream path, float) and
// processParametrisation() (one frame of CCS spectra, double).  An object driven through both keeps two states;
// setProbability reads the one of the path the object used last.
//
// mca::TemporalGCCBinauralLocalisation -- the time-domain 2-microphone localiser of the same reference header
// (BinauralLocalisation.h:43-185; BinauralLocalisation.cpp:66-314): nd delay pairs, each a (2 nd + 1)-lag cross-correlation
// of the raw frame, the first maximum of the normalised index -> DOA in degrees, the power gate, and
// _currentDOA = 0.5 _currentDOA + 0.5 DOA.  The same two ways in (process(): float PCM, batched; processParametrisation():
// one frame of doubles), each with its own state.  setProbability stays the base class's uniform value, as in the reference.
#ifndef MCA_HIP_BINAURALLOCALISATION_H
#define MCA_HIP_BINAURALLOCALISATION_H
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "mcadefs.h"

#include "../mcarray_hip.h"
#include "HipContext.h"
#include "SoundLocalisationImpl.h"
#include "microhponeArrayHelpers.h"

namespace mca {

class TemporalGCCBinauralLocalisation : public SoundLocalisationImpl {
public:
    // usePowerFloor = false (an extension, as FreqGCCBinauralLocalisation's flag): every frame passes the gate, power = logPower
    TemporalGCCBinauralLocalisation(int sampleRate, ArrayDescription microphonePositions, bool usePowerFloor = true)
        : SoundLocalisationImpl(microphonePositions)
    {
        if (microphonePositions.size() != 2) throw MCArrayException("TemporalGCCBinauralLocalisation needs an ArrayDescription with 2 microphones");
        std::vector<double> xyz = microphonePositions.xyz();
        mca_hip_tgcc_config cfg = mca_hip_tgcc_config();
        cfg.struct_size = static_cast<int>(sizeof(cfg));
        cfg.device = 0;
        cfg.sample_rate = sampleRate;
        for (int j = 0; j < 6; ++j) cfg.mic_xyz[j / 3][j % 3] = xyz[static_cast<size_t>(j)];
        cfg.use_power_floor = usePowerFloor ? 1 : 0;
        cfg.max_arrays = 1;
        if (mca_hip_tgcc_create(&cfg, &_ctx) != MCA_HIP_OK) throw MCArrayException(std::string("mca_hip_tgcc_create: ") + mca_hip_tgcc_last_error(nullptr));
        check(mca_hip_tgcc_get_geometry(_ctx, &_windowSize, &_hop, &_ndelays));
        _currentDOA.reset(new BaseType[1]);
        _prob.reset(new BaseType[1]);
        _currentDOA[0] = 0; _prob[0] = -1;                   // BinauralLocalisation.cpp:86-89
    }
    virtual ~TemporalGCCBinauralLocalisation() { mca_hip_tgcc_destroy(_ctx); }
    TemporalGCCBinauralLocalisation(const TemporalGCCBinauralLocalisation &) = delete;
    TemporalGCCBinauralLocalisation &operator=(const TemporalGCCBinauralLocalisation &) = delete;

    int getWindowSize() const { return _windowSize; }
    int getAnalysisLength() const { return _windowSize; }
    int getNumberOfDelays() const { return _ndelays; }
    int getNumberOfChannels() const { return 2; }

    // chunked PCM in (2 channels); fires setDOA(degrees, prob, power, 1) once per completed frame that passes the gate
    // (BinauralLocalisation.cpp:189-190).  Returns the number of frames completed by this chunk.
    template <typename Tin> int process(const std::vector<Tin *> &in, int nSamples)
    {
        const int W = _windowSize, hop = _hop;
        for (int c = 0; c < 2; ++c)
            for (int i = 0; i < nSamples; ++i) _pending[c].push_back(static_cast<float>(in[static_cast<size_t>(c)][i]));
        const int have = static_cast<int>(_pending[0].size());
        const int F = have >= W ? (have - W) / hop + 1 : 0;
        if (F == 0) return 0;
        const size_t L = static_cast<size_t>(F - 1) * static_cast<size_t>(hop) + static_cast<size_t>(W);
        std::vector<float> pcm(2 * L), doa(static_cast<size_t>(F)), prob(static_cast<size_t>(F)), power(static_cast<size_t>(F));
        std::vector<unsigned char> voiced(static_cast<size_t>(F));
        for (int c = 0; c < 2; ++c) std::copy(_pending[c].begin(), _pending[c].begin() + static_cast<long>(L), pcm.begin() + static_cast<long>(L) * c);
        check(mca_hip_tgcc_frames_host(_ctx, pcm.data(), 1, F, doa.data(), prob.data(), voiced.data(), power.data(), nullptr, nullptr));
        for (int t = 0; t < F; ++t) {
            _currentDOA[0] = doa[static_cast<size_t>(t)]; _prob[0] = prob[static_cast<size_t>(t)];
            if (voiced[static_cast<size_t>(t)] && _ptrCallback) _ptrCallback->setDOA(_currentDOA, _prob, power[static_cast<size_t>(t)], 1);
        }
        for (int c = 0; c < 2; ++c) _pending[c].erase(_pending[c].begin(), _pending[c].begin() + static_cast<long>(F) * hop);
        return F;
    }

    // the SignalVector / SignalVector16s overloads the reference's callers use (test_mcarray.cpp:618; mcadefs.h:86-88)
    int process(const SignalVector &in, int nSamples)
    {
        std::vector<const BaseType *> pi;
        for (size_t c = 0; c < in.size(); ++c) pi.push_back(in[c].get());
        return process(pi, nSamples);
    }
    int process(const SignalVector16s &in, int nSamples)
    {
        std::vector<const BaseType16s *> pi;
        for (size_t c = 0; c < in.size(); ++c) pi.push_back(in[c].get());
        return process(pi, nSamples);
    }

    // The per-frame hook (BinauralLocalisation.cpp:134-192): analysisFrames[0..1] = the raw frames, double[analysisLength]
    // (not modified).  The state advances on every frame; setDOA(degrees, prob, power, 1) fires on a voiced frame when a
    // callback is set (the reference would dereference a null one).
    virtual void processParametrisation(std::vector<double *> &analysisFrames, int analysisLength, std::vector<double *> &dataChannels,
                                        int dataLength)
    {
        (void)dataChannels; (void)dataLength;
        if (analysisLength != getAnalysisLength()) throw MCArrayException("analysisLength does not match the module's window size");
        if (analysisFrames.size() < 2) throw MCArrayException("processParametrisation needs 2 analysis frames");
        const double *fr[2] = {analysisFrames[0], analysisFrames[1]};
        int voiced = 0;
        double doa = 0, prob = 0, power = 0;
        check(mca_hip_tgcc_process_frame(_ctx, fr, analysisLength, &voiced, &doa, &prob, &power, nullptr, nullptr));
        _currentDOA[0] = doa; _prob[0] = prob;
        if (voiced && _ptrCallback) _ptrCallback->setDOA(_currentDOA, _prob, power, 1);
    }

private:
    void check(int rc) const
    {
        if (rc != MCA_HIP_OK) throw MCArrayException(std::string("libmcarray_hip: ") + mca_hip_tgcc_last_error(_ctx));
    }
    mca_hip_tgcc_ctx *_ctx = nullptr;
    int _windowSize = 0, _hop = 0, _ndelays = 0;
    std::vector<float> _pending[2];
};

class FreqGCCBinauralLocalisation : public SoundLocalisationImpl {
public:
    FreqGCCBinauralLocalisation(int sampleRate, ArrayDescription microphonePositions, bool usePowerFloor = true, double doaStepDeg = 3.0)
        : SoundLocalisationImpl(microphonePositions), _order(calculateOrderFromSampleRate(sampleRate, _frameRate))
    {
        if (microphonePositions.size() != 2) throw MCArrayException("FreqGCCBinauralLocalisation needs an ArrayDescription with 2 microphones");
        _usePowerFloor = usePowerFloor;
        _ctx.reset(new detail::HipContext(sampleRate, microphonePositions, 1 << _order, doaStepDeg, 1, usePowerFloor));
        _currentDOA.reset(new BaseType[1]);
        _prob.reset(new BaseType[1]);
        _currentDOA[0] = 0; _prob[0] = -1;                   // BinauralLocalisation.cpp:339-340
    }
    static int calculateOrderFromSampleRate(int sampleRate, double frameSeconds)
    {
        int order = static_cast<int>(std::lround(std::log2(sampleRate * frameSeconds)));
        return order < 8 ? 8 : (order > 14 ? 14 : order);
    }
    int getFrameSize() const { return 1 << (_order - 1); }
    int getWindowSize() const { return 1 << _order; }
    int getAnalysisLength() const { return (1 << _order) + 2; }
    int getOneSidedFFTLength() const { return (1 << (_order - 1)) + 1; }
    int getMaxLatency() const { return 1 << _order; }
    int getNumberOfChannels() const { return 2; }

    // Not in the reference (which is compiled with the filter, BinauralLocalisation.cpp:38): switch the DOA from the #else
    // branch's smoothing to the particle filter.  Call before the first frame, once.  nInject: particles re-drawn uniformly per
    // update (0 = nParticles / 20, -1 = none); sigmaInit / sigmaStep in radians (0 = the grid step).
    void useParticleFilter(unsigned long long seed = 0, int nParticles = 500, int nInject = 0, double sigmaInit = 0.0, double sigmaStep = 0.0)
    {
        mca_hip_gcc2_tracker_config cfg = mca_hip_gcc2_tracker_config();
        cfg.struct_size = static_cast<int>(sizeof(cfg));
        cfg.n_particles = nParticles; cfg.n_inject = nInject; cfg.seed = seed;
        cfg.sigma_init = sigmaInit; cfg.sigma_step = sigmaStep;
        _ctx->check(mca_hip_gcc2_tracker_attach(_ctx->get(), &cfg));
        _tracked = true;
    }
    bool usesParticleFilter() const { return _tracked; }
    // _sourceCounter (BinauralLocalisation.cpp:458): the number of the current or last track of the path used last; 0 without a filter
    int getSourceCounter() const { return _sourceCounter; }

    // chunked PCM in (2 channels); fires the callback once per completed frame: setDOA(degrees, prob, power, 1) (:521)
    template <typename Tin> int process(const std::vector<Tin *> &in, int nSamples)
    {
        if (_tracked) return processTracked(in, nSamples);
        const int N = getWindowSize(), hop = N / 2;
        for (int c = 0; c < 2; ++c)
            for (int i = 0; i < nSamples; ++i) _pending[c].push_back(static_cast<float>(in[static_cast<size_t>(c)][i]));
        const int have = static_cast<int>(_pending[0].size());
        const int F = have >= N ? (have - N) / hop + 1 : 0;
        if (F == 0) return 0;
        const size_t L = static_cast<size_t>(F + 1) * static_cast<size_t>(hop);
        std::vector<float> pcm(2 * L), doa(static_cast<size_t>(F)), prob(static_cast<size_t>(F));
        std::vector<int> idx(static_cast<size_t>(F));
        for (int c = 0; c < 2; ++c) std::copy(_pending[c].begin(), _pending[c].begin() + static_cast<long>(L), pcm.begin() + static_cast<long>(L) * c);
        _ctx->check(mca_hip_gcc2_frames_host(_ctx->get(), pcm.data(), 1, F, idx.data(), doa.data(), prob.data(), nullptr));
        _framePathLast = false;
        std::vector<unsigned char> voiced(static_cast<size_t>(F), 1);
        std::vector<float> power(static_cast<size_t>(F), 0.f);
        if (_usePowerFloor) _ctx->check(mca_hip_copy_gate(_ctx->get(), voiced.data(), power.data()));
        for (int t = 0; t < F; ++t) {
            if (!voiced[static_cast<size_t>(t)]) continue;       // gated out: the block of BinauralLocalisation.cpp:434 is skipped, no setDOA
            _currentDOA[0] = doa[static_cast<size_t>(t)]; _prob[0] = prob[static_cast<size_t>(t)];
            if (_ptrCallback) _ptrCallback->setDOA(toDegrees(_currentDOA, 1), _prob, static_cast<double>(power[static_cast<size_t>(t)]), 1);
        }
        for (int c = 0; c < 2; ++c) _pending[c].erase(_pending[c].begin(), _pending[c].begin() + static_cast<long>(F) * hop);
        _lastArgmax = idx;
        return F;
    }
    const std::vector<int> &lastArgmax() const { return _lastArgmax; }

    // The DSPONE per-frame hook (BinauralLocalisation.cpp:406-567): analysisFrames[0..1] = CCS spectra double[analysisLength]
    // (not modified).  Like the reference it computes nothing when no callback is set (:410-414).  On a frame that passes the
    // gate it updates _currentDOA / _prob and fires setDOA(degrees, prob, power, 1) (:521).
    virtual void processParametrisation(std::vector<double *> &analysisFrames, int analysisLength, std::vector<double *> &dataChannels,
                                        int dataLength)
    {
        (void)dataChannels; (void)dataLength;
        if (!_ptrCallback) return;
        if (analysisLength != getAnalysisLength()) throw MCArrayException("analysisLength does not match the module's FFT size");
        if (analysisFrames.size() < 2) throw MCArrayException("processParametrisation needs 2 analysis frames");
        const double *fr[2] = {analysisFrames[0], analysisFrames[1]};
        int voiced = 0;
        double doa = 0, prob = 0, power = 0;
        _ctx->check(mca_hip_gcc2_process_frame(_ctx->get(), fr, analysisLength, &voiced, &doa, &prob, &power, nullptr, nullptr));
        _framePathLast = true;
        if (_tracked) _ctx->check(mca_hip_gcc2_tracker_get_particles(_ctx->get(), -1, nullptr, nullptr, &_sourceCounter));
        if (!voiced) return;                                     // (with the filter: fired, 1 voiced or 2 a coasting track, :545-548)
        _currentDOA[0] = doa; _prob[0] = prob;
        _ptrCallback->setDOA(toDegrees(_currentDOA, 1), _prob, power, 1);
    }

    // setProbability (BinauralLocalisation.cpp:569-631) at caller-given angles in radians, on the smoothed correlation of the
    // path used last: processParametrisation's, or else process()'s.  Zeros before any frame has fired.
    void setProbability(const double *doas, double *probs, int size) override
    {
        if (_framePathLast) _ctx->check(mca_hip_gcc2_frame_set_probability(_ctx->get(), doas, probs, size));
        else _ctx->check(mca_hip_gcc2_set_probability(_ctx->get(), 0, doas, probs, size));
    }

    // the SignalVector / SignalVector16s overloads the reference's callers use (test_mcarray.cpp:618; mcadefs.h:86-88)
    int process(const SignalVector &in, int nSamples)
    {
        std::vector<const BaseType *> pi;
        for (size_t c = 0; c < in.size(); ++c) pi.push_back(in[c].get());
        return process(pi, nSamples);
    }
    int process(const SignalVector16s &in, int nSamples)
    {
        std::vector<const BaseType16s *> pi;
        for (size_t c = 0; c < in.size(); ++c) pi.push_back(in[c].get());
        return process(pi, nSamples);
    }

private:
    // process() with the particle filter: setDOA on every frame whose fired is 1 (voiced, :521) or 2 (coasting, :548)
    template <typename Tin> int processTracked(const std::vector<Tin *> &in, int nSamples)
    {
        const int N = getWindowSize(), hop = N / 2;
        for (int c = 0; c < 2; ++c)
            for (int i = 0; i < nSamples; ++i) _pending[c].push_back(static_cast<float>(in[static_cast<size_t>(c)][i]));
        const int have = static_cast<int>(_pending[0].size());
        const int F = have >= N ? (have - N) / hop + 1 : 0;
        if (F == 0) return 0;
        const size_t L = static_cast<size_t>(F + 1) * static_cast<size_t>(hop), nf = static_cast<size_t>(F);
        std::vector<float> pcm(2 * L), doa(nf), prob(nf), power(nf, 0.f);
        std::vector<int> idx(nf), track(nf);
        std::vector<unsigned char> fired(nf);
        for (int c = 0; c < 2; ++c) std::copy(_pending[c].begin(), _pending[c].begin() + static_cast<long>(L), pcm.begin() + static_cast<long>(L) * c);
        _ctx->check(mca_hip_gcc2_tracked_frames_host(_ctx->get(), pcm.data(), 1, F, idx.data(), doa.data(), prob.data(), fired.data(),
                                                     track.data(), nullptr));
        _framePathLast = false;
        if (_usePowerFloor) _ctx->check(mca_hip_copy_gate(_ctx->get(), nullptr, power.data()));
        for (size_t t = 0; t < nf; ++t) {
            _sourceCounter = track[t];
            if (!fired[t]) continue;
            _currentDOA[0] = doa[t]; _prob[0] = prob[t];
            if (_ptrCallback) _ptrCallback->setDOA(toDegrees(_currentDOA, 1), _prob, static_cast<double>(power[t]), 1);
        }
        for (int c = 0; c < 2; ++c) _pending[c].erase(_pending[c].begin(), _pending[c].begin() + static_cast<long>(F) * hop);
        _lastArgmax = idx;
        return F;
    }

    static constexpr float _frameRate = 0.075f;      // BinauralLocalisation.h:196
    const int _order;
    bool _usePowerFloor = true;
    std::shared_ptr<detail::HipContext> _ctx;
    std::vector<float> _pending[2];
    std::vector<int> _lastArgmax;
    bool _framePathLast = false;       // processParametrisation ran after the last process() (setProbability reads its state)
    bool _tracked = false;             // useParticleFilter() was called
    int _sourceCounter = 0;
};

}  // namespace mca
#endif
