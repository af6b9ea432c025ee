// mca::BinauralMaskingImpl -- 2-channel spatial + temporal masking on a 45-band mel filter bank in the time domain
// (Kim, Kumar, Stern 2011, with a mel instead of a gammatone bank): the constructor, the MaskingMethod, the getters and
// the three hooks frameAnalysis / processParametrisation / frameSynthesis of the reference class
// (include/mcarray/BinauralMaskingImpl.h:67-135; src/mcarray/BinauralMaskingImpl.cpp:41-335).  The hooks run on the GPU in
// double (mca_hip_bmask_frame_analysis / _process_frame / _frame_synthesis); process() is the batched stream path
// (windowing, filter bank, masking, re-summation and overlap-add on the GPU in one call), the stand-in for the
// dsp::ShortTimeProcess::process() the reference inherits (test_mcarray.cpp:937,1023).  DESIGN.md section 2b has the definition.
#ifndef MCA_HIP_BINAURALMASKINGIMPL_H
#define MCA_HIP_BINAURALMASKINGIMPL_H
#include <cmath>
#include <string>
#include <vector>

#include "../mcarray_hip.h"
#include "mcadefs.h"
#include "mcarray_exception.h"

namespace mca {

class BinauralMaskingImpl {
public:
    // FACTOR: a masked band is divided by the spatial / temporal factor; RELATIVE: it is scaled by
    // sqrt(0.01 * its power / the band's short-time power), per channel; FULL: it is divided by 1000 (-60 dB)
    typedef enum { FACTOR = 0, RELATIVE = 1, FULL = 3 } MaskingMethod;

    BinauralMaskingImpl(int samplerate, double microDistance, float lowFreq, float highFreq, MaskingMethod mmethod = RELATIVE)
        : _microDistance(microDistance), _order(calculateOrderFromSampleRate(samplerate, _frameRate))
    {
        mca_hip_bmask_config cfg;
        cfg.struct_size = static_cast<int>(sizeof(cfg));
        cfg.device = 0;
        cfg.sample_rate = samplerate;
        cfg.frame_size = 1 << _order;
        cfg.micro_distance = microDistance;
        cfg.low_freq = lowFreq;
        cfg.high_freq = highFreq;
        cfg.method = static_cast<int>(mmethod);
        cfg.max_streams = 1;
        if (mca_hip_bmask_create(&cfg, &_ctx) != MCA_HIP_OK) throw MCArrayException(std::string("mca_hip_bmask_create: ") + mca_hip_bmask_last_error(nullptr));
    }
    virtual ~BinauralMaskingImpl() { mca_hip_bmask_destroy(_ctx); }
    BinauralMaskingImpl(const BinauralMaskingImpl &) = delete;
    BinauralMaskingImpl &operator=(const BinauralMaskingImpl &) = delete;

    static int calculateOrderFromSampleRate(int sampleRate, double frameSeconds)   // [BUILD-DEFINES], SURVEY A.1
    {
        int order = static_cast<int>(std::lround(std::log2(sampleRate * frameSeconds)));
        return order < 8 ? 8 : (order > 14 ? 14 : order);
    }
    int getWindowSize() const { return 1 << _order; }
    int getAnalysisLength() const { return (_nBins + 1) * (1 << _order); }   // the 45 bands and the residual (.h:93-95)
    int getFrameSize() const { return 1 << (_order - 1); }
    int getMaxLatency() const { return 1 << _order; }
    int getNumberOfChannels() const { return 2; }
    int getNonMaskingAngle() { return 10; }                                  // _phi in degrees
    float getMicroPhoneDistance() { return static_cast<float>(_microDistance); }
    float getSpatialMaskingFactor() { return 1 / _spatialMaskingFactor; }
    float getTemporalMaskingFactor() { return 1 / _temporalMaskingFactor; }

    // one windowed frame of `channel` -> its band signals: band b at analysis[b * frameLength], the residual in slot 45 when
    // analysisLength has room for it
    virtual void frameAnalysis(BaseType *inFrame, BaseType *analysis, int frameLength, int analysisLength, int channel)
    {
        checkChannel(channel);
        check(mca_hip_bmask_frame_analysis(_ctx, inFrame, analysis, frameLength, analysisLength, channel));
    }

    // the masking itself: the band signals of analysisFrames[0,1] are scaled in place
    virtual void processParametrisation(std::vector<double *> &analysisFrames, int analysisLength,
                                        std::vector<double *> &dataChannels, int dataLength)
    {
        (void)dataChannels; (void)dataLength;
        if (analysisFrames.size() != 2) throw MCArrayException("Sound localisation is only working for 2 channels by now.");   // .cpp:76-79
        check(mca_hip_bmask_process_frame(_ctx, analysisFrames[0], analysisFrames[1], analysisLength, nullptr));
    }

    // the bands summed again (the slots below analysisLength - frameLength, at most 46)
    virtual void frameSynthesis(BaseType *outFrame, BaseType *analysis, int frameLength, int analysisLength, int channel)
    {
        checkChannel(channel);
        check(mca_hip_bmask_frame_synthesis(_ctx, outFrame, analysis, frameLength, analysisLength, channel));
    }

    // chunked PCM in, masked PCM out (2 channels each); returns samples written per channel
    template <typename Tin, typename Tout>
    int process(const std::vector<Tin *> &in, int nSamples, const std::vector<Tout *> &out, int outSize)
    {
        if (in.size() != 2 || out.size() != 2) throw MCArrayException("Sound localisation is only working for 2 channels by now.");
        const int N = getWindowSize(), hop = N / 2;
        for (int c = 0; c < 2; ++c)
            for (int i = 0; i < nSamples; ++i) _pending[c].push_back(static_cast<float>(in[static_cast<size_t>(c)][i]));
        const int have = static_cast<int>(_pending[0].size());
        const int F = have >= N ? (have - N) / hop + 1 : 0;
        if (F == 0) return 0;
        if (F * hop > outSize) throw MCArrayException("output buffer too small for the frames completed by this chunk");
        const size_t L = static_cast<size_t>(F + 1) * static_cast<size_t>(hop);
        std::vector<float> pcm(2 * L), res(2 * static_cast<size_t>(F) * static_cast<size_t>(hop));
        for (int c = 0; c < 2; ++c) std::copy(_pending[c].begin(), _pending[c].begin() + static_cast<long>(L), pcm.begin() + static_cast<long>(L) * c);
        check(mca_hip_bmask_frames_host(_ctx, pcm.data(), 1, F, res.data(), nullptr));
        for (int c = 0; c < 2; ++c) {
            for (int i = 0; i < F * hop; ++i) out[static_cast<size_t>(c)][i] = static_cast<Tout>(res[static_cast<size_t>(c) * static_cast<size_t>(F) * static_cast<size_t>(hop) + static_cast<size_t>(i)]);
            _pending[c].erase(_pending[c].begin(), _pending[c].begin() + static_cast<long>(F) * hop);
        }
        return F * hop;
    }

    // the SignalVector / SignalVector16s overloads the reference's callers use (mcadefs.h)
    int process(const SignalVector &in, int nSamples, SignalVector &out, int outSize)
    {
        std::vector<const BaseType *> pi; std::vector<BaseType *> po;
        for (size_t c = 0; c < in.size(); ++c) pi.push_back(in[c].get());
        for (size_t c = 0; c < out.size(); ++c) po.push_back(out[c].get());
        return process(pi, nSamples, po, outSize);
    }
    int process(const SignalVector16s &in, int nSamples, SignalVector16s &out, int outSize)
    {
        std::vector<const BaseType16s *> pi; std::vector<BaseType16s *> po;
        for (size_t c = 0; c < in.size(); ++c) pi.push_back(in[c].get());
        for (size_t c = 0; c < out.size(); ++c) po.push_back(out[c].get());
        return process(pi, nSamples, po, outSize);
    }

private:
    void check(int rc) const { if (rc != MCA_HIP_OK) throw MCArrayException(std::string("libmcarray_hip: ") + mca_hip_bmask_last_error(_ctx)); }
    static void checkChannel(int channel) { if (channel < 0 || channel > 1) throw MCArrayException("Sound localisation is only working for 2 channels by now."); }
    static const int _nBins = 45;
    static constexpr float _frameRate = 0.050f;              // seconds: the window, its half is the shift
    static constexpr float _temporalMaskingFactor = 1;       // FACTOR: a temporally masked band is divided by this
    static constexpr float _spatialMaskingFactor = 1;        // and a spatially masked one by this
    const double _microDistance;
    const int _order;
    mca_hip_bmask_ctx *_ctx = nullptr;
    std::vector<float> _pending[2];
};

}  // namespace mca
#endif
