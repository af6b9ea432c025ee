/*
 * mcarray_hip.h -- C ABI of libmcarray_hip.so: the MI355X (gfx950) implementation of
 * mcarray's per-frame localisation + beamforming hot path.
 *
 * This is the drop-in boundary.  Plain pointers and sizes only; no C++
 * or torch types cross it.  Every entry point names the reference interface it
 * replaces (paths relative to the reference root, jordi-adell/mcarray v0.3.0-alpha).
 * The C++ classes in include/mcarray/ (same names and signatures as the reference's)
 * are thin callers of these functions; INTEGRATION.md shows the binding a reference
 * maintainer would add.
 *
 * Conventions
 *   - return value: 0 = MCA_HIP_OK, < 0 = error (mca_hip_status); the message is
 *     available from mca_hip_last_error().  The C++ wrappers rethrow it as
 *     mca::MCArrayException (include/mcarray/mcarray_exception.h:51 in the reference).
 *   - "_dev" pointers are device (HBM) pointers, work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the null stream) and the call does
 *     not synchronise.  Functions without "_dev" pointers take host pointers and
 *     return after the result is on the host.
 *   - A context is stateful like the reference's module objects (E_prev of
 *     SteeringBeamforming.h:69, current DOA, overlap-add tails) and is not
 *     thread-safe; use one context per stream of arrays (SURVEY 8b "Ownership").
 *   - PCM layout (stream API): fp32, channel-major: sample n of microphone m of
 *     array a at pcm[a*array_stride + m*mic_stride + n]; a call that processes F
 *     frames reads (F+1)*hop samples per microphone (frame t = samples
 *     [t*hop, t*hop+N), hop = N/2, periodic Hann analysis window).
 *   - Spectrum layout (frame API): the reference's CCS layout, double[N+2], bin k at
 *     [2k],[2k+1], k = 0..N/2 (Beamformer.cpp:59, test_mcarray.cpp:662).
 */
#ifndef MCARRAY_HIP_H
#define MCARRAY_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    MCA_HIP_OK = 0,
    MCA_HIP_ERR_INVALID_ARGUMENT = -1,
    MCA_HIP_ERR_HIP = -2,            /* a HIP runtime call failed */
    MCA_HIP_ERR_OUT_OF_MEMORY = -3,
    MCA_HIP_ERR_UNSUPPORTED = -4,    /* configuration outside what the kernels cover */
    MCA_HIP_ERR_NO_DEVICE = -5       /* no gfx950 device visible: there is NO CPU fallback */
} mca_hip_status;

typedef enum {
    MCA_HIP_SRP_FP32 = 0,    /* v_mfma_f32_32x32x2_f32, exact fp32 (parity anchor) */
    MCA_HIP_SRP_FP16X3 = 1,  /* fp16 hi/lo split operands, 3 MFMAs per k-step, ~fp32 accuracy */
    MCA_HIP_SRP_FP16 = 2,    /* single fp16 MFMA per k-step (fast; energy map error ~1.5e-5 of the peak) */
    MCA_HIP_SRP_ADAPTIVE = 3 /* fp16 coarse scan of every frame + exact repair: the frames whose peak pick is sensitive to the
                                fp16 error (and the rows their energy depends on) are recomputed with the FP16X3 split and
                                picked again, so the DOA bins are those of FP16X3 at about the cost of FP16.  Applies to large
                                batches (>= 4096 frames per call) of 1024-sample frames -- and of 2048- or 512-sample frames
                                with up to 8 microphones -- with more than two microphones and
                                ONE source (with several, the S-th pick is a near tie too often), with or without the power
                                gate; every other call of such a context runs as FP16X3 -- as do its calls while most rows
                                need the repair (noise only, silence: the context backs off by itself and probes again
                                later; mca_hip_config.adaptive_fallback = OFF pins the mode).  The optional energy map
                                keeps fp16 accuracy on unrepaired frames.
                                GUARANTEE: an unflagged frame carries the picks of the exact (FP16X3) map under the error model of
                                the sensitivity test; a flagged frame is picked on energies recomputed exactly for its own row and
                                the 16 rows before it (0.8^17 of the coarse error remains: within ~4e-7 of the map's peak of
                                FP16X3's energies).  Picks that are TIES at that level -- two candidates, or a first difference
                                against zero, closer than 1e-6 of the row's largest normalised energy: the bar of the parity tests
                                -- may resolve differently from FP16X3 and between calls of different shapes.  Measured over 40
                                random configurations / 696 320 frames: 41 picks on 29 frames differ from FP16X3, all 29 such ties
                                (profiles/r05_adaptive_check.json; the warm-row count of 16 against 24: r04_adaptive_check_warm24.json).
                                ROUND 5, device-pointer calls of 4 / 8-microphone contexts without the gate: (a) LAZY TAILS -- the
                                call does not repeat its last frame for the state's sake; it keeps its last 16 frames of PCM, their
                                coarse rows and the energies in front of them, and the next call repairs them only if one of its
                                first 16 frames is flagged.  Every other consumer of the state (host-pointer calls, graph launches,
                                mca_hip_state_save, calls of another batch size or too small for the mode) first makes the carried
                                energies exact, so what they see is what the eager form left.  (b) CANDIDATE COLUMNS (AUTO policy,
                                one source) -- a flagged frame's rows are recomputed exactly at the delays its pick can be among
                                (those whose coarse energy reaches the lowest value the exact pick can have, and two either side),
                                not at all D; the second pick runs on rows that are exact there and coarse elsewhere, and the
                                optional energy map of a flagged frame is exact at those delays only.
                                MCA_HIP_ADAPT_LAZY=0 restores the eager, whole-row form.
                                OUTSIDE THE MODEL, in any precision: a frame in which a channel's DC or Nyquist bin -- the two real
                                bins -- is at the rounding level of an fp32 transform (about one frame in 10^5 per 8 channels).
                                PHAT keeps only the SIGN of such a bin, and no two implementations, the reference's double-precision
                                one included, need agree on it; the frame's normalised energies then differ by up to
                                2 (M - 1) / (30 P) x 0.2 between them, decaying 0.8 per frame.  Inside this mode the coarse and the
                                exact pass agree on such a bin: with 4 and 8 microphones both run the same transform; with 16 they
                                are two kernels, so the coarse one marks the frame and it is repaired with its six successors
                                whatever the map says (profiles/r04_case23_real_bin_at_rounding_level.log). */
} mca_hip_srp_precision;

/* Weighting of the generalised cross-correlation inside dsp::GeneralisedCrossCorrelation::calculateCorrelationsForPrecomputedTauMatrix
 * (call site SteeringBeamforming.cpp:115-119; the code itself is in DSPONE, which the reference does not vendor).
 * PHAT is the build's reading and what BASELINE.json's north_star names.  NONE -- the plain cross-spectrum
 * X_a conj X_b -- is the reading under which the reference's own SRP test stimulus (1 kHz sines, test_mcarray.cpp:384-423)
 * localises within its 7 degrees; it is offered so that a maintainer who has DSPONE can switch once
 * tools/pin_against_dspone.cpp has settled which one DSPONE implements.  NONE needs MCA_HIP_SRP_FP32 (un-normalised spectra
 * do not fit fp16 operands): frame API always, stream API at N = 1024 with 4 or 8 microphones. */
typedef enum { MCA_HIP_GCC_PHAT = 0, MCA_HIP_GCC_NONE = 1 } mca_hip_gcc_weighting;

typedef struct mca_hip_ctx mca_hip_ctx;

/* Configuration = the constructor arguments of the reference's modules
 * (SourceSeparationAndLocalisation.h:47, BeamformingSeparationAndLocalistaion.h:40,
 * SteeringBeamforming.h:43, Beamformer.h:39) plus the constants the reference
 * hard-codes and BASELINE.json needs as parameters (SURVEY section 5 "config"). */
typedef struct {
    int struct_size;           /* sizeof(mca_hip_config), for ABI evolution */
    int device;                /* HIP device ordinal */
    int sample_rate;           /* Hz */
    int fft_size;              /* N; the reference derives it with calculateOrderFromSampleRate
                                  (SourceSeparationAndLocalisation.cpp:52).  Stream API: N = 1024 and N = 512 (up to 8
                                  microphones) run the tuned kernels, any other power of two 64..8192 the any-length kernels as long as
                                  (n_mics + n_sources) spectra of N/2+1 bins fit the 160 KiB LDS; the frame API
                                  takes any even N with N/2+1 <= 4097 */
    int n_mics;                /* M, 2..16 */
    const double *mic_xyz;     /* [M][3] metres, ArrayDescription coordinates (ArrayDescription.h:31-92) */
    double doa_step_deg;       /* SteeringBeamforming.cpp:39 hard-codes 5.0; BASELINE uses 0.5 */
    int n_sources;             /* numOfSources, 1..4 (a limit of this build -- the reference's loops, SteeringBeamforming.cpp:185-194, take any count;
                                  more is refused with MCA_HIP_ERR_INVALID_ARGUMENT, never truncated) */
    int use_power_floor;       /* usePowerFloor (reference default true, SourceSeparationAndLocalisation.h:47): the stream API
                                  then runs the power gate of BeamformingSeparationAndLocalisation.cpp:55-87 on the GPU;
                                  the frame API exposes mca_hip_fft_log_power for the caller's gate */
    int srp_precision;         /* mca_hip_srp_precision */
    int max_arrays;            /* number of independent arrays whose state the context holds (>= 1) */
    int gcc_weighting;         /* mca_hip_gcc_weighting; 0 = PHAT.  (Appended in round 3: a struct_size that ends before this
                                  field is accepted and means PHAT.) */
    /* Appended in round 4 (a struct_size that ends before them is accepted; zero = the default of each): */
    int adaptive_fallback;     /* mca_hip_adaptive_fallback.  MCA_HIP_SRP_ADAPTIVE only.  0 = AUTO: the context backs off to
                                  FP16X3 by itself while most rows need the repair (noise only, silence) and probes again later.
                                  Round 6: a call's report is consumed by the eligible call TWO calls after it, which waits for it
                                  if it has not arrived (the call in between is still queued behind it: the device does not idle),
                                  so which call switches depends on the sequence of calls and their content only -- two runs of the
                                  same calls return the same bits in every output under AUTO as well (tests/test_gpu_adaptive.py).
                                  A report that stays away for 4 s (a stream held up by something only the calling thread would
                                  release) ends the policy until mca_hip_reset.  HIP-graph recordings never switch.
                                  1 = OFF: the mode is pinned -- every eligible call runs coarse + repair. */
    int adaptive_min_rows;     /* ADAPTIVE: calls of fewer rows (arrays x frames) run as FP16X3; 0 = 4096 */
    int adaptive_max_sources;  /* ADAPTIVE: contexts with more sources run as FP16X3; 0 = 1 */
    int scan_carry;            /* 1: the chunk start values of the energy recursion always come from the serial carry pass
                                  (k_scan_carry) instead of the four-chunk look-back of ungated PHAT calls; results agree to the
                                  last bits (tests cross-check the two) */
} mca_hip_config;

typedef enum { MCA_HIP_ADAPT_FALLBACK_AUTO = 0, MCA_HIP_ADAPT_FALLBACK_OFF = 1 } mca_hip_adaptive_fallback;

/* ---- page-locked host memory ---------------------------------------------- */
/* Thin wrappers over hipHostMalloc / hipHostFree / hipHostRegister / hipHostUnregister so that a caller of the host-pointer
 * entry points need not link HIP.  A registered range must stay allocated until it is unregistered.  The reference has no
 * counterpart (its SignalVector buffers are plain new[] arrays, mcadefs.h:86-88). */
void *mca_hip_host_alloc(long long bytes);
void mca_hip_host_free(void *p);
int mca_hip_host_register(void *p, long long bytes);
int mca_hip_host_unregister(void *p);

/* ---- lifetime ------------------------------------------------------------ */
/* Replaces the constructors SteeringBeamforming::SteeringBeamforming + generateLookupTable
 * (SteeringBeamforming.cpp:34-94), Beamformer::Beamformer (Beamformer.cpp:33-49) and
 * BeamformingSeparationAndLocalisation's (BeamformingSeparationAndLocalisation.cpp:29-53). */
int mca_hip_create(const mca_hip_config *cfg, mca_hip_ctx **out);
void mca_hip_destroy(mca_hip_ctx *ctx);
/* message of the last failure on this context (ctx == NULL: last failed create) */
const char *mca_hip_last_error(const mca_hip_ctx *ctx);

/* ---- introspection --------------------------------------------------------- */
int mca_hip_num_steps(const mca_hip_ctx *ctx);   /* D = _numSteps (SteeringBeamforming.cpp:40) */
int mca_hip_num_pairs(const mca_hip_ctx *ctx);   /* P = M(M-1)/2 */
int mca_hip_num_groups(const mca_hip_ctx *ctx);  /* pairs sharing a bit-identical delay table are merged */
/* delaysForMicroPair (SteeringBeamforming.cpp:69-73): out[P][D], the float delays in samples */
int mca_hip_get_pair_delays(const mca_hip_ctx *ctx, float *out);
/* doaIdx2angle for every grid point (microhponeArrayHelpers.cpp:117-120): out[D] radians */
int mca_hip_get_doa_grid(const mca_hip_ctx *ctx, float *out);

/* ---- state ----------------------------------------------------------------- */
/* zero E_prev / DOA / overlap-add tails of every array and the FreqGCC frame hook's state (a freshly constructed module) */
int mca_hip_reset(mca_hip_ctx *ctx, void *stream);
/* pre-size the internal workspace so later *_dev calls allocate nothing (graph capture) */
int mca_hip_reserve(mca_hip_ctx *ctx, int n_arrays, int n_frames);
/* Checkpoint / resume of everything a module object carries between process() calls, for all max_arrays
 * arrays: E_prev (SteeringBeamforming.h:69), the overlap-add tails, the power-floor estimation
 * (SoundLocalisationImpl.h:84-86), _currentDOA / _prob (BeamformingSeparationAndLocalisation.cpp:51-52), the 2-mic
 * path's smoothed DOA and frame count, the frame API's E_prev.  A blob is only valid for a context created with
 * the same geometry, grid, frame length, n_sources and max_arrays (checked: MCA_HIP_ERR_INVALID_ARGUMENT).
 * mca_hip_state_size returns the number of bytes (or a negative status).
 * Version 3 blobs end with the FreqGCC frame hook's part (mca_hip_gcc2_process_frame), 8 * (D + 8) bytes: its smoothed
 * correlation double[D], then 8 doubles _powerFloor, samples consumed for it, _noiseEstimated, _silenceFramesCounter,
 * _corrMemoryFactor, _doaMemoryFactor, _currentDOA, _prob.  Version 1 and 2 blobs (without that part) still load and leave
 * the frame hook as a newly built module.  A context with a DOA tracker (mca_hip_gcc2_tracker_attach) writes version 4. */
long long mca_hip_state_size(const mca_hip_ctx *ctx);
int mca_hip_state_save(mca_hip_ctx *ctx, void *blob, long long blob_bytes);
int mca_hip_state_load(mca_hip_ctx *ctx, const void *blob, long long blob_bytes);

/* ---- stream API: batched frames, device pointers ---------------------------- */
/* STFT analysis + SteeringBeamforming::processFrame (SteeringBeamforming.cpp:96-195) for
 * n_frames consecutive frames of n_arrays independent arrays: GCC-PHAT over all pairs,
 * SRP scan, 0.8 IIR over frames (continuing from the context state), selectDOA.
 * Outputs (any may be NULL except doa_bin_dev):
 *   doa_bin_dev [A][F][S] int32   maxIdx+1 of selectDOA (:191) -- the "DOA bin"
 *   doa_rad_dev [A][F][S] float   doaIdx2angle(maxIdx+1) (:191), radians
 *   prob_dev    [A][F][S] float   the max (:193)
 *   energy_dev  [A][F][D] float   un-normalised smoothed _energyInDOA (before :155) */
int mca_hip_localise_frames_dev(mca_hip_ctx *ctx, const float *pcm_dev, long long array_stride,
                                long long mic_stride, int n_arrays, int n_frames,
                                int *doa_bin_dev, float *doa_rad_dev, float *prob_dev,
                                float *energy_dev, void *stream);

/* STFT analysis + BeamformingSeparationAndLocalisation::processFrameSeparation
 * (BeamformingSeparationAndLocalisation.cpp:103-119 -> Beamformer::processFrame,
 * Beamformer.cpp:51-71) + inverse FFT and overlap-add, steering frame t of array a at
 * doa_rad_dev[a][t][s].  out_pcm_dev [A][S][F*hop] fp32. */
int mca_hip_separate_frames_dev(mca_hip_ctx *ctx, const float *pcm_dev, long long array_stride,
                                long long mic_stride, int n_arrays, int n_frames,
                                const float *doa_rad_dev, float *out_pcm_dev, void *stream);

/* The same with the grid bins behind the angles: doa_bin_dev[a][t][s] as written by
 * mca_hip_localise_frames_dev (-1 = no frame has fired yet, the initial _currentDOA = 0,
 * BeamformingSeparationAndLocalisation.cpp:51), doa_rad_dev = the grid angles of those bins.  With
 * one or two sources on the 1024-sample path the steering phasors then come from a per-angle table built
 * once per context (no sincos per frame); other configurations run as mca_hip_separate_frames_dev. */
int mca_hip_separate_frames_bins_dev(mca_hip_ctx *ctx, const float *pcm_dev, long long array_stride,
                                     long long mic_stride, int n_arrays, int n_frames,
                                     const int *doa_bin_dev, const float *doa_rad_dev,
                                     float *out_pcm_dev, void *stream);

/* Both of the above in sequence = SourceSeparationAndLocalisation::processParametrisation
 * (SourceSeparationAndLocalisation.cpp:79-94) for every frame. */
int mca_hip_process_frames_dev(mca_hip_ctx *ctx, const float *pcm_dev, long long array_stride,
                               long long mic_stride, int n_arrays, int n_frames,
                               int *doa_bin_dev, float *doa_rad_dev, float *prob_dev,
                               float *energy_dev, float *out_pcm_dev, void *stream);

/* The same for 16-bit PCM, the sample type of the reference's process(std::vector<int16_t*>&, ...) overloads and of the
 * WAV / raw files its tools read (mcabeamf.cpp:112, test_mcarray.cpp:618).  pcm is [A][M][(F+1)*hop] int16; the samples
 * are taken at face value (+-32768, like a cast to double: PHAT and the DOA do not depend on the scale, the audio out is
 * in the same units).  Half the bytes cross PCIe; the conversion to fp32 runs on the GPU. */
int mca_hip_process_frames_host_i16(mca_hip_ctx *ctx, const short *pcm, int n_arrays, int n_frames,
                                    int *doa_bin, float *doa_rad, float *prob, float *energy, float *out_pcm);

/* After a stream call on a context with use_power_floor = 1: copies, for the frames of that call,
 * voiced[A][F] (1 where processFrameLocalisation passed the gate and the callback fires,
 * BeamformingSeparationAndLocalisation.cpp:87-94) and power[A][F] (the value handed to setDOA).  Either may be NULL.
 * Gated-out frames repeat the previous _currentDOA/_prob in the DOA outputs (initially 0 rad / -1, bin -1). */
int mca_hip_copy_gate(mca_hip_ctx *ctx, unsigned char *voiced, float *power);

/* Host-buffer variant of mca_hip_process_frames_dev (copies in, runs, copies out, synchronises);
 * pcm is [A][M][(F+1)*hop] contiguous; outputs as above, any of doa_rad/prob/energy/out_pcm may be NULL.
 * This is what a drop-in process() caller hits (src/programs/mcabeamf.cpp:101-112, test/test_mcarray.cpp:869,937).
 * If pcm is page-locked (mca_hip_host_alloc / mca_hip_host_register below, or hipHostMalloc / hipHostRegister), the arrays
 * go up in up to four chunks and the upload of chunk i+1, the kernels of chunk i and the download of chunk i-1 (into
 * page-locked result buffers) overlap; pageable buffers take one synchronous copy each way.  Same results either way. */
int mca_hip_process_frames_host(mca_hip_ctx *ctx, const float *pcm, int n_arrays, int n_frames,
                                int *doa_bin, float *doa_rad, float *prob, float *energy, float *out_pcm);

/* ---- frame API: one frame of CCS spectra, host pointers, double precision ------ */
/* SteeringBeamforming::processFrame(const SignalVector&, SignalPtr DOA, SignalPtr prob,
 * int numOfSources, SignalVector& wienerCoefs) (SteeringBeamforming.h:54).  frames[c] ->
 * double[ccs_len]; DOA[S] radians, prob[S]; doa_bin (may be NULL) [S].  State of array 0. */
int mca_hip_steering_process_frame(mca_hip_ctx *ctx, const double *const *frames, int ccs_len,
                                   double *DOA, double *prob, int *doa_bin, int n_sources);
/* Beamformer::processFrame(SignalVector&, SignalPtr outputFrame, double DOA) (Beamformer.h:49) */
int mca_hip_beamformer_process_frame(mca_hip_ctx *ctx, const double *const *frames, int ccs_len,
                                     double *out, double DOA);
/* dsp::SignalPower::FFTLogPower as used by the power gate
 * (BeamformingSeparationAndLocalisation.cpp:83); *power_db = 10 log10(mean-square) */
int mca_hip_fft_log_power(mca_hip_ctx *ctx, const double *const *frames, int ccs_len, double *power_db);
/* copy of the current un-normalised _prevEnergyInDOA of array 0: out[D] */
int mca_hip_get_energy(mca_hip_ctx *ctx, double *out);

/* ---- real-time mode: the stream call as a HIP graph --------------------------------------------
 * A caller that hands over a stream chunk by chunk (SourceSeparationAndLocalisation::process() on a live input,
 * mcabeamf.cpp:112; BASELINE configs[1]) is bound by the launches of a call, not by its kernels: one frame is 18 KB.
 * mca_hip_graph_create fixes the shape and the device buffers of a mca_hip_process_frames_dev call (out_pcm_dev NULL:
 * of a mca_hip_localise_frames_dev call; doa_bin_dev NULL: of a mca_hip_separate_frames_dev call, the delay-and-sum stage
 * alone at the caller's angles in doa_rad_dev); mca_hip_graph_launch replays the kernels of that call as ONE graph launch on
 * whatever the caller has put into pcm_dev since the last launch, continuing the context state exactly like the plain
 * call (results are bit-identical).  The graphs (one per parity of the double-buffered state) are recorded on first
 * use; recording executes nothing.  Plain stream calls and graph launches on the same context may be mixed. */
typedef struct mca_hip_graph mca_hip_graph;
int mca_hip_graph_create(mca_hip_ctx *ctx, const float *pcm_dev, long long array_stride, long long mic_stride,
                         int n_arrays, int n_frames, int *doa_bin_dev, float *doa_rad_dev, float *prob_dev,
                         float *energy_dev, float *out_pcm_dev, mca_hip_graph **out);
int mca_hip_graph_launch(mca_hip_graph *g, void *stream);
void mca_hip_graph_destroy(mca_hip_graph *g);

/* ---- 2-microphone GCC-PHAT localisation (FreqGCCBinauralLocalisation) ----------------- */
/* Deterministic part of FreqGCCBinauralLocalisation::processParametrisation
 * (BinauralLocalisation.cpp:406-567) for n_frames consecutive frames of n_arrays independent
 * 2-microphone arrays, on a context created with n_mics == 2 (the reference grid is
 * doa_step_deg = 3, BinauralLocalisation.cpp:328): GCC-PHAT at the D steering delays (:438-444),
 * correlation smoothing corr = (1-mu) corr + mu prev with mu = 0 on a stream's first frame and
 * 0.8f afterwards (:445-448, :523), first-max argmax and the author's deterministic DOA smoothing
 * DOA = m DOA + (1-m) angle, m = 0 then 0.6f (the #else branch :502-504; the particle filter of
 * :456-473, which the reference is compiled with, is the DOA tracker below: mca_hip_gcc2_tracker_attach),
 * and setProbability of the previous DOA (:454, :569-631).  With use_power_floor = 1 the gate of :387-404 / :425-434 runs on the GPU (3 s of floor
 * estimation, then a frame fires when its FFTLogPower exceeds the floor + 6 dB): the recursions only see the frames that
 * fired, the others repeat the outputs of the last fired frame (argmax -1, DOA 0, prob -1 before the first), and
 * mca_hip_copy_gate returns voiced[A][F] / power[A][F] of the call.
 *   argmax_dev [A][F] int32, doa_rad_dev [A][F] float (smoothed), prob_dev [A][F] float,
 *   corr_dev [A][F][D] float smoothed correlation (any but argmax_dev may be NULL). */
int mca_hip_gcc2_frames_dev(mca_hip_ctx *ctx, const float *pcm_dev, long long array_stride,
                            long long mic_stride, int n_arrays, int n_frames, int *argmax_dev,
                            float *doa_rad_dev, float *prob_dev, float *corr_dev, void *stream);
int mca_hip_gcc2_frames_host(mca_hip_ctx *ctx, const float *pcm, int n_arrays, int n_frames,
                             int *argmax, float *doa_rad, float *prob, float *corr);

/* FreqGCCBinauralLocalisation::setProbability (BinauralLocalisation.cpp:569-631) at caller-given angles (radians), what the
 * particle filter's observation model asks for (SoundLocalisationParticleFilter.cpp:51): min and sum of the smoothed
 * correlation, linear interpolation between the neighbouring grid points (the two edge cells take their own value), values
 * below 0.01 set to 0, in the reference's float/double sequence (angle2DOAidx on a float angle).  A correlation whose
 * sum - min * D is not positive -- a context freshly created or reset -- gives all zeros (the reference reads its
 * uninitialised buffer there).  n == 0 is a no-op; n_mics != 2, n < 0 and NULL pointers with n > 0 are invalid.
 * On the smoothed correlation the last mca_hip_gcc2_frames_* call left for array `array_index` (gated-out frames do not
 * change it), array_index in [0, max_arrays).  Synchronises the device. */
int mca_hip_gcc2_set_probability(mca_hip_ctx *ctx, int array_index, const double *doas, double *probs, int n);
/* The same for arrays 0..n_arrays-1 in one launch: doas_dev / probs_dev [n_arrays][n] float, n_arrays <= max_arrays.
 * Enqueued on `stream`: no allocation and no synchronisation (usable between gcc2_frames_dev calls of a tracker loop).
 * Row a of the result equals float(mca_hip_gcc2_set_probability(a, double(doas[a]))) bit for bit. */
int mca_hip_gcc2_set_probability_dev(mca_hip_ctx *ctx, int n_arrays, const float *doas_dev, float *probs_dev, int n,
                                     void *stream);
/* FreqGCCBinauralLocalisation::processParametrisation (BinauralLocalisation.cpp:406-567, deterministic branch) for one
 * frame: frames[0..1] -> double[ccs_len] CCS spectra, ccs_len = fft_size + 2; double on the GPU; its own state, separate
 * from the stream state (a context driven through both keeps two).  The power-floor estimation runs for the first 3 s
 * whether use_power_floor is set or not, and `power` is the floor meanwhile (:387-404, :429); then FFTLogPower.
 * voiced = 1 where the gate passed (the reference's callback fires: setDOA(degrees(doa_rad), prob, power, 1), :521).
 * doa_rad / prob = _currentDOA / _prob after the frame (0 / -1 before the first voiced frame); prob is setProbability of
 * the previous DOA on the new correlation (:454).  power = the value handed to setDOA.  argmax (may be NULL) = first-max
 * index, -1 on gated-out frames.  corr (may be NULL) = double[D], the smoothed correlation after the frame. */
int mca_hip_gcc2_process_frame(mca_hip_ctx *ctx, const double *const *frames, int ccs_len, int *voiced,
                               double *doa_rad, double *prob, double *power, int *argmax, double *corr);
/* setProbability, as mca_hip_gcc2_set_probability, on the frame hook's correlation */
int mca_hip_gcc2_frame_set_probability(mca_hip_ctx *ctx, const double *doas, double *probs, int n);

/* ---- the particle-filter DOA tracker of FreqGCCBinauralLocalisation (BinauralLocalisation.cpp:38 USE_PARTICLE_FILTER) ----
 * As the reference is compiled, _currentDOA is the estimate of a 500-particle filter seeded at the first voiced frame
 * (:457-465), updated on every voiced frame (:473) and through up to windowsToDecay gated-out frames, which still fire the
 * callback (:536-548), and dropped after that (:551-558).  The filter engine is DSPONE's and not available: what the reference
 * pins is kept (500 particles, the observation model = setProbability of the particles on the smoothed correlation, the
 * prediction's clamp to [-pi/2, pi/2], the control flow), the rest is defined in DESIGN.md ("The DOA tracker") so that the
 * result is a pure function of (seed, array index, track number, update number) and the rows: counter-based integer random
 * numbers, integer weights, systematic resampling, a few particles re-injected uniformly per update.  It runs on the GPU, one
 * wave per array, inside the stream call and the frame hook; tests/gcc2_tracker_twin.py restates it and matches bit for bit.
 * Opt-in: a context without a tracker behaves, and writes state blobs, exactly as before. */
typedef struct {
    int struct_size;
    int n_particles;            /* 0 = 500 (BinauralLocalisation.cpp:463); 16..1024 */
    int n_inject;               /* particles re-drawn uniformly over [-pi/2, pi/2] per update: 0 = n_particles / 20, -1 = none, < n_particles */
    unsigned long long seed;
    double sigma_init, sigma_step;   /* radians: spread around the argmax at seeding, random-walk step per update; 0 = the grid step */
} mca_hip_gcc2_tracker_config;
/* n_mics == 2 only; allocates the state of max_arrays arrays and of the frame hook; a second attach is refused.  From then on
 * mca_hip_gcc2_process_frame runs the tracker on the hook's state (`voiced` becomes fired: 1 voiced, 2 a coasting track whose
 * callback fires, 0 nothing; doa_rad / prob the tracked ones), mca_hip_gcc2_frames_* are refused (call the tracked form),
 * mca_hip_reset forgets every track (track numbers start at 1 again), mca_hip_gcc2_set_probability* work as before, and state
 * blobs are version 4 = version 3 + the tracker's part (its configuration, checked on load; per array and for the hook alive,
 * track, update number, DOA, prob, the particles).  Blobs of version <= 3 load and leave every track unstarted. */
int mca_hip_gcc2_tracker_attach(mca_hip_ctx *ctx, const mca_hip_gcc2_tracker_config *cfg);
/* mca_hip_gcc2_frames_dev with the tracker in place of the DOA recursion.  All outputs [A][F]; corr_dev [A][F][D]; only
 * doa_rad_dev is required.  Per frame: fired_dev 1 = voiced (seeds a track if none is alive, then DOA = updateFilter()),
 * 2 = gated out with a live track and fewer than windowsToDecay silent frames (DOA = updateFilter() on the unchanged row),
 * 0 = nothing (the track is dropped once the silence counter reaches windowsToDecay).  doa_rad_dev = float(_currentDOA),
 * prob_dev = float(setProbability(DOA before the frame)) of the last voiced frame, track_dev = the number of the array's
 * current or last track (_sourceCounter; 0 before the first).  mca_hip_copy_gate returns voiced / power of the call.
 * Cannot be recorded into a HIP graph (MCA_HIP_ERR_UNSUPPORTED). */
int mca_hip_gcc2_tracked_frames_dev(mca_hip_ctx *ctx, const float *pcm_dev, long long array_stride, long long mic_stride,
                                    int n_arrays, int n_frames, int *argmax_dev, float *doa_rad_dev, float *prob_dev,
                                    unsigned char *fired_dev, int *track_dev, float *corr_dev, void *stream);
int mca_hip_gcc2_tracked_frames_host(mca_hip_ctx *ctx, const float *pcm, int n_arrays, int n_frames, int *argmax,
                                     float *doa_rad, float *prob, unsigned char *fired, int *track, float *corr);
/* the particles double[n_particles] (radians), whether a track is alive and its number, of array `array_index` of the stream
 * state, or of the frame hook with array_index = -1.  Any output may be NULL.  Synchronises the device. */
int mca_hip_gcc2_tracker_get_particles(mca_hip_ctx *ctx, int array_index, double *particles, int *alive, int *track);

/* ---- binaural masking (FastBinauralMasking) --------------------------------------------- */
typedef struct mca_hip_mask_ctx mca_hip_mask_ctx;
/* BinauralMasking::MaskingMethod / MaskingAlg (ArrayModules.h:81,89) */
typedef enum { MCA_HIP_MASK_FACTOR = 0, MCA_HIP_MASK_RELATIVE = 1, MCA_HIP_MASK_FULL = 3, MCA_HIP_MASK_NOISY = 4, MCA_HIP_MASK_NOTHING = 5 } mca_hip_mask_method;
typedef enum { MCA_HIP_MASK_BOTH = 0, MCA_HIP_MASK_SPATIAL = 1, MCA_HIP_MASK_TEMPORAL = 2 } mca_hip_mask_alg;
/* constructor arguments of FastBinauralMasking(int samplerate, double microDistance, float lowFreq,
 * float highFreq, MaskingMethod, MaskingAlg) (FastBinauralMasking.h:71-76) */
typedef struct {
    int struct_size;
    int device;
    int sample_rate;
    int fft_size;            /* N = 2^calculateOrderFromSampleRate(fs, 0.050): 1024 at 16 kHz (tuned kernel), 2048 at 44.1 / 48 kHz;
                                the stream API takes powers of two up to 8192, the frame hook any even N */
    double micro_distance;
    float low_freq, high_freq;
    int method;              /* mca_hip_mask_method */
    int algorithm;           /* mca_hip_mask_alg */
    int max_streams;
} mca_hip_mask_config;
/* FastBinauralMasking::FastBinauralMasking + init + calculateThresholds (FastBinauralMasking.cpp:51-123, :342-366) */
int mca_hip_mask_create(const mca_hip_mask_config *cfg, mca_hip_mask_ctx **out);
void mca_hip_mask_destroy(mca_hip_mask_ctx *ctx);
const char *mca_hip_mask_last_error(const mca_hip_mask_ctx *ctx);
int mca_hip_mask_reset(mca_hip_mask_ctx *ctx);
/* _thresholds (:361-362) and getBinCenterFrequency (cycles/sample): out[45] each */
int mca_hip_mask_get_thresholds(const mca_hip_mask_ctx *ctx, double *thresholds, double *center_freqs);
/* STFT + FastBinauralMasking::processParametrisation (FastBinauralMasking.cpp:126-210) + inverse FFT +
 * overlap-add for n_frames frames of n_streams independent 2-channel streams.
 * pcm_dev: sample n of channel c of stream s at pcm[s*stream_stride + c*ch_stride + n], (F+1)*hop samples;
 * The streams of a context start and advance together (the module's first-frame behaviour, FastBinauralMasking.cpp:186-197,
 * is tracked once per context): every call after create / reset must pass the same n_streams, else INVALID_ARGUMENT.
 * out_pcm_dev [streams][2][F*hop]; decisions_dev (may be NULL) [streams][F][45] int32:
 * 0 enhance, 1 temporal mask, 2 spatial mask. */
int mca_hip_mask_frames_dev(mca_hip_mask_ctx *ctx, const float *pcm_dev, long long stream_stride, long long ch_stride,
                            int n_streams, int n_frames, float *out_pcm_dev, int *decisions_dev, void *stream);
int mca_hip_mask_frames_host(mca_hip_mask_ctx *ctx, const float *pcm, int n_streams, int n_frames, float *out_pcm,
                             int *decisions);
/* the DSPONE hook itself: one frame, left/right CCS double[N+2] modified in place (:199-200), double on the GPU */
int mca_hip_mask_process_frame(mca_hip_mask_ctx *ctx, double *left, double *right, int ccs_len, int *decisions);
/* checkpoint / resume as mca_hip_state_*: the short-time powers Q and noise estimates of every stream, the overlap-add
 * tails, the frame counters (and the state of the frame hook) */
long long mca_hip_mask_state_size(const mca_hip_mask_ctx *ctx);
int mca_hip_mask_state_save(mca_hip_mask_ctx *ctx, void *blob, long long blob_bytes);
int mca_hip_mask_state_load(mca_hip_mask_ctx *ctx, const void *blob, long long blob_bytes);

/* ---- filter-bank binaural masking (BinauralMaskingImpl) --------------------------------------
 * The time-domain formulation of the same masking: every windowed frame goes through 45 mel filters, each band signal
 * pair is kept, temporally masked or spatially masked, the bands are summed again.  It is its own
 * module: its own decision rule (plain means, no reject factor), three methods, a per-channel RELATIVE gain. */
typedef struct mca_hip_bmask_ctx mca_hip_bmask_ctx;
/* BinauralMaskingImpl::MaskingMethod (BinauralMaskingImpl.h:67) */
typedef enum { MCA_HIP_BMASK_FACTOR = 0, MCA_HIP_BMASK_RELATIVE = 1, MCA_HIP_BMASK_FULL = 3 } mca_hip_bmask_method;
/* constructor arguments of BinauralMaskingImpl(int samplerate, double microDistance, float lowFreq, float highFreq,
 * MaskingMethod) (BinauralMaskingImpl.h:78-82) */
typedef struct {
    int struct_size;
    int device;
    int sample_rate;
    int frame_size;          /* W = 2^calculateOrderFromSampleRate(fs, 0.050): 1024 at 16 kHz and 2048 at 44.1 / 48 kHz have tuned
                                kernels, the other powers of two in [256, 8192] (256, 512, 4096, 8192) run on the any-length
                                transform.  Everything else is refused with INVALID_ARGUMENT: 64, 128 and 16384, which
                                mca_hip_mask_create takes, and every length that is not a power of two */
    double micro_distance;
    float low_freq, high_freq;
    int method;              /* mca_hip_bmask_method */
    int max_streams;
} mca_hip_bmask_config;
int mca_hip_bmask_create(const mca_hip_bmask_config *cfg, mca_hip_bmask_ctx **out);
void mca_hip_bmask_destroy(mca_hip_bmask_ctx *ctx);
const char *mca_hip_bmask_last_error(const mca_hip_bmask_ctx *ctx);
/* zeroes the short-time powers, the overlap-add tails and the frame counters of every stream and the hook's powers */
int mca_hip_bmask_reset(mca_hip_bmask_ctx *ctx);
/* _thresholds (cos(2 pi f_b d sin(10 deg) / c) * 0.9) and the band centres (cycles/sample): out[45] each */
int mca_hip_bmask_get_thresholds(const mca_hip_bmask_ctx *ctx, double *thresholds, double *center_freqs);
/* windowing + filter bank + BinauralMaskingImpl::processParametrisation + re-summation + overlap-add for n_frames frames
 * (hop W/2, periodic Hann) of n_streams independent 2-channel streams, fp32.
 * pcm_dev: sample n of channel c of stream s at pcm[s*stream_stride + c*ch_stride + n], (F+1)*hop samples; 8-byte aligned, even
 * strides.  Streams are independent: stream s of a call continues slot s of the context, any n_streams <= max_streams.
 * out_pcm_dev [streams][2][F*hop]; decisions_dev (may be NULL) [streams][F][45] int32: 0 enhance, 1 temporal mask, 2 spatial
 * mask.  Asynchronous on `stream`; a call that needs a larger workspace than any before it allocates (and synchronises). */
int mca_hip_bmask_frames_dev(mca_hip_bmask_ctx *ctx, const float *pcm_dev, long long stream_stride, long long ch_stride,
                             int n_streams, int n_frames, float *out_pcm_dev, int *decisions_dev, void *stream);
int mca_hip_bmask_frames_host(mca_hip_bmask_ctx *ctx, const float *pcm, int n_streams, int n_frames, float *out_pcm,
                              int *decisions);
/* the three hooks of the class, one frame of one channel (pair) each, double on the GPU; they keep a short-time power of their own.
 * frame_analysis: band b of in_frame[W] to analysis[b*W .. b*W+W) for every b < 45 that fits into analysis_length, and the
 * residual (the frame minus its 45 bands) to slot 45 when analysis_length >= 46*W; the rest of the buffer is not written. */
int mca_hip_bmask_frame_analysis(mca_hip_bmask_ctx *ctx, const double *in_frame, double *analysis, int frame_length,
                                 int analysis_length, int channel);
/* processParametrisation: left/right hold 45 band signals of W doubles each (analysis_length >= 45*W), scaled in place;
 * decisions (may be NULL) int[45] */
int mca_hip_bmask_process_frame(mca_hip_bmask_ctx *ctx, double *left, double *right, int analysis_length, int *decisions);
/* frameSynthesis, the reference's literal loop: out_frame[W] = the sum of the slots 0, 1, ... while slot <= 45 and
 * slot*W < analysis_length - W (46*W: the 45 bands, no residual; 45*W: the first 44 bands) */
int mca_hip_bmask_frame_synthesis(mca_hip_bmask_ctx *ctx, double *out_frame, const double *analysis, int frame_length,
                                  int analysis_length, int channel);
/* checkpoint / resume as mca_hip_state_*: the short-time powers of every stream, the overlap-add tails, the frame counters
 * and the hook's short-time powers */
long long mca_hip_bmask_state_size(const mca_hip_bmask_ctx *ctx);
int mca_hip_bmask_state_save(mca_hip_bmask_ctx *ctx, void *blob, long long blob_bytes);
int mca_hip_bmask_state_load(mca_hip_bmask_ctx *ctx, const void *blob, long long blob_bytes);

/* ---- MultibandBinarualLocalisation (2 microphones) ---------------------------
 * Replaces mca::MultibandBinarualLocalisation(int sampleRate, ArrayDescription, int nbins = 15, bool usePowerFloor = 1)
 * (include/mcarray/MultibandBinarualLocalisation.h:38) with its per-frame hooks processSetup / processOneSubband /
 * processSumamry (src/mcarray/MultibandBinarualLocalisation.cpp:145-258) for batches of frames.  The sub-band
 * splitting (dsp::SubBandSTFTAnalysis, DSPONE) is [BUILD-DEFINES]: nbins unit-peak triangular filters, edges
 * linearly spaced between 100 Hz and maxFreqForSpatialAliasing(distance(0,1)) (ctor call :54-60). */
typedef struct mca_hip_mb_ctx mca_hip_mb_ctx;
typedef struct {
    int struct_size;
    int device;
    int sample_rate;
    int fft_size;            /* N = 2^calculateOrderFromSampleRate(fs, 0.025) (MultibandBinarualLocalisation.h:43); power of two 64..8192 */
    const double *mic_xyz;   /* [2][3] metres */
    int nbins;               /* sub-bands, reference default 15; 1..27 */
    int use_power_floor;     /* usePowerFloor (reference default true) */
    int max_arrays;          /* independent module objects (streams) this context holds state for */
} mca_hip_mb_config;
int  mca_hip_mb_create(const mca_hip_mb_config *cfg, mca_hip_mb_ctx **out);
void mca_hip_mb_destroy(mca_hip_mb_ctx *ctx);
const char *mca_hip_mb_last_error(const mca_hip_mb_ctx *ctx);
int  mca_hip_mb_reset(mca_hip_mb_ctx *ctx, void *stream);
int  mca_hip_mb_num_steps(const mca_hip_mb_ctx *ctx);                 /* _numSteps = floor(pi/step)+1 = 37 (:63) */
int  mca_hip_mb_get_filters(const mca_hip_mb_ctx *ctx, double *out);  /* [nbins][N/2+1] filter magnitudes */
/* n_frames frames of n_arrays independent 2-channel streams; pcm_dev as in mca_hip_mask_frames_dev.
 * Per frame (all [arrays][F]): doa_rad = _currentDOA[0] after the frame (:239/:254), prob = _prob[0] (:233/:255),
 * voiced (may be NULL) = 1 where setDOA fires (:225,:248), power (may be NULL) = the value handed to setDOA.
 * Optional: band_idx [arrays][F][nbins] first-max delay index per band (:184), energy_in_doa [arrays][F][D]
 * (_energyInDOA :190), band_corr [arrays][F][nbins][D] smoothed band correlations (:180-183). */
int mca_hip_mb_frames_dev(mca_hip_mb_ctx *ctx, const float *pcm_dev, long long array_stride, long long ch_stride,
                          int n_arrays, int n_frames, float *doa_rad_dev, float *prob_dev, unsigned char *voiced_dev,
                          float *power_dev, int *band_idx_dev, float *energy_in_doa_dev, float *band_corr_dev, void *stream);
int mca_hip_mb_frames_host(mca_hip_mb_ctx *ctx, const float *pcm, int n_arrays, int n_frames, float *doa_rad, float *prob,
                           unsigned char *voiced, float *power, int *band_idx, float *energy_in_doa, float *band_corr);
/* checkpoint / resume as mca_hip_state_*: smoothed band correlations, power-floor estimation, _currentDOA / _prob of every array */
long long mca_hip_mb_state_size(const mca_hip_mb_ctx *ctx);
int mca_hip_mb_state_save(mca_hip_mb_ctx *ctx, void *blob, long long blob_bytes);
int mca_hip_mb_state_load(mca_hip_mb_ctx *ctx, const void *blob, long long blob_bytes);

/* ---- TemporalGCCBinauralLocalisation (2 microphones, time domain) -------------
 * Replaces mca::TemporalGCCBinauralLocalisation(int sampleRate, ArrayDescription) (include/mcarray/BinauralLocalisation.h:43)
 * and its per-frame hook processParametrisation (src/mcarray/BinauralLocalisation.cpp:134-192), in double.  Frames of
 * W = (int)(2 * (0.075 * fs)) raw samples at hop W / 2; nd = (int)(distance(0,1) * fs / 346.1) delay pairs, each a
 * (2 nd + 1)-lag cross-correlation divided by the two deviations and summed in magnitude; + a small triangle, max-min
 * normalisation, first maximum -> DOA = samples2Degrees - 90 (degrees); the power gate of setPowerFloor / logPower;
 * _currentDOA = 0.5 _currentDOA + 0.5 DOA.  The [BUILD-DEFINES] decisions are listed in DESIGN.md.
 * Supported: 2 <= nd <= 32 and sample_rate <= 96000 (MCA_HIP_ERR_INVALID_ARGUMENT at create otherwise). */
typedef struct mca_hip_tgcc_ctx mca_hip_tgcc_ctx;
typedef struct {
    int struct_size;
    int device;
    int sample_rate;
    double mic_xyz[2][3];    /* metres */
    int use_power_floor;     /* 1 = the reference (3 s floor estimation, then the gate); 0 = every frame voiced, power = logPower */
    int max_arrays;          /* independent module objects (streams) this context holds state for, <= 65535 */
} mca_hip_tgcc_config;
int  mca_hip_tgcc_create(const mca_hip_tgcc_config *cfg, mca_hip_tgcc_ctx **out);
void mca_hip_tgcc_destroy(mca_hip_tgcc_ctx *ctx);
const char *mca_hip_tgcc_last_error(const mca_hip_tgcc_ctx *ctx);
int  mca_hip_tgcc_reset(mca_hip_tgcc_ctx *ctx, void *stream);     /* every array and the frame hook back to a new module */
/* window W (= analysis length), hop W / 2 and the number of delay pairs nd; any pointer may be NULL */
int  mca_hip_tgcc_get_geometry(const mca_hip_tgcc_ctx *ctx, int *window, int *hop, int *nd);
/* n_frames frames of arrays 0..n_arrays-1: array a, channel ch starts at pcm_dev + a * array_stride + ch * ch_stride and
 * holds (n_frames - 1) * hop + W samples; frame f starts at sample f * hop.  Each array continues its own state.
 * Per frame (all [arrays][F]): doa_deg = _currentDOA[0] after the frame (degrees), prob = _prob[0], voiced = 1 where setDOA
 * fires, power = the value handed to setDOA (during the floor estimation: the floor so far), delay_idx = the first-max
 * pair index, -1 on gated frames.  index [arrays][F][nd] = the normalised index of every frame (voiced or not).  Every
 * output except doa_deg may be NULL. */
int mca_hip_tgcc_frames_dev(mca_hip_tgcc_ctx *ctx, const float *pcm_dev, long long array_stride, long long ch_stride,
                            int n_arrays, int n_frames, float *doa_deg_dev, float *prob_dev, unsigned char *voiced_dev,
                            float *power_dev, int *delay_idx_dev, double *index_dev, void *stream);
/* the same from host memory: pcm [arrays][2][(n_frames - 1) * hop + W] */
int mca_hip_tgcc_frames_host(mca_hip_tgcc_ctx *ctx, const float *pcm, int n_arrays, int n_frames, float *doa_deg, float *prob,
                             unsigned char *voiced, float *power, int *delay_idx, double *index);
/* the per-frame hook processParametrisation: frames[0..1] = the two channels' double[length] analysis frames, length == W;
 * its own state (separate from every array's).  Outputs as above, in double; any may be NULL. */
int mca_hip_tgcc_process_frame(mca_hip_tgcc_ctx *ctx, const double *const *frames, int length, int *voiced, double *doa_deg,
                               double *prob, double *power, int *delay_idx, double *index);
/* checkpoint / resume as mca_hip_state_*: _currentDOA, _prob and the power-floor estimation of every array and of the hook */
long long mca_hip_tgcc_state_size(const mca_hip_tgcc_ctx *ctx);
int mca_hip_tgcc_state_save(mca_hip_tgcc_ctx *ctx, void *blob, long long blob_bytes);
int mca_hip_tgcc_state_load(mca_hip_tgcc_ctx *ctx, const void *blob, long long blob_bytes);

/* ---- MVDR-style beamformer with a per-bin spatial covariance (BASELINE.json configs[3]) ---------
 * [BUILD-DEFINES -- NO REFERENCE COUNTERPART]: the reference's only beamformer is the delay-and-sum of
 * mca::Beamformer::processFrame (src/mcarray/Beamformer.cpp:51-71); this module keeps its interface shape
 * (frames in, one output channel, a look direction in radians) and its steering convention (Beamformer.cpp:59:
 * x coordinate only, cos(DOA + pi/2); mca_hip_mvdr_set_geometry opts into all three coordinates), and replaces the uniform weights 1/M by the minimum-variance
 * distortionless-response weights of SURVEY A.9.  Per stream and bin k:
 *     Phi_t = alpha Phi_{t-1} + (1 - alpha) x x^H,   PhiL = Phi_t + loading tr(Phi_t)/M I,
 *     w = PhiL^-1 d / (d^H PhiL^-1 d),  d_m = exp(+j 2 pi k fs x_m sin(DOA) / (N c)),   Y[k] = w^H x.
 * A bin whose covariance trace is <= 1e-30 (digital silence so far) uses w = d/M, i.e. the reference's
 * delay-and-sum.  With alpha = 0 ... 1 and loading > 0 the response towards DOA is exactly 1 (w^H d = 1). */
typedef struct mca_hip_mvdr_ctx mca_hip_mvdr_ctx;
typedef struct {
    int struct_size;
    int device;
    int sample_rate;
    int fft_size;            /* N, power of two 64..8192 with n_mics spectra of N/2+1 bins within the 160 KiB LDS */
    int n_mics;              /* M, 2..16 */
    const double *mic_xyz;   /* [M][3] metres */
    double alpha;            /* covariance memory, SURVEY A.9: 0.95 */
    double loading;          /* diagonal loading relative to tr(Phi)/M, SURVEY A.9: 1e-3 */
    int max_streams;         /* independent streams whose covariance / overlap-add state the context holds */
} mca_hip_mvdr_config;
int  mca_hip_mvdr_create(const mca_hip_mvdr_config *cfg, mca_hip_mvdr_ctx **out);
void mca_hip_mvdr_destroy(mca_hip_mvdr_ctx *ctx);
const char *mca_hip_mvdr_last_error(const mca_hip_mvdr_ctx *ctx);
int  mca_hip_mvdr_reset(mca_hip_mvdr_ctx *ctx, void *stream);      /* Phi = 0, overlap-add tails = 0 */
/* STFT analysis + the recursion above + inverse FFT + overlap-add for n_frames consecutive frames of n_streams
 * independent M-microphone streams (PCM layout as in mca_hip_process_frames_dev).
 *   doa_rad_dev  [streams][F] float   look direction per frame (e.g. the doa_rad output of mca_hip_localise_frames_dev)
 *   out_pcm_dev  [streams][F*hop] float (may be NULL)
 *   out_spec_dev [streams][F][N/2+1] interleaved re,im float: the beamformed spectra Y (may be NULL) */
int mca_hip_mvdr_frames_dev(mca_hip_mvdr_ctx *ctx, const float *pcm_dev, long long stream_stride, long long mic_stride,
                            int n_streams, int n_frames, const float *doa_rad_dev, float *out_pcm_dev,
                            float *out_spec_dev, void *stream);
int mca_hip_mvdr_frames_host(mca_hip_mvdr_ctx *ctx, const float *pcm, int n_streams, int n_frames, const float *doa_rad,
                             float *out_pcm, float *out_spec);
/* Several look directions per frame from ONE analysis, covariance recursion and factorisation (e.g. the talkers a localiser with
 * n_sources > 1 reports).  Output s is what the single-look call gives on the same stream state with doa[:, :, s]; the covariance
 * afterwards is what any of those calls leaves.  Opt-in: mca_hip_mvdr_set_max_sources(ctx, 1 ... 4) gives every stream that many
 * overlap-add tails (slots both sizes have keep their content, new ones start at zero; default 1).
 *   doa_rad_dev  [streams][F][n_sources] float -- the layout mca_hip_localise_frames_dev writes
 *   out_pcm_dev  [streams][n_sources][F*hop] float (may be NULL)
 *   out_spec_dev [streams][n_sources][F][N/2+1] interleaved re,im float (may be NULL; not both)
 * n_sources <= the context's maximum.  The tail slots s >= n_sources of the streams in the call are zeroed: a source a call
 * leaves out restarts from silence.  The single-look entry points use slot 0 on any context, and n_sources = 1 here gives
 * their bytes.  A context with a maximum above 1 writes state blobs of a second version that also carry the extra tails and the
 * maximum; a blob loads only into a context with the maximum it was saved with. */
int mca_hip_mvdr_set_max_sources(mca_hip_mvdr_ctx *ctx, int max_sources);
int mca_hip_mvdr_sources_frames_dev(mca_hip_mvdr_ctx *ctx, const float *pcm_dev, long long stream_stride, long long mic_stride,
                                    int n_streams, int n_frames, int n_sources, const float *doa_rad_dev, float *out_pcm_dev,
                                    float *out_spec_dev, void *stream);
int mca_hip_mvdr_sources_frames_host(mca_hip_mvdr_ctx *ctx, const float *pcm, int n_streams, int n_frames, int n_sources,
                                     const float *doa_rad, float *out_pcm, float *out_spec);
/* Soft nulls at the other look directions of a mca_hip_mvdr_sources_frames_* call (n_sources >= 2).  With d_s the steering
 * vector of look direction s, PhiL the loaded covariance as above and g = null_gain >= 0, per stream, bin and frame:
 *     p_r   = 1 / (d_r^H PhiL^-1 d_r)                     the MVDR power estimate towards r
 *     Phi_s = PhiL + g * sum_{r != s} p_r d_r d_r^H        a virtual interferer at every other look direction, g times that power
 *     w_s   = Phi_s^-1 d_s / (d_s^H Phi_s^-1 d_s),  Y_s[k] = w_s^H x
 * g = 0 (the default) is the plain MVDR output of the call above, by the same kernel and with the same bytes; g -> infinity tends
 * to the hard LCMV nulls.  Every finite g is well posed, coincident directions, bin 0 (where all d_s are equal) and
 * n_sources > n_mics included: there the output tends to the plain MVDR output.  The response towards the own direction is 1 for
 * every g, and a bin in digital silence (trace <= 1e-30) keeps w = d/M per direction.
 * Accepted: finite values in [0, 1000]; anything else is MCA_HIP_ERR_INVALID_ARGUMENT and leaves the gain as it was (the output's
 * denominator cancels by up to 1 + g where directions coincide: fp32 eps * 1001 stays an order of magnitude under the 5e-4 of the
 * peak this module is held to).  The gain is a processing parameter, not stream state: it may change between calls, the
 * covariance a call leaves does not depend on it, state blobs neither carry nor check it.  With n_sources = 1 and through the
 * single-look entry points it has no effect. */
int mca_hip_mvdr_set_null_gain(mca_hip_mvdr_ctx *ctx, double null_gain);
int mca_hip_mvdr_get_null_gain(const mca_hip_mvdr_ctx *ctx, double *null_gain);
/* Per-frame covariance update weights: the covariance learns only where the caller lets it, e.g. where a voice-activity decision
 * says that the target is absent (a noise-only covariance: MVDR proper, where the unweighted recursion gives the minimum-power
 * beamformer that cancels a target whose look direction is a little off).
 *   update_dev [streams][F] float   one weight per stream and frame, for all look directions of the frame (they share one
 *                                   covariance); NULL = all 1
 * With u = fminf(fmaxf(update, 0), 1), per stream, bin and frame:
 *     a_t   = 1 - (1 - alpha) u_t
 *     Phi_t = a_t Phi_{t-1} + (1 - a_t) x x^H
 *     tr_t  = a_t tr_{t-1} + (1 - a_t) |x|^2
 * and everything behind the recursion is as stated above: the loading, the weights, the outputs, the delay-and-sum rule of a
 * trace <= 1e-30, the soft nulls and the Capon spectrum of the held covariance.  Nothing is refused on the device: a weight
 * below 0 counts as 0, one above 1 as 1, and a NaN as 0 (the fminf(fmaxf()) form).  Three points are exact:
 *   - u_t == 1 uses the context's own fp32 alpha and 1 - alpha and the operations of the unweighted call.  A call whose weights
 *     are all 1, or whose weight pointer is NULL, returns the bytes of mca_hip_mvdr_sources_frames_* and leaves the same
 *     covariance bytes;
 *   - u_t == 0 leaves Phi and tr bit for bit as they were.  The frame is still beamformed, with the frozen covariance and its
 *     own x and look directions;
 *   - a frozen fresh stream (tr = 0) gives the reference's delay-and-sum, as an unweighted call on silence does.
 * The weights are an input of the call like doa_rad, not stream state: state blobs neither carry nor check them.  n_sources = 1
 * on any context is the single-look form.  The argument checks are those of mca_hip_mvdr_sources_frames_dev; how a call is cut
 * into calls does not change its bytes.  The localisers' voiced[A][F] bytes become weights as INTEGRATION.md shows. */
int mca_hip_mvdr_sources_frames_weighted_dev(mca_hip_mvdr_ctx *ctx, const float *pcm_dev, long long stream_stride, long long mic_stride,
                                             int n_streams, int n_frames, int n_sources, const float *doa_rad_dev,
                                             const float *update_dev, float *out_pcm_dev, float *out_spec_dev, void *stream);
int mca_hip_mvdr_sources_frames_weighted_host(mca_hip_mvdr_ctx *ctx, const float *pcm, int n_streams, int n_frames, int n_sources,
                                              const float *doa_rad, const float *update, float *out_pcm, float *out_spec);
/* Time-frequency update masks: the same with one weight per stream, frame AND bin.  A target such as speech is sparse in time and
 * frequency: after its onset almost every frame holds it in some bins and only noise in the others, so no per-frame weight both
 * keeps the target and lets the covariance follow the noise.  The mask of a mask estimator, of a coherence or SNR
 * rule, or the expanded per-band decisions of the masking modules goes in as it is.
 *   update_mask_dev [streams][F][K] float   contiguous, K = N/2 + 1, for all look directions of the frame; NULL = all 1.  The
 *                                           index (a F + t) K + k is formed in 64 bits.
 * With u = fminf(fmaxf(update_mask[a][t][k], 0), 1) (a NaN counts as 0), per stream a, frame t and bin k:
 *     a_tk     = 1 - (1 - alpha) u
 *     Phi_t[k] = a_tk Phi_{t-1}[k] + (1 - a_tk) x[k] x[k]^H
 *     tr_t[k]  = a_tk tr_{t-1}[k] + (1 - a_tk) |x[k]|^2
 * and everything behind the recursion is as stated for the weighted call: the loading, the weights for one to four look
 * directions, the soft nulls, the post-filter (whose p, A and G are per bin already), the Capon spectrum of the held covariance,
 * and the delay-and-sum rule of a trace <= 1e-30 -- now per bin: a bin whose cells were all closed since the reset stays
 * delay-and-sum while its neighbours are MVDR.  Exact points:
 *   - a NULL mask, or a mask whose every cell is 1, gives the bytes of mca_hip_mvdr_sources_frames_* in spectra, audio,
 *     covariance, traces and post-filter state;
 *   - update_mask[a][t][k] == update[a][t] for all k gives the bytes of mca_hip_mvdr_sources_frames_weighted_* with that update;
 *   - a cell with u == 0 leaves Phi[k] and tr[k] bit for bit; the frame is still beamformed in that bin, and the other bins of the
 *     frame update;
 *   - the bytes of bin k (spectra, covariance) depend on column k of the mask only, whatever its neighbours' cells are;
 *   - how a stream is cut into calls does not change its bytes.
 * Per-frame weights and a mask are not combined: a caller who has both multiplies them.  The mask is an input of the call: state
 * blobs neither carry nor check it.  The argument checks are those of the weighted call; n_sources = 1 on any context is the
 * single-look form.  The host call stages the mask in a stage slot of its own. */
int mca_hip_mvdr_sources_frames_masked_dev(mca_hip_mvdr_ctx *ctx, const float *pcm_dev, long long stream_stride, long long mic_stride,
                                           int n_streams, int n_frames, int n_sources, const float *doa_rad_dev,
                                           const float *update_mask_dev, float *out_pcm_dev, float *out_spec_dev, void *stream);
int mca_hip_mvdr_sources_frames_masked_host(mca_hip_mvdr_ctx *ctx, const float *pcm, int n_streams, int n_frames, int n_sources,
                                            const float *doa_rad, const float *update_mask, float *out_pcm, float *out_spec);
/* Decision-directed Wiener post-filter on the beamformed spectra: the single-channel stage that turns an MVDR with a noise-only
 * covariance (the update weights above) into the multichannel Wiener filter.  MVDR removes what is spatially separable; the
 * residual noise at its output has the power 1 / (d^H PhiL^-1 d), the p_r of the soft nulls.  Per stream, output slot s (look
 * direction), bin k and frame t, with Y the output of the call as stated above (plain, sources or nulls; weighted or not), PhiL_t
 * the loaded covariance AFTER the frame's update, tr_t its trace and d_s the frame's steering vector:
 *     p   = noise_scale / (d_s^H PhiL_t^-1 d_s)      if tr_t > 1e-30, else 0
 *           (for every null gain the PLAIN estimate p_s of the soft-null definition, not the nulled denominator)
 *     N   = smoothing * A_{t-1} + (1 - smoothing) * max(|Y|^2 - p, 0)
 *     G   = 1                                        if p == 0   (digital silence so far: delay-and-sum, nothing to subtract)
 *           fmaxf(gain_floor, N / (N + p))           otherwise   (N + p > 0 there)
 *     Z   = G * Y,      A_t = |Z|^2
 * the decision-directed Wiener gain with a priori SNR N/p, written without a division by p.  out_spec and out_pcm carry Z in
 * place of Y; the covariance, its trace, the Capon spectrum and the update weights are untouched by the filter.
 * A is stream state: fp32 [max_streams][max_sources][K], zero on a fresh context, after mca_hip_mvdr_reset and on enabling.  The
 * slots s >= n_sources of the streams in a call are zeroed by that call, whether it has out_pcm or not (the tails' rule: a source
 * that a call leaves out restarts from silence); the single-look entry points use slot 0; mca_hip_mvdr_set_max_sources on an
 * enabled context keeps the slots that both sizes have and zeroes the others, as it does for the tails.
 * Accepted, all finite: smoothing in [0, 1) (default 0.98), gain_floor in [0, 1] (default 0.1), noise_scale in (0, 100] (default
 * 1); anything else, a wrong struct_size included, is MCA_HIP_ERR_INVALID_ARGUMENT and leaves configuration and state as they were.
 * The three values are processing parameters like the null gain: they may change between calls without touching A, state blobs
 * neither carry nor check them.  enable 1 -> 0 frees A, 0 -> 1 starts from zero.  All six mca_hip_mvdr_*frames* calls honour the
 * setting.  Exact points:
 *   - disabled (the default) is the call as it was: the same kernels launched, the same bytes;
 *   - gain_floor == 1 gives the bytes of the disabled call (fmaxf(1, x <= 1) == 1 and 1 * Y is exact), in spectra and audio, and
 *     the same covariance bytes;
 *   - how a stream is cut into calls does not change its bytes.
 * State blobs: an enabled context writes version 3 -- covariances, traces, tails, then A, host[0] = max_sources, host[1] = 1 -- which
 * loads only into an enabled context with the same max_sources.  Version 1 and 2 blobs are refused by an enabled context, a
 * version 3 blob by a disabled one (MCA_HIP_ERR_INVALID_ARGUMENT, the state untouched); disabled contexts read and write what
 * they always did. */
typedef struct {
    int struct_size;
    int enable;
    double smoothing;
    double gain_floor;
    double noise_scale;
} mca_hip_mvdr_postfilter_config;
int mca_hip_mvdr_set_postfilter(mca_hip_mvdr_ctx *ctx, const mca_hip_mvdr_postfilter_config *cfg);
int mca_hip_mvdr_get_postfilter(const mca_hip_mvdr_ctx *ctx, mca_hip_mvdr_postfilter_config *cfg);
/* Steering vectors estimated from the data: the relative transfer function (RTF) towards a reference microphone, from a second
 * covariance kept over the cells in which the target is present.  The geometric vector d_m = exp(-j k ... x_m cos(theta + pi/2)) of
 * every other call knows nothing of microphone gains, position errors or a look direction a few degrees off, and a distortionless
 * constraint towards the wrong vector distorts the target whatever the noise covariance does.  A target mask is
 * the same kind of array as the update mask: INTEGRATION.md says how a mask estimator's output becomes the two.
 * State of an enabled context, fp32: Psi [max_streams][max_sources][K] packed triangles, stored as Phi is; cpsi
 * [max_streams][max_sources][K] and cphi [max_streams][K], the sums of the weights that Psi and Phi hold.  On enabling Psi = 0,
 * cpsi = 0 and cphi = 1 where the bin's trace is > 1e-30, else 0; after mca_hip_mvdr_reset all are zero;
 * mca_hip_mvdr_set_max_sources keeps the slots that both sizes have and zeroes the others; the slots s >= n_sources of the streams
 * in a mca_hip_mvdr_sources_frames_rtf_* call are zeroed by that call (the tails' rule).
 * Per stream a, slot s, bin k and frame t, with x the frame's spectra, u and a_tk of the masked call above,
 * m = fminf(fmaxf(target_mask[a][s][t][k], 0), 1) (a NaN counts as 0), b = 1 - (1 - target_alpha) m, g0 the geometric vector of
 * doa_rad[a][t][s]:
 *     Phi_t, tr_t   exactly the masked call's recursion under update_mask
 *     cphi_t = a_tk cphi + (1 - a_tk)                                   (untouched where u == 0)
 *     Psi_t  = b Psi + (1 - b) x x^H,   cpsi_t = b cpsi + (1 - b)        (both untouched, bit for bit, where m == 0)
 *     tau    = tr(Psi_t) / cpsi_t                                        needs cpsi_t > 0 and tau > 1e-30
 *     Delta  = Psi_t / (cpsi_t tau) - [cphi_t > 0] Phi_t / (cphi_t tau)
 *     v = g0 / sqrt(M);  `iterations` times:  g = Delta v,  n = |g|^2 (needs n > 1e-20),  v_prev = v,  v = g / sqrt(n)
 *     rho    = Re(v_prev^H g)                                            needs rho > min_share
 *                                                                        needs |g[ref_mic]|^2 > 1e-6 n
 *     d      = g / g[ref_mic]                                            the RTF: d[ref_mic] = 1
 *     any "needs" not met, or a non-finite value: d = g0
 *     w = PhiL_t^-1 d / (d^H PhiL_t^-1 d),  Y = w^H x                    with the loaded covariance as everywhere
 * The output is the target as the reference microphone records it.  A bin whose noise trace is <= 1e-30 keeps the delay-and-sum
 * with the GEOMETRIC vector (w = g0 / M).  The post-filter's p is noise_scale / (d^H PhiL^-1 d) with the d the frame used.
 * Accepted, all finite: target_alpha in [0, 1) (default: the context's alpha), iterations 1 ... 4 (default 2), ref_mic 0 ... M-1
 * (default 0), min_share in [0, 1) (default 0.05); anything else, a wrong struct_size included, is MCA_HIP_ERR_INVALID_ARGUMENT and
 * leaves configuration and state as they were.  The four values are processing parameters like the null gain; enable 0 -> 1
 * allocates the state as stated, 1 -> 0 frees it.
 *   target_mask_dev [streams][n_sources][F][K] float   contiguous; NULL = all 0: nothing is learned and the held Psi steers
 *   update_mask_dev [streams][F][K] float              as in the masked call; NULL = all 1
 * mca_hip_mvdr_sources_frames_rtf_* on a context without RTF enabled is MCA_HIP_ERR_INVALID_ARGUMENT; with a null gain != 0 it is
 * MCA_HIP_ERR_UNSUPPORTED unless mca_hip_mvdr_set_rtf_nulls (below) has enabled nulls at estimated vectors; the other argument checks are those of the masked call.  The
 * steering plane [streams][n_sources][frames][K][M] (8 bytes each) is workspace with a cap of 1 GiB
 * (mca_hip_mvdr_set_rtf_workspace(ctx, max_bytes >= 8) sets another; a processing parameter): a call above it is cut along the
 * frames internally, a frame at a time at the least, which changes no byte.  The host call stages both masks.  Exact points:
 *   - with a NULL or all-zero target mask on fresh RTF state the call gives the bytes of mca_hip_mvdr_sources_frames_masked_* under
 *     the same update mask, in spectra, audio and covariance;
 *   - the bytes of bin k depend on column k of both masks only; how a stream is cut into calls, and where it sits in the batch, do
 *     not change its bytes.
 * The six other mca_hip_mvdr_*frames* calls are untouched on any context, enabled or not: the same kernels launched, geometric
 * steering, Psi, cpsi and cphi not advanced.  cphi therefore UNDER-COUNTS the weights in Phi when entry points are mixed on one
 * stream: keep a stream on the RTF entry point while RTF is enabled.
 * State blobs: an RTF-enabled context writes version 4 -- covariances, traces, tails, A if the post-filter is enabled, then Psi, cpsi
 * and cphi; host[0] = max_sources, host[1] = post-filter enabled, host[2] = 1 -- which loads only into a context with the same
 * max_sources, post-filter enablement and RTF enablement; every other combination is refused with the state untouched
 * (MCA_HIP_ERR_INVALID_ARGUMENT).  Contexts without RTF read and write what they always did. */
typedef struct {
    int struct_size;
    int enable;
    double target_alpha;
    int iterations;
    int ref_mic;
    double min_share;
} mca_hip_mvdr_rtf_config;
int mca_hip_mvdr_set_rtf(mca_hip_mvdr_ctx *ctx, const mca_hip_mvdr_rtf_config *cfg);
int mca_hip_mvdr_get_rtf(const mca_hip_mvdr_ctx *ctx, mca_hip_mvdr_rtf_config *cfg);
int mca_hip_mvdr_set_rtf_workspace(mca_hip_mvdr_ctx *ctx, long long max_bytes);
int mca_hip_mvdr_sources_frames_rtf_dev(mca_hip_mvdr_ctx *ctx, const float *pcm_dev, long long stream_stride, long long mic_stride,
                                        int n_streams, int n_frames, int n_sources, const float *doa_rad_dev,
                                        const float *update_mask_dev, const float *target_mask_dev, float *out_pcm_dev,
                                        float *out_spec_dev, void *stream);
int mca_hip_mvdr_sources_frames_rtf_host(mca_hip_mvdr_ctx *ctx, const float *pcm, int n_streams, int n_frames, int n_sources,
                                         const float *doa_rad, const float *update_mask, const float *target_mask, float *out_pcm,
                                         float *out_spec);
/* the estimator above on the state the context holds now, for look direction doa_rad: out [K][M] interleaved re,im double,
 * estimated [K] bytes (1: the RTF, 0: the geometric vector).  A pure function of state and configuration, like the spectrum call;
 * the silence rule of the frames call is not part of it.  RTF must be enabled; source in 0 ... max_sources - 1. */
int mca_hip_mvdr_get_steering(mca_hip_mvdr_ctx *ctx, int stream_index, int source, double doa_rad, double *out, unsigned char *estimated);
/* copy of the target covariance of one stream and slot: out [K][M][M] interleaved re,im double (full Hermitian matrices), norm [K]
 * double (cpsi); either may be NULL, not both */
int mca_hip_mvdr_get_target_covariance(mca_hip_mvdr_ctx *ctx, int stream_index, int source, double *out, double *norm);
/* Masks estimated on the device from the call's own spectra: the update mask of the masked call and the target masks of the RTF
 * call, formed by the steered coherence of every cell towards the call's look directions, between the analysis and the rest of the
 * call (k_mvdr_estmask).  No second transform, no host step: the look directions may be the peaks the Capon spectrum
 * returned for the chunk before.  Per stream a, frame t and bin k, with x the frame's M spectra of that bin, g_s the
 * geometric steering vector of doa_rad[a][t][s] as everywhere in this module, and S the call's n_sources:
 *     e    = sum_m |x_m|^2
 *     c_s  = |g_s^H x|^2 / (M e)                 in [0, 1]; 0 for every s where e <= 1e-30
 *     w    = the s with the largest c_s, searched s = 0 ... S-1 with a strict '>' (ties and NaNs stay with the lower index)
 *     v    = fminf(fmaxf((c_w - coherence_lo) / (coherence_hi - coherence_lo), 0), 1)        (a NaN counts as 0)
 *     target_mask[a][s][t][k] = v if s == w, else 0
 *     update_mask[a][t][k]    = 1 - max over s < P of target_mask[a][s][t][k]
 *                               P = n_protected, or S where n_protected is 0 or above S
 * Outside the band [bin_lo, bin_hi] every target mask is 0 and the update mask is 1: the plain recursion, meant for the lowest bins,
 * where all steering vectors coincide and the assignment means nothing.  Look directions s >= P are competitors: directions of known
 * interferers (further Capon peaks, say) that take cells away from the protected sources and get their own target mask and output,
 * but do not close the noise covariance.  The estimator is stateless: the masks of bin k of frame t depend on that cell's spectra
 * and on the frame's look directions only; nothing is added to the stream state or to state blobs.
 * Accepted, all finite: 0 <= bin_lo <= bin_hi <= N/2 (defaults 0 and N/2); 0 <= coherence_lo < coherence_hi <= 1 with
 * coherence_hi - coherence_lo >= 1e-3 (defaults 0 and 0.05: RELATIVE thresholds, for calls in which a competitor takes the cells
 * that are not the target's -- a call with ONE look direction has no competitor and needs absolute thresholds such as 0.2 / 0.4);
 * n_protected 0 ... 4 (default 0: all).  Anything else, a wrong struct_size included, is MCA_HIP_ERR_INVALID_ARGUMENT and leaves the
 * configuration as it was.  The values are processing parameters like the null gain; enable allocates (with the first call, growing
 * with the call's shape) or frees the mask workspace, and opens timing slot 6.
 *   update_mask_out_dev [streams][F][K] float                 contiguous; NULL: the mask lives in the workspace only
 *   target_mask_out_dev [streams][n_sources][F][K] float      contiguous; NULL likewise
 * mca_hip_mvdr_sources_frames_auto_* runs the analysis once, the estimator over the whole call, and then
 *   - on a context with RTF enabled exactly what mca_hip_mvdr_sources_frames_rtf_* does with these two masks, the cut along the frames
 *     under the workspace cap included (the masks are formed once ahead of the chunks, as the analysis is);
 *   - on a context without RTF exactly what mca_hip_mvdr_sources_frames_masked_* does with the update mask (the target masks are
 *     still written if asked for).
 * The bytes of spectra, audio and state are those of that call fed the masks this one returns.  Without the estimator enabled the
 * call is MCA_HIP_ERR_INVALID_ARGUMENT; whatever the underlying call refuses is refused with that call's code (a null gain with RTF and
 * without mca_hip_mvdr_set_rtf_nulls: MCA_HIP_ERR_UNSUPPORTED).  The seven other mca_hip_mvdr_*frames* calls are untouched on any context: the same kernels launched, the
 * same bytes.  The host call stages the masks it hands back. */
typedef struct {
    int struct_size;
    int enable;
    int bin_lo, bin_hi;      /* the band, both ends included */
    double coherence_lo;
    double coherence_hi;
    int n_protected;
} mca_hip_mvdr_estmask_config;
int mca_hip_mvdr_set_mask_estimator(mca_hip_mvdr_ctx *ctx, const mca_hip_mvdr_estmask_config *cfg);
int mca_hip_mvdr_get_mask_estimator(const mca_hip_mvdr_ctx *ctx, mca_hip_mvdr_estmask_config *cfg);
int mca_hip_mvdr_sources_frames_auto_dev(mca_hip_mvdr_ctx *ctx, const float *pcm_dev, long long stream_stride, long long mic_stride,
                                         int n_streams, int n_frames, int n_sources, const float *doa_rad_dev,
                                         float *update_mask_out_dev, float *target_mask_out_dev, float *out_pcm_dev, float *out_spec_dev, void *stream);
int mca_hip_mvdr_sources_frames_auto_host(mca_hip_mvdr_ctx *ctx, const float *pcm, int n_streams, int n_frames, int n_sources,
                                          const float *doa_rad, float *update_mask_out, float *target_mask_out, float *out_pcm, float *out_spec);
/* Soft nulls at ESTIMATED steering vectors: with enable = 1 the calls that steer by the RTF -- mca_hip_mvdr_sources_frames_rtf_* and,
 * on a context with RTF enabled, mca_hip_mvdr_sources_frames_auto_* -- honour the null gain (mca_hip_mvdr_set_null_gain) instead of
 * refusing it.  A talker whose cells the update mask protects is kept out of the noise covariance, so the weights of output s do
 * nothing against talker r; the null puts it back as a virtual interferer along the vector the frame itself uses for r (DESIGN.md
 * 4.10).  Per stream, bin and frame, with d_s the vector the frame uses for slot s -- the RTF, or g0 where the estimator fell back:
 * exactly what the estimator above left for the solve -- PhiL the loaded covariance and g = null_gain:
 *     p_r   = 1 / (d_r^H PhiL^-1 d_r)
 *     Phi_s = PhiL + g * sum_{r != s} p_r d_r d_r^H
 *     w_s   = Phi_s^-1 d_s / (d_s^H Phi_s^-1 d_s),  Y_s = w_s^H x
 *   - scale: p_r d_r d_r^H does not depend on the scale of d_r, so the normalisation of the RTF to the reference microphone does not
 *     enter the nulls; it sets only the scale of the own output, as without nulls (w_s^H d_s = 1 for every g);
 *   - a bin whose noise trace is <= 1e-30 keeps w = g0 / M per direction;
 *   - the post-filter's p stays the plain noise_scale / (d_s^H PhiL^-1 d_s) with the d_s the frame used, as under geometric nulls;
 *   - the recursions of Phi, tr, Psi, cpsi and cphi see neither the gain nor this switch: the state a call leaves is the same bytes
 *     for every g (the exceptions follow the output: the post-filter's A, and the overlap-add tails of a call with out_pcm);
 *   - g == 0, a gain that rounds to 0 in fp32, or n_sources == 1 launch the kernels of the call without nulls and give its bytes,
 *     whatever the switch is;
 *   - on fresh RTF state with a NULL target mask every d is g0, and the RTF call gives the bytes of
 *     mca_hip_mvdr_sources_frames_masked_* under the same update mask and the same g, in spectra, audio and covariance;
 *   - how a stream is cut into calls, the workspace cap and where a stream sits in the batch change no byte, as without nulls.
 * With enable = 0 (the default) those calls are as they were: a null gain != 0 is MCA_HIP_ERR_UNSUPPORTED.  The seven other
 * mca_hip_mvdr_*frames* calls are untouched by the switch, the auto call on a context without RTF among them (it honours the null
 * gain at the geometric vectors, through the masked call).  Accepted: 0 or 1; anything else is MCA_HIP_ERR_INVALID_ARGUMENT and
 * leaves the switch as it was.  A processing parameter like the null gain: it may change between calls, may be set whether or not
 * RTF is enabled, and state blobs neither carry nor check it. */
int mca_hip_mvdr_set_rtf_nulls(mca_hip_mvdr_ctx *ctx, int enable);
int mca_hip_mvdr_get_rtf_nulls(const mca_hip_mvdr_ctx *ctx, int *enable);
/* Capon (minimum-variance) spatial spectrum of the covariance the context holds now (after its last frames call or state load),
 * and its peaks: the MVDR power estimate p = 1 / (d^H PhiL^-1 d) of the nulls above on a grid of angles.  Per stream, with
 *     theta_i      = -pi/2 + i pi/(D-1), i = 0 ... D-1 (in double),       D = n_angles
 *     d(theta,k)_m = exp(-j k 2 pi fs/(N c) x_m cos(theta + pi/2))        the steering of this module (Beamformer.cpp:59)
 *     PhiL[k]      = Phi[k] + loading tr[k]/M I                           the module's loading
 *     q[k][i]      = d(theta_i,k)^H PhiL[k]^-1 d(theta_i,k)               real, > 0
 *     P[i]         = sum over k in [bin_lo, bin_hi] with tr[k] > 1e-30 of w[k] / q[k][i]
 * MCA_HIP_MVDR_SPECTRUM_POWER: w[k] = 1, the sum of the per-bin Capon power estimates.  MCA_HIP_MVDR_SPECTRUM_NORMALISED:
 * w[k] = M / tr[k], every bin weighted by its own level (the PHAT-like choice; a spatially white bin adds (1 + loading)/M at every
 * angle).  Bins in digital silence (trace <= 1e-30) add nothing; a stream with no live bin in the band has P = 0 everywhere.
 * Peaks: i is a local maximum if P[i] > 0, P[i] > P[i-1] (or i = 0) and P[i] >= P[i+1] (or i = D-1); local maxima are ranked by
 * value, descending, ties to the lower index; slot r < n_peaks gets peak_doa[r] = (float) theta_i and peak_val[r] = P[i].  Slots
 * beyond the number of local maxima get peak_val = 0 and the peak_doa of slot 0 (0.0 rad if there is no local maximum at all):
 * repeating slot 0 is safe to hand to mca_hip_mvdr_sources_frames_*, where coincident directions are well posed.  A peak angle
 * means what every other look direction of this module means.
 * Accepted: n_angles 2 ... 361, 0 <= bin_lo <= bin_hi <= N/2, weighting 0 or 1, n_peaks 1 ... 4 (the most look directions a call carries); anything else is
 * MCA_HIP_ERR_INVALID_ARGUMENT and leaves the former configuration in place.  A spectrum call before configure, with n_streams
 * outside 1 ... max_streams or with all three outputs NULL is MCA_HIP_ERR_INVALID_ARGUMENT.  Streams 0 ... n_streams-1 are
 * scanned.  The configuration is a processing parameter like the null gain: it may change between calls, state blobs neither
 * carry nor check it.  The call reads the stream state and writes none of it; its result is a pure function of state and
 * configuration (no atomics: the same bytes on every run).
 *   spectrum_dev [streams][D] float, peak_doa_dev / peak_val_dev [streams][n_peaks] float; each may be NULL, not all three */
#define MCA_HIP_MVDR_SPECTRUM_POWER 0
#define MCA_HIP_MVDR_SPECTRUM_NORMALISED 1
typedef struct {
    int struct_size;
    int n_angles;            /* D */
    int bin_lo, bin_hi;      /* the band, both ends included */
    int weighting;           /* MCA_HIP_MVDR_SPECTRUM_POWER / _NORMALISED */
    int n_peaks;
} mca_hip_mvdr_spectrum_config;
int mca_hip_mvdr_spectrum_configure(mca_hip_mvdr_ctx *ctx, const mca_hip_mvdr_spectrum_config *cfg);
int mca_hip_mvdr_spectrum_get_grid(const mca_hip_mvdr_ctx *ctx, float *doa_rad);      /* [D] (float) theta_i */
int mca_hip_mvdr_spectrum_dev(mca_hip_mvdr_ctx *ctx, int n_streams, float *spectrum_dev, float *peak_doa_dev, float *peak_val_dev,
                              void *stream);
int mca_hip_mvdr_spectrum_host(mca_hip_mvdr_ctx *ctx, int n_streams, float *spectrum, float *peak_doa, float *peak_val);
/* The Capon spectrum on a grid of azimuths x elevations (XYZ geometry only; mca_hip_mvdr_set_geometry below defines e(theta, eps) and
 * the phase).  The spectrum above scans the one cone of the context's elevation: a talker off that elevation shows at a biased
 * azimuth with a lowered peak, and no call tells the elevation.  Per stream, with
 *     theta_i = -pi + i 2 pi / n_az, i = 0 ... n_az-1                    the periodic grid of XYZ mode (in double)
 *     eps_j   = el_lo + j step, step = (el_hi - el_lo)/(n_el - 1)         j = 0 ... n_el-1 (in double; n_el == 1: eps_0 = el_lo)
 *     P[j][i] = sum over k in [bin_lo, bin_hi] with tr[k] > 1e-30 of w[k] / (d^H PhiL[k]^-1 d),   d = d(theta_i, eps_j, k)
 * d is the XYZ steering vector of set_geometry with cos eps_j, sin eps_j in place of the context's, its phase formed in double the
 * same way; PhiL, w[k] (weighting), the silence threshold and the zero map of a stream with no live bin in the band are the
 * spectrum's.  With n_el = 1 and el_lo = el_hi = the context's elevation, map, peak azimuths and peak values are the bytes of
 * mca_hip_mvdr_spectrum_dev with n_angles = n_az.
 * Peaks: the neighbours of cell (j, i) are the 8 cells around it, periodic in azimuth ((i +- 1) mod n_az), none beyond rows 0 and
 * n_el-1.  (j, i) is a local maximum if P > 0, P is strictly greater than (j, i-1) and the three cells of row j-1, and P is >=
 * (j, i+1) and the three cells of row j+1: a plateau counts once.  With n_el = 1 this is the circular rule of the spectrum in XYZ
 * mode.  Local maxima are ranked by value, descending, ties to the lower flat index j n_az + i; slot r < n_peaks gets
 * peak_az[r] = (float) theta_i, peak_el[r] = (float) eps_j, peak_val[r] = P[j][i].  Slots beyond the number of local maxima get
 * peak_val = 0 and the angles of slot 0; if there is no local maximum at all, azimuth 0.0 and (float) the context's elevation.  A
 * row at exactly +-pi/2 is one direction n_az times over: its cells differ by rounding alone, and which of them is picked there,
 * if any, is decided by that rounding.
 * Accepted: struct_size as compiled, XYZ geometry, n_az 3 ... 360, n_el 1 ... 91, n_az n_el <= 2048, el_lo and el_hi finite with
 * -pi/2 <= el_lo <= el_hi <= pi/2 and el_lo == el_hi where n_el == 1, the band, weighting and n_peaks as for the spectrum; anything
 * else is MCA_HIP_ERR_INVALID_ARGUMENT and leaves the former configuration in place.  A map call before configure, with n_streams
 * outside 1 ... max_streams or with all four outputs NULL is MCA_HIP_ERR_INVALID_ARGUMENT.  A geometry change un-configures the
 * map, as it does the spectrum.  The configuration is a processing parameter: state blobs neither carry nor check it.  The call
 * reads the stream state and writes none of it; no atomics: the same bytes on every run, wherever a stream sits in the batch and
 * whatever n_streams is.  The partial sums of the scan are workspace taken in passes of streams under the cap of
 * mca_hip_mvdr_set_rtf_workspace (one stream a pass at the least); the cap changes no byte.  Timing: kernel_id 8.
 *   map_dev [streams][n_el][n_az] float, peak_az_dev / peak_el_dev / peak_val_dev [streams][n_peaks] float; each may be NULL, not all */
typedef struct {
    int struct_size;
    int n_az;                /* 3 ... 360 */
    int n_el;                /* 1 ... 91; n_az n_el <= 2048 */
    double el_lo_rad, el_hi_rad;   /* -pi/2 <= el_lo <= el_hi <= pi/2; n_el == 1 needs el_lo == el_hi */
    int bin_lo, bin_hi;      /* the band, both ends included */
    int weighting;           /* MCA_HIP_MVDR_SPECTRUM_POWER / _NORMALISED */
    int n_peaks;
} mca_hip_mvdr_map_config;
int mca_hip_mvdr_map_configure(mca_hip_mvdr_ctx *ctx, const mca_hip_mvdr_map_config *cfg);
int mca_hip_mvdr_map_get_grid(const mca_hip_mvdr_ctx *ctx, float *az, float *el);   /* [n_az] (float) theta_i, [n_el] (float) eps_j; either may be NULL */
int mca_hip_mvdr_map_dev(mca_hip_mvdr_ctx *ctx, int n_streams, float *map_dev, float *peak_az_dev, float *peak_el_dev, float *peak_val_dev,
                         void *stream);
int mca_hip_mvdr_map_host(mca_hip_mvdr_ctx *ctx, int n_streams, float *map, float *peak_az, float *peak_el, float *peak_val);
/* Tracks of the look directions, kept on the device between chunks: which talker owns which slot.  The spectrum's peaks are ranked
 * by value, so two talkers swap slots when their levels cross -- and a slot is more than an output index: it owns a target covariance
 * Psi and cpsi, the RTF estimated from it, a place among the first n_protected directions of the mask estimator and the null aimed
 * at it.  A context with tracks configured holds, per stream and slot s < n_tracks: theta (float, rad), alive (0/1), miss (int,
 * updates in a row without a match) and gen (int, incremented by every seed and birth: a new gen means a new talker in the slot).
 * All are zero after configure, after mca_hip_mvdr_reset and after mca_hip_mvdr_state_load: state blobs do not carry the tracks and
 * keep their versions; a loaded context is seeded again.
 *
 * Slots s < n_own are OWN tracks: talkers to keep, whom the update mask keeps out of Phi and who therefore fade from the Capon
 * spectrum.  They follow a steered spectrum of their own estimated steering vector.  For every stream, own slot s that is alive and
 * bin k of the spectrum's band, the estimator of mca_hip_mvdr_set_rtf runs on the held state (Psi_s, cpsi_s, Phi, cphi) with the
 * context's iterations, ref_mic and min_share; g0 is the geometric vector the frames calls form for doa = theta_s (the steering
 * tables of the analysis, operation for operation).  A bin is USED if the estimator did not fall back and the bin's noise trace is
 * > 1e-30.  With d the estimate, u = d / |d| and d(theta_i, k) the grid vectors of the Capon spectrum (its phasor table):
 *     T_s[i] = sum over the used bins k of |d(theta_i,k)^H u_k|^2 / M        every used bin adds a value in [0, 1]
 *     phi_s  = the grid angle that maximises T_s among the angles with |theta_i - theta_s| <= max_step_rad (both as float, the
 *              comparison in float, the lower index wins ties); NaN if no bin is used, if no grid angle lies in the window or if
 *              the maximum is not > 0
 * The slots n_own <= s < n_tracks follow the Capon peaks of the call -- exactly those of mca_hip_mvdr_spectrum_dev, from the same
 * kernels, n_peaks of them.
 *
 * The association, per stream, all in float32 (mca_hip_mvdr_tracks_associate_dev runs it on candidates the caller gives -- the picks of
 * an SRP-PHAT context for instance; mca_hip_mvdr_tracks_update_dev on phi and the Capon peaks):
 *   1. own slots: s < n_own, alive and own_doa[s] finite: theta_s += clamp(own_doa[s] - theta_s, +-max_step_rad), miss = 0.  An
 *      alive own slot without a finite own_doa: miss += 1.  Own tracks are never released; a dead own slot stays dead, untouched,
 *      until it is seeded.
 *   2. candidates in the order given: one whose val is not > 0 or whose angle psi is not finite is skipped; so is one within
 *      min_sep_rad of an alive own track (|psi - theta_s| <= min_sep_rad, the updated angle): that is the talker, not an
 *      interferer.  Otherwise the nearest slot among the alive slots s >= n_own not yet matched in this call with
 *      |psi - theta_s| <= max_step_rad, the lower slot winning ties, takes theta = psi, miss = 0 and is matched.  If there is none
 *      the candidate waits as a birth.
 *   3. alive slots s >= n_own that were not matched: miss += 1; if miss > hold, alive = 0.
 *   4. births in candidate order: the lowest slot s >= n_own with alive == 0 (one released in step 3 among them) takes theta = psi,
 *      alive = 1, miss = 0, gen += 1; on a context with RTF enabled Psi and cpsi of that slot are set to zero -- they belong to
 *      whoever held the slot before.  Candidates without a free slot are dropped.
 * mca_hip_mvdr_tracks_seed_*: doa[streams][n_tracks]; a finite value sets theta, alive = 1, miss = 0, gen += 1 and leaves Psi alone;
 * a NaN (or an infinity) leaves the slot as it is.  mca_hip_mvdr_tracks_fill_dev writes the doa_rad array of the next frames call,
 * [streams][n_frames][n_tracks]: theta of every alive slot for every frame; a dead slot reports theta of the lowest alive slot, or
 * 0 rad if none is alive (coincident directions are well posed everywhere).  mca_hip_mvdr_tracks_get copies [streams][n_tracks] of each
 * array that is not NULL to the host (it synchronises the device).
 *   own_spectrum_dev [streams][n_own][D] float: T_s, or NULL; own_used_dev [streams][n_own][N/2+1] bytes: used, or NULL (0 outside the
 *   band; both all zero for a dead slot); neither is touched when n_own == 0
 * Accepted: struct_size as compiled, enable 0 or 1, n_tracks 1 ... max_sources, n_own 0 ... n_tracks, max_step_rad in (0, pi],
 * min_sep_rad in [0, pi], hold 0 ... 1000, all finite; the spectrum configured first (its grid, band and n_peaks are the ones the
 * tracks use, as they are at the time of a call); n_own > 0 needs RTF enabled.  Anything else is MCA_HIP_ERR_INVALID_ARGUMENT and
 * leaves configuration and state as they were.  seed, update, associate, fill and get before a configure with enable = 1, with
 * n_streams outside 1 ... max_streams, n_cand outside 1 ... 8 or a NULL array they need are MCA_HIP_ERR_INVALID_ARGUMENT.  Disabling RTF
 * disables the tracks, and so does mca_hip_mvdr_set_max_sources below n_tracks; they are configured anew.
 * update, fill and get change no byte of Phi, tr, Psi, cpsi, cphi or the tails, but Psi and cpsi of a slot at its birth.  The result
 * is a pure function of state and configuration (no atomics) and does not depend on where a stream sits in the batch.  No
 * mca_hip_mvdr_*frames* or spectrum call changes behaviour or bytes.  Timing: kernel_id 7 = the track kernels (the Capon kernels of an
 * update count under 3; an update with n_own == n_tracks launches none, since no peak can change an own track); it exists on a context that has had tracks configured at some time. */
typedef struct {
    int struct_size;
    int enable;
    int n_tracks;            /* 1 ... max_sources */
    int n_own;               /* 0 ... n_tracks: slots that follow their own target covariance; > 0 needs RTF enabled */
    double max_step_rad;     /* (0, pi]: association gate and search window */
    double min_sep_rad;      /* [0, pi]: a Capon peak this close to an own track is that talker, not an interferer */
    int hold;                /* 0 ... 1000: updates an unmatched interferer track keeps its direction */
} mca_hip_mvdr_tracks_config;
int mca_hip_mvdr_tracks_configure(mca_hip_mvdr_ctx *ctx, const mca_hip_mvdr_tracks_config *cfg);
int mca_hip_mvdr_tracks_get_config(const mca_hip_mvdr_ctx *ctx, mca_hip_mvdr_tracks_config *cfg);
int mca_hip_mvdr_tracks_seed_dev(mca_hip_mvdr_ctx *ctx, int n_streams, const float *doa_dev, void *stream);
int mca_hip_mvdr_tracks_seed_host(mca_hip_mvdr_ctx *ctx, int n_streams, const float *doa);
int mca_hip_mvdr_tracks_update_dev(mca_hip_mvdr_ctx *ctx, int n_streams, float *own_spectrum_dev, unsigned char *own_used_dev, void *stream);
int mca_hip_mvdr_tracks_update_host(mca_hip_mvdr_ctx *ctx, int n_streams, float *own_spectrum, unsigned char *own_used);
int mca_hip_mvdr_tracks_associate_dev(mca_hip_mvdr_ctx *ctx, int n_streams, const float *own_doa_dev, int n_cand, const float *cand_doa_dev,
                                      const float *cand_val_dev, void *stream);
int mca_hip_mvdr_tracks_fill_dev(mca_hip_mvdr_ctx *ctx, int n_streams, int n_frames, float *doa_rad_dev, void *stream);
int mca_hip_mvdr_tracks_fill_host(mca_hip_mvdr_ctx *ctx, int n_streams, int n_frames, float *doa_rad);   /* fill_dev through a staging buffer */
int mca_hip_mvdr_tracks_get(mca_hip_mvdr_ctx *ctx, int n_streams, float *theta, int *alive, int *miss, int *gen);
/* MAP MODE of the tracks: a second angle per slot, the candidates from the azimuth x elevation Capon map (mca_hip_mvdr_map_*) in the
 * place of the spectrum's peaks.  Opt-in, XYZ geometry.  Every slot s < n_tracks then holds (theta, eps): theta on the circle as
 * above (mca_hip_mvdr_set_geometry: reduce, wrap), eps a float clamped to +-1.57079637f with fminf / fmaxf on entry and after every
 * step.  n_tracks, n_own, max_step_rad, min_sep_rad and hold stay those of mca_hip_mvdr_tracks_configure; the grid, band, weighting and
 * n_peaks are the map's, as they are at the time of each call.  Everything in float32 is one rounded operation per step or an explicit
 * fmaf, as above.
 *
 * OWN tracks (s < n_own, alive): the estimator runs as above on the held (Psi_s, cpsi_s, Phi, cphi) at g0 = the XYZ geometric vector
 * of (theta_s, eps_s) -- the steering table of the frames calls with the pair cos((double) eps_s), sin((double) eps_s) where it reads
 * the context's.  With used, u_k as above and d(theta_i, eps_j, k) the vectors of the map's phasor table:
 *     T_s[j][i]       = sum over the used bins k of |d(theta_i, eps_j, k)^H u_k|^2 / M
 *     (phi_az, phi_el) = the cell that maximises T_s among the cells with |wrap(theta_i - theta_s)| <= max_step_rad and
 *                        |eps_j - eps_s| <= max_step_el_rad (grid values as mca_hip_mvdr_map_get_grid reports them, comparisons in
 *                        float); the maximum must be > 0 and the lower flat index j n_az + i wins ties; NaN if there is no such cell
 * The association, per stream, is the one above with pairs:
 *   1. own slots: s < n_own, alive, (o_az, o_el) both finite: theta_s = wrap(theta_s + clamp(wrap(reduce(o_az) - theta_s), +-max_step_rad)),
 *      eps_s = clamp(eps_s + clamp(clamp(o_el, +-pi/2_f) - eps_s, +-max_step_el_rad), +-pi/2_f), miss = 0.  An alive own slot whose
 *      target has an angle that is not finite: miss += 1.
 *   2. candidates (psi, eta, val) in the order given -- the map's peaks in rank order (peak_az, peak_el, peak_val of mca_hip_mvdr_map_dev)
 *      in an update: one with !(val > 0) or with an angle that is not finite is skipped; psi = reduce(psi), eta = clamp(eta, +-pi/2_f);
 *      one inside the box |wrap(psi - theta_s)| <= min_sep_rad && |eta - eps_s| <= min_sep_el_rad of an alive own track is skipped.
 *      Otherwise, among the alive slots s >= n_own not yet matched in this call with |wrap(psi - theta_s)| <= max_step_rad &&
 *      |eta - eps_s| <= max_step_el_rad, the one with the least |wrap(psi - theta_s)| + |eta - eps_s| (one rounded addition), the lower
 *      slot winning ties, takes (theta, eps) = (psi, eta), miss = 0 and is matched.  If there is none the candidate waits as a birth.
 *   3., 4. as above; a slot born takes (psi, eta), and its Psi and cpsi are cleared.
 * With every elevation equal the distance is |d theta| + 0 and the result is the association on the circle, bit for bit.  The distance
 * is in grid angles, not along a great circle: an azimuth gate loses its meaning near eps = +-pi/2, where the map calls a row
 * degenerate (every azimuth of it is one direction); keep tracked talkers away from the poles of the grid.
 *
 * mca_hip_mvdr_tracks_set_map(enable = 1) needs XYZ geometry, tracks configured with enable = 1 and the map configured;
 * max_step_el_rad and min_sep_el_rad finite and in [0, pi]; anything else is MCA_HIP_ERR_INVALID_ARGUMENT and changes nothing.
 * Enabling zeroes theta, eps, alive, miss and gen (it synchronises the device); enable = 0 on a context in map mode zeroes them too
 * and resets the elevation of every look-direction slot to unset.  Everything that disables the tracks leaves map mode: a geometry
 * change, a caller's mca_hip_mvdr_set_elevations_*, disabling RTF, mca_hip_mvdr_set_max_sources below n_tracks; so does
 * mca_hip_mvdr_tracks_configure.  mca_hip_mvdr_reset and mca_hip_mvdr_state_load zero eps with the rest; state blobs do not carry
 * the tracks and keep their versions.  In map mode the calls on one angle -- mca_hip_mvdr_tracks_seed_*, _update_*, _associate_dev --
 * are refused, for they would leave eps undefined; outside it the _map calls are refused.  mca_hip_mvdr_tracks_get works in both.
 *   seed_map: az, el [streams][n_tracks]; a slot whose az or el is not finite is left as it is; else theta = reduce(az),
 *     eps = clamp(el), alive = 1, miss = 0, gen += 1.
 *   update_map: own_map_dev [streams][n_own][n_el][n_az] float: T_s, or NULL; own_used_dev [streams][n_own][N/2+1] bytes, or NULL (both
 *     all zero for a dead slot); neither is touched when n_own == 0.  Without own_map_dev only the cells of the search windows are
 *     evaluated; the tracks are the same bytes either way.
 *   associate_map: own_az_dev, own_el_dev [streams][n_own] (may be NULL when n_own == 0), n_cand 1 ... 8 candidates per stream.
 *   get_map: [streams][n_tracks] of each array that is not NULL (it synchronises the device).
 * mca_hip_mvdr_tracks_fill_dev / _host in map mode write doa_rad as above and, on the same stream, the (cos eps, sin eps) pairs of the
 * slots s < n_tracks of the streams < n_streams: an alive slot its own eps, a dead slot (theta, eps) of the lowest alive slot, a
 * stream without an alive slot 0 rad and unset (the context's pair).  The pairs are formed as mca_hip_mvdr_set_elevations_dev forms
 * them -- the clamp in double, then the device's double cos and sin -- so the fill leaves the bytes that call would leave for the same
 * angles; unlike that call it does not disable the tracks.  mca_hip_mvdr_get_elevations reports the filled angles.
 * update_map, fill and get_map change no byte of Phi, tr, Psi, cpsi, cphi or the tails, but Psi and cpsi of a slot at its birth; the
 * result is a pure function of state and configuration (no atomics), independent of the place in the batch, of n_streams and of the
 * workspace cap (mca_hip_mvdr_set_rtf_workspace: u and the partial sums are taken in passes of streams under it).  Timing: kernel_id
 * 9 = the kernels of this mode; the two map kernels of an update count under 8, and an update with n_own == n_tracks launches none. */
typedef struct {
    int struct_size;
    int enable;
    double max_step_el_rad;  /* [0, pi]: gate and search window in elevation */
    double min_sep_el_rad;   /* [0, pi]: with min_sep_rad, the box within which a map peak is an own talker */
} mca_hip_mvdr_tracks_map_config;
int mca_hip_mvdr_tracks_set_map(mca_hip_mvdr_ctx *ctx, const mca_hip_mvdr_tracks_map_config *cfg);
int mca_hip_mvdr_tracks_get_map_config(const mca_hip_mvdr_ctx *ctx, mca_hip_mvdr_tracks_map_config *cfg);
int mca_hip_mvdr_tracks_seed_map_dev(mca_hip_mvdr_ctx *ctx, int n_streams, const float *az_dev, const float *el_dev, void *stream);
int mca_hip_mvdr_tracks_seed_map_host(mca_hip_mvdr_ctx *ctx, int n_streams, const float *az, const float *el);
int mca_hip_mvdr_tracks_update_map_dev(mca_hip_mvdr_ctx *ctx, int n_streams, float *own_map_dev, unsigned char *own_used_dev, void *stream);
int mca_hip_mvdr_tracks_update_map_host(mca_hip_mvdr_ctx *ctx, int n_streams, float *own_map, unsigned char *own_used);
int mca_hip_mvdr_tracks_associate_map_dev(mca_hip_mvdr_ctx *ctx, int n_streams, const float *own_az_dev, const float *own_el_dev, int n_cand,
                                          const float *cand_az_dev, const float *cand_el_dev, const float *cand_val_dev, void *stream);
int mca_hip_mvdr_tracks_get_map(mca_hip_mvdr_ctx *ctx, int n_streams, float *theta, float *eps, int *alive, int *miss, int *gen);
/* The geometry of the steering vectors.  MCA_HIP_MVDR_GEOMETRY_LINEAR_X (the default, and the bytes of every release before this
 * setter): the steering of Beamformer.cpp:59 above, which reads the x coordinate of mic_xyz alone -- right for a line array on the x
 * axis, wrong without an error for any other.  MCA_HIP_MVDR_GEOMETRY_XYZ: all three coordinates of mic_xyz (the context keeps them
 * from create on) and look directions round the whole circle.  Every look direction of the module -- doa_rad of the frames calls, of
 * mca_hip_mvdr_get_steering, the spectrum's grid and peaks, theta of the tracks -- is then an azimuth theta, any finite float; the
 * elevation eps is one value per context.  The unit vector towards the source and the steering vector are
 *     e(theta, eps) = (sin theta cos eps, cos theta cos eps, sin eps)
 *     d_m           = exp(+j 2 pi k fs (r_m . e) / (N c)),   c = 346.1
 * theta = 0 is +y, the broadside of a line array on the x axis; theta = +pi/2 is +x.  The phase is formed in double, from
 *     cd = cos((double) theta + pi/2), cy = -cos((double) theta), u = fs / N / c,
 *     p_m = (u x_m) (cd cos eps)  [+ (u y_m) (cy cos eps) if y_m != 0]  [- (u z_m) sin eps if z_m != 0]
 *     table entry kk of microphone m: turns = kk p_m, reduced by its nearest integer, exp(-j 2 pi turns) in float
 * (kk = 32 i and i: the factored tables of the module).  A coordinate that is 0 adds no term, so an array on the x axis with eps = 0
 * gives the bytes of LINEAR_X in every call.  LINEAR_X ignores elevation_rad, which must still be finite and within +-pi/2, and
 * mca_hip_mvdr_get_geometry reports 0 for it.
 *
 * The Capon spectrum in XYZ mode has a periodic grid, theta_i = -pi + i 2 pi / D, i = 0 ... D-1 (in double, reported as float;
 * n_angles 3 ... 361), and the peak rule holds on the circle: i is a local maximum if P[i] > 0, P[i] > P[(i-1) mod D] and
 * P[i] >= P[(i+1) mod D].  Ranking, ties and empty slots are as above.  A line array cannot tell front from back: in XYZ mode it shows
 * every talker twice, at theta and at pi - theta, with equal values up to rounding -- ties go to the lower index.
 *
 * The tracks in XYZ mode live on the circle, in float32, with pi_f = 3.14159274f, two_pi_f = 6.28318548f, inv_f = 0.159154937f:
 *     reduce(v) = clamp(wrap(fmaf(-two_pi_f, rintf(v * inv_f), v)), -pi_f, pi_f)         for a finite v; a NaN or an infinity stays
 *     wrap(d)   = d - two_pi_f if d > pi_f;  d + two_pi_f if d < -pi_f;  d otherwise      one rounded addition
 * Seeds, candidates and own_doa are reduced on entry, so a stored theta is always in [-pi_f, pi_f].  Every difference of the
 * association above is wrap(x - y): own_doa[s] - theta_s in step 1, |psi - theta_s| in the min_sep test and in the gate of step 2,
 * and |theta_i - theta_s| of the own track's search window.  Step 1 stores wrap(theta_s + clamp(...)).  LINEAR_X arithmetic is
 * as it was.
 *
 * Accepted: struct_size as compiled, mode 0 or 1, elevation_rad finite with |elevation_rad| <= pi/2; anything else is
 * MCA_HIP_ERR_INVALID_ARGUMENT and leaves everything as it was.  Geometry is a processing parameter like the null gain: state blobs
 * neither carry nor check it, and Phi, tr, Psi, cpsi, cphi, the post-filter state and the tails do not depend on it and are kept.  A
 * call that changes mode or elevation synchronises the device, un-configures the spectrum (its phasor table and grid are stale) and
 * disables the tracks (their angles change meaning); both are configured anew.  A call that changes nothing is a no-op. */
#define MCA_HIP_MVDR_GEOMETRY_LINEAR_X 0
#define MCA_HIP_MVDR_GEOMETRY_XYZ 1
typedef struct {
    int struct_size;
    int mode;                /* MCA_HIP_MVDR_GEOMETRY_LINEAR_X / _XYZ */
    double elevation_rad;    /* eps, [-pi/2, pi/2] */
} mca_hip_mvdr_geometry_config;
int mca_hip_mvdr_set_geometry(mca_hip_mvdr_ctx *ctx, const mca_hip_mvdr_geometry_config *cfg);
int mca_hip_mvdr_get_geometry(const mca_hip_mvdr_ctx *ctx, mca_hip_mvdr_geometry_config *cfg);
/* An elevation per look-direction slot (XYZ geometry).  The context holds, per stream and slot s < MCA_MAX_SOURCES, a pair
 * (cos eps, sin eps) in double on the device.  In XYZ mode the steering tables of every mca_hip_mvdr_*frames* call -- plain, sources,
 * weighted, masked, RTF and auto -- form the look direction s of a frame of stream a with the pair of (a, s) where set_geometry above
 * writes cos eps and sin eps, and mca_hip_mvdr_get_steering does so for its (stream_index, source).  LINEAR_X never reads the pairs.
 *   elev_rad [streams][max_sources] float: a NaN entry means "the context's elevation" and stores the context's own pair, bit for bit
 *   -- the state of every slot after create.  Any other entry must be within +-pi/2, compared as float (the float nearest to pi/2,
 *   1.57079637f, is accepted), and is clamped to [-pi/2, pi/2] in double before its cosine and sine are taken.
 * mca_hip_mvdr_set_elevations_host refuses the whole array if one entry is outside (an infinity is), and changes nothing; it forms the
 * pairs with the host's cos and sin, as set_geometry does, so that a context at elevation 0 with eps in every slot computes the bytes
 * of a context created at eps; it synchronises the device.  mca_hip_mvdr_set_elevations_dev reads the array on `stream` and cannot
 * refuse a value: it CLAMPS (an infinity goes to the end of the range; NaN still means unset) and forms the pairs with the device's
 * double cos and sin, which may differ from the host's in the last place.  The slots max_sources ... and the streams n_streams ... keep
 * what they hold.  mca_hip_mvdr_get_elevations reports [streams][max_sources] float: NaN for an unset slot, else the angle as given
 * (host call) or as clamped (device call); it synchronises.
 * The elevations are a processing parameter like the null gain: state blobs neither carry nor check them, and mca_hip_mvdr_reset keeps
 * them.  A geometry change that changes mode or elevation resets every slot to unset.  The tracks, the Capon spectrum and its peaks
 * keep the context's one elevation: a set_elevations call -- either one, whatever it carries -- disables the tracks, as a geometry
 * change does, and mca_hip_mvdr_tracks_configure with enable = 1 resets every slot to unset.  The loop with a second angle is
 * mca_hip_mvdr_map_dev -> peak_az_dev as doa_rad, peak_el_dev to mca_hip_mvdr_set_elevations_dev -> the next chunk, with no host step;
 * with identity per slot it is the tracks' map mode (mca_hip_mvdr_tracks_set_map), whose fill writes the pairs itself.
 * n_streams outside 1 ... max_streams or a NULL array is MCA_HIP_ERR_INVALID_ARGUMENT. */
int mca_hip_mvdr_set_elevations_host(mca_hip_mvdr_ctx *ctx, int n_streams, const float *elev_rad);
int mca_hip_mvdr_set_elevations_dev(mca_hip_mvdr_ctx *ctx, int n_streams, const float *elev_rad_dev, void *stream);
int mca_hip_mvdr_get_elevations(mca_hip_mvdr_ctx *ctx, int n_streams, float *elev_rad);
/* copy of the covariance of one stream: out[N/2+1][M][M] interleaved re,im double (full Hermitian matrices) */
int mca_hip_mvdr_get_covariance(mca_hip_mvdr_ctx *ctx, int stream_index, double *out);
/* checkpoint / resume as mca_hip_state_*: the covariances, their traces and the overlap-add tails of every stream (and the
 * post-filter's A of a context that has it enabled: version 3, above; Psi, cpsi and cphi of one with RTF enabled: version 4, above) */
long long mca_hip_mvdr_state_size(const mca_hip_mvdr_ctx *ctx);
int mca_hip_mvdr_state_save(mca_hip_mvdr_ctx *ctx, void *blob, long long blob_bytes);
int mca_hip_mvdr_state_load(mca_hip_mvdr_ctx *ctx, const void *blob, long long blob_bytes);
/* per-kernel timing as mca_hip_set_timing / mca_hip_get_timing: kernel_id 0 = analysis, 1 = solve, 2 = synthesis,
 * 3 = spectrum (both kernels of a mca_hip_mvdr_spectrum_* call), 4 = post-filter.  kernel_id 4 exists on a context that has had the
 * post-filter enabled at some time (it stays readable after disabling); a context that never enabled it refuses 4 like every
 * other id outside 0 ... 3, as it always did (MCA_HIP_ERR_INVALID_ARGUMENT).  5 = k_mvdr_rtf, by the same rule: it exists on a
 * context that has had RTF enabled at some time.  6 = k_mvdr_estmask, by the same rule (the mask estimator).  7 = the track
 * kernels (mca_hip_mvdr_tracks_*), by the same rule: it exists once tracks have been configured.  8 = both kernels of a
 * mca_hip_mvdr_map_* call, by the same rule: it exists once the map has been configured.  9 = the kernels of the tracks' map mode
 * (mca_hip_mvdr_tracks_*_map and the fill in that mode), by the same rule: it exists once map mode has been enabled */
int mca_hip_mvdr_set_timing(mca_hip_mvdr_ctx *ctx, int enable);
int mca_hip_mvdr_get_timing(mca_hip_mvdr_ctx *ctx, int kernel_id, int *launches, double *total_ms);

/* ---- measurement ------------------------------------------------------------ */
typedef enum {
    MCA_HIP_K_STFT_PHAT = 0,   /* STFT + PHAT whitening + pair-group sums */
    MCA_HIP_K_SRP_GEMM = 1,    /* steering contraction (MFMA) */
    MCA_HIP_K_SCAN_PICK = 2,   /* IIR over frames + selectDOA */
    MCA_HIP_K_BEAMFORM = 3,    /* STFT + delay-and-sum + inverse FFT + overlap-add */
    MCA_HIP_K_GCC2_SCAN = 4,   /* 2-mic correlation smoothing + argmax + probability */
    MCA_HIP_K_MASK = 5,        /* binaural masking */
    MCA_HIP_K_FOLD = 6,        /* sum of the partial maps of a deep split-K contraction (small batches only) */
    MCA_HIP_K_REPAIR = 7,      /* MCA_HIP_SRP_ADAPTIVE: plan + exact recomputation of the sensitive rows + second pick */
    MCA_HIP_K_COUNT = 8
} mca_hip_kernel_id;
/* enable = 1: bracket every launch of the stream API with hipEvents on its stream */
int mca_hip_set_timing(mca_hip_ctx *ctx, int enable);
/* as mca_hip_set_timing for the kernel ids whose bit (1u << id) is set only: every event pair costs the stream ~1.5 us, a
 * throughput measurement brackets the one kernel it reports on */
int mca_hip_set_timing_mask(mca_hip_ctx *ctx, unsigned kernel_mask);
/* synchronises the recorded events; *launches and *total_ms accumulate since the last reset */
int mca_hip_get_timing(mca_hip_ctx *ctx, int kernel_id, int *launches, double *total_ms);
int mca_hip_reset_timing(mca_hip_ctx *ctx);
/* MCA_HIP_SRP_ADAPTIVE: totals since the last mca_hip_reset_timing (synchronises the device): frames that went through the
 * adaptive path, frames whose pick was flagged as sensitive to the fp16 error (in the eager form this includes the last frame of
 * every array and call, which is repeated so that the carried state is exact; lazy calls flag no frame for that), and frames
 * whose rows went through the exact analysis.  The
 * reference has no counterpart (it computes every pair and delay in double, SteeringBeamforming.cpp:104-130). */
int mca_hip_get_repair_stats(mca_hip_ctx *ctx, unsigned long long *frames, unsigned long long *flagged_frames,
                             unsigned long long *recomputed_frames);
/* ... and how much of those rows was recomputed (round 5, candidate columns): the exact contraction runs at the delays a flagged
 * frame's picks can be among -- the positions whose coarse energy reaches the lowest value the exact picks can have, plus the two
 * delays either side that feed the sign / median chain of SteeringBeamforming.cpp:159-173 -- instead of at all D of them.
 * candidate_columns: their number summed over the flagged frames; whole_row_frames: the flagged frames that took every delay
 * (no lower bound from the coarse row, a frame repeated for the carried state's sake, a row the coarse analysis could not vouch for). */
int mca_hip_get_repair_columns(mca_hip_ctx *ctx, unsigned long long *candidate_columns, unsigned long long *whole_row_frames);
/* Delay-and-sum on the half spectrum (mca_hip_process_frames_dev of a one-source, ungated 8-microphone ULA at 1024-sample frames, ADAPTIVE or
 * FP16): the analysis steers every frame at the array's PREDICTED bin -- its last pick of the previous call -- and a patch pass redoes the
 * frames whose pick came out different.  frames: frames such calls have processed since creation; missed_frames: those whose pick was not
 * the predicted bin; fused_calls: calls whose analysis steered ahead (the others steered every frame after the picks).  The audio does not
 * depend on any of this: both passes run one routine. */
int mca_hip_get_steer_stats(mca_hip_ctx *ctx, unsigned long long *frames, unsigned long long *missed_frames, unsigned long long *fused_calls);

/* library version string */
const char *mca_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MCARRAY_HIP_H */
