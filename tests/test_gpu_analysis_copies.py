"""The separation block of the fused, merged analysis kernel (k_stft_phat_wave<8, ULA, fp16, MERGE, FUSE>; csrc/kernels_wave.hip) forms
2 X_a and 2 X_b of a bin in one packed instruction each (mirror_split, csrc/steer.h) and whitens the two channels with both scales in one
register pair (whiten4_pair): signs, crossed halves and the broadcast of a scale ride on op_sel / neg_hi instead of register copies.
The arithmetic is the parent's, bit for bit; these cases aim at what an operand select can get wrong and broadband noise would hide:

  balanced content in a full run of 16 frames plus a ragged one, and across two calls;
  the scaled path of the pair balance (pair_balance.h), every pair in turn with a channel 60 / 80 / 100 dB below its partner -- and the
  same input through a context that steers every frame in k_steer_patch (steer_patch_frame keeps the scalar form of the separation):
  the same audio bits, whichever routine produced the hop;
  a channel of exact zeros and a whole frame of exact zeros (the scale is zeroed by the select in front of the packed multiply);
  tones in the bins that lanes 0 and 32 hold (k = 0, 64 s, 32 + 64 s, 512), the lanes that are their own mirror partners.

FP16 context, 8-microphone ULA, 1024-sample frames, 361 angles, device-pointer calls (the fused kernel runs at any batch size there).
A context's first call predicts no bin, so k_steer_patch redoes all its hops; the hops of a second call come from the analysis kernel
itself wherever the pick stayed -- every case but the single-call one therefore makes two calls.
Every case: DOA bins equal to the fp64 oracle's (oracle.pyoracle.ssl_stream), audio on every hop against the oracle's delay-and-sum
stream at the GPU's own picks (das_stream).  Tolerances: tests/test_gpu_steer.py's audio bar, quoted in _check."""
import numpy as np
import pytest

from mcarray_amd import api, synth
from oracle import pyoracle as po
from test_gpu_steer import FS, HOP, N, XS, _calls, _ctx

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F1 = 17                                                        # a run of 16 frames and a ragged one
SPECIAL_BINS = [0] + [64 * s for s in range(1, 8)] + [32 + 64 * s for s in range(8)] + [512]     # lane 0: 0, 64 s, 512; lane 32: 32 + 64 s


def _source(F, A, seed, base=23.0, snr_db=20.0):
    return np.stack([synth.noise_source_stream(XS, np.deg2rad(base - 41 * a), FS, (F + 1) * HOP, seed + a, snr_db=snr_db) for a in range(A)]).astype(np.float32)


def tone_stream(F, theta_deg, amplitude, seed, noise_db=None):
    """a source at theta made of tones at SPECIAL_BINS of the 1024-sample frame (random phases, amplitudes within 2 dB of each other so
    that no two map values coincide); noise_db: a broadband source at the SAME angle that many dB below the tones' sum; [1][8][(F + 1) hop]"""
    rng = np.random.default_rng(seed)
    n = (F + 1) * HOP
    t = np.arange(n)
    s = np.zeros(n)
    for k in SPECIAL_BINS:
        s += 10.0 ** (rng.uniform(-1.0, 1.0) / 10.0) * np.cos(2 * np.pi * k * t / N + rng.uniform(0, 2 * np.pi))
    s *= amplitude / np.abs(s).max()
    if noise_db is not None:
        s += rng.standard_normal(n) * (np.sqrt(np.mean(s ** 2)) * 10.0 ** (-noise_db / 20.0))
    return synth.delay_channels(s, XS, np.deg2rad(theta_deg), FS)[None].astype(np.float32)


def oracle_picks(pcm_a):
    return po.ssl_stream(FS, N, XS, pcm_a.astype(np.float64), 1, 0.5, want_map=True, want_audio=False)


def pick_margins(o):
    """per frame: the oracle's largest map value minus its largest value at any OTHER bin (0: an exact tie), over the map's largest magnitude"""
    e = o["energy"]
    top = e.max(axis=1)
    rest = np.where(np.arange(e.shape[1])[None, :] == o["bin"][:, :1], -np.inf, e).max(axis=1)
    return (top - rest) / np.abs(e).max()


def _check(bins, rad, audio, pcm, zero_frames=()):
    """bins: equal to the oracle's on every frame (zero_frames: frames without a non-zero sample -- a flat map, no pick to compare);
    audio: tests/test_gpu_steer.py's bar, 2e-5 of the oracle stream's peak + 1e-7 on every hop, steered at the GPU's own picks"""
    for a in range(pcm.shape[0]):
        o = oracle_picks(pcm[a])
        keep = np.ones(bins.shape[1], dtype=bool)
        keep[list(zero_frames)] = False
        diff = np.flatnonzero((bins[a] != o["bin"][:, 0]) & keep)
        print("array %d: %d of %d frames compared, %d differ; smallest oracle margin %.3e of the map's peak"
              % (a, int(keep.sum()), keep.size, diff.size, float(pick_margins(o)[keep].min())))
        assert diff.size == 0, (a, diff.tolist(), bins[a][diff].tolist(), o["bin"][diff, 0].tolist(), pick_margins(o)[diff].tolist())
        assert np.isfinite(audio[a]).all()
        ref = po.das_stream(FS, N, XS, pcm[a].astype(np.float64), rad[a].astype(np.float64))
        err = float(np.abs(audio[a] - ref).max())
        print("array %d: audio error %.3e of the peak (%.3e)" % (a, err / max(np.abs(ref).max(), 1e-300), np.abs(ref).max()))
        assert err <= 2e-5 * np.abs(ref).max() + 1e-7, (a, err, np.abs(ref).max())


def _run(pcm, sizes):
    ctx = _ctx(pcm.shape[0])
    res = _calls(ctx, pcm, sizes)
    st = ctx.steer_stats()
    ctx.close()
    assert st["fused_calls"] == len(sizes), st                 # every call's analysis was the fused kernel
    return res


@pytest.mark.parametrize("A,sizes", [(1, [F1]), (2, [F1, 16])])
def test_balanced_content_in_a_full_and_a_ragged_run_and_across_two_calls(A, sizes):
    pcm = _source(sum(sizes), A, 2600)
    _check(*_run(pcm, sizes), pcm)


@pytest.mark.parametrize("db", [60, 80, 100])
def test_each_pair_in_turn_with_a_quiet_channel_and_the_patch_kernel_gives_the_same_bits(db, monkeypatch):
    """array p: a channel of pair p (its first or its second, alternating) db below the rest -- the pair's transform scales it up by a
    power of two.  Then the same calls under a workspace budget too small to steer ahead: k_steer_patch takes every frame."""
    sizes = [65, 65]                                           # four runs of 16 and a ragged one; 4 x 65 rows of Y: more than 1 MB holds (252)
    pcm = _source(sum(sizes), 4, 2610 + db, base=50.0)
    for p in range(4):
        pcm[p, 2 * p + (p & 1)] *= np.float32(10.0 ** (-db / 20.0))
    b0, r0, o0 = _run(pcm, sizes)
    _check(b0, r0, o0, pcm)
    monkeypatch.setenv("MCA_HIP_WS_MAX_MB", "1")
    ctx = _ctx(4)
    b1, r1, o1 = _calls(ctx, pcm, sizes)
    st = ctx.steer_stats()
    ctx.close()
    assert st["fused_calls"] == 0 and st["frames"] == 4 * sum(sizes), st
    assert np.array_equal(b0, b1)
    assert np.array_equal(o0, o1)


def test_a_channel_of_exact_zeros_and_a_whole_frame_of_exact_zeros():
    pcm = _source(2 * F1, 2, 2620)
    pcm[0, 5] = 0.0
    for f in (6, F1 + 6):                                      # frame f = samples [f hop, (f + 2) hop): every channel zero; frames f - 1 and f + 1 half
        pcm[1, :, f * HOP:(f + 2) * HOP] = 0.0
    res = _run(pcm, [F1, F1])
    _check(res[0][:1], res[1][:1], res[2][:1], pcm[:1])
    _check(res[0][1:], res[1][1:], res[2][1:], pcm[1:], zero_frames=(6, F1 + 6))


# amplitude 1e-11: the tones' bins hold |2 X|^2 ~ 1e-17, far above the whitening threshold 4e-30, while the rounding noise of the fp32
# transform in all other bins (~1e-6 of a tone bin in amplitude) stays far below it -- the map is the special lanes' bins (and the
# window's two neighbours of each) alone, on the GPU as in the oracle: that case is about the PICK (its audio, 1e-11, sits under the
# bar's absolute term).  amplitude 0.5 with the same source's noise 40 dB down: every bin
# has a phase, and the audio is the tones'.
TONE_CASES = {"tones alone": dict(amplitude=1e-11, noise_db=None), "tones over a floor": dict(amplitude=0.5, noise_db=40.0)}


def _tone_input(case):
    return tone_stream(2 * F1, -33.0, seed=2630, **TONE_CASES[case])


@pytest.mark.parametrize("case", list(TONE_CASES))
def test_tones_in_the_bins_of_lanes_0_and_32(case):
    pcm = _tone_input(case)
    _check(*_run(pcm, [F1, F1]), pcm)
