"""CPU: the numpy twin of BinauralMaskingImpl (tests/bmask_twin.py) has the reference's executed properties
(testTemporalMasking / testSpatialMasking, test/test_mcarray.cpp:892-1065), its time-domain means equal the half-spectrum
sums the kernels take, the parity inputs of the GPU tests stay clear of ties, and the C ABI declares and binds the module."""
import os
import re

import numpy as np
import pytest

import bmask_twin as bt
from mcarray_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, D, LO, HI = 16000, 0.086, 500, 5000


@pytest.fixture(scope="module")
def temporal():
    pcm, start, step = bt.temporal_signal(FS)
    return bt.whole_frames(pcm, bt.frame_size(FS)), start, step


@pytest.mark.parametrize("method", [bt.FULL, bt.RELATIVE])
def test_temporal_masking_power_windows(temporal, method):
    pcm, start, step = temporal
    res = bt.Twin(FS, D, LO, HI, method).stream(pcm)
    n = res["out"].shape[1]
    before = bt.temporal_difference(pcm[0], start, step, n)
    print("temporal, method %d: before %.3f dB" % (method, before))
    assert abs(before - 2) < 0.5, before
    for c in range(2):
        after = bt.temporal_difference(res["out"][c], start, step, n)
        print("temporal, method %d, channel %d: after %.3f dB" % (method, c, after))
        assert abs(after - 5) < 1.0, after


def test_temporal_masking_factor_is_the_identity(temporal):
    pcm, start, step = temporal
    res = bt.Twin(FS, D, LO, HI, bt.FACTOR).stream(pcm)
    n = res["out"].shape[1]
    before = bt.temporal_difference(pcm[0], start, step, n)
    after = bt.temporal_difference(res["out"][0], start, step, n)
    print("temporal, FACTOR: before %.3f after %.3f" % (before, after))
    assert (res["dec"] == 1).any()
    # both factors are 1: the band-power difference stays inside the "before" window (the filter bank removes what lies out of band)
    assert abs(after - 2) < 0.5, after
    assert abs(after - before) < 0.05, (before, after)


def test_spatial_masking_power_windows_and_the_44_band_reading():
    pcm = bt.whole_frames(bt.spatial_signal(), bt.frame_size(FS))
    res = bt.Twin(FS, D, LO, HI, bt.FULL).stream(pcm)
    p_sig, p_int = bt.spatial_powers(res["out"][0])
    print("spatial, 45 bands: signal %.2f dB, interferer %.2f dB" % (p_sig, p_int))
    assert abs(70 - p_sig) <= 10
    assert abs(70 - p_int) <= 10
    # analysisLength = 45 W read literally drops band 44 (centre 4810 Hz): the 4800 Hz interferer band falls out of the window
    lit = bt.Twin(FS, D, LO, HI, bt.FULL, n_sum=44).stream(pcm)
    _, p_int44 = bt.spatial_powers(lit["out"][0])
    print("spatial, 44 bands: interferer %.2f dB" % p_int44)
    assert abs(p_int44 - 45.7) < 1.0
    assert abs(70 - p_int44) > 10


@pytest.mark.parametrize("fs, lo, hi", [(16000, 500, 5000), (16000, 300, 8000), (48000, 500, 5000)])
def test_parseval_identity(fs, lo, hi):
    """mean over W samples of band products == (1 / W^2) sum_k c_k (.) H_b[k]^2, c = 1 at DC and Nyquist, else 2"""
    tw = bt.Twin(fs, D, lo, hi)
    W = tw.W
    rng = np.random.default_rng(7)
    l, r = rng.standard_normal(W) * tw.win, (rng.standard_normal(W) * 0.7) * tw.win
    bl, br = tw.bands(l), tw.bands(r)
    L, R = np.fft.rfft(l), np.fft.rfft(r)
    ck = np.full(W // 2 + 1, 2.0)
    ck[0] = ck[-1] = 1.0
    w = ck[None, :] * tw.H ** 2 / W ** 2
    pairs = [(np.mean(bl * bl, axis=1), (w * np.abs(L) ** 2).sum(axis=1)),
             (np.mean(br * br, axis=1), (w * np.abs(R) ** 2).sum(axis=1)),
             (np.mean(bl * br, axis=1), (w * (L * np.conj(R)).real).sum(axis=1)),
             (np.mean(((bl + br) / 2) ** 2, axis=1), (w * np.abs(L + R) ** 2 / 4).sum(axis=1))]
    scale = pairs[0][0].max()
    for time_mean, spec_sum in pairs:
        assert np.abs(time_mean - spec_sum).max() <= 1e-12 * scale
    assert (tw.H > 0).sum(axis=0).max() <= 2          # every bin lies in at most two triangles


@pytest.mark.parametrize("seed", sorted(bt.PARITY))
def test_parity_inputs_stay_clear_of_ties(seed):
    res = bt.Twin(FS, D, LO, HI, bt.RELATIVE).stream(bt.parity_input(seed))
    ties = bt.near_tie(res)
    share = [float((res["dec"] == k).mean()) for k in range(3)]
    print("seed %d: enhance/temporal/spatial %.3f/%.3f/%.3f, near ties %d of %d" % (seed, *share, ties.sum(), ties.size))
    assert ties.mean() <= 0.005
    assert (res["dec"] == 0).any() and (res["dec"] == 1).any() and (res["dec"] == 2).any()


def test_rising_tones_never_fire_the_temporal_rule():
    x = bt.rising_tones(FS, D, LO, HI, 40)
    x[1] = 0
    res = bt.Twin(FS, D, LO, HI, bt.RELATIVE).stream(x)
    assert (res["dec"] == 0).all()
    assert res["mt"].min() > 1e-3 and res["ms"].min() > 0.01      # far from both thresholds: an fp32 path decides the same


def test_hooks_compose_to_the_stream_path():
    tw = bt.Twin(FS, D, LO, HI, bt.FULL)
    W = tw.W
    rng = np.random.default_rng(3)
    x = rng.standard_normal(W)
    ana = tw.frame_analysis(x)
    assert np.abs(ana.reshape(46, W).sum(axis=0) - x).max() <= 1e-12          # bands + residual = the frame
    assert np.array_equal(tw.frame_synthesis(ana, 46 * W), ana[:45 * W].reshape(45, W).sum(axis=0))
    assert np.array_equal(tw.frame_synthesis(ana, 45 * W), ana[:44 * W].reshape(44, W).sum(axis=0))
    short = tw.frame_analysis(x, 45 * W)
    assert np.array_equal(short, ana[:45 * W])


def test_abi_declares_and_binds_the_module():
    text = open(os.path.join(ROOT, "include", "mcarray_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mca_hip_bmask_[a-z0-9_]+)\s*\(", text))
    want = {"mca_hip_bmask_" + n for n in ("create", "destroy", "last_error", "reset", "get_thresholds", "frames_dev", "frames_host",
                                           "process_frame", "frame_analysis", "frame_synthesis", "state_size", "state_save", "state_load")}
    assert declared == want
    assert want <= {name for name, _, _ in _lib.SYMBOLS}
    from mcarray_amd import api
    assert (api.BinauralMaskingImpl.N_BANDS, api.FACTOR, api.RELATIVE, api.FULL) == (45, 0, 1, 3)
