"""GPU: BinauralMaskingImpl (mca_hip_bmask_*) against the float64 numpy twin tests/bmask_twin.py: thresholds, decisions on
every cell that is not near a tie, audio on the hops whose frames agree, the reference's band-power windows on the long
signals, bit-identical results across call splits / batch positions / state blobs, the three hooks in double, 48 kHz, a
muted channel, the Q guard, a band that falls silent, and the C++ class."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import bmask_twin as bt
from mcarray_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, D, LO, HI = 16000, 0.086, 500, 5000


@functools.lru_cache(maxsize=None)
def _twin_stream(seed, method, fs=FS):
    return bt.Twin(fs, D, LO, HI, method).stream(bt.parity_input(seed, fs))


def _check_stream(label, out, dec, tw):
    """decisions: equal off the near-tie cells, differences no more than those cells; audio on the hops whose frames agree"""
    ties = bt.near_tie(tw)
    diff = dec != tw["dec"]
    F, hop = dec.shape[0], out.shape[1] // dec.shape[0]
    agree = ~diff.any(axis=1)
    ok = agree.copy()
    ok[1:] &= agree[:-1]                    # output hop t = frame t - 1's second half + frame t's first half
    err = np.abs(out.astype(np.float64) - tw["out"]).reshape(2, F, hop).max(axis=(0, 2))
    bound = 2e-5 * np.abs(tw["out"]).max() + 1e-7
    print("%s: %d cells, %d near ties, %d differ; audio on %d of %d hops: worst %.3g (bound %.3g)"
          % (label, diff.size, ties.sum(), diff.sum(), ok.sum(), F, err[ok].max(), bound))
    assert not (diff & ~ties).any(), label
    assert diff.sum() <= ties.sum(), label
    assert ok.sum() > F // 2, label
    assert err[ok].max() <= bound, label


def test_thresholds_and_centres():
    for fs in (16000, 48000):
        m = api.BinauralMaskingImpl(fs, D, LO, HI)
        tw = bt.Twin(fs, D, LO, HI)
        assert m.W == tw.W
        thr, cen = m.thresholds()
        np.testing.assert_allclose(thr, tw.thr, rtol=0, atol=1e-14)
        np.testing.assert_allclose(cen, tw.center, rtol=0, atol=1e-15)
        m.close()


@pytest.mark.parametrize("method", bt.METHODS)
@pytest.mark.parametrize("seed", sorted(bt.PARITY))
def test_stream_parity(seed, method):
    m = api.BinauralMaskingImpl(FS, D, LO, HI, method)
    out, dec = m.process(bt.parity_input(seed))
    _check_stream("seed %d method %d" % (seed, method), out[0], dec[0], _twin_stream(seed, method))
    m.close()


@pytest.mark.parametrize("method", bt.METHODS)
def test_stream_parity_48k(method):
    fs = 48000
    m = api.BinauralMaskingImpl(fs, D, LO, HI, method)
    assert m.W == 2048
    out, dec = m.process(bt.parity_input(42, fs))
    _check_stream("48 kHz seed 42 method %d" % method, out[0], dec[0], _twin_stream(42, method, fs))
    m.close()


def test_any_length_path_parity():
    """8 kHz: W = 512 runs on the any-length transform"""
    fs = 8000
    m = api.BinauralMaskingImpl(fs, D, 300, 3400, bt.RELATIVE)
    assert m.W == 512
    pcm = bt.parity_input(42, fs)
    out, dec = m.process(pcm)
    _check_stream("8 kHz seed 42", out[0], dec[0], bt.Twin(fs, D, 300, 3400, bt.RELATIVE).stream(pcm))
    m.close()


def test_reference_windows_on_the_long_signals():
    """testTemporalMaskingCore (100 frames, crossing the passes and runs of the kernels) and testSpatialMaskingCore on the GPU"""
    pcm, start, step = bt.temporal_signal(FS)
    pcm = bt.whole_frames(pcm, 1024)
    n = pcm.shape[1] - 512
    before = bt.temporal_difference(pcm[0], start, step, n)
    print("temporal before %.3f dB" % before)
    assert abs(before - 2) < 0.5
    for method in (bt.FULL, bt.RELATIVE):
        m = api.BinauralMaskingImpl(FS, D, LO, HI, method)
        out, _ = m.process(pcm.astype(np.float32))
        for c in range(2):
            after = bt.temporal_difference(out[0, c].astype(np.float64), start, step, n)
            print("temporal after, method %d channel %d: %.3f dB" % (method, c, after))
            assert abs(after - 5) < 1.0
        m.close()
    m = api.BinauralMaskingImpl(FS, D, LO, HI, bt.FULL)
    out, _ = m.process(bt.whole_frames(bt.spatial_signal(), 1024).astype(np.float32))
    p_sig, p_int = bt.spatial_powers(out[0, 0].astype(np.float64))
    print("spatial: signal %.2f dB, interferer %.2f dB" % (p_sig, p_int))
    assert abs(70 - p_sig) <= 10
    assert abs(70 - p_int) <= 10
    m.close()


def _run_cuts(m, pcm, cuts):
    """frames [0, sum(cuts)) of pcm [S][2][n] in calls of the given numbers of frames"""
    outs, decs, f0 = [], [], 0
    for n in cuts:
        o, d = m.process(pcm[:, :, f0 * m.hop:(f0 + n + 1) * m.hop])
        outs.append(o)
        decs.append(d)
        f0 += n
    return np.concatenate(outs, axis=2), np.concatenate(decs, axis=1)


def _same_bits(a, b):
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape
    assert a[0].tobytes() == b[0].tobytes(), "audio bits differ"
    assert a[1].tobytes() == b[1].tobytes(), "decisions differ"


@pytest.mark.parametrize("fs", [16000, 48000])
def test_bits_across_call_splits_batches_and_state_blobs(fs):
    x = bt.parity_input(42, fs)[None]
    F = bt.PARITY_FRAMES
    whole = _run_cuts(api.BinauralMaskingImpl(fs, D, LO, HI), x, [F])
    _same_bits(whole, _run_cuts(api.BinauralMaskingImpl(fs, D, LO, HI), x, [1, 7, F - 8]))

    batch = np.stack([bt.parity_input(41 + (i % 3), fs) * np.float32(1 + 0.1 * i) for i in range(8)])
    for pos in (0, 5):
        b = batch.copy()
        b[pos] = x[0]
        o, d = _run_cuts(api.BinauralMaskingImpl(fs, D, LO, HI, max_streams=8), b, [F])
        _same_bits(whole, (o[pos:pos + 1], d[pos:pos + 1]))

    m1 = api.BinauralMaskingImpl(fs, D, LO, HI)
    first = _run_cuts(m1, x, [60])
    blob = m1.state()
    m2 = api.BinauralMaskingImpl(fs, D, LO, HI)
    m2.load_state(blob)
    second = _run_cuts(m2, x[:, :, 60 * m2.hop:], [F - 60])
    _same_bits(whole, (np.concatenate([first[0], second[0]], axis=2), np.concatenate([first[1], second[1]], axis=1)))


@pytest.mark.parametrize("method", bt.METHODS)
def test_hooks_in_double_match_the_twin(method):
    m = api.BinauralMaskingImpl(FS, D, LO, HI, method)
    tw = bt.Twin(FS, D, LO, HI, method)
    W, hop = tw.W, tw.hop
    pcm = bt.parity_input(42).astype(np.float64)
    worst = 0.0
    seen = set()
    for t in range(20):
        fr = [pcm[c, t * hop:t * hop + W] * tw.win for c in range(2)]
        ana = [m.frame_analysis(fr[c], channel=c) for c in range(2)]
        ref = [tw.frame_analysis(fr[c]) for c in range(2)]
        for c in range(2):
            e = np.abs(ana[c] - ref[c]).max() / np.abs(ref[c]).max()
            worst = max(worst, e)
            assert e <= 1e-10, (t, c, e)
        # the decision stage is compared on the same input: the twin's analysis buffers
        l, r, dec = m.process_parametrisation(ref[0], ref[1])
        tl, tr, tdec, (mt, ms) = tw.process_parametrisation(ref[0], ref[1])
        clear = (mt >= 1e-9) & (ms >= 1e-9)
        assert np.array_equal(dec[clear], tdec[clear]), t
        seen |= set(dec.tolist())
        same = np.repeat(dec == tdec, W)                # a band decided otherwise (closer than 1e-9 to a tie) is scaled otherwise
        assert same.sum() >= 44 * W
        for g, w in ((l, tl), (r, tr)):
            assert g.shape == w.shape
            e = np.abs(g[:45 * W] - w[:45 * W])[same].max() / np.abs(w).max()
            worst = max(worst, e)
            assert e <= 1e-10, (t, e)
            assert np.array_equal(g[45 * W:], w[45 * W:])      # the residual slot is not touched
        for n in (46 * W, 45 * W):
            for w in (tl, tr):
                y, ty = m.frame_synthesis(w, n), tw.frame_synthesis(w, n)
                e = np.abs(y - ty).max() / np.abs(ty).max()
                worst = max(worst, e)
                assert e <= 1e-10, (t, n, e)
    print("hooks, method %d: worst relative error %.3g, decisions seen %s" % (method, worst, sorted(seen)))
    assert seen == {0, 1, 2}
    m.close()


def test_hook_analysis_length_follows_the_literal_loop():
    m = api.BinauralMaskingImpl(FS, D, LO, HI)
    tw = bt.Twin(FS, D, LO, HI)
    W = tw.W
    x = np.random.default_rng(5).standard_normal(W) * tw.win
    full = m.frame_analysis(x)                       # 46 W: 45 bands + the residual
    assert np.abs(full.reshape(46, W).sum(axis=0) - x).max() <= 1e-10 * np.abs(x).max()
    short = m.frame_analysis(x, 45 * W)              # 45 W: 45 bands, no residual
    assert np.array_equal(short, full[:45 * W])
    odd = m.frame_analysis(x, 3 * W + 5)             # three bands fit, the rest is not written
    assert np.array_equal(odd[:3 * W], full[:3 * W]) and not odd[3 * W:].any()
    bands = full.reshape(46, W)
    y46, y45 = m.frame_synthesis(full, 46 * W), m.frame_synthesis(full, 45 * W)
    assert np.abs(y46 - bands[:45].sum(axis=0)).max() <= 1e-10 * np.abs(x).max()      # all 45 bands, no residual
    assert np.abs(y45 - bands[:44].sum(axis=0)).max() <= 1e-10 * np.abs(x).max()      # band 44 dropped
    assert np.abs(y46 - y45 - bands[44]).max() <= 1e-10 * np.abs(x).max()
    with pytest.raises(api.MCArrayHipError):
        m.process_parametrisation(full[:44 * W], full[:44 * W])
    m.close()


def test_muted_channel_and_q_guard():
    """right = 0: the correlation's denominator is 0, ncorr = 1, no band is ever masked spatially.  On a signal whose band
    powers rise from frame to frame (P >= the updated Q) that leaves enhance everywhere; on the parity input the temporal
    rule still fires, as in the twin."""
    rising = bt.rising_tones(FS, D, LO, HI, 40)
    rising[1] = 0
    noisy = bt.parity_input(42).copy()
    noisy[1] = 0
    for method in bt.METHODS:
        m = api.BinauralMaskingImpl(FS, D, LO, HI, method)
        out, dec = m.process(rising)
        assert np.isfinite(out).all()
        assert (dec == 0).all(), method
        m.reset()
        out, dec = m.process(noisy)
        assert np.isfinite(out).all()
        assert not (dec == 2).any(), method
        _check_stream("muted right channel, method %d" % method, out[0], dec[0], bt.Twin(FS, D, LO, HI, method).stream(noisy))
        m.close()
    anti = bt.parity_input(42).copy()
    anti[1] = -anti[0]                           # l = -r: P = 0 and Q = 0 in every band, the RELATIVE gain would divide by zero
    m = api.BinauralMaskingImpl(FS, D, LO, HI, bt.RELATIVE)
    out, dec = m.process(anti)
    assert np.isfinite(out).all()
    assert (dec == 2).all()                      # ncorr = -1
    tw = bt.Twin(FS, D, LO, HI, bt.RELATIVE).stream(anti)
    assert np.abs(out[0] - tw["out"]).max() <= 2e-5 * np.abs(tw["out"]).max() + 1e-7
    m.close()


def test_silent_band_keeps_its_temporal_decision():
    """60 frames of exact digital silence after 41 frames of signal: P is 0 and Q decays by 0.04 per frame, to about 1e-87 of
    its value.  The stream path carries Q in double like the twin, so every silent cell still decides temporal (margin 1,
    nowhere near a tie); an fp32 Q would have reached 0 after about 27 frames and decided enhance from there on."""
    hop = bt.Twin(FS, D, LO, HI).W // 2
    x = bt.parity_input(41)[:, :101 * hop].copy()
    x[:, 41 * hop:] = 0
    for method in bt.METHODS:
        m = api.BinauralMaskingImpl(FS, D, LO, HI, method)
        out, dec = m.process(x)
        tw = bt.Twin(FS, D, LO, HI, method).stream(x)
        assert (tw["dec"][41:] == 1).all()
        assert (dec[0][41:] == 1).all(), method
        assert np.isfinite(out).all()
        _check_stream("silence after 41 frames, method %d" % method, out[0], dec[0], tw)
        m.close()


def test_cxx_class_end_to_end(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "test_binaural_masking_impl"
    lib_dir = os.path.join(ROOT, "mcarray_amd")
    subprocess.check_call([cxx, "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "test_binaural_masking_impl.cpp"), "-o", str(exe), "-L" + lib_dir,
                           "-lmcarray_hip", "-Wl,-rpath," + lib_dir], timeout=300)
    bt.spatial_signal().T.astype(np.int16).tofile(str(tmp_path / "spatial.raw"))      # interleaved
    r = subprocess.run([str(exe), str(tmp_path / "spatial.raw"), str(tmp_path / "out.raw")], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL PASSED" in r.stdout
    out = np.fromfile(str(tmp_path / "out.raw"), dtype=np.int16).reshape(-1, 2).T.astype(np.float64)
    p_sig, p_int = bt.spatial_powers(out[0])
    print("C++ process(SignalVector16s): signal %.2f dB, interferer %.2f dB" % (p_sig, p_int))
    assert abs(70 - p_sig) <= 10
    assert abs(70 - p_int) <= 10
