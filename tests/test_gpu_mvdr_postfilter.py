"""GPU: the decision-directed Wiener post-filter of the MVDR calls (mca_hip_mvdr_set_postfilter; k_mvdr_solve_t<..., NOISE = true> of
mvdr_solve.h, k_mvdr_postfilter in kernels_mvdr_postfilter.hip) against the float64 twin of the dense definition
(tests/mvdr_postfilter_twin.py).

The bars: 5e-4 of the peak of the twin's UNFILTERED spectra (audio) of the call for the filtered spectra (audio) -- the absolute bar
the plain call is held to: the filter does not amplify the solve's fp32 error (G <= 1, and an error of p moves G Y by less than it
moves p) -- and 5e-6 for the covariance.  tests/test_mvdr_postfilter_twin.py shows that filtered and unfiltered spectra are at least
20 bars apart on every parity scene, so a kernel that ignores the filter cannot pass.  Every case prints its worst values."""
import struct

import numpy as np
import pytest

from mcarray_amd import api, synth

import mvdr_gate_twin as gt
import mvdr_nulls_twin as nt
import mvdr_postfilter_twin as pt

pytestmark = pytest.mark.gpu

SPEC_TOL, AUDIO_TOL, COV_TOL = pt.PARITY_BAR, pt.PARITY_BAR, 5e-6
NAN = float("nan")
W12 = pt.W12


def _same(r, q, what=""):
    assert np.array_equal(r["spec"].view(np.float32), q["spec"].view(np.float32), equal_nan=True), what
    assert np.array_equal(r["out"], q["out"], equal_nan=True), what


def _cat(rs, axis):
    return dict(spec=np.concatenate([r["spec"] for r in rs], axis=axis), out=np.concatenate([r["out"] for r in rs], axis=axis))


def _check_against_twin(r, tw, a, what, worst, audio=True):
    """every source of stream a of the GPU result r ([A][S][...]) against the twin's filtered result, on the scale of its unfiltered one"""
    for s in range(tw["spec"].shape[0]):
        assert np.all(np.isfinite(r["spec"][a, s])), (what, a, s)
        es = np.abs(r["spec"][a, s] - tw["spec"][s]).max() / np.abs(tw["raw"][s]).max()
        ea = 0.0
        if audio:
            assert np.all(np.isfinite(r["out"][a, s])), (what, a, s)
            ea = np.abs(r["out"][a, s] - tw["out"][s]).max() / np.abs(tw["raw_out"][s]).max()
        print("%s stream %d source %d: spectra %.2e audio %.2e of the unfiltered peak" % (what, a, s, es, ea))
        worst[0], worst[1] = max(worst[0], es), max(worst[1], ea)
        assert es <= SPEC_TOL, (what, a, s)
        assert ea <= AUDIO_TOL, (what, a, s)


def _check_covariance(bf, tw, a, what, worst):
    ec = np.abs(bf.covariance(a) - tw["phi"]).max() / np.abs(tw["phi"]).max()
    print("%s stream %d: covariance %.2e" % (what, a, ec))
    worst[2] = max(worst[2], ec)
    assert ec <= COV_TOL, (what, a)


def _bf(fs, xs, N, A, S, gain, pf=None):
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=gain)
    if pf is not None:
        bf.set_postfilter(True, **pf)
    return bf


@pytest.mark.parametrize("case", pt.parity_cases(), ids=lambda c: c[0])
def test_postfilter_parity(case):
    """a fresh enabled context, two calls (the second continues the recursion, A and every source's overlap-add) against the twin:
    every number of row slots per lane, the plain, the multi-source and the nulling solve, the two instantiations that gave up the
    load a frame ahead, long frames, and a call without weights (the buffer of ones)"""
    name, M, fs, N, F, S, gain, weighted = case
    p = pt.parity(case)
    A, hop = p["pcm"].shape[0], N // 2
    bf = _bf(fs, p["xs"], N, A, S, gain, pt.PARITY_PF)
    bf.set_timing(True)
    worst = [0.0, 0.0, 0.0]
    for i, (t0, t1) in enumerate([(0, F), (F, 2 * F)]):
        upd = None if p["weights"] is None else p["weights"][:, t0:t1]
        r = bf.process_sources(p["pcm"][:, :, t0 * hop:(t1 + 1) * hop].copy(), p["doa"][:, t0:t1].copy(), update=upd)
        assert r["out"].shape == (A, S, F * hop) and r["spec"].shape == (A, S, F, N // 2 + 1)
        for a in range(A):
            _check_against_twin(r, p["calls"][i][a], a, "%s call %d" % (name, i), worst)
            _check_covariance(bf, p["calls"][i][a], a, "%s call %d" % (name, i), worst)
    assert bf.get_timing(bf.K_POSTFILTER)[0] == 2 and bf.get_timing(bf.K_SOLVE)[0] == 2
    bf.close()
    print("%s: worst spectra %.2e audio %.2e covariance %.2e" % (name, worst[0], worst[1], worst[2]))


@pytest.mark.parametrize("geo", ["ula16_s1", "m13_s3", "five_s2", "m13_s3_nulls", "ula16_s4_nulls"])
@pytest.mark.parametrize("weights", ["weights", "none"])
def test_gain_floor_one_is_the_disabled_call(geo, weights):
    """gain_floor = 1: the bytes of a context that never enabled the filter, in spectra, audio and covariance, through the plain,
    the sources and the nulls kernels, with weights and without (the ones buffer against the unweighted kernels).  Stream 2 stays in
    digital silence (p = 0).  Enabling and disabling again gives the never-enabled bytes as well, by the kernels it always took."""
    xs, fs, N, F = {"ula16": (synth.ULA16, 48000, 256, 7), "m13": (pt.irregular(13), 16000, 256, 6),
                    "five": ([0.0, 0.03, 0.07, 0.10, 0.20], 8000, 256, 9)}[geo.split("_")[0]]
    S = int(geo.split("_")[1][1])
    gain = 100.0 if geo.endswith("nulls") else 0.0
    A, hop = 3, N // 2
    pcm = np.stack([nt.scene(xs, fs, N, 2 * F, a) for a in range(A)])
    pcm[2] = pcm[0] * np.float32(1e-18)
    doa = nt.drifting_doa(A, 2 * F, S)
    w = None if weights == "none" else np.tile(W12[[0, 1, 0]], (1, 2))[:, :2 * F]

    def run(bf, single):
        rs = []
        for t0, t1 in ((0, F), (F, 2 * F)):
            x, u = pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), None if w is None else w[:, t0:t1]
            if single:
                r = bf.process(x, doa[:, t0:t1, 0].copy(), want_spec=True, update=u)
                r = dict(out=r["out"][:, None], spec=r["spec"][:, None])
            else:
                r = bf.process_sources(x, doa[:, t0:t1].copy(), update=u)
            rs.append(r)
        return _cat(rs, 2), [bf.covariance(a) for a in range(A)]

    ref, ref_cov = run(_bf(fs, xs, N, A, S, gain), S == 1)
    one_bf = _bf(fs, xs, N, A, S, gain, dict(smoothing=0.7, gain_floor=1.0, noise_scale=3.0))
    one_bf.set_timing(True)
    one, one_cov = run(one_bf, S == 1)
    _same(one, ref, "gain_floor 1")
    assert all(np.array_equal(x, y) for x, y in zip(one_cov, ref_cov))
    assert one_bf.get_timing(one_bf.K_POSTFILTER)[0] == 2
    # a filter that filters is another output, with the same covariance; silence passes unchanged
    filt, filt_cov = run(_bf(fs, xs, N, A, S, gain, pt.PARITY_PF), S == 1)
    assert not np.array_equal(filt["spec"][:2], ref["spec"][:2])
    assert np.array_equal(filt["spec"][2], ref["spec"][2]) and np.array_equal(filt["out"][2], ref["out"][2])
    assert all(np.array_equal(x, y) for x, y in zip(filt_cov, ref_cov))
    # enabled, then disabled: never enabled
    off_bf = _bf(fs, xs, N, A, S, gain, pt.PARITY_PF)
    off_bf.set_postfilter(False)
    off_bf.set_timing(True)
    assert off_bf.get_postfilter() == dict(enable=False, smoothing=0.98, gain_floor=0.1, noise_scale=1.0)
    off, off_cov = run(off_bf, S == 1)
    _same(off, ref, "enabled, then disabled")
    assert all(np.array_equal(x, y) for x, y in zip(off_cov, ref_cov))
    assert off_bf.get_timing(off_bf.K_POSTFILTER)[0] == 0


@pytest.mark.parametrize("M,S,gain", [(16, 1, 0.0), (13, 3, 0.0), (8, 4, 10.0), (5, 2, 0.0)])
def test_postfilter_cut_invariance(M, S, gain):
    """12 frames in one call, as 5 + 7 and as 12 calls of one frame: the same bytes (A carries everything); the same input at
    streams 0 and 3 gives the same bytes; re-enabling starts from zero like a fresh context"""
    fs, N, F, A = 16000, 256, 12, 4
    xs = pt.irregular(M)
    hop = N // 2
    pcm = np.stack([nt.scene(xs, fs, N, F, a % 3) for a in range(A)])
    doa = np.stack([nt.drifting_doa(3, F, S)[a % 3] for a in range(A)])
    w = np.array([[1, .5, 1, 0, 0, 0, 0, 1, 0, 0, .25, 0], [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], [1] * 12, [0] * 12], dtype=np.float32)
    w[3] = w[0]
    one_bf = _bf(fs, xs, N, A, S, gain, pt.PARITY_PF)
    one = one_bf.process_sources(pcm, doa, update=w)
    assert np.array_equal(one["spec"][0], one["spec"][3]) and np.array_equal(one["out"][0], one["out"][3])
    assert np.array_equal(one_bf.covariance(0), one_bf.covariance(3))
    for cuts in ([0, 5, 12], list(range(13))):
        bf = _bf(fs, xs, N, A, S, gain, pt.PARITY_PF)
        rs = [bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy(), update=w[:, t0:t1])
              for t0, t1 in zip(cuts[:-1], cuts[1:])]
        _same(_cat(rs, 2), one, "%d calls" % (len(cuts) - 1))
        for a in range(A):
            assert np.array_equal(bf.covariance(a), one_bf.covariance(a)), a
        bf.close()
    # the three values may change between calls without touching A; disable + enable + reset start over
    one_bf.set_postfilter(False)
    one_bf.set_postfilter(True, **pt.PARITY_PF)
    one_bf.reset()
    _same(one_bf.process_sources(pcm, doa, update=w), one, "re-enabled and reset")
    one_bf.reset()
    _same(one_bf.process_sources(pcm, doa, update=w), one, "reset")


def test_postfilter_pieced_tail_launch():
    """256 streams x 129 bins = 516 solve workgroups: the 4 behind the last whole round go in a second launch cut along the frames
    into pieces, each of which stores Y and the noise plane of its own frames only; two calls of 8 frames cut theirs differently.
    Streams 0 (main launch) and 255 (pieced) against the twin, and the two cuts agree bit for bit."""
    fs, N, F, A, M = 16000, 256, 16, 256, 4
    xs = pt.irregular(M)
    hop = N // 2
    base = np.stack([nt.scene(xs, fs, N, F, a) for a in range(3)])
    pick = np.arange(A) % 3
    pick[255] = 0
    pcm = base[pick]
    doa = nt.drifting_doa(3, F, 1)[pick][:, :, 0].copy()
    rng = np.random.default_rng(7)
    w = rng.choice(np.array([0, 0, 1, 1, .5, .125], dtype=np.float32), size=(A, F))
    w[0] = [1, 1, .5, 0, 0, 1, .25, 0, 0, 0, 1, .75, 0, 1, 0, 0]
    w[255, :3] = [1, .5, 1]
    w[255, 3:] = 0
    w[3] = w[0]
    bf = _bf(fs, xs, N, A, 1, 0.0, pt.PARITY_PF)
    one = bf.process(pcm, doa, want_spec=True, update=w)
    worst = [0.0, 0.0, 0.0]
    for a in (0, 255):
        tw = pt.mvdr_postfilter_stream(fs, N, xs, pcm[a].astype(np.float64), doa[a], 0.0, w[a], **pt.PARITY_PF)
        _check_against_twin(dict(spec=one["spec"][:, None], out=one["out"][:, None]), tw, a, "256 streams", worst)
        _check_covariance(bf, tw, a, "256 streams", worst)
    assert np.array_equal(one["spec"][0], one["spec"][3]) and np.array_equal(bf.covariance(0), bf.covariance(3))
    two_bf = _bf(fs, xs, N, A, 1, 0.0, pt.PARITY_PF)
    r1 = two_bf.process(pcm[:, :, :(8 + 1) * hop].copy(), doa[:, :8].copy(), want_spec=True, update=w[:, :8])
    r2 = two_bf.process(pcm[:, :, 8 * hop:].copy(), doa[:, 8:].copy(), want_spec=True, update=w[:, 8:])
    _same(_cat([r1, r2], 1), one, "two calls of 8 frames")
    for a in (0, 1, 2, 254, 255):
        assert np.array_equal(two_bf.covariance(a), bf.covariance(a)), a


@pytest.mark.parametrize("middle_audio", [True, False])
def test_postfilter_slots(middle_audio):
    """S = 2, then S = 1, then S = 2 on a context of two slots: the call that leaves slot 1 out zeroes its A, with out_pcm or without
    (without, the overlap-add tails stay as they were, so the third call is compared in its spectra only)"""
    fs, N, F, A, S = 16000, 256, 4, 2, 2
    xs = pt.irregular(6)
    hop = N // 2
    pcm = np.stack([nt.scene(xs, fs, N, 3 * F, a) for a in range(A)])
    doa = nt.drifting_doa(A, 3 * F, S)
    bf = _bf(fs, xs, N, A, S, 0.0, pt.PARITY_PF)
    state, worst = [None] * A, [0.0, 0.0, 0.0]
    for i, ns in enumerate((2, 1, 2)):
        t0, t1 = i * F, (i + 1) * F
        audio = middle_audio or i != 1
        r = bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1, :ns].copy(), want_audio=audio, update=W12[:, t0:t1])
        for a in range(A):
            state[a] = pt.mvdr_postfilter_stream(fs, N, xs, pcm[a, :, t0 * hop:(t1 + 1) * hop].astype(np.float64), doa[a, t0:t1, :ns], 0.0,
                                                 W12[a, t0:t1], state=state[a], **pt.PARITY_PF)
            _check_against_twin(r, state[a], a, "call %d (%d sources)" % (i, ns), worst, audio=middle_audio and audio)
    # slot 1 of the third call is NOT what an uninterrupted two-source stream gives: its A restarted
    full = _bf(fs, xs, N, A, S, 0.0, pt.PARITY_PF)
    for i in range(3):
        q = full.process_sources(pcm[:, :, i * F * hop:((i + 1) * F + 1) * hop].copy(), doa[:, i * F:(i + 1) * F].copy(), update=W12[:, i * F:(i + 1) * F])
    assert np.array_equal(q["spec"][:, 0], r["spec"][:, 0]) and not np.array_equal(q["spec"][:, 1], r["spec"][:, 1])
    # set_max_sources keeps the slots both sizes have
    full.set_max_sources(3)
    bf2 = _bf(fs, xs, N, A, S, 0.0, pt.PARITY_PF)
    for i in range(3):
        bf2.process_sources(pcm[:, :, i * F * hop:((i + 1) * F + 1) * hop].copy(), doa[:, i * F:(i + 1) * F].copy(), update=W12[:, i * F:(i + 1) * F])
    x, d = pcm[:, :, :(F + 1) * hop].copy(), doa[:, :F].copy()
    _same(full.process_sources(x, d), bf2.process_sources(x, d), "three slots against two")
    full.set_max_sources(1)
    bf2.set_max_sources(1)
    _same(full.process_sources(x, d[:, :, :1].copy()), bf2.process_sources(x, d[:, :, :1].copy()), "one slot")


def _header(blob):
    magic, version, cfg_hash, pad, h0, h1, h2, h3 = struct.unpack("<IiIi4q", blob[:48])
    return version, h0, h1


def test_postfilter_state_blobs():
    fs, N, F, A, S = 16000, 256, 5, 2, 2
    xs = synth.REEM_C
    hop, K = N // 2, N // 2 + 1
    pcm = np.stack([nt.scene(xs, fs, N, 2 * F, a) for a in range(A)])
    doa = nt.drifting_doa(A, 2 * F, S)
    x1, d1, x2, d2 = pcm[:, :, :(F + 1) * hop].copy(), doa[:, :F].copy(), pcm[:, :, F * hop:].copy(), doa[:, F:].copy()
    bf = _bf(fs, xs, N, A, S, 10.0, pt.PARITY_PF)
    bf.process_sources(x1, d1, update=W12[:, :F])
    blob = bf.state_save()
    plain = _bf(fs, xs, N, A, S, 10.0)
    plain.process_sources(x1, d1, update=W12[:, :F])
    blob2 = plain.state_save()
    assert _header(blob) == (3, S, 1) and _header(blob2)[0] == 2
    assert len(blob) == len(blob2) + A * S * K * 4 and blob[48:len(blob2)] != blob2[48:]      # the tails differ: filtered audio
    assert blob[48:48 + A * K * (len(xs) * (len(xs) + 1) // 2) * 8] == blob2[48:48 + A * K * (len(xs) * (len(xs) + 1) // 2) * 8]   # the covariance does not
    ref = bf.process_sources(x2, d2, update=W12[:, F:2 * F])
    # save mid-stream, load into a second enabled context (other parameter values are no obstacle: they are not in the blob)
    other = _bf(fs, xs, N, A, S, 10.0, dict(smoothing=0.1, gain_floor=0.9, noise_scale=7.0))
    other.process_sources(x2, d2)                                  # (something else in its state)
    other.state_load(blob)
    other.set_postfilter(True, **pt.PARITY_PF)
    _same(other.process_sources(x2, d2, update=W12[:, F:2 * F]), ref, "continued from the blob")
    assert all(np.array_equal(other.covariance(a), bf.covariance(a)) for a in range(A))
    # the refusals, each leaving the state as it was
    one_slot = api.MvdrBeamformer(fs, xs, N, max_streams=A)
    one_slot.process(x1, d1[:, :, 0].copy())
    blob1 = one_slot.state_save()
    assert _header(blob1)[0] == 1
    three = _bf(fs, xs, N, A, 3, 10.0, pt.PARITY_PF)
    blob3 = three.state_save()
    assert _header(blob3) == (3, 3, 1)

    def refused(ctx, bad, match):
        twin_ctx = _bf(fs, xs, N, A, S, 10.0, pt.PARITY_PF if ctx.get_postfilter()["enable"] else None)
        twin_ctx.state_load(ctx.state_save())
        with pytest.raises(api.MCArrayHipError, match=match):
            ctx.state_load(bad)
        _same(ctx.process_sources(x2, d2, update=W12[:, F:2 * F]), twin_ctx.process_sources(x2, d2, update=W12[:, F:2 * F]), match)

    en = _bf(fs, xs, N, A, S, 10.0, pt.PARITY_PF)
    en.process_sources(x1, d1)
    refused(en, blob2, "without the post-filter")                   # version 2 into an enabled context
    refused(en, blob1, "without the post-filter")                   # version 1
    refused(en, blob3, "max_sources")                               # version 3 of another max_sources
    refused(plain, blob, "post-filter enabled")                     # version 3 into a disabled context
    plain.state_load(blob2)                                          # and disabled contexts read what they always did


def test_postfilter_refusals_leave_configuration_and_state():
    import ctypes as C
    fs, N, F, A = 16000, 256, 4, 2
    xs = synth.REEM_C
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    doa = nt.drifting_doa(A, F, 1)[:, :, 0].copy()
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A)
    assert bf.get_postfilter() == dict(enable=False, smoothing=0.98, gain_floor=0.1, noise_scale=1.0)
    # timing slot 4 exists once the filter has been enabled, and stays after disabling; before, the id is refused as it always was
    assert bf._lib.mca_hip_mvdr_get_timing(bf.h, 4, None, None) == -1
    with pytest.raises(api.MCArrayHipError):
        bf.set_postfilter(True, smoothing=1.0)
    assert bf._lib.mca_hip_mvdr_get_timing(bf.h, 4, None, None) == -1          # a refused enable does not create it
    held = dict(smoothing=0.5, gain_floor=0.25, noise_scale=2.0)
    bf.set_postfilter(True, **held)
    bf.process(pcm, doa)
    blob = bf.state_save()
    inf = float("inf")
    bad = [dict(smoothing=-0.01), dict(smoothing=1.0), dict(smoothing=NAN), dict(smoothing=inf), dict(smoothing=-inf),
           dict(gain_floor=-0.01), dict(gain_floor=1.01), dict(gain_floor=NAN), dict(gain_floor=inf),
           dict(noise_scale=0.0), dict(noise_scale=-1.0), dict(noise_scale=100.5), dict(noise_scale=NAN), dict(noise_scale=inf)]
    for kw in bad:
        for enable in (True, False):                                # a refused disable does not disable either
            with pytest.raises(api.MCArrayHipError, match="must be finite"):
                bf.set_postfilter(enable, **dict(dict(smoothing=0.9, gain_floor=0.3, noise_scale=4.0), **kw))
            assert bf.get_postfilter() == dict(enable=True, **held), kw
    cfg = api._lib.MvdrPostfilterConfig(C.sizeof(api._lib.MvdrPostfilterConfig) - 8, 0, 0.9, 0.3, 4.0)
    assert bf._lib.mca_hip_mvdr_set_postfilter(bf.h, C.byref(cfg)) == -1
    assert bf._lib.mca_hip_mvdr_set_postfilter(bf.h, None) == -1
    assert bf.get_postfilter() == dict(enable=True, **held)
    assert bf.state_save() == blob
    # the limits themselves are accepted
    bf.set_postfilter(True, smoothing=0.0, gain_floor=0.0, noise_scale=100.0)
    bf.set_postfilter(True, smoothing=0.999, gain_floor=1.0, noise_scale=1e-3)
    assert bf.state_save() == blob                                  # and changing the three values does not touch A
    assert bf.get_postfilter() == dict(enable=True, smoothing=0.999, gain_floor=1.0, noise_scale=1e-3)
    assert bf.get_timing(bf.K_POSTFILTER) == (0, 0.0) and bf._lib.mca_hip_mvdr_get_timing(bf.h, 5, None, None) == -1
    bf.set_postfilter(False)
    assert bf.get_timing(bf.K_POSTFILTER) == (0, 0.0)


@pytest.mark.parametrize("S,gain", [(1, 0.0), (3, 100.0)])
def test_postfilter_dev_entry_under_a_padded_offset_stride(S, gain):
    """the _dev entry with PCM at padded, offset strides in a poisoned allocation and guarded outputs equals the contiguous call bit
    for bit, with weights and without, spectra to the caller's buffer and to the workspace"""
    import torch
    from dev_layout_helpers import guarded, strided_pcm
    fs, N, F, A = 48000, 1024, 6, 2
    xs = synth.ULA8
    hop, K = N // 2, N // 2 + 1
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    doa = nt.drifting_doa(A, F, S)
    w = W12[:, 3:3 + F].copy()
    for upd in (w, None):
        ref_bf = _bf(fs, xs, N, A, S, gain, pt.PARITY_PF)
        ref = ref_bf.process_sources(pcm, doa, update=upd)
        bf = _bf(fs, xs, N, A, S, gain, pt.PARITY_PF)
        view, whole = strided_pcm(pcm)
        t_doa, t_w = torch.from_numpy(doa).cuda(), None if upd is None else torch.from_numpy(upd).cuda()
        g_out, g_spec = guarded((A, S, F * hop), torch.float32), guarded((A, S, F, K, 2), torch.float32)
        if S == 1:
            bf.process_dev(view, F, t_doa[:, :, 0].contiguous(), out_pcm=g_out.t, out_spec=g_spec.t, update=t_w)
        else:
            bf.process_sources_dev(view, F, t_doa, out_pcm=g_out.t, out_spec=g_spec.t, update=t_w)
        torch.cuda.synchronize()
        g_out.assert_guards_intact("out"); g_spec.assert_guards_intact("spec")
        spec = g_spec.t.cpu().numpy()
        assert np.array_equal(spec.reshape(ref["spec"].shape + (2,)), ref["spec"].view(np.float32).reshape(ref["spec"].shape + (2,)))
        assert np.array_equal(g_out.t.cpu().numpy(), ref["out"])
        for a in range(A):
            assert np.array_equal(bf.covariance(a), ref_bf.covariance(a)), a
        # audio alone: the spectra are filtered in the workspace
        bf.reset()
        g_out2 = guarded((A, S, F * hop), torch.float32)
        bf.process_sources_dev(view, F, t_doa, out_pcm=g_out2.t, update=t_w)
        torch.cuda.synchronize()
        g_out2.assert_guards_intact("out alone")
        assert np.array_equal(g_out2.t.cpu().numpy(), ref["out"])


def test_postfilter_scene_interferer_down_target_kept():
    """the self-cancellation scene with a noise-only covariance at look 20 degrees, the defaults, powers over the frames 36 ... 47, from
    the GPU's own filtered and unfiltered spectra: interferer alone < 0.03, with the target > 0.95 (the twin: 0.0146 and 0.9685)"""
    ratio = {}
    for target in (False, True):
        xs, pcm, update = gt.cancellation_scene(target=target)
        bf = api.MvdrBeamformer(gt.CANCEL_FS, xs, gt.CANCEL_N)
        raw = bf.process(pcm, np.deg2rad(20.0), want_spec=True, update=update)
        bf.reset()
        bf.set_postfilter()
        fil = bf.process(pcm, np.deg2rad(20.0), want_spec=True, update=update)
        pu, pf = gt.last_frames_power(raw["spec"][0]), gt.last_frames_power(fil["spec"][0])
        ratio[target] = pf / pu
        print("target %s: unfiltered %.4g filtered %.4g ratio %.4f" % (target, pu, pf, pf / pu))
    assert ratio[False] < 0.03
    assert ratio[True] > 0.95


def test_postfilter_results_do_not_move_beside_a_matrix_core_neighbour():
    """the solve with the noise plane and the post-filter beside the neighbour of tests/test_gpu_coresidency.py (the procedure of
    test_gate_results_do_not_move_beside_a_matrix_core_neighbour): 16 microphones, three look directions"""
    import ctypes as C
    import time
    import torch
    import test_gpu_coresidency as tc
    nb = tc._neighbour()
    dev = torch.device("cuda:0")
    F, A, N, S, xs = 60, 16, 1024, 3, synth.ULA16
    pcm = np.stack([synth.noise_source_stream(xs, np.deg2rad(20.0 - 7 * a), 48000, (F + 1) * N // 2, 80 + a) for a in range(A)]).astype(np.float32)
    doa = (np.deg2rad(20.0 - 7 * np.arange(A))[:, None, None] + 0.01 * np.arange(F)[None, :, None] + nt.OFFSETS[None, None, :S]).astype(np.float32)
    w = np.tile(W12[0], (A, F // 12))

    def fn():
        bf = api.MvdrBeamformer(48000, xs, N, max_streams=A, max_sources=S)
        bf.set_postfilter(True, **pt.PARITY_PF)
        r = bf.process_sources(pcm, doa, update=w)
        cov = bf.covariance(A - 1)
        bf.close()
        return r["out"], r["spec"], cov

    side = torch.cuda.Stream(device=dev)
    sink = torch.zeros(1024 * 256, dtype=torch.float32, device=dev)
    fn()                                                                      # (loads code objects)
    t0 = time.perf_counter()
    ref = fn()
    call_s = time.perf_counter() - t0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record()
        assert nb.neighbour_launch(tc._cus(dev), 20000, C.c_void_p(sink.data_ptr()), C.c_void_p(side.cuda_stream)) == 0
        e1.record()
    torch.cuda.synchronize()
    per_iter_s = e0.elapsed_time(e1) * 1e-3 / 20000
    iters = int(min(max(2.0 * call_s, 0.02), 3.0) / per_iter_s)
    for rep in range(2):
        torch.cuda.synchronize()
        assert nb.neighbour_launch(tc._cus(dev), iters, C.c_void_p(sink.data_ptr()), C.c_void_p(side.cuda_stream)) == 0
        got = fn()
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip(ref, got)):
            assert np.array_equal(x, y), "output %d moved beside the neighbour (%d values)" % (i, int((x != y).sum()))
