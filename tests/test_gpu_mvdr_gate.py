"""GPU: per-frame covariance update weights of the MVDR calls (mca_hip_mvdr_sources_frames_weighted_*; k_mvdr_solve_t<..., WEIGHT = FRAME, ...>
of mvdr_solve.h) against the float64 twin of the dense definition (tests/mvdr_gate_twin.py).

The bars are the ones tests/test_gpu_mvdr.py sets for this solve: 5e-4 of the peak for spectra and audio, 5e-6 for the covariance.
tests/test_mvdr_gate_twin.py shows that the weighted spectra and covariance differ from the unweighted ones by more than 0.1 of
the peak on the scene used here, so a kernel that ignores the weights cannot pass.  Every test prints the worst case over its
streams, sources and calls (spectra / audio / covariance, of the peak); no MI355X figures are recorded here yet."""
import numpy as np
import pytest

from mcarray_amd import api, synth
from oracle import pyoracle as po

import mvdr_gate_twin as gt
import mvdr_nulls_twin as nt

pytestmark = pytest.mark.gpu

SPEC_TOL, AUDIO_TOL, COV_TOL = 5e-4, 5e-4, 5e-6
NAN = float("nan")
# 12 weights per stream for two calls of 6 frames: 1, fractional values, a zero on the first frame of the second call inside a run
# of zeros that crosses the call boundary; stream 1 also a NaN (counts as 0) and a 2.0 (counts as 1)
W12 = np.array([[1, 1, .5, 0, 1, 0, 0, 0, .25, 1, 0, .75],
                [1, .3, 1, 2.0, 0, 0, 0, NAN, 1, .6, 0, 0]], dtype=np.float32)


def _irregular(M):
    return np.sort(np.random.default_rng(M).uniform(0.0, 0.04 * M, M))


def _same(r, q, what=""):
    assert np.array_equal(r["spec"].view(np.float32), q["spec"].view(np.float32), equal_nan=True), what
    assert np.array_equal(r["out"], q["out"], equal_nan=True), what


def _cat(rs, axis):
    return dict(spec=np.concatenate([r["spec"] for r in rs], axis=axis), out=np.concatenate([r["out"] for r in rs], axis=axis))


def _check_against_twin(r, tw, a, what, worst):
    """every source of stream a of the GPU result r ([A][S][...]) against the twin's result tw"""
    for s in range(tw["spec"].shape[0]):
        assert np.all(np.isfinite(r["spec"][a, s])) and np.all(np.isfinite(r["out"][a, s])), (what, a, s)
        es = np.abs(r["spec"][a, s] - tw["spec"][s]).max() / np.abs(tw["spec"][s]).max()
        ea = np.abs(r["out"][a, s] - tw["out"][s]).max() / np.abs(tw["out"][s]).max()
        print("%s stream %d source %d: spectra %.2e audio %.2e of the peak" % (what, a, s, es, ea))
        worst[0], worst[1] = max(worst[0], es), max(worst[1], ea)
        assert es <= SPEC_TOL, (what, a, s)
        assert ea <= AUDIO_TOL, (what, a, s)


def _check_covariance(bf, tw, a, what, worst):
    ec = np.abs(bf.covariance(a) - tw["phi"]).max() / np.abs(tw["phi"]).max()
    print("%s stream %d: covariance %.2e" % (what, a, ec))
    worst[2] = max(worst[2], ec)
    assert ec <= COV_TOL, (what, a)


def _two_calls_against_twin(xs, fs, N, F, S, gain, weights, what):
    """a fresh context, two calls of F frames (the second continues the recursion and every source's overlap-add) against the twin"""
    A, hop = weights.shape[0], N // 2
    pcm = np.stack([nt.scene(xs, fs, N, 2 * F, a) for a in range(A)])
    doa = nt.drifting_doa(A, 2 * F, S)
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=gain)
    worst = [0.0, 0.0, 0.0]
    state = [None] * A
    for i, (t0, t1) in enumerate([(0, F), (F, 2 * F)]):
        r = bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy(), update=weights[:, t0:t1])
        assert r["out"].shape == (A, S, F * hop) and r["spec"].shape == (A, S, F, N // 2 + 1)
        for a in range(A):
            state[a] = gt.mvdr_gate_stream(fs, N, xs, pcm[a, :, t0 * hop:(t1 + 1) * hop].astype(np.float64), doa[a, t0:t1], gain,
                                           weights[a, t0:t1], state=state[a])
            _check_against_twin(r, state[a], a, "%s call %d" % (what, i), worst)
            _check_covariance(bf, state[a], a, "%s call %d" % (what, i), worst)
    bf.close()
    print("%s: worst spectra %.2e audio %.2e covariance %.2e" % (what, worst[0], worst[1], worst[2]))


@pytest.mark.parametrize("S,gain", [(1, 0.0), (2, 0.0), (2, 10.0), (4, 0.0), (4, 10.0)])
@pytest.mark.parametrize("M", [2, 3, 4, 5, 8, 11, 13, 16])
def test_gate_every_row_slot_count(M, S, gain):
    """every number of row slots per lane with a full and a partly empty last slot, the plain, the multi-source and the nulling
    solve; the instantiations that reuse the factor on frozen frames and those that factorise again"""
    _two_calls_against_twin(_irregular(M), 16000, 256, 6, S, gain, W12, "M %d S %d gain %g" % (M, S, gain))


@pytest.mark.parametrize("N,fs,F,S,gain", [(1024, 48000, 6, 3, 100.0), (2048, 96000, 4, 4, 0.0)])
def test_gate_long_frames(N, fs, F, S, gain):
    w = np.concatenate([W12[:, :F], W12[:, 6:6 + F]], axis=1)
    _two_calls_against_twin(synth.ULA16, fs, N, F, S, gain, w, "N %d" % N)


@pytest.mark.parametrize("geo", ["ula16_s1", "ula16_s4", "m13_s3", "five_s2", "ula16_s4_nulls", "m13_s3_nulls", "five_s2_nulls"])
def test_gate_all_ones_and_null_pointer_are_the_unweighted_call(geo):
    """weights all 1 run the weighted kernel, None passes the NULL pointer: both give the bytes of the unweighted entry point in
    spectra, audio and covariance.  Stream 2 stays in digital silence: the w = d/M branch."""
    xs, fs, N, F, S = {"ula16": (synth.ULA16, 48000, 256, 7), "m13": (_irregular(13), 16000, 256, 6),
                       "five": ([0.0, 0.03, 0.07, 0.10, 0.20], 8000, 256, 9)}[geo.split("_")[0]] + (int(geo.split("_")[1][1]),)
    gain = 100.0 if geo.endswith("nulls") else 0.0
    A = 3
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    pcm[2] = pcm[0] * np.float32(1e-18)
    doa = nt.drifting_doa(A, F, S)
    ref_bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=gain)
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=gain)
    if S == 1:
        ref = ref_bf.process(pcm, doa[:, :, 0].copy(), want_spec=True)
        ones = bf.process(pcm, doa[:, :, 0].copy(), want_spec=True, update=np.ones((A, F), dtype=np.float32))
    else:
        ref = ref_bf.process_sources(pcm, doa)
        ones = bf.process_sources(pcm, doa, update=1.0)
    _same(ones, ref, "all ones")
    for a in range(A):
        assert np.array_equal(bf.covariance(a), ref_bf.covariance(a)), a
    # the NULL pointer through the weighted entry points, host and device
    bf.reset()
    fp = api._lib.c_fp
    out, spec = np.empty_like(ref["out"]), np.empty_like(ref["spec"])
    bf._check(bf._lib.mca_hip_mvdr_sources_frames_weighted_host(bf.h, pcm.ctypes.data_as(fp), A, F, S, doa.ctypes.data_as(fp), None,
                                                               out.ctypes.data_as(fp), spec.ctypes.data_as(fp)))
    _same(dict(out=out, spec=spec), ref, "NULL weights")
    for a in range(A):
        assert np.array_equal(bf.covariance(a), ref_bf.covariance(a)), a
    # and the weights are not ignored
    bf.reset()
    w = np.ones((A, F), dtype=np.float32)
    w[:, 2:4] = 0.5
    other = bf.process_sources(pcm, doa, update=w) if S > 1 else bf.process(pcm, doa[:, :, 0].copy(), want_spec=True, update=w)
    assert not np.array_equal(other["spec"][:2], ref["spec"][:2])
    assert np.array_equal(other["spec"][2], ref["spec"][2])            # silence: delay-and-sum whatever the weights


@pytest.mark.parametrize("M,S,gain", [(16, 1, 0.0), (11, 2, 10.0), (16, 4, 0.0)])
def test_gate_weight_zero_leaves_the_covariance(M, S, gain):
    """frames with weight 0 (and NaN, and -1) leave get_covariance bit-identical across the call and are still beamformed"""
    fs, N, F, A = 16000, 256, 5, 2
    xs = _irregular(M)
    hop = N // 2
    pcm = np.stack([nt.scene(xs, fs, N, 2 * F, a) for a in range(A)])
    doa = nt.drifting_doa(A, 2 * F, S)
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=gain)
    bf.process_sources(pcm[:, :, :(F + 1) * hop].copy(), doa[:, :F].copy())
    before = [bf.covariance(a) for a in range(A)]
    w = np.array([[0, 0, 0, 0, 0], [0, NAN, -1, 0, -0.0]], dtype=np.float32)
    r = bf.process_sources(pcm[:, :, F * hop:].copy(), doa[:, F:].copy(), update=w)
    for a in range(A):
        assert np.array_equal(bf.covariance(a), before[a]), a
    assert np.all(np.isfinite(r["spec"])) and np.abs(r["spec"]).max(axis=3).min() > 0.0
    # the frozen frames against the twin
    worst = [0.0, 0.0, 0.0]
    for a in range(A):
        lead = gt.mvdr_gate_stream(fs, N, xs, pcm[a, :, :(F + 1) * hop].astype(np.float64), doa[a, :F], gain, None)
        tw = gt.mvdr_gate_stream(fs, N, xs, pcm[a, :, F * hop:].astype(np.float64), doa[a, F:], gain, w[a], state=lead)
        _check_against_twin(r, tw, a, "frozen", worst)


def test_gate_frozen_fresh_context_is_delay_and_sum():
    """a fresh context whose every frame is frozen: tr = 0, the delay-and-sum limit tests/test_gpu_mvdr.py checks under heavy
    loading (Beamformer.cpp:51-71 as restated in the oracle), and the covariance stays zero"""
    fs, N, F = 48000, 1024, 6
    xs = synth.ULA8
    pcm = nt.scene(xs, fs, N, F, 1)
    bf = api.MvdrBeamformer(fs, xs, N)
    r = bf.process(pcm, 0.4, want_spec=True, update=0.0)
    X = po.stft_frames(pcm.astype(np.float64), N)
    for t in range(F):
        ref = po.beamformer_process_frame(fs, xs, X[t], float(np.float32(0.4)))
        refc = ref[0::2] + 1j * ref[1::2]
        assert np.abs(r["spec"][0, t] - refc).max() <= 2e-5 * np.abs(refc).max(), t
    assert not bf.covariance(0).any()


@pytest.mark.parametrize("M,S,gain", [(16, 1, 0.0), (16, 2, 0.0), (12, 3, 0.0), (8, 4, 10.0), (16, 3, 10.0), (5, 1, 0.0)])
def test_gate_cut_invariance(M, S, gain):
    """12 frames in one call, as 5 + 7 and as 12 calls of one frame, with a frozen run across every cut: the same bytes.  A frozen
    frame that follows a solved frame of its launch reuses the factor (where the instantiation does), the first frame of a call
    factorises: the two agree bit for bit."""
    fs, N, F, A = 16000, 256, 12, 2
    xs = _irregular(M)
    hop = N // 2
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    doa = nt.drifting_doa(A, F, S)
    w = np.array([[1, .5, 1, 0, 0, 0, 0, 1, 0, 0, .25, 0], [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.float32)
    one_bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=gain)
    one = one_bf.process_sources(pcm, doa, update=w)
    for cuts in ([0, 5, 12], list(range(13))):
        bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=gain)
        rs = [bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy(), update=w[:, t0:t1])
              for t0, t1 in zip(cuts[:-1], cuts[1:])]
        _same(_cat(rs, 2), one, "%d calls" % (len(cuts) - 1))
        for a in range(A):
            assert np.array_equal(bf.covariance(a), one_bf.covariance(a)), a
        bf.close()


def test_gate_pieced_tail_launch():
    """256 streams x 129 bins = 516 solve workgroups: the 4 behind the last whole round go in a second launch cut along the frames
    into 4 pieces (api_mvdr.hip); two calls of 8 frames cut theirs into 2.  The frames before a piece's own run the same weighted
    recursion, so pieces give the bits of an unsplit launch."""
    fs, N, F, A, M = 16000, 256, 16, 256, 4
    xs = _irregular(M)
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
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A)
    one = bf.process(pcm, doa, want_spec=True, update=w)
    worst = [0.0, 0.0, 0.0]
    for a in (0, 255):
        tw = gt.mvdr_gate_stream(fs, N, xs, pcm[a].astype(np.float64), doa[a], 0.0, w[a])
        _check_against_twin(dict(spec=one["spec"][:, None], out=one["out"][:, None]), tw, a, "256 streams", worst)
        _check_covariance(bf, tw, a, "256 streams", worst)
    # the same input and weights give the same bytes wherever the stream sits (stream 3: the main launch)
    assert np.array_equal(one["spec"][0], one["spec"][3]) and np.array_equal(bf.covariance(0), bf.covariance(3))
    two_bf = api.MvdrBeamformer(fs, xs, N, max_streams=A)
    r1 = two_bf.process(pcm[:, :, :(8 + 1) * hop].copy(), doa[:, :8].copy(), want_spec=True, update=w[:, :8])
    r2 = two_bf.process(pcm[:, :, 8 * hop:].copy(), doa[:, 8:].copy(), want_spec=True, update=w[:, 8:])
    _same(_cat([r1, r2], 1), one, "two calls of 8 frames")
    for a in (0, 1, 2, 254, 255):
        assert np.array_equal(two_bf.covariance(a), bf.covariance(a)), a


def test_gate_noise_only_covariance_keeps_the_target():
    """the self-cancellation scene of tests/test_mvdr_gate_twin.py on the GPU: frozen from the target's onset on, the last 12
    frames carry at least 4 times the power of the all-ones run"""
    xs, pcm, update = gt.cancellation_scene()
    bf = api.MvdrBeamformer(gt.CANCEL_FS, xs, gt.CANCEL_N)
    ones = bf.process(pcm, gt.CANCEL_LOOK, want_spec=True, update=np.ones_like(update))
    bf.reset()
    gated = bf.process(pcm, gt.CANCEL_LOOK, want_spec=True, update=update)
    p1, pg = gt.last_frames_power(ones["spec"][0]), gt.last_frames_power(gated["spec"][0])
    print("last 12 frames: all ones %.1f, frozen from the onset %.1f: %.1f times" % (p1, pg, pg / p1))
    assert pg >= 4.0 * p1


@pytest.mark.parametrize("S,gain", [(1, 0.0), (3, 100.0)])
def test_gate_dev_entry_under_a_padded_offset_stride(S, gain):
    """the _dev entry with PCM at padded, offset strides in a poisoned allocation equals the contiguous call bit for bit"""
    import torch
    from dev_layout_helpers import guarded, strided_pcm
    fs, N, F, A = 48000, 1024, 6, 2
    xs = synth.ULA8
    hop, K = N // 2, N // 2 + 1
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    doa = nt.drifting_doa(A, F, S)
    w = W12[:, 3:3 + F].copy()
    ref_bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=gain)
    ref = ref_bf.process_sources(pcm, doa, update=w)
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=gain)
    view, whole = strided_pcm(pcm)
    t_doa, t_w = torch.from_numpy(doa).cuda(), torch.from_numpy(w).cuda()
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
    with pytest.raises(api.MCArrayHipError, match="update"):
        bf.process_sources_dev(view, F, t_doa, out_pcm=g_out.t, update=t_w[:, :F - 1])


def test_gate_refusals_leave_the_state():
    fs, N, F, A = 16000, 256, 4, 2
    xs = synth.REEM_C
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    w = np.ones((A, F), dtype=np.float32)
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=2)
    bf.process_sources(pcm, nt.drifting_doa(A, F, 2), update=w)
    before, blob = [bf.covariance(a) for a in range(A)], bf.state_save()
    with pytest.raises(api.MCArrayHipError, match="n_sources"):
        bf.process_sources(pcm, nt.drifting_doa(A, F, 3), update=w)          # above the context's maximum
    with pytest.raises(api.MCArrayHipError, match="both NULL"):
        bf.process_sources(pcm, nt.drifting_doa(A, F, 2), want_audio=False, want_spec=False, update=w)
    with pytest.raises(api.MCArrayHipError, match="update"):
        bf.process_sources(pcm, nt.drifting_doa(A, F, 2), update=np.ones((A, F + 1), dtype=np.float32))
    for a in range(A):
        assert np.array_equal(bf.covariance(a), before[a]), a
    assert bf.state_save() == blob


def test_gate_results_do_not_move_beside_a_matrix_core_neighbour():
    """the weighted solve kernel beside the neighbour of tests/test_gpu_coresidency.py (the procedure of its module test): 16
    microphones, the instantiation that reuses the factor, weights with frozen runs"""
    import ctypes as C
    import time
    import torch
    import test_gpu_coresidency as tc
    nb = tc._neighbour()
    dev = torch.device("cuda:0")
    F, A, N, xs = 60, 16, 1024, synth.ULA16
    pcm = np.stack([synth.noise_source_stream(xs, np.deg2rad(20.0 - 7 * a), 48000, (F + 1) * N // 2, 80 + a) for a in range(A)]).astype(np.float32)
    doa = (np.deg2rad(20.0 - 7 * np.arange(A))[:, None] + 0.01 * np.arange(F)[None, :]).astype(np.float32)
    w = np.tile(W12[0], (A, F // 12))

    def fn():
        bf = api.MvdrBeamformer(48000, xs, N, max_streams=A)
        r = bf.process(pcm, doa, want_spec=True, update=w)
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
