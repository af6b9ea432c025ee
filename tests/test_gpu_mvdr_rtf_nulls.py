"""GPU: soft nulls at estimated steering vectors (mca_hip_mvdr_set_rtf_nulls; k_mvdr_solve_rtf_nulls_t of mvdr_solve.h behind
k_mvdr_rtf) against the float64 twin of the definition (tests/mvdr_rtf_nulls_twin.py), and the identities of DESIGN.md 4.10.

Bars: the module's 5e-6 for the covariances; for spectra and audio the module's 5e-4 of the peak at g = 10, and at g = 1000 (the cap
of the gain) four times what the float32 estimator alone costs the twin in that case (mvdr_rtf_nulls_twin.GAIN_CAP_FIGURES, measured
by tests/test_mvdr_rtf_nulls_twin.py), never below 5e-4.  A null uses every slot's vector, so a cell is left out of the spectra if
any slot of it sits at a decision edge of the twin or is decided differently by the float32 and the float64 estimator; at most 3 %
of a case's cells.  The audio is compared whole, against the twin's synthesis of its spectra in which only those cells carry the
GPU's values.  Every test prints its worst case.  On an MI355X the parity cases stay under 3.36e-4 (spectra) and 1.27e-4 (audio) of
the peak at g = 10 and, at g = 1000, between 2.10e-4 (M = 2, S = 2; bar 6.0e-4) and 2.28e-2 (M = 13, S = 4; bar 4.4e-2), each at 10 to 83 % of
its bar; covariances 4.03e-7; at most 1.52 % of a case's cells left out.  The scene meets the twin at 1.75e-5 and its held state gives
0.994 / 0.995 of the own talker with the other 14.03 / 13.77 dB down, the twin's figures for that state."""
import functools

import numpy as np
import pytest

from mcarray_amd import api, synth
from oracle import np_twin

import mvdr_estmask_twin as et
import mvdr_mask_twin as mt
import mvdr_nulls_twin as nt
import mvdr_postfilter_twin as pt
import mvdr_rtf_nulls_twin as xt
import mvdr_rtf_twin as rt

pytestmark = pytest.mark.gpu

COV_TOL = 5e-6
F6 = rt.PARITY_F
_irregular = pt.irregular
K_SLOTS = (api.MvdrBeamformer.K_ANALYSE, api.MvdrBeamformer.K_SOLVE, api.MvdrBeamformer.K_SYNTH, api.MvdrBeamformer.K_RTF)


def _same(r, q, what=""):
    assert np.array_equal(r["spec"].view(np.float32), q["spec"].view(np.float32), equal_nan=True), what
    assert np.array_equal(r["out"], q["out"], equal_nan=True), what


def _cat(rs, axis=2):
    return dict(spec=np.concatenate([r["spec"] for r in rs], axis=axis), out=np.concatenate([r["out"] for r in rs], axis=axis))


def _bf(fs, xs, N, A, S, gain, cfg=None, pf=None, rtf=True, nulls=True, est=None):
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=gain, rtf_nulls=nulls)
    if pf is not None:
        bf.set_postfilter(True, **pf)
    if rtf:
        bf.set_rtf(True, **(cfg or {}))
    if est is not None:
        bf.set_mask_estimator(True, **est)
    return bf


def _state(bf, A, S):
    return [bf.covariance(a) for a in range(A)] + [x for a in range(A) for s in range(S) for x in bf.target_covariance(a, s)]


def _timing(bf):
    return [bf.get_timing(k)[0] for k in K_SLOTS]


# ---- 1. parity with the twin ----
@functools.lru_cache(maxsize=None)
def _twins(run, gain):
    M, fs, N, S, pf = run
    xs, pfc = xt.parity_xs(M), pt.PARITY_PF if pf else None
    return xt.parity_twin(xs, fs, N, S, gain, pfc), xt.parity_twin(xs, fs, N, S, gain, pfc, est_dtype=np.float32)


def _check_call(r, tw, lo, a, what, bar, tail, pf):
    """stream a of the GPU result r ([A][S][...]) against the twin's run tw; lo [F][K]: the cells left out of the spectra.  The
    audio whole, against the twin's synthesis of its spectra in which only those cells carry the GPU's values (tail [S][hop]: the
    carry of that synthesis from the call before); returns (the carry for the next call, worst spectra, worst audio)"""
    S, F, K = tw["spec"].shape
    N = 2 * (K - 1)
    hop = N // 2
    ks, ka = ("raw", "raw_out") if pf else ("spec", "out")
    patched = np.where(lo[None], r["spec"][a].astype(np.complex128), tw["spec"])
    ref = np.zeros((S, F * hop))
    for t in range(F):
        y = np_twin.irfft_ccs(patched[:, t], N)
        ref[:, t * hop:(t + 1) * hop] = tail + y[:, :hop]
        tail = y[:, hop:]
    ws = wa = 0.0
    for s in range(S):
        assert np.all(np.isfinite(r["spec"][a, s])) and np.all(np.isfinite(r["out"][a, s])), (what, a, s)
        es = (np.abs(r["spec"][a, s] - tw["spec"][s]) * ~lo).max() / np.abs(tw[ks][s]).max()
        ea = np.abs(r["out"][a, s] - ref[s]).max() / np.abs(tw[ka][s]).max()
        print("%s stream %d source %d: spectra %.2e audio %.2e of the peak (bar %.2e); %d of %d cells (%.2f %%) left out"
              % (what, a, s, es, ea, bar, int(lo.sum()), lo.size, 100.0 * lo.mean()))
        ws, wa = max(ws, es), max(wa, ea)
        assert es <= bar and ea <= bar, (what, a, s, es, ea, bar)
    return tail, ws, wa


def _parity(run, gain, bar):
    import test_gpu_mvdr_rtf as tr
    M, fs, N, S, pf = run
    xs = xt.parity_xs(M)
    cfg = rt.parity_config(len(xs))
    t64, t32 = _twins(run, gain)
    pcm, doa, upd, tmask = rt.parity_inputs(xs, fs, N, S)
    A, hop = pcm.shape[0], N // 2
    bf = _bf(fs, xs, N, A, S, gain, cfg, pt.PARITY_PF if pf else None)
    assert bf.get_rtf_nulls() is True and bf.get_null_gain() == gain
    prev = [np.zeros((S, hop)) for _ in range(A)]
    what = "M %s N %d S %d g %g%s" % (M, N, S, gain, " post-filter" if pf else "")
    ws = wa = 0.0
    n_out = n_all = 0
    worst = [0.0, 0.0, 0.0, 0.0]
    for i, (t0, t1) in enumerate([(0, F6), (F6, 2 * F6)]):
        r = bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy(), update_mask=upd[:, t0:t1], target_mask=tmask[:, :, t0:t1])
        assert r["out"].shape == (A, S, F6 * hop) and r["spec"].shape == (A, S, F6, N // 2 + 1)
        for a in range(A):
            lo = xt.left_out(t64[a][i], t32[a][i])
            n_out, n_all = n_out + int(lo.sum()), n_all + lo.size
            prev[a], es, ea = _check_call(r, t64[a][i], lo, a, "%s call %d" % (what, i), bar, prev[a], pf)
            ws, wa = max(ws, es), max(wa, ea)
            # the state does not see the gain: covariances and held steering vectors against the twin's, as in the RTF module
            tr._check_state(bf, t64[a][i], a, "%s call %d" % (what, i), worst, fs, N, xs, doa[a, t1 - 1], cfg)
            assert t64[a][i]["est"].any() and not t64[a][i]["est"].all()
    bf.close()
    print("%s: worst spectra %.2e audio %.2e (bar %.2e) covariances %.2e; %.2f %% of the cells left out" % (what, ws, wa, bar, worst[2], 100.0 * n_out / n_all))
    assert worst[2] <= COV_TOL
    assert n_out <= xt.EDGE_CAP * n_all, (what, n_out, n_all)


_IDS = ["M%s_N%d_S%d%s" % (r[0], r[2], r[3], "_pf" if r[4] else "") for r in xt.PARITY_RUNS]


@pytest.mark.parametrize("run", xt.PARITY_RUNS, ids=_IDS)
def test_rtf_nulls_parity(run):
    """g = 10: every number of row slots, M = 4Q through the `j < M` form, the two-pass row, more directions than microphones; the
    post-filter; N = 1024.  The module's bar."""
    _parity(run, xt.PARITY_GAIN, xt.SPEC_TOL)


@pytest.mark.parametrize("run", xt.PARITY_RUNS, ids=_IDS)
def test_rtf_nulls_parity_at_the_cap_of_the_gain(run):
    """g = 1000: the float32 estimator's own error is amplified; the bar is four times what it costs the twin"""
    _parity(run, xt.PARITY_GAIN_CAP, xt.gain_cap_bar(run))


# ---- 2. the geometric plane ----
@pytest.mark.parametrize("pf", [None, "postfilter"])
@pytest.mark.parametrize("gain", [10.0, 1000.0])
@pytest.mark.parametrize("M,S", [(11, 2), (13, 4), (16, 3)])
def test_rtf_nulls_without_a_target_mask_are_the_masked_call_under_the_same_gain(M, S, gain, pf):
    """fresh RTF state, target mask NULL: every d is cmul(T_hi, T_lo), and spectra, audio and covariance over two calls have the bytes
    of mca_hip_mvdr_sources_frames_masked_* under the same update mask and the same gain"""
    fs, N, A = 16000, 256, 2
    xs = _irregular(M)
    hop, K = N // 2, N // 2 + 1
    pcm, doa, upd, _ = rt.parity_inputs(xs, fs, N, S)
    pfc = pt.PARITY_PF if pf else None
    fp = api._lib.c_fp

    def run(masked):
        bf = _bf(fs, xs, N, A, S, gain, None, pfc, rtf=not masked, nulls=not masked)
        rs = []
        for t0, t1 in ((0, F6), (F6, 2 * F6)):
            x, dd, u = pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy(), np.ascontiguousarray(upd[:, t0:t1])
            if masked:
                rs.append(bf.process_sources(x, dd, update_mask=u))
            else:
                out, spec = np.empty((A, S, F6 * hop), dtype=np.float32), np.empty((A, S, F6, K), dtype=np.complex64)
                bf._check(bf._lib.mca_hip_mvdr_sources_frames_rtf_host(bf.h, x.ctypes.data_as(fp), A, F6, S, dd.ctypes.data_as(fp), u.ctypes.data_as(fp),
                                                                      None, out.ctypes.data_as(fp), spec.ctypes.data_as(fp)))
                rs.append(dict(out=out, spec=spec))
        res = _cat(rs), [bf.covariance(a) for a in range(A)]
        bf.close()
        return res

    ref, got = run(True), run(False)
    _same(got[0], ref[0])
    assert all(np.array_equal(p, q) for p, q in zip(got[1], ref[1]))


# ---- 3. the switch and the degenerate gains ----
def test_rtf_nulls_switch_and_degenerate_gains():
    fs, N, A, S, M = 16000, 256, 2, 2, 7
    xs = _irregular(M)
    pcm, doa, upd, tmask = rt.parity_inputs(xs, fs, N, S)
    cfg = rt.parity_config(M)

    def run(gain, nulls, S_=S, before=None):
        bf = _bf(fs, xs, N, A, S, gain, cfg, nulls=nulls)
        assert bf.get_rtf_nulls() is nulls
        if before:
            before(bf)
        bf.set_timing(True)
        r = bf.process_sources(pcm, doa[:, :, :S_].copy(), update_mask=upd, target_mask=tmask[:, :S_].copy())
        res = r, bf.state_save(), _timing(bf)
        bf.close()
        return res

    plain = run(0.0, False)
    # switch 0 and g = 10: refused with -4, the state blob untouched; the switch may be set before RTF is enabled and toggled
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S)
    assert bf.get_rtf_nulls() is False
    bf.set_rtf_nulls(True)
    bf.set_rtf_nulls(False)
    for bad in (2, -1, 256):
        assert bf._lib.mca_hip_mvdr_set_rtf_nulls(bf.h, bad) == -1
        assert b"0 or 1" in bf._lib.mca_hip_mvdr_last_error(bf.h)
    assert bf.get_rtf_nulls() is False
    bf.set_rtf(True, **cfg)
    bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask)
    blob = bf.state_save()
    bf.set_null_gain(10.0)
    fp = api._lib.c_fp
    out = np.empty((A, S, 2 * F6 * (N // 2)), dtype=np.float32)
    rc = bf._lib.mca_hip_mvdr_sources_frames_rtf_host(bf.h, pcm.ctypes.data_as(fp), A, 2 * F6, S, doa.ctypes.data_as(fp), upd.ctypes.data_as(fp),
                                                      tmask.ctypes.data_as(fp), out.ctypes.data_as(fp), None)
    assert rc == -4 and bf._lib.mca_hip_mvdr_last_error(bf.h).startswith(b"nulls at estimated steering vectors are not built")
    assert b"mca_hip_mvdr_set_rtf_nulls" in bf._lib.mca_hip_mvdr_last_error(bf.h)
    assert bf.state_save() == blob
    assert bf.get_rtf() == dict(enable=True, **cfg)                         # the switch is no part of it
    # ... and switched on, the same context runs the call (a processing parameter: it may change between calls)
    bf.set_rtf_nulls(True)
    moved = bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask)
    assert np.all(np.isfinite(moved["out"]))
    bf.close()
    # switch 1 and g = 0, or a gain that rounds to 0 in fp32: the bytes and the launches of today's RTF call
    for gain in (0.0, 1e-60):
        armed = run(gain, True)
        _same(armed[0], plain[0], gain)
        assert armed[1] == plain[1] and armed[2] == plain[2], gain
    # switch 1, g = 10 and one look direction: the bytes and the launches of g = 0
    one0, one10 = run(0.0, True, 1), run(10.0, True, 1)
    _same(one10[0], one0[0])
    assert one10[1] == one0[1] and one10[2] == one0[2]
    # with two directions the gain moves the outputs and nothing of the launches' count
    nulled = run(10.0, True)
    assert not np.array_equal(nulled[0]["spec"], plain[0]["spec"]) and nulled[2] == plain[2]


# ---- 4. the gain does not enter the state ----
@pytest.mark.parametrize("M,S", [(5, 2), (16, 4)])
def test_rtf_nulls_gain_does_not_enter_the_state(M, S):
    """the same stream at g = 0 and g = 100, post-filter off: the outputs differ, the state blobs are equal.  The calls ask for the
    spectra alone: the overlap-add tails of the audio are stream state that follows the output, like the post-filter's A; with
    audio, covariance() and target_covariance() are equal all the same"""
    fs, N, A = 16000, 256, 2
    xs = _irregular(M)
    hop, K = N // 2, N // 2 + 1
    pcm, doa, upd, tmask = rt.parity_inputs(xs, fs, N, S)
    fp = api._lib.c_fp
    res = []
    for gain in (0.0, 100.0):
        bf = _bf(fs, xs, N, A, S, gain, rt.parity_config(M))
        specs = []
        for t0, t1 in ((0, F6), (F6, 2 * F6)):
            x, dd = pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy()
            u, tm = np.ascontiguousarray(upd[:, t0:t1]), np.ascontiguousarray(tmask[:, :, t0:t1])
            spec = np.empty((A, S, F6, K), dtype=np.complex64)
            bf._check(bf._lib.mca_hip_mvdr_sources_frames_rtf_host(bf.h, x.ctypes.data_as(fp), A, F6, S, dd.ctypes.data_as(fp), u.ctypes.data_as(fp),
                                                                  tm.ctypes.data_as(fp), None, spec.ctypes.data_as(fp)))
            specs.append(spec)
        blob = bf.state_save()
        bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask)       # with audio: the tails move with the output
        res.append((np.concatenate(specs, axis=2), blob, _state(bf, A, S), bf.state_save()))
        bf.close()
    assert res[0][1] == res[1][1]
    assert all(np.array_equal(u, v) for u, v in zip(res[0][2], res[1][2]))
    assert res[0][3] != res[1][3]
    for s in range(S):
        assert not np.array_equal(res[0][0][:, s], res[1][0][:, s]), s


# ---- 5. cuts and placement change no byte ----
@pytest.mark.parametrize("M,S,pf", [(12, 3, None), (16, 4, None), (8, 2, "pf")])
def test_rtf_nulls_cut_invariance(M, S, pf):
    """12 frames in one call, as 6 + 6 and as 12 calls of one frame: the same bytes, the state blob included"""
    fs, N, A, gain = 16000, 256, 2, 100.0
    xs = _irregular(M)
    hop = N // 2
    pcm, doa, upd, tmask = rt.parity_inputs(xs, fs, N, S)
    cfg, pfc = rt.parity_config(M), pt.PARITY_PF if pf else None
    one_bf = _bf(fs, xs, N, A, S, gain, cfg, pfc)
    one = one_bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask)
    blob = one_bf.state_save()
    for cuts in ([0, 6, 12], list(range(13))):
        bf = _bf(fs, xs, N, A, S, gain, cfg, pfc)
        rs = [bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy(), update_mask=upd[:, t0:t1], target_mask=tmask[:, :, t0:t1])
              for t0, t1 in zip(cuts[:-1], cuts[1:])]
        _same(_cat(rs), one, "%d calls" % (len(cuts) - 1))
        assert bf.state_save() == blob, "%d calls" % (len(cuts) - 1)
        bf.close()
    one_bf.close()


@pytest.mark.parametrize("M,S,cap_kb,launches", [(8, 2, 100, 4), (13, 4, 250, 6)])
def test_rtf_nulls_plane_above_the_workspace_cap(M, S, cap_kb, launches):
    """a workspace cap that cuts the call into at least three chunks of frames: the bytes of the uncut call.  12 frames of 2 streams x
    S look directions x 129 bins x M microphones x 8 bytes: 33 KB a frame at (8, 2) -- 100 KB takes 3 frames; 107 KB at (13, 4) --
    250 KB takes 2"""
    fs, N, A, gain = 16000, 256, 2, 100.0
    xs = _irregular(M)
    pcm, doa, upd, tmask = rt.parity_inputs(xs, fs, N, S)
    res = []
    for kb in (None, cap_kb):
        bf = _bf(fs, xs, N, A, S, gain, rt.parity_config(M), pt.PARITY_PF)
        if kb is not None:
            bf.set_rtf_workspace(kb * 1024)
        bf.set_timing(True)
        r = bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask)
        res.append((r, bf.state_save(), bf.get_timing(api.MvdrBeamformer.K_RTF)[0], bf.get_timing(api.MvdrBeamformer.K_SOLVE)[0]))
        bf.close()
    _same(res[1][0], res[0][0], "cut along the frames")
    assert res[1][1] == res[0][1]
    assert res[0][2:] == (1, 1) and res[1][2] == res[1][3] == launches and launches >= 3


@pytest.mark.parametrize("M,S", [(5, 3), (16, 4)])
def test_rtf_nulls_pieced_tail_launch_and_placement(M, S):
    """128 streams x 257 bins = 514 solve workgroups, 19 frames: the 2 workgroups behind the 512 resident ones go in a tail launch
    cut into 4 pieces along the frames (the sizes of tests/test_gpu_launch_geometry.py for the nulls kernel; (16, 4): the two-pass
    instantiation inside a pieced launch).  Every copy of a scene -- the last stream lies in the tail launch -- has the bits of its first
    copy, and those are the bits of the three scenes alone in a batch of three, which takes no tail launch; the state likewise."""
    import test_gpu_launch_geometry as tg
    fs, N, F, A, gain = tg.FS, tg.N, 19, 128, 100.0
    K = N // 2 + 1
    assert tg._mvdr_shapes(A, F, S)[2] == 4 and tg._mvdr_shapes(3, F, S)[2] == 1
    xs = _irregular(M)
    pcm3 = np.stack([nt.scene(xs, fs, N, F, a) for a in range(3)])
    doa3 = nt.drifting_doa(3, F, S)
    rng = np.random.default_rng(19)
    upd3 = rng.choice(np.array([0, 0, 1, 1, .5, .125], dtype=np.float32), size=(3, F, K))
    tm3 = rng.choice(np.array([0, 0, 1, 1, .5, .125], dtype=np.float32), size=(3, S, F, K))
    pick = np.arange(A) % 3
    cfg = rt.parity_config(M)
    small = _bf(fs, xs, N, 3, S, gain, cfg)
    ref = small.process_sources(pcm3, doa3, update_mask=upd3, target_mask=tm3)
    ref_state = _state(small, 3, S)
    small.close()
    bf = _bf(fs, xs, N, A, S, gain, cfg)
    r = bf.process_sources(pcm3[pick], doa3[pick], update_mask=upd3[pick], target_mask=tm3[pick])
    assert np.isfinite(r["out"]).all()
    for a in range(A):
        b = pick[a]
        assert r["spec"][a].tobytes() == ref["spec"][b].tobytes(), ("spectra", a)
        assert r["out"][a].tobytes() == ref["out"][b].tobytes(), ("audio", a)
    for a in (0, 1, 2, 64, 125, 126, 127):
        b = pick[a]
        assert np.array_equal(bf.covariance(a), ref_state[b]), ("covariance", a)
        for s in range(S):
            psi, cpsi = bf.target_covariance(a, s)
            assert np.array_equal(psi, ref_state[3 + 2 * (b * S + s)]) and np.array_equal(cpsi, ref_state[3 + 2 * (b * S + s) + 1]), (a, s)
    bf.close()


# ---- 6. the auto call ----
@pytest.mark.parametrize("M,S,P,pf", [(8, 2, 0, None), (13, 3, 2, None), (8, 2, 0, "pf")])
def test_auto_call_under_nulls_is_the_rtf_call_fed_its_masks(M, S, P, pf):
    """RTF, the estimator and the switch enabled: the auto call and the RTF call on a twin context fed the masks the auto call
    returned give the same bytes and the same state over two calls.  S = 2 both protected; S = 3 with one competitor"""
    fs, N, A, gain = 16000, 256, 2, 100.0
    xs = et.parity_xs(M)
    pcm, doa = et.parity_inputs(xs, fs, N, S)
    hop = N // 2
    est, rcfg, pfc = et.parity_config(N, S, P), dict(target_alpha=0.9, iterations=2, ref_mic=1, min_share=0.05), pt.PARITY_PF if pf else None
    auto, fed, plain = _bf(fs, xs, N, A, S, gain, rcfg, pfc, est=est), _bf(fs, xs, N, A, S, gain, rcfg, pfc), _bf(fs, xs, N, A, S, 0.0, rcfg, pfc, est=est)
    for t0, t1 in ((0, F6), (F6, 2 * F6)):
        x, dd = pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy()
        r = auto.process_sources(x, dd, estimate_masks=True)
        q = fed.process_sources(x, dd, update_mask=r["update_mask"], target_mask=r["target_mask"])
        p = plain.process_sources(x, dd, estimate_masks=True)
        _same(r, q, (t0, t1))
        assert np.array_equal(r["update_mask"], p["update_mask"]) and np.array_equal(r["target_mask"], p["target_mask"])     # the masks do not see the gain
        assert not np.array_equal(r["spec"], p["spec"])
        assert all(np.array_equal(u, v) for u, v in zip(_state(auto, A, S), _state(fed, A, S)))
    assert auto.state_save() == fed.state_save()
    # switched off, the auto call of an RTF context refuses the gain as before
    auto.set_rtf_nulls(False)
    with pytest.raises(api.MCArrayHipError, match="nulls at estimated"):
        auto.process_sources(pcm, doa, estimate_masks=True)
    for b in (auto, fed, plain):
        b.close()


# ---- 7. column independence ----
@pytest.mark.parametrize("M,S,pf", [(11, 3, None), (16, 4, None), (8, 2, "pf")])
@pytest.mark.parametrize("agree", ["every_other_bin", "bins_0_63"])
def test_rtf_nulls_column_independence(agree, M, S, pf):
    """two pairs of masks that agree on a set of bins and differ at random elsewhere: the bytes of the agreeing bins are equal"""
    fs, N, A, gain = 16000, 256, 2, 100.0
    xs = _irregular(M)
    K = N // 2 + 1
    pcm, doa, u1, t1 = rt.parity_inputs(xs, fs, N, S)
    keep = (np.arange(K) % 2 == 0) if agree == "every_other_bin" else (np.arange(K) < 64)
    rng = np.random.default_rng(3)
    u2 = rng.choice(np.array([0, 0, 1, .5], dtype=np.float32), size=u1.shape)
    t2 = rng.choice(np.array([0, 0, 1, .5], dtype=np.float32), size=t1.shape)
    u2[..., keep], t2[..., keep] = u1[..., keep], t1[..., keep]
    res = []
    for u, t in ((u1, t1), (u2, t2)):
        bf = _bf(fs, xs, N, A, S, gain, rt.parity_config(M), pt.PARITY_PF if pf else None)
        r = bf.process_sources(pcm, doa, update_mask=u, target_mask=t)
        res.append((r, [bf.covariance(a) for a in range(A)]))
        bf.close()
    (r1, c1), (r2, c2) = res
    assert np.array_equal(np.ascontiguousarray(r1["spec"][..., keep]).view(np.float32), np.ascontiguousarray(r2["spec"][..., keep]).view(np.float32))
    assert not np.array_equal(r1["spec"][..., ~keep], r2["spec"][..., ~keep])
    for a in range(A):
        assert np.array_equal(c1[a][keep], c2[a][keep]) and not np.array_equal(c1[a][~keep], c2[a][~keep])


# ---- 8. the device entry ----
def test_rtf_nulls_dev_entry_under_a_padded_offset_stride():
    """the _dev entry with PCM at padded, offset strides in a poisoned allocation equals the contiguous call bit for bit"""
    import torch
    from dev_layout_helpers import guarded, strided_pcm
    fs, N, A, S, gain = 48000, 1024, 2, 3, 100.0
    xs = synth.ULA8
    F, hop, K = F6, N // 2, N // 2 + 1
    pcm, doa, upd, tmask = rt.parity_inputs(xs, fs, N, S)
    pcm, doa, upd, tmask = pcm[:, :, :(F + 1) * hop].copy(), doa[:, :F].copy(), np.ascontiguousarray(upd[:, :F]), np.ascontiguousarray(tmask[:, :, :F])
    cfg = rt.parity_config(len(xs))
    ref_bf = _bf(fs, xs, N, A, S, gain, cfg)
    ref = ref_bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask)
    plain_bf = _bf(fs, xs, N, A, S, 0.0, cfg)
    assert not np.array_equal(plain_bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask)["spec"], ref["spec"])
    bf = _bf(fs, xs, N, A, S, gain, cfg)
    view, whole = strided_pcm(pcm)
    t_doa, t_u, t_m = torch.from_numpy(doa).cuda(), torch.from_numpy(upd).cuda(), torch.from_numpy(tmask).cuda()
    g_out, g_spec = guarded((A, S, F * hop), torch.float32), guarded((A, S, F, K, 2), torch.float32)
    bf.process_sources_dev(view, F, t_doa, out_pcm=g_out.t, out_spec=g_spec.t, update_mask=t_u, target_mask=t_m)
    torch.cuda.synchronize()
    g_out.assert_guards_intact("out"); g_spec.assert_guards_intact("spec")
    spec = g_spec.t.cpu().numpy()
    assert np.array_equal(spec.reshape(ref["spec"].shape + (2,)), ref["spec"].view(np.float32).reshape(ref["spec"].shape + (2,)))
    assert np.array_equal(g_out.t.cpu().numpy(), ref["out"])
    assert bf.state_save() == ref_bf.state_save()
    for b in (bf, ref_bf, plain_bf):
        b.close()


# ---- 9. the scene ----
def _frozen_figures(phi, d, g0, sc, gain, loading=1e-3):
    """the scene's figures with the weights of the held state: phi [K][M][M], d, g0 [K][S][M]"""
    K, S, M = d.shape
    tr = np.real(np.trace(phi, axis1=1, axis2=2))
    live = tr > 1e-30
    PL = np.where(live[:, None, None], phi + (loading * tr / M)[:, None, None] * np.eye(M), np.eye(M))
    w = nt.null_weights(PL, d, gain)
    w[~live] = g0[~live] / M
    return xt.scene_figures(np.broadcast_to(np.swapaxes(w, 0, 1), (xt.SCENE_LAST, S, K, M)), sc)


def test_rtf_nulls_scene():
    """two_talker_scene() from the mixture at g = 100: the GPU run meets the twin at the parity bar, which carries the twin's figures
    over (own talker 0.957 / 0.968, other talker 13.7 / 14.1 dB down).  Printed beside them, and held to the scene's bars (share
    within [0.85, 1.15], the other talker at least the twin's figure for that state less 3 dB): the figures of the weights formed on
    the host from the GPU's held covariance() and steering() after the last frame."""
    import test_gpu_mvdr_rtf as tr
    sc = xt.two_talker_scene()
    fs, N, gain = xt.SCENE_FS, xt.SCENE_N, xt.SCENE_GAIN
    doa = sc["doa"][None]
    bf = _bf(fs, sc["xs"], N, 1, 2, gain)
    r = bf.process_sources(sc["pcm"][None], doa, update_mask=sc["update"][None], target_mask=sc["tmask"][None])
    t64, t32 = xt.scene_twin(sc), xt.scene_twin(sc, np.float32)
    lo = xt.left_out(t64, t32)
    assert lo.sum() <= xt.EDGE_CAP * lo.size
    _check_call(r, t64, lo, 0, "scene", xt.scene_bar(), np.zeros((2, N // 2)), None)
    worst = [0.0, 0.0, 0.0, 0.0]
    tr._check_state(bf, t64, 0, "scene", worst, fs, N, sc["xs"], doa[0, -1], dict(rt.DEFAULTS))
    g0 = nt.steering(fs, N, sc["xs"], xt.SCENE_LOOKS)
    steer = [bf.steering(float(doa[0, -1, s]), 0, s) for s in range(2)]
    gd = np.stack([d for d, _ in steer], axis=1)
    f_gpu = _frozen_figures(bf.covariance(0), gd, g0, sc, gain)
    f_twin = _frozen_figures(t64["phi"], np.swapaxes(t64["d"][-1], 0, 1), g0, sc, gain)
    f_run = xt.scene_figures(t64["w"], sc)
    b = xt.SCENE_BARS
    for s in range(2):
        print("scene out %d: twin, frame by frame: share %.3f, other %.2f dB, background %.2f dB; held state, twin: %.3f, %.2f dB, %.2f dB; held state, GPU: %.3f, %.2f dB, %.2f dB; %d of %d cells estimated"
              % ((s,) + tuple(f_run[s]) + tuple(f_twin[s]) + tuple(f_gpu[s]) + (int(steer[s][1].sum()), steer[s][1].size)))
        assert b["share_lo"] <= f_gpu[s][0] <= b["share_hi"], s
        assert f_gpu[s][1] >= f_twin[s][1] - b["gpu_margin_db"], s
    bf.close()


# ---- 10. beside a matrix-core neighbour ----
def test_rtf_nulls_results_do_not_move_beside_a_matrix_core_neighbour():
    """k_mvdr_rtf and the nulls solve behind it beside the neighbour of tests/test_gpu_coresidency.py (the procedure of its module
    test, as tests/test_gpu_mvdr_rtf.py runs it): 16 microphones, two look directions, masks whose quads diverge"""
    import ctypes as C
    import time
    import torch
    import test_gpu_coresidency as tc
    nb = tc._neighbour()
    dev = torch.device("cuda:0")
    F, A, N, S, xs = 24, 16, 1024, 2, synth.ULA16
    K = N // 2 + 1
    pcm = np.stack([synth.noise_source_stream(xs, np.deg2rad(20.0 - 7 * a), 48000, (F + 1) * N // 2, 80 + a) for a in range(A)]).astype(np.float32)
    doa = np.ascontiguousarray(nt.drifting_doa(A, F, S))
    upd = np.ascontiguousarray(np.tile(mt.mask_for(K, 2, 12), (A // 2, F // 12, 1)))
    tmask = np.ascontiguousarray(np.tile(rt.target_parity_mask(S, 2, 12, K), (A // 2, 1, F // 12, 1)))

    def fn():
        bf = _bf(48000, xs, N, A, S, 100.0, dict(iterations=3, ref_mic=5))
        r = bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask)
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
    torch.cuda.synchronize()
    assert nb.neighbour_launch(tc._cus(dev), iters, C.c_void_p(sink.data_ptr()), C.c_void_p(side.cuda_stream)) == 0
    got = fn()
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(ref, got)):
        assert np.array_equal(x, y), "output %d moved beside the neighbour (%d values)" % (i, int((x != y).sum()))
