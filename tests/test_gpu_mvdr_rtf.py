"""GPU: steering vectors estimated from a target covariance (mca_hip_mvdr_set_rtf, mca_hip_mvdr_sources_frames_rtf_*; k_mvdr_rtf of
kernels_mvdr_rtf.hip and k_mvdr_solve_rtf_t of mvdr_solve.h) against the float64 twin of the definition (tests/mvdr_rtf_twin.py).

Bars: the module's 5e-6 for the covariances (noise and target), 5e-4 of the peak for spectra, audio and steering vectors.  The last
three would be four times the float32 estimator's own error if that were above 1.25e-4; tests/test_mvdr_rtf_twin.py
(test_parity_cases_keep_clear_of_the_decision_edges) measures it on the CPU, on the inputs used here: at most 2.4e-5 in the spectra
and 2.8e-5 in the steering vectors, so the module's bars stand.  Cells at a decision edge of the twin (mvdr_rtf_twin.edge_cells) are
left out of the spectra and steering comparisons; that test holds them under 1 % of a case's cells.  The audio is compared whole,
against the twin's synthesis of its spectra in which only those cells carry the GPU's values.  Every test prints its worst case.  On an MI355X the parity cases stay under 2.96e-4 (spectra),
1.04e-4 (audio, whole), 4.23e-7 (covariances) and 3.12e-5 (steering vectors) of the peak, with at most 0.58 % of a case's cells left
out of the spectra; the scene's held state gives 0.995 of the target and 19.16 dB, the twin's figures for that state."""
import functools

import numpy as np
import pytest

from mcarray_amd import api, synth
from oracle import np_twin

import mvdr_mask_twin as mt
import mvdr_nulls_twin as nt
import mvdr_postfilter_twin as pt
import mvdr_rtf_twin as rt

pytestmark = pytest.mark.gpu

SPEC_TOL, AUDIO_TOL, STEER_TOL, COV_TOL = 5e-4, 5e-4, 5e-4, 5e-6
_irregular = pt.irregular
F6 = rt.PARITY_F


def _same(r, q, what=""):
    assert np.array_equal(r["spec"].view(np.float32), q["spec"].view(np.float32), equal_nan=True), what
    assert np.array_equal(r["out"], q["out"], equal_nan=True), what


def _cat(rs, axis=2):
    return dict(spec=np.concatenate([r["spec"] for r in rs], axis=axis), out=np.concatenate([r["out"] for r in rs], axis=axis))


def _bf(fs, xs, N, A, S, cfg=None, pf=None, rtf=True):
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S)
    if pf is not None:
        bf.set_postfilter(True, **pf)
    if rtf:
        bf.set_rtf(True, **(cfg or {}))
    return bf


@functools.lru_cache(maxsize=None)
def _twin(M, fs, N, S, pf):
    xs = synth.ULA16 if M == "ula16" else _irregular(M)
    return rt.parity_twin(xs, fs, N, S, pt.PARITY_PF if pf else None)


def _check_call(r, tw, a, what, worst, tail, pf):
    """stream a of the GPU result r ([A][S][...]) against the twin's run tw.  Spectra: the cells at a decision edge of the twin
    left out.  Audio: the WHOLE output against the twin's synthesis of its own spectra in which only those cells carry the GPU's
    values (tail [S][hop]: the overlap-add carry of that synthesis from the call before, zeros on a fresh stream); returns the
    carry for the next call"""
    S, F, K = tw["spec"].shape
    N = 2 * (K - 1)
    hop = N // 2
    edge = np.swapaxes(rt.edges_of(tw), 0, 1)                              # [S][F][K]
    ks, ka = ("raw", "raw_out") if pf else ("spec", "out")
    patched = np.where(edge, r["spec"][a].astype(np.complex128), tw["spec"])
    ref = np.zeros((S, F * hop))
    for t in range(F):
        y = np_twin.irfft_ccs(patched[:, t], N)
        ref[:, t * hop:(t + 1) * hop] = tail + y[:, :hop]
        tail = y[:, hop:]
    for s in range(S):
        assert np.all(np.isfinite(r["spec"][a, s])) and np.all(np.isfinite(r["out"][a, s])), (what, a, s)
        es = (np.abs(r["spec"][a, s] - tw["spec"][s]) * ~edge[s]).max() / np.abs(tw[ks][s]).max()
        ea = np.abs(r["out"][a, s] - ref[s]).max() / np.abs(tw[ka][s]).max()
        print("%s stream %d source %d: spectra %.2e audio %.2e of the peak; %d of %d cells (%.2f %%) at a decision edge"
              % (what, a, s, es, ea, int(edge[s].sum()), edge[s].size, 100.0 * edge[s].mean()))
        worst[0], worst[1] = max(worst[0], es), max(worst[1], ea)
        assert es <= SPEC_TOL and ea <= AUDIO_TOL, (what, a, s, es, ea)
    return tail


def _check_state(bf, tw, a, what, worst, fs, N, xs, doa_last, cfg):
    """covariance(), target_covariance() and steering() of stream a against the twin's state"""
    ec = np.abs(bf.covariance(a) - tw["phi"]).max() / np.abs(tw["phi"]).max()
    worst[2] = max(worst[2], ec)
    assert ec <= COV_TOL, (what, a, ec)
    n_est = n_fb = 0
    for s in range(tw["psi"].shape[0]):
        psi, cpsi = bf.target_covariance(a, s)
        ep = np.abs(psi - tw["psi"][s]).max() / np.abs(tw["psi"][s]).max()
        en = np.abs(cpsi - tw["cpsi"][s]).max()
        worst[2] = max(worst[2], ep, en)
        assert ep <= COV_TOL and en <= COV_TOL, (what, a, s, ep, en)
        doa = float(doa_last[s])
        g0 = nt.steering(fs, N, xs, [doa])[:, 0]
        d, est, dg = rt.estimate(tw["psi"][s], tw["cpsi"][s], tw["phi"], tw["cphi"], g0, cfg["iterations"], cfg["ref_mic"], cfg["min_share"])
        keep = ~rt.edge_cells(dg, cfg["min_share"])
        gd, gest = bf.steering(doa, a, s)
        assert np.array_equal(gest[keep], est[keep]), (what, a, s, np.flatnonzero(gest != est))
        ed = (np.abs(gd - d) * keep[:, None]).max() / np.abs(d).max()
        worst[3] = max(worst[3], ed)
        assert ed <= STEER_TOL, (what, a, s, ed)
        assert np.array_equal(gd[gest][:, cfg["ref_mic"]], np.ones(int(gest.sum())))
        n_est, n_fb = n_est + int(gest.sum()), n_fb + int((~gest).sum())
    print("%s stream %d: covariances %.2e steering %.2e; %d estimated, %d fallback cells" % (what, a, worst[2], worst[3], n_est, n_fb))
    return n_est, n_fb


def _parity(M, fs, N, S, pf):
    xs = synth.ULA16 if M == "ula16" else _irregular(M)
    cfg = rt.parity_config(len(xs))
    tw = _twin(M, fs, N, S, pf)
    pcm, doa, upd, tmask = rt.parity_inputs(xs, fs, N, S)
    A, hop = pcm.shape[0], N // 2
    bf = _bf(fs, xs, N, A, S, cfg, pt.PARITY_PF if pf else None)
    assert bf.get_rtf() == dict(enable=True, **cfg)
    worst = [0.0, 0.0, 0.0, 0.0]
    prev = [np.zeros((S, hop)) for _ in range(A)]
    what = "M %s S %d%s" % (M, S, " post-filter" if pf else "")
    for i, (t0, t1) in enumerate([(0, F6), (F6, 2 * F6)]):
        r = bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy(), update_mask=upd[:, t0:t1], target_mask=tmask[:, :, t0:t1])
        assert r["out"].shape == (A, S, F6 * hop) and r["spec"].shape == (A, S, F6, N // 2 + 1)
        for a in range(A):
            prev[a] = _check_call(r, tw[a][i], a, "%s call %d" % (what, i), worst, prev[a], pf)
            n_est, n_fb = _check_state(bf, tw[a][i], a, "%s call %d" % (what, i), worst, fs, N, xs, doa[a, t1 - 1], cfg)
            assert tw[a][i]["est"].any() and not tw[a][i]["est"].all()
            assert n_est > 0 and n_fb > 0, (what, a, i)
    bf.close()
    share = float(np.mean([rt.edges_of(tw[a][i]).mean() for a in range(A) for i in range(2)]))
    print("%s: worst spectra %.2e audio %.2e covariances %.2e steering %.2e; %.2f %% of the cells left out of the spectra" % ((what,) + tuple(worst) + (100.0 * share,)))
    assert share <= 0.01, (what, share)


@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("M", [2, 3, 4, 5, 8, 11, 13, 16])
def test_rtf_parity(M, S):
    """every number of row slots per lane with a full and a partly empty last slot; one, two and four look directions"""
    _parity(M, 16000, 256, S, False)


def test_rtf_parity_postfilter():
    _parity(11, 16000, 256, 3, True)


def test_rtf_parity_long_frames():
    _parity("ula16", 48000, 1024, 3, False)


# ---- bit identities ----
@pytest.mark.parametrize("pf", [None, "postfilter"])
@pytest.mark.parametrize("M,S", [(16, 1), (13, 3), (5, 2)])
def test_rtf_without_a_target_mask_is_the_masked_call(M, S, pf):
    """RTF enabled on a fresh context, target mask NULL and then all zeros: every cell falls back to cmul(T_hi, T_lo), and spectra,
    audio, covariance and a follow-up call have the bytes of mca_hip_mvdr_sources_frames_masked_* under the same update mask"""
    fs, N, A = 16000, 256, 2
    xs = _irregular(M)
    hop, K = N // 2, N // 2 + 1
    pcm, doa, upd, _ = rt.parity_inputs(xs, fs, N, S)
    pfc = pt.PARITY_PF if pf else None
    fp = api._lib.c_fp

    def run(kind):
        bf = _bf(fs, xs, N, A, S, None, pfc, rtf=kind != "masked")
        rs = []
        for t0, t1 in ((0, F6), (F6, 2 * F6)):
            x, dd, u = pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy(), np.ascontiguousarray(upd[:, t0:t1])
            if kind == "null":
                out, spec = np.empty((A, S, F6 * hop), dtype=np.float32), np.empty((A, S, F6, K), dtype=np.complex64)
                bf._check(bf._lib.mca_hip_mvdr_sources_frames_rtf_host(bf.h, x.ctypes.data_as(fp), A, F6, S, dd.ctypes.data_as(fp), u.ctypes.data_as(fp),
                                                                      None, out.ctypes.data_as(fp), spec.ctypes.data_as(fp)))
                rs.append(dict(out=out, spec=spec))
            elif kind == "zeros":
                rs.append(bf.process_sources(x, dd, update_mask=u, target_mask=np.zeros((A, S, F6, K), dtype=np.float32)))
            else:
                rs.append(bf.process_sources(x, dd, update_mask=u))
        res = _cat(rs), [bf.covariance(a) for a in range(A)]
        if kind != "masked":
            for a in range(A):
                for s in range(S):
                    psi, cpsi = bf.target_covariance(a, s)
                    assert not psi.any() and not cpsi.any()
                    assert not bf.steering(0.3, a, s)[1].any()
        bf.close()
        return res

    ref = run("masked")
    for kind in ("null", "zeros"):
        got = run(kind)
        _same(got[0], ref[0], kind)
        assert all(np.array_equal(p, q) for p, q in zip(got[1], ref[1])), kind


def test_rtf_null_update_mask_is_all_ones():
    fs, N, A, S = 16000, 256, 2, 2
    xs = _irregular(8)
    K = N // 2 + 1
    pcm, doa, _, tmask = rt.parity_inputs(xs, fs, N, S)
    res = []
    for u in (None, np.ones((A, 2 * F6, K), dtype=np.float32)):
        bf = _bf(fs, xs, N, A, S, rt.parity_config(8))
        r = bf.process_sources(pcm, doa, update_mask=u, target_mask=tmask)
        res.append((r, bf.state_save()))
        bf.close()
    _same(res[0][0], res[1][0])
    assert res[0][1] == res[1][1]


def test_rtf_disabled_refuses_the_entry_point_and_unsupported_nulls():
    fs, N, A, S = 16000, 256, 2, 2
    xs = synth.REEM_C
    pcm, doa, upd, tmask = rt.parity_inputs(xs, fs, N, S)
    bf = _bf(fs, xs, N, A, S, rtf=False)
    bf.process_sources(pcm, doa, update_mask=upd)
    before, blob = [bf.covariance(a) for a in range(A)], bf.state_save()
    with pytest.raises(api.MCArrayHipError, match="RTF is not enabled"):
        bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask)
    with pytest.raises(api.MCArrayHipError, match="RTF is not enabled"):
        bf.target_covariance(0, 0)
    with pytest.raises(api.MCArrayHipError, match="RTF is not enabled"):
        bf.steering(0.1)
    assert bf._lib.mca_hip_mvdr_get_timing(bf.h, 5, None, None) == -1        # no timing slot 5 before RTF was ever enabled
    assert bf.state_save() == blob and all(np.array_equal(bf.covariance(a), before[a]) for a in range(A))
    # configuration refusals leave configuration and state
    for bad in (dict(target_alpha=1.0), dict(target_alpha=float("nan")), dict(iterations=0), dict(iterations=5), dict(ref_mic=len(xs)), dict(ref_mic=-1),
                dict(min_share=1.0), dict(min_share=-0.1), dict(min_share=float("inf"))):
        with pytest.raises(api.MCArrayHipError):
            bf.set_rtf(True, **bad)
    cfg = api._lib.MvdrRtfConfig()
    cfg.struct_size, cfg.enable, cfg.iterations = 8, 1, 2
    assert bf._lib.mca_hip_mvdr_set_rtf(bf.h, cfg) == -1
    assert bf.get_rtf() == dict(enable=False, target_alpha=0.95, iterations=2, ref_mic=0, min_share=0.05)
    assert bf.state_save() == blob
    # enabled: a null gain is refused as unsupported, and leaves the state
    bf.set_rtf(True, iterations=3)
    assert bf.get_rtf() == dict(enable=True, target_alpha=0.95, iterations=3, ref_mic=0, min_share=0.05)
    bf.get_timing(5)
    psi0 = bf.state_save()
    bf.set_null_gain(10.0)
    with pytest.raises(api.MCArrayHipError, match="nulls at estimated"):
        bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask)
    assert bf.state_save() == psi0
    # cphi on enabling (the last part of the blob): 1 where the bin's trace is above 1e-30 -- the closed bin of the parity mask holds nothing
    K = N // 2 + 1
    cphi = np.frombuffer(psi0[-A * K * 4:], dtype=np.float32).reshape(A, K)
    for a in range(A):
        live = np.real(np.trace(bf.covariance(a), axis1=1, axis2=2)) > 1e-30
        assert live.any() and not live.all() and np.array_equal(cphi[a], live.astype(np.float32)), a
    bf.close()


@pytest.mark.parametrize("M,S", [(16, 1), (11, 2), (13, 4)])
def test_rtf_closed_target_cells_leave_psi(M, S):
    """target_covariance() before and after a call, bin by bin: the bins whose cells are all closed (0, NaN, -1, -0.0) keep Psi and
    cpsi bit for bit, every other bin has moved"""
    fs, N, F, A = 16000, 256, 5, 2
    xs = _irregular(M)
    hop, K = N // 2, N // 2 + 1
    pcm = np.stack([nt.scene(xs, fs, N, 2 * F, a) for a in range(A)])
    doa = nt.drifting_doa(A, 2 * F, S)
    bf = _bf(fs, xs, N, A, S)
    bf.process_sources(pcm[:, :, :(F + 1) * hop].copy(), doa[:, :F].copy(), target_mask=1.0)
    before = [[bf.target_covariance(a, s) for s in range(S)] for a in range(A)]
    rng = np.random.default_rng(5)
    tm = rng.choice(np.array([0, 1, .5], dtype=np.float32), size=(A, S, F, K))
    closed = rng.random((A, S, K)) < 0.4
    closed[:, :, 1:16:2] = True                                         # bins 1, 3, ... 15 closed between open ones
    closed[:, :, 0:16:2] = False
    for a in range(A):
        for s in range(S):
            tm[a, s][:, closed[a, s]] = rng.choice(np.array([0.0, np.nan, -1.0, -0.0], dtype=np.float32), size=(F, int(closed[a, s].sum())))
            tm[a, s][0, ~closed[a, s]] = 1.0
    bf.process_sources(pcm[:, :, F * hop:].copy(), doa[:, F:].copy(), target_mask=tm)
    for a in range(A):
        for s in range(S):
            psi, cpsi = bf.target_covariance(a, s)
            moved = np.array([not np.array_equal(psi[k], before[a][s][0][k]) for k in range(K)])
            assert np.array_equal(moved, ~closed[a, s]), (a, s, np.flatnonzero(moved == closed[a, s]))
            assert np.array_equal(cpsi != before[a][s][1], ~closed[a, s]), (a, s)
    bf.close()


# ---- cut and placement invariance ----
@pytest.mark.parametrize("M,S,pf", [(16, 1, None), (12, 3, None), (8, 4, "pf")])
def test_rtf_cut_invariance(M, S, pf):
    """12 frames in one call, as 5 + 7 and as 12 calls of one frame: the same bytes, the state blob included"""
    fs, N, F, A = 16000, 256, 12, 2
    xs = _irregular(M)
    hop = N // 2
    pcm, doa, upd, tmask = rt.parity_inputs(xs, fs, N, S)
    cfg, pfc = rt.parity_config(M), pt.PARITY_PF if pf else None
    one_bf = _bf(fs, xs, N, A, S, cfg, pfc)
    one = one_bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask)
    blob = one_bf.state_save()
    for cuts in ([0, 5, 12], list(range(13))):
        bf = _bf(fs, xs, N, A, S, cfg, pfc)
        rs = [bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy(), update_mask=upd[:, t0:t1], target_mask=tmask[:, :, t0:t1])
              for t0, t1 in zip(cuts[:-1], cuts[1:])]
        _same(_cat(rs), one, "%d calls" % (len(cuts) - 1))
        assert bf.state_save() == blob, "%d calls" % (len(cuts) - 1)
        bf.close()
    one_bf.close()


@pytest.mark.parametrize("cap_kb,launches", [(100, 4), (1, 12)])
def test_rtf_plane_above_the_workspace_cap_is_cut_along_the_frames(cap_kb, launches):
    """a call whose steering plane exceeds the workspace cap (mca_hip_mvdr_set_rtf_workspace; 1 GiB by default) runs k_mvdr_rtf and
    the solve chunk by chunk of frames: the bytes of the uncut call, the state blob included.  12 frames of 2 streams x 2 look
    directions x 129 bins x 8 microphones are 33 KB each: 100 KB takes 3 frames, 1 KB one"""
    fs, N, A, S, M = 16000, 256, 2, 2, 8
    xs = _irregular(M)
    pcm, doa, upd, tmask = rt.parity_inputs(xs, fs, N, S)
    cfg = rt.parity_config(M)
    res = []
    for kb in (None, cap_kb):
        bf = _bf(fs, xs, N, A, S, cfg, pt.PARITY_PF)
        if kb is not None:
            bf.set_rtf_workspace(kb * 1024)
            with pytest.raises(api.MCArrayHipError, match="max_bytes"):
                bf.set_rtf_workspace(0)
        bf.set_timing(True)
        r = bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask)
        res.append((r, bf.state_save(), bf.get_timing(api.MvdrBeamformer.K_RTF)[0]))
        bf.close()
    _same(res[1][0], res[0][0], "cut along the frames")
    assert res[1][1] == res[0][1]
    assert res[0][2] == 1 and res[1][2] == launches


def test_rtf_where_a_stream_sits_does_not_change_bytes():
    """256 streams x 129 bins of 4 microphones, 16 frames -- the shape whose solve goes in a main and a pieced tail launch: stream 0
    and stream 255 with equal input give equal bytes, and both meet the twin"""
    fs, N, F, A, M = 16000, 256, 16, 256, 4
    xs = _irregular(M)
    K = N // 2 + 1
    base = np.stack([nt.scene(xs, fs, N, F, a) for a in range(3)])
    pick = np.arange(A) % 3
    pick[255] = 0
    pcm = base[pick]
    doa = nt.drifting_doa(3, F, 1)[pick]
    rng = np.random.default_rng(7)
    upd = rng.choice(np.array([0, 0, 1, 1, .5, .125], dtype=np.float32), size=(A, F, K))
    tmask = rng.choice(np.array([0, 0, 1, 1, .5, .125], dtype=np.float32), size=(A, 1, F, K))
    upd[0], tmask[0] = mt.parity_mask(1, 12)[0][np.arange(F) % 12], rt.target_parity_mask(1, 1, 12)[0][:, np.arange(F) % 12]
    upd[255], tmask[255] = upd[0], tmask[0]
    cfg = rt.parity_config(M)
    bf = _bf(fs, xs, N, A, 1, cfg)
    r = bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask)
    assert np.array_equal(r["spec"][0].view(np.float32), r["spec"][255].view(np.float32)) and np.array_equal(r["out"][0], r["out"][255])
    assert np.array_equal(bf.covariance(0), bf.covariance(255))
    p0, p255 = bf.target_covariance(0), bf.target_covariance(255)
    assert np.array_equal(p0[0], p255[0]) and np.array_equal(p0[1], p255[1])
    assert not np.array_equal(r["spec"][0], r["spec"][3])                 # (stream 3: the same PCM under other masks)
    tw = rt.mvdr_rtf_stream(fs, N, xs, pcm[0].astype(np.float64), doa[0], upd[0], tmask[0], **cfg)
    worst = [0.0, 0.0, 0.0, 0.0]
    for a in (0, 255):
        _check_call(r, tw, a, "256 streams", worst, np.zeros((1, N // 2)), None)
        _check_state(bf, tw, a, "256 streams", worst, fs, N, xs, doa[a, -1], cfg)
    bf.close()


@pytest.mark.parametrize("M,S,pf", [(16, 1, None), (11, 3, None), (8, 2, "pf")])
@pytest.mark.parametrize("agree", ["every_other_bin", "bins_0_63"])
def test_rtf_column_independence(agree, M, S, pf):
    """two pairs of masks that agree on a set of bins and differ at random elsewhere: the bytes of the agreeing bins are equal"""
    fs, N, F, A = 16000, 256, 12, 2
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
        bf = _bf(fs, xs, N, A, S, rt.parity_config(M), pt.PARITY_PF if pf else None)
        r = bf.process_sources(pcm, doa, update_mask=u, target_mask=t)
        res.append((r, [bf.covariance(a) for a in range(A)], [[bf.target_covariance(a, s) for s in range(S)] for a in range(A)]))
        bf.close()
    (r1, c1, p1), (r2, c2, p2) = res
    assert np.array_equal(np.ascontiguousarray(r1["spec"][..., keep]).view(np.float32), np.ascontiguousarray(r2["spec"][..., keep]).view(np.float32))
    assert not np.array_equal(r1["spec"][..., ~keep], r2["spec"][..., ~keep])
    for a in range(A):
        assert np.array_equal(c1[a][keep], c2[a][keep]) and not np.array_equal(c1[a][~keep], c2[a][~keep])
        for s in range(S):
            assert np.array_equal(p1[a][s][0][keep], p2[a][s][0][keep]) and np.array_equal(p1[a][s][1][keep], p2[a][s][1][keep])
            assert not np.array_equal(p1[a][s][0][~keep], p2[a][s][0][~keep])


# ---- state ----
@pytest.mark.parametrize("pf", [None, "pf"])
def test_rtf_state_round_trip_and_refusals(pf):
    fs, N, A, S = 16000, 256, 2, 2
    xs = _irregular(5)
    hop = N // 2
    pcm, doa, upd, tmask = rt.parity_inputs(xs, fs, N, S)
    cfg, pfc = rt.parity_config(5), pt.PARITY_PF if pf else None

    def call(bf, t0, t1):
        return bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy(), update_mask=upd[:, t0:t1], target_mask=tmask[:, :, t0:t1])

    one = _bf(fs, xs, N, A, S, cfg, pfc)
    call(one, 0, F6)
    blob = one.state_save()
    second = call(one, F6, 2 * F6)
    end = one.state_save()
    other = _bf(fs, xs, N, A, S, cfg, pfc)
    call(other, 0, 3)                                                     # (some other state, to be replaced)
    other.state_load(blob)
    _same(call(other, F6, 2 * F6), second, "resumed")
    assert other.state_save() == end
    # the blob of an RTF context is larger by Psi, cpsi and cphi
    K, tri = N // 2 + 1, 5 * 6 // 2
    plain = _bf(fs, xs, N, A, S, None, pfc, rtf=False)
    assert len(blob) - len(plain.state_save()) == A * S * K * tri * 8 + A * S * K * 4 + A * K * 4
    # refusals: every mismatch of RTF, post-filter or max_sources leaves blob and covariances as they were
    plain.process_sources(pcm[:, :, :4 * hop].copy(), doa[:, :3].copy(), update_mask=upd[:, :3])
    pblob = plain.state_save()
    mism_pf = _bf(fs, xs, N, A, S, cfg, None if pf else pt.PARITY_PF)
    mism_src = _bf(fs, xs, N, A, S + 1, cfg, pfc)
    for target, src in ((plain, blob), (other, pblob), (mism_pf, blob), (mism_src, blob)):
        before, cov = target.state_save(), target.covariance(1)
        with pytest.raises(api.MCArrayHipError):
            target.state_load(src)
        assert target.state_save() == before and np.array_equal(target.covariance(1), cov)
    for b in (one, other, plain, mism_pf, mism_src):
        b.close()


def test_rtf_slots_reset_and_max_sources():
    fs, N, A = 16000, 256, 2
    xs = _irregular(8)
    hop, K = N // 2, N // 2 + 1
    pcm, doa, upd, tmask = rt.parity_inputs(xs, fs, N, 3)
    bf = _bf(fs, xs, N, A, 3, rt.parity_config(8))
    bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask)
    held = [[bf.target_covariance(a, s) for s in range(3)] for a in range(A)]
    assert all(h[0].any() and h[1].any() for row in held for h in row)
    # a call of stream 0 alone with two sources zeroes slot 2 of stream 0 and leaves stream 1
    bf.process_sources(pcm[:1, :, :(F6 + 1) * hop].copy(), doa[:1, :F6, :2].copy(), update_mask=upd[:1, :F6], target_mask=tmask[:1, :2, :F6])
    assert not bf.target_covariance(0, 2)[0].any() and not bf.target_covariance(0, 2)[1].any()
    assert bf.target_covariance(0, 1)[0].any()
    for s in range(3):
        assert np.array_equal(bf.target_covariance(1, s)[0], held[1][s][0]) and np.array_equal(bf.target_covariance(1, s)[1], held[1][s][1])
    # set_max_sources keeps the slots both sizes have and zeroes the others
    keep = [bf.target_covariance(1, s) for s in range(2)]
    bf.set_max_sources(2)
    with pytest.raises(api.MCArrayHipError, match="source"):
        bf.target_covariance(1, 2)
    bf.set_max_sources(4)
    for s in range(2):
        assert np.array_equal(bf.target_covariance(1, s)[0], keep[s][0]) and np.array_equal(bf.target_covariance(1, s)[1], keep[s][1])
    for s in (2, 3):
        assert not bf.target_covariance(1, s)[0].any() and not bf.target_covariance(1, s)[1].any()
    # the other entry points leave the RTF state alone
    blob_psi = [bf.target_covariance(1, s) for s in range(2)]
    bf.process_sources(pcm, doa[:, :, :2].copy(), update_mask=upd)
    for s in range(2):
        assert np.array_equal(bf.target_covariance(1, s)[0], blob_psi[s][0])
    # reset: everything zero
    bf.reset()
    for a in range(A):
        assert not bf.covariance(a).any()
        for s in range(4):
            assert not bf.target_covariance(a, s)[0].any() and not bf.target_covariance(a, s)[1].any()
    bf.close()


def test_rtf_timing_slot():
    fs, N, A, S = 16000, 256, 2, 2
    xs = _irregular(5)
    pcm, doa, upd, tmask = rt.parity_inputs(xs, fs, N, S)
    bf = _bf(fs, xs, N, A, S)
    bf.set_timing(True)
    bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask)
    bf.process_sources(pcm, doa, update_mask=upd)                         # the masked entry point launches no k_mvdr_rtf
    n, ms = bf.get_timing(api.MvdrBeamformer.K_RTF)
    assert n == 1 and ms > 0.0
    assert bf.get_timing(api.MvdrBeamformer.K_SOLVE)[0] == 2
    bf.set_rtf(False)
    assert bf.get_timing(api.MvdrBeamformer.K_RTF)[0] == 1               # readable after disabling
    bf.close()


# ---- the scene ----
def _frozen_figures(phi, d, g0, sc, loading=1e-3):
    """the scene's figures with the weights of the held state: phi [K][M][M], d, g0 [K][M]"""
    K, M = d.shape
    tr = np.real(np.trace(phi, axis1=1, axis2=2))
    live = tr > 1e-30
    PL = np.where(live[:, None, None], phi + (loading * tr / M)[:, None, None] * np.eye(M), np.eye(M))
    w = nt.null_weights(PL, d[:, None, :], 0.0)[:, 0]
    w[~live] = g0[~live] / M
    return rt.scene_figures(np.broadcast_to(w, (rt.SCENE_LAST, K, M)), sc)


def test_rtf_scene():
    """rtf_scene() from the mixture: the GPU run meets the twin at the parity bars, which carries the twin's figures over (0.998 of the
    target's power at the reference microphone, interferer 19.52 dB down; geometric vector: 0.462).  Printed beside them, and held
    to the scene's bars (share within [0.85, 1.15], suppression at least the twin's figure of the run, 19.52 dB, less 3 dB): the figures of the weights
    formed from the GPU's held covariance() and steering() after the last frame."""
    sc = rt.rtf_scene()
    fs, N, F = rt.SCENE_FS, rt.SCENE_N, rt.SCENE_F
    doa = np.full((1, F, 1), rt.SCENE_LOOK, dtype=np.float32)
    look = float(doa[0, 0, 0])
    bf = _bf(fs, sc["xs"], N, 1, 1)
    r = bf.process_sources(sc["pcm"][None], doa, update_mask=sc["update"][None], target_mask=sc["tmask"][None])
    tw = rt.mvdr_rtf_stream(fs, N, sc["xs"], sc["pcm"].astype(np.float64), doa[0].astype(np.float64), sc["update"], sc["tmask"], want_weights=True)
    worst = [0.0, 0.0, 0.0, 0.0]
    cfg = dict(rt.DEFAULTS)
    _check_call(r, tw, 0, "scene", worst, np.zeros((1, N // 2)), None)
    _check_state(bf, tw, 0, "scene", worst, fs, N, sc["xs"], doa[0, -1], cfg)
    g0 = nt.steering(fs, N, sc["xs"], [look])[:, 0]
    gd, gest = bf.steering(look, 0, 0)
    f_gpu = _frozen_figures(bf.covariance(0), gd, g0, sc)
    f_twin = _frozen_figures(tw["phi"], tw["d"][-1, 0], g0, sc)
    f_run = rt.scene_figures(tw["w"][:, 0], sc)
    print("scene: twin, frame by frame: share %.3f, %.2f dB; held state, twin: %.3f, %.2f dB; held state, GPU: %.3f, %.2f dB; %d of %d cells estimated"
          % (f_run + f_twin + f_gpu + (int(gest.sum()), gest.size)))
    b = rt.SCENE_BARS
    assert b["share_lo"] <= f_gpu[0] <= b["share_hi"]
    assert f_gpu[1] >= f_run[1] - b["suppression_margin_db"]              # the twin's own figure of this scene, frame by frame
    bf.close()


# ---- the device entry ----
@pytest.mark.parametrize("S", [1, 3])
def test_rtf_dev_entry_under_a_padded_offset_stride(S):
    """the _dev entry with PCM at padded, offset strides in a poisoned allocation equals the contiguous call bit for bit"""
    import torch
    from dev_layout_helpers import guarded, strided_pcm
    fs, N, A = 48000, 1024, 2
    xs = synth.ULA8
    F, hop, K = F6, N // 2, N // 2 + 1
    pcm, doa, upd, tmask = rt.parity_inputs(xs, fs, N, S)
    pcm, doa, upd, tmask = pcm[:, :, :(F + 1) * hop].copy(), doa[:, :F].copy(), np.ascontiguousarray(upd[:, :F]), np.ascontiguousarray(tmask[:, :, :F])
    cfg = rt.parity_config(len(xs))
    ref_bf = _bf(fs, xs, N, A, S, cfg)
    ref = ref_bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask)
    bf = _bf(fs, xs, N, A, S, cfg)
    view, whole = strided_pcm(pcm)
    t_doa, t_u, t_m = torch.from_numpy(doa).cuda(), torch.from_numpy(upd).cuda(), torch.from_numpy(tmask).cuda()
    g_out, g_spec = guarded((A, S, F * hop), torch.float32), guarded((A, S, F, K, 2), torch.float32)
    if S == 1:
        bf.process_dev(view, F, t_doa[:, :, 0].contiguous(), out_pcm=g_out.t, out_spec=g_spec.t, update_mask=t_u, target_mask=t_m)
    else:
        bf.process_sources_dev(view, F, t_doa, out_pcm=g_out.t, out_spec=g_spec.t, update_mask=t_u, target_mask=t_m)
    torch.cuda.synchronize()
    g_out.assert_guards_intact("out"); g_spec.assert_guards_intact("spec")
    spec = g_spec.t.cpu().numpy()
    assert np.array_equal(spec.reshape(ref["spec"].shape + (2,)), ref["spec"].view(np.float32).reshape(ref["spec"].shape + (2,)))
    assert np.array_equal(g_out.t.cpu().numpy(), ref["out"])
    assert bf.state_save() == ref_bf.state_save()
    blob = bf.state_save()
    for bad in (t_m[:, :, :F - 1].contiguous(), t_m[:, :, :, :K - 1].contiguous(), t_m[:, :, :, ::2], t_m.double(), t_m[:, 0].contiguous(), t_m.cpu()):
        with pytest.raises(api.MCArrayHipError, match="target_mask"):
            bf.process_sources_dev(view, F, t_doa, out_pcm=g_out.t, update_mask=t_u, target_mask=bad)
    for bad in (t_u[:, :F - 1].contiguous(), t_u[:, :, ::2], t_u.double()):
        with pytest.raises(api.MCArrayHipError, match="update_mask"):
            bf.process_sources_dev(view, F, t_doa, out_pcm=g_out.t, update_mask=bad, target_mask=t_m)
    with pytest.raises(api.MCArrayHipError, match="not with update"):
        bf.process_sources_dev(view, F, t_doa, out_pcm=g_out.t, update=t_u[:, :, 0].contiguous(), target_mask=t_m)
    with pytest.raises(api.MCArrayHipError, match="both NULL"):
        bf.process_sources_dev(view, F, t_doa, update_mask=t_u, target_mask=t_m)
    assert bf.state_save() == blob
    bf.close(); ref_bf.close()


def test_rtf_results_do_not_move_beside_a_matrix_core_neighbour():
    """k_mvdr_rtf and the solve behind it beside the neighbour of tests/test_gpu_coresidency.py (the procedure of its module test, as
    tests/test_gpu_mvdr_mask.py runs it): 16 microphones, masks whose quads diverge"""
    import ctypes as C
    import time
    import torch
    import test_gpu_coresidency as tc
    nb = tc._neighbour()
    dev = torch.device("cuda:0")
    F, A, N, xs = 60, 16, 1024, synth.ULA16
    K = N // 2 + 1
    pcm = np.stack([synth.noise_source_stream(xs, np.deg2rad(20.0 - 7 * a), 48000, (F + 1) * N // 2, 80 + a) for a in range(A)]).astype(np.float32)
    doa = (np.deg2rad(20.0 - 7 * np.arange(A))[:, None] + 0.01 * np.arange(F)[None, :]).astype(np.float32)
    upd = np.ascontiguousarray(np.tile(mt.mask_for(K, 2, 12), (A // 2, F // 12, 1)))
    tmask = np.ascontiguousarray(np.tile(rt.target_parity_mask(1, 2, 12, K), (A // 2, 1, F // 12, 1)))

    def fn():
        bf = _bf(48000, xs, N, A, 1, dict(iterations=3, ref_mic=5))
        r = bf.process(pcm, doa, want_spec=True, update_mask=upd, target_mask=tmask)
        psi = bf.target_covariance(A - 1, 0)[0]
        d = bf.steering(float(doa[A - 1, -1]), A - 1, 0)[0]
        bf.close()
        return r["out"], r["spec"], psi, d

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
