"""GPU: the masks estimated from the call's own spectra (mca_hip_mvdr_set_mask_estimator, mca_hip_mvdr_sources_frames_auto_*;
k_mvdr_estmask of kernels_mvdr_estmask.hip) against the float64 twin of the definition (tests/mvdr_estmask_twin.py), and the auto call
against the masked / RTF call fed the masks it returned, bit for bit.

The mask bar is four times the distance of the twin's float32 variant from the float64 twin outside edge cells, the rule of
tests/test_gpu_mvdr_rtf.py: tests/test_mvdr_estmask_twin.py measures 1.031e-6 at the most on the inputs used here (recorded as
mvdr_estmask_twin.MASK_F32_MEASURED), so the bar is MASK_BAR = 4.124e-6 in both masks.  Edge cells (two largest c within
1e-4, e under 1e-6 of the frame's largest, another winner in float32) are left out of the target masks' comparison, at most 1 % of a
case's cells; the update mask of a case whose directions are all protected is continuous across a winner tie and is compared
everywhere but in the low-energy cells.  Every test prints its worst case.  On an MI355X the parity cases stay under 3.61e-6 (two
microphones, one direction, thresholds 0.2 / 0.4), 2.57e-6 (eight, one direction) and 2.3e-6 (every case with two or four directions)
in both masks, 1.02e-6 at N = 1024, with at most 0.28 % of a case's cells left out; the scene's held state gives 0.978 of the target
and 13.26 dB, the twin's figures for that state."""
import functools

import numpy as np
import pytest

from mcarray_amd import api

import mvdr_estmask_twin as et
import mvdr_nulls_twin as nt
import mvdr_postfilter_twin as pt
import mvdr_rtf_twin as rt

pytestmark = pytest.mark.gpu

F6 = et.PARITY_F
RTF_CFG = dict(target_alpha=0.9, iterations=2, ref_mic=1, min_share=0.05)


def _same(r, q, what=""):
    assert np.array_equal(r["spec"].view(np.float32), q["spec"].view(np.float32), equal_nan=True), what
    assert np.array_equal(r["out"], q["out"], equal_nan=True), what


def _same_masks(r, q, what=""):
    assert np.array_equal(r["update_mask"], q["update_mask"]) and np.array_equal(r["target_mask"], q["target_mask"]), what


def _cat(rs):
    return dict(spec=np.concatenate([r["spec"] for r in rs], axis=2), out=np.concatenate([r["out"] for r in rs], axis=2),
                update_mask=np.concatenate([r["update_mask"] for r in rs], axis=1), target_mask=np.concatenate([r["target_mask"] for r in rs], axis=2))


def _bf(fs, xs, N, A, S, est=None, rtf=None, pf=None, null_gain=0.0):
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=null_gain)
    if pf is not None:
        bf.set_postfilter(True, **pf)
    if rtf is not None:
        bf.set_rtf(True, **rtf)
    if est is not None:
        bf.set_mask_estimator(True, **est)
    return bf


def _state(bf, A, S, rtf):
    st = [bf.covariance(a) for a in range(A)]
    if rtf:
        st += [x for a in range(A) for s in range(S) for x in bf.target_covariance(a, s)]
    return st


def _inputs(M, S, N=256, fs=16000):
    xs = et.parity_xs(M)
    pcm, doa = et.parity_inputs(xs, fs, N, S)
    return xs, pcm, doa


# ---- parity of the masks ----
def _parity(case):
    name, M, fs, N, S, P = case
    p = et.parity(case)
    xs, cfg, pcm, doa = p["xs"], p["cfg"], p["pcm"], p["doa"]
    A, hop, K = pcm.shape[0], N // 2, N // 2 + 1
    # RTF on the contexts of an odd number of microphones: the masks do not depend on what the call does behind them
    bf = _bf(fs, xs, N, A, S, cfg, RTF_CFG if len(xs) % 2 else None)
    assert bf.get_mask_estimator() == dict(enable=True, **cfg)
    wt = wu = 0.0
    n_edge = n_all = 0
    band = p["d64"][0]["band"]
    for i, (t0, t1) in enumerate([(0, F6), (F6, 2 * F6)]):
        r = bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy(), estimate_masks=True)
        assert r["update_mask"].shape == (A, F6, K) and r["target_mask"].shape == (A, S, F6, K) and r["spec"].shape == (A, S, F6, K)
        assert r["update_mask"].dtype == np.float32 and r["target_mask"].dtype == np.float32
        for a in range(A):
            d, low, edge = p["d64"][a], p["low"][a][t0:t1], p["edge"][a][t0:t1]
            tm, um = r["target_mask"][a].astype(np.float64), r["update_mask"][a].astype(np.float64)
            assert np.all((tm >= 0) & (tm <= 1)) and np.all((um >= 0) & (um <= 1)), (name, a, i)
            # outside the band: exactly the plain recursion
            assert not tm[:, :, ~band].any() and np.array_equal(um[:, ~band], np.ones((F6, int((~band).sum())))), (name, a, i)
            # at most one look direction holds a cell
            assert np.all((tm > 0).sum(axis=0) <= 1), (name, a, i)
            e_t = float((np.abs(tm - d["target"][:, t0:t1]) * ~edge[None]).max())
            e_u = float((np.abs(um - d["update"][t0:t1]) * ~(low if P == 0 else edge)).max())
            n_edge, n_all = n_edge + int(edge.sum()), n_all + edge.size
            print("%s call %d stream %d: target masks %.2e update mask %.2e (bar %.2e); %d of %d cells (%.2f %%) edge cells, %d of low energy"
                  % (name, i, a, e_t, e_u, et.MASK_BAR, int(edge.sum()), edge.size, 100.0 * edge.mean(), int(low.sum())))
            wt, wu = max(wt, e_t), max(wu, e_u)
    bf.close()
    share = n_edge / n_all
    print("%s: worst target masks %.2e update mask %.2e; %.2f %% of the cells left out" % (name, wt, wu, 100.0 * share))
    assert share <= 0.01, (name, share)
    assert wt <= et.MASK_BAR and wu <= et.MASK_BAR, (name, wt, wu)


@pytest.mark.parametrize("S", et.PARITY_S)
@pytest.mark.parametrize("M", et.PARITY_M)
def test_estmask_parity(M, S):
    """every number of row slots per lane with a full and a partly empty last slot; one (thresholds 0.2 / 0.4), two and four look
    directions, all protected: both masks against the twin under MASK_BAR, the update mask everywhere but in low-energy cells"""
    _parity(("M%d_S%d" % (M, S), M, 16000, 256, S, 0))


def test_estmask_parity_competitor():
    """two look directions, the first protected: the update mask jumps where the winner changes, and is compared outside edge cells"""
    _parity(("M8_S2_P1", 8, 16000, 256, 2, 1))


def test_estmask_parity_long_frames():
    """N = 1024: the tables of k_mvdr_analyse_1024, with another number of high-order phasors"""
    _parity(("ula16_N1024_S2", "ula16", 48000, 1024, 2, 0))


# ---- exactness of the orchestration ----
@pytest.mark.parametrize("M,S,pf,cap", [(8, 2, None, None), (8, 2, "pf", None), (8, 2, "pf", 1), (13, 4, None, 100), (16, 1, "pf", None)])
def test_auto_with_rtf_is_the_rtf_call_fed_its_masks(M, S, pf, cap):
    """RTF enabled: the auto call and process_sources(update_mask=, target_mask=) on a twin context fed the masks the auto call
    returned give the same spectra, audio, covariance() and target_covariance(), over two calls; with the post-filter, and with a
    workspace cap (KB) that cuts the call along the frames"""
    fs, N, A = 16000, 256, 2
    xs, pcm, doa = _inputs(M, S)
    hop = N // 2
    cfg, pfc = et.parity_config(N, S, 1 if S > 1 else 0), pt.PARITY_PF if pf else None
    auto, fed = _bf(fs, xs, N, A, S, cfg, RTF_CFG, pfc), _bf(fs, xs, N, A, S, None, RTF_CFG, pfc)
    if cap:
        auto.set_rtf_workspace(cap * 1024)
    auto.set_timing(True)
    for t0, t1 in ((0, F6), (F6, 2 * F6)):
        x, dd = pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy()
        r = auto.process_sources(x, dd, estimate_masks=True)
        q = fed.process_sources(x, dd, update_mask=r["update_mask"], target_mask=r["target_mask"])
        _same(r, q, (t0, t1))
        assert 0.0 < r["target_mask"].mean() < 1.0 and 0.0 < r["update_mask"].mean() < 1.0
        assert all(np.array_equal(u, v) for u, v in zip(_state(auto, A, S, True), _state(fed, A, S, True)))
    assert auto.state_save() == fed.state_save()                           # nothing of the estimator is stream state
    n_est, n_rtf = auto.get_timing(api.MvdrBeamformer.K_ESTMASK)[0], auto.get_timing(api.MvdrBeamformer.K_RTF)[0]
    print("M %d S %d: %d k_mvdr_estmask and %d k_mvdr_rtf launches in two calls" % (M, S, n_est, n_rtf))
    assert n_est == 2 and (n_rtf > 2 if cap else n_rtf == 2)               # the masks once per call, ahead of the chunks
    auto.close(); fed.close()


@pytest.mark.parametrize("M,S,gain,pf", [(8, 2, 0.0, None), (8, 2, 10.0, None), (11, 4, 10.0, "pf"), (5, 1, 0.0, "pf")])
def test_auto_without_rtf_is_the_masked_call_fed_its_mask(M, S, gain, pf):
    fs, N, A = 16000, 256, 2
    xs, pcm, doa = _inputs(M, S)
    hop = N // 2
    cfg, pfc = et.parity_config(N, S), pt.PARITY_PF if pf else None
    auto, fed = _bf(fs, xs, N, A, S, cfg, None, pfc, gain), _bf(fs, xs, N, A, S, None, None, pfc, gain)
    for t0, t1 in ((0, F6), (F6, 2 * F6)):
        x, dd = pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy()
        r = auto.process_sources(x, dd, estimate_masks=True)
        q = fed.process_sources(x, dd, update_mask=r["update_mask"])
        _same(r, q, (t0, t1))
        assert 0.0 < r["target_mask"].mean() < 1.0                       # still written
        assert all(np.array_equal(u, v) for u, v in zip(_state(auto, A, S, False), _state(fed, A, S, False)))
    assert auto.state_save() == fed.state_save()
    auto.close(); fed.close()


@pytest.mark.parametrize("M,S,rtf", [(16, 1, True), (12, 3, True), (8, 4, False)])
def test_auto_cut_invariance(M, S, rtf):
    """12 frames in one call and as two calls of 6: the same masks, spectra, audio and state blob"""
    fs, N, A = 16000, 256, 2
    xs, pcm, doa = _inputs(M, S)
    hop = N // 2
    cfg, rc = et.parity_config(N, S), RTF_CFG if rtf else None
    one_bf = _bf(fs, xs, N, A, S, cfg, rc)
    one = one_bf.process_sources(pcm, doa, estimate_masks=True)
    bf = _bf(fs, xs, N, A, S, cfg, rc)
    two = _cat([bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy(), estimate_masks=True) for t0, t1 in ((0, F6), (F6, 2 * F6))])
    _same_masks(two, one)
    _same(two, one)
    assert bf.state_save() == one_bf.state_save()
    bf.close(); one_bf.close()


def test_auto_where_a_stream_sits_does_not_change_bytes():
    """a stream alone gives the bytes of the same stream as the second of three"""
    fs, N, S, M = 16000, 256, 2, 11
    xs = et.parity_xs(M)
    pcm, doa = et.parity_inputs(xs, fs, N, S, A=3)
    cfg = et.parity_config(N, S, 1)
    three_bf, alone_bf = _bf(fs, xs, N, 3, S, cfg, RTF_CFG), _bf(fs, xs, N, 1, S, cfg, RTF_CFG)
    three = three_bf.process_sources(pcm, doa, estimate_masks=True)
    alone = alone_bf.process_sources(pcm[1:2].copy(), doa[1:2].copy(), estimate_masks=True)
    for key in ("update_mask", "target_mask", "out"):
        assert np.array_equal(alone[key][0], three[key][1]), key
    assert np.array_equal(alone["spec"][0].view(np.float32), three["spec"][1].view(np.float32))
    assert np.array_equal(alone_bf.covariance(0), three_bf.covariance(1))
    assert not np.array_equal(three["target_mask"][0], three["target_mask"][1])
    three_bf.close(); alone_bf.close()


def test_single_look_process_and_the_dev_entry():
    """process(estimate_masks=True) is process_sources() with one direction; the _dev entries fill new device tensors with the same
    bytes, and a direct call with NULL mask outputs (the masks in the workspace only) gives the same spectra"""
    import torch
    from dev_layout_helpers import guarded, strided_pcm
    fs, N, A, M = 16000, 256, 2, 5
    xs, pcm, doa = _inputs(M, 2)
    F, hop, K = F6, N // 2, N // 2 + 1
    pcm, doa = pcm[:, :, :(F + 1) * hop].copy(), doa[:, :F].copy()
    for S in (1, 2):
        cfg = et.parity_config(N, S, 1)
        dd = np.ascontiguousarray(doa[:, :, :S])
        ref_bf = _bf(fs, xs, N, A, S, cfg, RTF_CFG)
        ref = ref_bf.process_sources(pcm, dd, estimate_masks=True)
        if S == 1:
            bf = _bf(fs, xs, N, A, 1, cfg, RTF_CFG)
            one = bf.process(pcm, dd[:, :, 0], want_spec=True, estimate_masks=True)
            assert np.array_equal(one["out"], ref["out"][:, 0]) and np.array_equal(one["spec"].view(np.float32), ref["spec"][:, 0].view(np.float32))
            _same_masks(one, ref)
            bf.close()
        bf = _bf(fs, xs, N, A, S, cfg, RTF_CFG)
        view, whole = strided_pcm(pcm)
        t_doa = torch.from_numpy(dd).cuda()
        g_out, g_spec = guarded((A, S, F * hop), torch.float32), guarded((A, S, F, K, 2), torch.float32)
        if S == 1:
            m = bf.process_dev(view, F, t_doa[:, :, 0].contiguous(), out_pcm=g_out.t, out_spec=g_spec.t, estimate_masks=True)
        else:
            mine = (torch.empty((A, F, K), dtype=torch.float32, device="cuda"), torch.empty((A, S, F, K), dtype=torch.float32, device="cuda"))
            m = bf.process_sources_dev(view, F, t_doa, out_pcm=g_out.t, out_spec=g_spec.t, estimate_masks=True, masks_out=mine)
            assert m["update_mask"] is mine[0] and m["target_mask"] is mine[1]
            with pytest.raises(api.MCArrayHipError, match="masks_out"):
                bf.process_sources_dev(view, F, t_doa, out_pcm=g_out.t, estimate_masks=True, masks_out=(mine[0], mine[1][:, :1].contiguous()))
        torch.cuda.synchronize()
        g_out.assert_guards_intact("out"); g_spec.assert_guards_intact("spec")
        assert np.array_equal(m["update_mask"].cpu().numpy(), ref["update_mask"]) and np.array_equal(m["target_mask"].cpu().numpy(), ref["target_mask"])
        assert np.array_equal(g_spec.t.cpu().numpy().reshape(ref["spec"].shape + (2,)), ref["spec"].view(np.float32).reshape(ref["spec"].shape + (2,)))
        assert np.array_equal(g_out.t.cpu().numpy(), ref["out"])
        assert bf.state_save() == ref_bf.state_save()
        bf.close()
        # guarded mask outputs, then none at all
        bf = _bf(fs, xs, N, A, S, cfg, RTF_CFG)
        g_um, g_tm = guarded((A, F, K), torch.float32), guarded((A, S, F, K), torch.float32)
        p, sa, sc = api.pcm_layout(view)
        for um, tm in ((g_um.t, g_tm.t), (None, None)):
            bf.reset()
            g_spec.t.zero_()
            bf._check(bf._lib.mca_hip_mvdr_sources_frames_auto_dev(bf.h, p, sa, sc, A, F, S, api._ptr(t_doa), api._ptr(um), api._ptr(tm), None,
                                                                   api._ptr(g_spec.t), None))
            torch.cuda.synchronize()
            assert np.array_equal(g_spec.t.cpu().numpy().reshape(ref["spec"].shape + (2,)), ref["spec"].view(np.float32).reshape(ref["spec"].shape + (2,)))
        g_um.assert_guards_intact("update mask"); g_tm.assert_guards_intact("target masks")
        assert np.array_equal(g_um.t.cpu().numpy(), ref["update_mask"]) and np.array_equal(g_tm.t.cpu().numpy(), ref["target_mask"])
        with pytest.raises(api.MCArrayHipError, match="forms the masks itself"):
            bf.process_sources_dev(view, F, t_doa, out_pcm=g_out.t, update_mask=g_um.t, estimate_masks=True)
        bf.close(); ref_bf.close()


# ---- refusals ----
def test_estimator_refusals_and_timing_slot():
    fs, N, A, S = 16000, 256, 2, 2
    xs, pcm, doa = _inputs(8, S)
    bf = _bf(fs, xs, N, A, S, None, RTF_CFG)
    defaults = dict(enable=False, bin_lo=0, bin_hi=N // 2, coherence_lo=0.0, coherence_hi=0.05, n_protected=0)
    assert bf.get_mask_estimator() == defaults
    bf.process_sources(pcm, doa, update_mask=1.0, target_mask=0.0)
    blob = bf.state_save()
    with pytest.raises(api.MCArrayHipError, match="mask estimator is not enabled"):
        bf.process_sources(pcm, doa, estimate_masks=True)
    assert bf._lib.mca_hip_mvdr_get_timing(bf.h, 6, None, None) == -1        # no timing slot 6 before the estimator was ever enabled
    assert bf.state_save() == blob
    # every bad value leaves the former configuration
    good = dict(bin_lo=3, bin_hi=100, coherence_lo=0.1, coherence_hi=0.6, n_protected=1)
    bf.set_mask_estimator(True, **good)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(bin_lo=-1), dict(bin_lo=101), dict(bin_hi=N // 2 + 1), dict(bin_hi=2), dict(coherence_lo=-0.1), dict(coherence_lo=nan),
                dict(coherence_hi=1.5), dict(coherence_hi=nan), dict(coherence_hi=inf), dict(coherence_lo=0.6), dict(coherence_lo=0.5995),
                dict(coherence_lo=0.7), dict(n_protected=-1), dict(n_protected=5)):
        with pytest.raises(api.MCArrayHipError):
            bf.set_mask_estimator(True, **dict(good, **bad))
        assert bf.get_mask_estimator() == dict(enable=True, **good), bad
    cfg = api._lib.MvdrEstmaskConfig()
    cfg.struct_size, cfg.enable, cfg.bin_hi, cfg.coherence_hi = 36, 1, 10, 0.5
    assert bf._lib.mca_hip_mvdr_set_mask_estimator(bf.h, cfg) == -1
    assert bf.get_mask_estimator() == dict(enable=True, **good)
    bf.set_mask_estimator(True, **dict(good, coherence_hi=0.101, n_protected=4))       # the least span; n_protected above S is all
    # the underlying call's refusals pass through with their codes, and leave the state
    bf.set_timing(True)
    r = bf.process_sources(pcm, doa, estimate_masks=True)
    assert np.all(np.isfinite(r["out"]))
    blob = bf.state_save()
    bf.set_null_gain(10.0)
    with pytest.raises(api.MCArrayHipError, match="error -4: nulls at estimated"):
        bf.process_sources(pcm, doa, estimate_masks=True)
    bf.set_null_gain(0.0)
    with pytest.raises(api.MCArrayHipError, match="n_sources outside"):
        bf.process_sources(pcm, np.concatenate([doa, doa[:, :, :1]], axis=2), estimate_masks=True)
    for kw in (dict(update=1.0), dict(update_mask=1.0), dict(target_mask=0.0)):
        with pytest.raises(api.MCArrayHipError, match="forms the masks itself"):
            bf.process_sources(pcm, doa, estimate_masks=True, **kw)
        with pytest.raises(api.MCArrayHipError, match="forms the masks itself"):
            bf.process(pcm, doa[:, :, 0], estimate_masks=True, **kw)
    fp = api._lib.c_fp
    assert bf._lib.mca_hip_mvdr_sources_frames_auto_host(bf.h, pcm.ctypes.data_as(fp), A, 2 * F6, S, doa.ctypes.data_as(fp), None, None, None, None) == -1
    assert bf.state_save() == blob
    # timing slot 6: one launch per auto call, none by the other entry points, readable after disabling
    bf.process_sources(pcm, doa, update_mask=1.0, target_mask=0.0)
    n, ms = bf.get_timing(api.MvdrBeamformer.K_ESTMASK)
    assert n == 1 and ms > 0.0
    bf.set_mask_estimator(False)
    assert bf.get_timing(api.MvdrBeamformer.K_ESTMASK)[0] == 1
    with pytest.raises(api.MCArrayHipError, match="mask estimator is not enabled"):
        bf.process_sources(pcm, doa, estimate_masks=True)
    bf.close()


# ---- the other entry points ----
@pytest.mark.parametrize("pf", [None, "pf"])
def test_enabling_the_estimator_leaves_the_other_entry_points(pf):
    """with the estimator enabled (and used in between on another context's behalf: its workspace allocated), the plain, weighted,
    masked and RTF calls give the bytes of a context that never enabled it, launch by launch"""
    fs, N, A, S = 16000, 256, 2, 2
    xs, pcm, doa = _inputs(13, S)
    pcm2, doa2, upd, tmask = rt.parity_inputs(xs, fs, N, S)
    assert np.array_equal(pcm, pcm2) and np.array_equal(doa, doa2)
    pfc = pt.PARITY_PF if pf else None
    res = []
    for est in (None, et.parity_config(N, S, 1)):
        out = []
        for rtf in (None, RTF_CFG):
            bf = _bf(fs, xs, N, A, S, est, rtf, pfc)
            bf.set_timing(True)
            if est is not None:
                bf.process_sources(pcm, doa, estimate_masks=True)         # (allocates the mask workspace)
                bf.reset()
            out.append(bf.process_sources(pcm, doa))
            out.append(bf.process_sources(pcm, doa, update=upd[:, :, 70]))
            out.append(bf.process_sources(pcm, doa, update_mask=upd))
            out.append(bf.process(pcm, doa[:, :, 0], want_spec=True, update_mask=upd))
            if rtf is not None:
                out.append(bf.process_sources(pcm, doa, update_mask=upd, target_mask=tmask))
            if est is not None:
                assert bf.get_timing(api.MvdrBeamformer.K_ESTMASK)[0] == 1
            out.append(dict(spec=np.zeros(1, dtype=np.complex64), out=np.frombuffer(bf.state_save(), dtype=np.uint8)))
            bf.close()
        res.append(out)
    assert len(res[0]) == len(res[1])
    for i, (r, q) in enumerate(zip(*res)):
        _same(r, q, i)


# ---- the scene ----
def _frozen_figures(phi, d, g0, sc, loading=1e-3):
    """the scene's figures with the weights of the held state: phi [K][M][M], d, g0 [K][M] (as tests/test_gpu_mvdr_rtf.py recovers them)"""
    K, M = d.shape
    tr = np.real(np.trace(phi, axis1=1, axis2=2))
    live = tr > 1e-30
    PL = np.where(live[:, None, None], phi + (loading * tr / M)[:, None, None] * np.eye(M), np.eye(M))
    w = nt.null_weights(PL, d[:, None, :], 0.0)[:, 0]
    w[~live] = g0[~live] / M
    return rt.scene_figures(np.broadcast_to(w, (rt.SCENE_LAST, K, M)), sc)


@functools.lru_cache(maxsize=None)
def _scene_twin():
    return et.scene_runs()


def test_auto_scene():
    """rtf_scene() from the mixture alone: look directions (+24, -40 degrees), the first protected, thresholds 0 / 0.05, whole band, RTF
    with two iterations.  The twin keeps 0.982 of the target's power at the reference microphone with the interferer 12.54 dB down
    (0.009 and 17.21 dB without masks; oracle masks 0.998 and 19.52 dB).  Held to the scene's bars -- share within [0.85, 1.15],
    suppression at least the twin's recorded 12.54 dB less 3 dB: the figures of the weights formed from the GPU's held covariance() and
    steering() of output 0 after the last frame; the twin's figures of its own held state are printed beside them."""
    sc = rt.rtf_scene()
    fs, N, F = rt.SCENE_FS, rt.SCENE_N, rt.SCENE_F
    doa = np.tile(et.SCENE_DOAS.astype(np.float32), (1, F, 1))
    look = float(doa[0, 0, 0])
    bf = _bf(fs, sc["xs"], N, 1, 2, dict(et.SCENE_CFG, bin_hi=N // 2), et.SCENE_RTF)
    r = bf.process_sources(sc["pcm"][None], doa, estimate_masks=True)
    tw = _scene_twin()["run"]
    low, edge = et.edge_cells(tw["masks"], et.masks(fs, N, sc["xs"], sc["pcm"], doa[0], dtype=np.float32, **et.SCENE_CFG))
    e_t = float((np.abs(r["target_mask"][0] - tw["target_mask"]) * ~edge[None]).max())
    g0 = nt.steering(fs, N, sc["xs"], [look])[:, 0]
    gd, gest = bf.steering(look, 0, 0)
    f_gpu = _frozen_figures(bf.covariance(0), gd, g0, sc)
    f_twin = _frozen_figures(tw["phi"], tw["d"][-1, 0], g0, sc)
    print("scene: twin, frame by frame: share %.3f, %.2f dB; held state, twin: %.3f, %.2f dB; held state, GPU: %.3f, %.2f dB; %d of %d cells "
          "estimated; target masks within %.2e of the twin's outside %.2f %% edge cells; protected cells %.1f %% (oracle %.1f %%)"
          % (_scene_twin()["estimated"] + f_twin + f_gpu + (int(gest.sum()), gest.size, e_t, 100.0 * edge.mean(),
                                                          100.0 * (r["update_mask"] < 1).mean(), 100.0 * sc["tmask"].mean())))
    b = rt.SCENE_BARS
    assert b["share_lo"] <= f_gpu[0] <= b["share_hi"]
    assert f_gpu[1] >= et.SCENE_TWIN["estimated"][1] - b["suppression_margin_db"]
    bf.close()
