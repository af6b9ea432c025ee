"""GPU: time-frequency update masks of the MVDR calls (mca_hip_mvdr_sources_frames_masked_*; k_mvdr_solve_t<..., WEIGHT = CELL, ...>
of mvdr_solve.h) against the float64 twin of the dense definition (tests/mvdr_mask_twin.py).

The bars are those of tests/test_gpu_mvdr_gate.py, from tests/test_gpu_mvdr.py: 5e-4 of the peak for spectra and audio, 5e-6 for the
covariance.  tests/test_mvdr_mask_twin.py shows that on the scene and mask used here the masked spectra and covariance differ from
the all-ones run and from the per-frame run at the mask's mean by more than 0.1 of the peak, so a kernel that ignores the bin index
cannot pass.  Every test prints its worst case.  On an MI355X (spectra / audio / covariance of the peak): the row-slot cases stay
under 1.93e-4 / 1.34e-4 / 3.90e-7, N = 1024 3.61e-4 / 2.05e-4 / 2.85e-7, N = 2048 8.44e-5 / 9.96e-5 / 3.51e-7, the post-filter cases
1.41e-4 / 1.04e-4 / 3.01e-7; the scene gives 12.84 dB and 0.866 (all ones: 6.41 dB and 0.095), the twin's figures."""
import numpy as np
import pytest

from mcarray_amd import api, synth
from oracle import pyoracle as po

import mvdr_gate_twin as gt
import mvdr_mask_twin as mt
import mvdr_nulls_twin as nt
import mvdr_postfilter_twin as pt

pytestmark = pytest.mark.gpu

SPEC_TOL, AUDIO_TOL, COV_TOL = 5e-4, 5e-4, 5e-6
W12 = pt.W12                                   # the weights of tests/test_gpu_mvdr_gate.py
_irregular = pt.irregular


def _same(r, q, what=""):
    assert np.array_equal(r["spec"].view(np.float32), q["spec"].view(np.float32), equal_nan=True), what
    assert np.array_equal(r["out"], q["out"], equal_nan=True), what


def _cat(rs, axis):
    return dict(spec=np.concatenate([r["spec"] for r in rs], axis=axis), out=np.concatenate([r["out"] for r in rs], axis=axis))


def _bf(fs, xs, N, A, S, gain, pf=None):
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=gain)
    if pf is not None:
        bf.set_postfilter(True, **pf)
    return bf


def _check_against_twin(r, tw, a, what, worst, scale=None):
    """every source of stream a of the GPU result r ([A][S][...]) against the twin's result tw (scale: the keys of the twin whose
    peaks the errors are taken of; the post-filter tests take the unfiltered ones, as tests/test_gpu_mvdr_postfilter.py does)"""
    ks, ka = scale or ("spec", "out")
    for s in range(tw["spec"].shape[0]):
        assert np.all(np.isfinite(r["spec"][a, s])) and np.all(np.isfinite(r["out"][a, s])), (what, a, s)
        es = np.abs(r["spec"][a, s] - tw["spec"][s]).max() / np.abs(tw[ks][s]).max()
        ea = np.abs(r["out"][a, s] - tw["out"][s]).max() / np.abs(tw[ka][s]).max()
        print("%s stream %d source %d: spectra %.2e audio %.2e of the peak" % (what, a, s, es, ea))
        worst[0], worst[1] = max(worst[0], es), max(worst[1], ea)
        assert es <= SPEC_TOL, (what, a, s)
        assert ea <= AUDIO_TOL, (what, a, s)


def _check_covariance(bf, tw, a, what, worst):
    ec = np.abs(bf.covariance(a) - tw["phi"]).max() / np.abs(tw["phi"]).max()
    print("%s stream %d: covariance %.2e" % (what, a, ec))
    worst[2] = max(worst[2], ec)
    assert ec <= COV_TOL, (what, a)


def _two_calls_against_twin(xs, fs, N, F, S, gain, mask, what, pf=None):
    """a fresh context, two calls of F frames (the second continues the recursion and every source's overlap-add) against the twin"""
    A, hop = mask.shape[0], N // 2
    pcm = np.stack([nt.scene(xs, fs, N, 2 * F, a) for a in range(A)])
    doa = nt.drifting_doa(A, 2 * F, S)
    bf = _bf(fs, xs, N, A, S, gain, pf)
    worst = [0.0, 0.0, 0.0]
    state = [None] * A
    for i, (t0, t1) in enumerate([(0, F), (F, 2 * F)]):
        r = bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy(), update_mask=mask[:, t0:t1])
        assert r["out"].shape == (A, S, F * hop) and r["spec"].shape == (A, S, F, N // 2 + 1)
        for a in range(A):
            x = pcm[a, :, t0 * hop:(t1 + 1) * hop].astype(np.float64)
            if pf is None:
                state[a] = mt.mvdr_mask_stream(fs, N, xs, x, doa[a, t0:t1], gain, mask[a, t0:t1], state=state[a])
                _check_against_twin(r, state[a], a, "%s call %d" % (what, i), worst)
            else:
                state[a] = mt.mvdr_mask_postfilter_stream(fs, N, xs, x, doa[a, t0:t1], gain, mask[a, t0:t1], state=state[a], **pf)
                _check_against_twin(r, state[a], a, "%s call %d" % (what, i), worst, ("raw", "raw_out"))
            _check_covariance(bf, state[a], a, "%s call %d" % (what, i), worst)
    # the bin closed throughout is the delay-and-sum still: its covariance is zero, its open neighbour's is not
    K = N // 2 + 1
    if pf is None and K > mt.OPEN_BIN:
        assert not bf.covariance(0)[mt.CLOSED_BIN].any() and bf.covariance(0)[mt.OPEN_BIN].any()
    bf.close()
    print("%s: worst spectra %.2e audio %.2e covariance %.2e" % (what, worst[0], worst[1], worst[2]))


@pytest.mark.parametrize("S,gain", [(1, 0.0), (2, 0.0), (2, 10.0), (4, 0.0), (4, 10.0)])
@pytest.mark.parametrize("M", [2, 3, 4, 5, 8, 11, 13, 16])
def test_mask_every_row_slot_count(M, S, gain):
    """every number of row slots per lane with a full and a partly empty last slot; the plain, the multi-source and the nulling solve"""
    _two_calls_against_twin(_irregular(M), 16000, 256, 6, S, gain, mt.parity_mask(), "M %d S %d gain %g" % (M, S, gain))


@pytest.mark.parametrize("N,fs,F,S,gain", [(1024, 48000, 6, 3, 100.0), (2048, 96000, 4, 4, 0.0)])
def test_mask_long_frames(N, fs, F, S, gain):
    m = mt.mask_for(N // 2 + 1)
    _two_calls_against_twin(synth.ULA16, fs, N, F, S, gain, np.ascontiguousarray(np.concatenate([m[:, :F], m[:, 6:6 + F]], axis=1)), "N %d" % N)


@pytest.mark.parametrize("S,gain", [(1, 0.0), (3, 10.0)])
def test_mask_postfilter_parity(S, gain):
    """the masked solve that emits the noise plane, and the filter behind it, against the masked post-filter twin"""
    _two_calls_against_twin(_irregular(11), 16000, 256, 6, S, gain, mt.parity_mask(), "post-filter S %d" % S, pt.PARITY_PF)


GEOS = {"ula16": (synth.ULA16, 48000, 256, 7), "m13": (_irregular(13), 16000, 256, 6), "five": ([0.0, 0.03, 0.07, 0.10, 0.20], 8000, 256, 9)}


@pytest.mark.parametrize("pf", [None, "postfilter", "floor_one"])
@pytest.mark.parametrize("geo", ["ula16_s1", "m13_s3", "five_s2", "ula16_s4_nulls", "m13_s3_nulls"])
def test_mask_bit_identities(geo, pf):
    """a mask of ones and the NULL mask give the bytes of the unweighted call; a mask that is constant along the bins gives the bytes
    of the per-frame weighted call with those weights (W12 of the gate tests) -- in spectra, audio, covariance, and with the
    post-filter enabled also in the bytes of a follow-up call and of the state blob, which show that A agrees.  gain_floor == 1 under a
    mask gives the bytes of the disabled filter.  Stream 2 stays in digital silence."""
    xs, fs, N, F = GEOS[geo.split("_")[0]]
    S = int(geo.split("_")[1][1])
    gain = 100.0 if geo.endswith("nulls") else 0.0
    A, hop, K = 3, N // 2, N // 2 + 1
    pcm = np.stack([nt.scene(xs, fs, N, 2 * F, a) for a in range(A)])
    pcm[2] = pcm[0] * np.float32(1e-18)
    doa = nt.drifting_doa(A, 2 * F, S)
    w = np.tile(W12[[0, 1, 0]], (1, 2))[:, :2 * F]
    pfc = {None: None, "postfilter": pt.PARITY_PF, "floor_one": dict(smoothing=0.7, gain_floor=1.0, noise_scale=3.0)}[pf]

    def run(kw_of, conf, single=False):
        """two calls; kw_of(t0, t1) -> the update keywords of a call; the second call's bytes and the blob show the carried state"""
        bf = _bf(fs, xs, N, A, S, gain, conf)
        rs = []
        for t0, t1 in ((0, F), (F, 2 * F)):
            x = pcm[:, :, t0 * hop:(t1 + 1) * hop].copy()
            if single:
                r = bf.process(x, doa[:, t0:t1, 0].copy(), want_spec=True, **kw_of(t0, t1))
                r = dict(out=r["out"][:, None], spec=r["spec"][:, None])
            else:
                r = bf.process_sources(x, doa[:, t0:t1].copy(), **kw_of(t0, t1))
            rs.append(r)
        res = _cat(rs, 2), [bf.covariance(a) for a in range(A)], bf.state_save()
        bf.close()
        return res

    def same(x, y, what):
        _same(x[0], y[0], what)
        assert all(np.array_equal(p, q) for p, q in zip(x[1], y[1])), what
        assert x[2] == y[2], what

    for single in ([False, True] if S == 1 else [False]):
        plain = run(lambda t0, t1: {}, pfc, single)
        same(run(lambda t0, t1: dict(update_mask=np.ones((A, t1 - t0, K), dtype=np.float32)), pfc, single), plain, "mask of ones")
        same(run(lambda t0, t1: dict(update_mask=1.0), pfc, single), plain, "scalar 1")
        weighted = run(lambda t0, t1: dict(update=w[:, t0:t1]), pfc, single)
        masked = run(lambda t0, t1: dict(update_mask=np.repeat(w[:, t0:t1, None], K, axis=2)), pfc, single)
        same(masked, weighted, "per-frame constant mask")
        same(run(lambda t0, t1: dict(update_mask=w[:, t0:t1, None]), pfc, single), weighted, "broadcast [A][F][1]")
        assert not np.array_equal(weighted[0]["spec"][:2], plain[0]["spec"][:2])
    if pf == "floor_one":
        m = mt.parity_mask(A, 2 * F)
        same(run(lambda t0, t1: dict(update_mask=m[:, t0:t1]), pfc)[:2] + (b"",), run(lambda t0, t1: dict(update_mask=m[:, t0:t1]), None)[:2] + (b"",),
             "gain_floor 1 under a mask")
    # the NULL pointer through the masked entry points, host and device
    if pf is None:
        import torch
        bf = _bf(fs, xs, N, A, S, gain)
        fp = api._lib.c_fp
        x, dd = pcm[:, :, :(F + 1) * hop].copy(), doa[:, :F].copy()
        ref = bf.process_sources(x, dd)
        cov = [bf.covariance(a) for a in range(A)]
        bf.reset()
        out, spec = np.empty_like(ref["out"]), np.empty_like(ref["spec"])
        bf._check(bf._lib.mca_hip_mvdr_sources_frames_masked_host(bf.h, x.ctypes.data_as(fp), A, F, S, dd.ctypes.data_as(fp), None,
                                                                 out.ctypes.data_as(fp), spec.ctypes.data_as(fp)))
        _same(dict(out=out, spec=spec), ref, "NULL mask, host")
        assert all(np.array_equal(bf.covariance(a), cov[a]) for a in range(A))
        bf.reset()
        tx, td = torch.from_numpy(x).cuda(), torch.from_numpy(dd).cuda()
        to, ts = torch.empty(ref["out"].shape, device="cuda"), torch.empty(ref["spec"].shape + (2,), device="cuda")
        p, sa, sc = api.pcm_layout(tx)
        bf._check(bf._lib.mca_hip_mvdr_sources_frames_masked_dev(bf.h, p, sa, sc, A, F, S, api._ptr(td), None, api._ptr(to), api._ptr(ts), None))
        torch.cuda.synchronize()
        assert np.array_equal(to.cpu().numpy(), ref["out"]) and np.array_equal(ts.cpu().numpy().reshape(-1), ref["spec"].view(np.float32).reshape(-1))
        bf.close()


@pytest.mark.parametrize("M,S,gain", [(16, 1, 0.0), (11, 2, 10.0), (13, 4, 0.0)])
def test_mask_closed_cells_leave_the_covariance(M, S, gain):
    """get_covariance before and after a call, bin by bin: the bins whose cells are all closed (0, NaN, -1, -0.0) are bit-identical,
    every other bin has moved; the closed cells are still beamformed, against the twin"""
    fs, N, F, A = 16000, 256, 5, 2
    xs = _irregular(M)
    hop, K = N // 2, N // 2 + 1
    pcm = np.stack([nt.scene(xs, fs, N, 2 * F, a) for a in range(A)])
    doa = nt.drifting_doa(A, 2 * F, S)
    bf = _bf(fs, xs, N, A, S, gain)
    bf.process_sources(pcm[:, :, :(F + 1) * hop].copy(), doa[:, :F].copy())
    before = [bf.covariance(a) for a in range(A)]
    rng = np.random.default_rng(5)
    mask = rng.choice(np.array([0, 1, .5], dtype=np.float32), size=(A, F, K))
    closed = rng.random((A, K)) < 0.4
    closed[:, 1::2][:, :8] = True                                      # bins 1, 3, ... 15 closed between open ones
    closed[:, 0:16:2] = False
    for a in range(A):
        mask[a][:, closed[a]] = rng.choice(np.array([0.0, np.nan, -1.0, -0.0], dtype=np.float32), size=(F, int(closed[a].sum())))
        mask[a][0, ~closed[a]] = 1.0                                   # every other bin learns at least once
    r = bf.process_sources(pcm[:, :, F * hop:].copy(), doa[:, F:].copy(), update_mask=mask)
    worst = [0.0, 0.0, 0.0]
    for a in range(A):
        after = bf.covariance(a)
        moved = np.array([not np.array_equal(after[k], before[a][k]) for k in range(K)])
        assert np.array_equal(moved, ~closed[a]), (a, np.flatnonzero(moved == closed[a]))
        lead = mt.mvdr_mask_stream(fs, N, xs, pcm[a, :, :(F + 1) * hop].astype(np.float64), doa[a, :F], gain, None)
        tw = mt.mvdr_mask_stream(fs, N, xs, pcm[a, :, F * hop:].astype(np.float64), doa[a, F:], gain, mask[a], state=lead)
        _check_against_twin(r, tw, a, "closed cells", worst)
        _check_covariance(bf, tw, a, "closed cells", worst)
    assert np.abs(r["spec"]).max(axis=3).min() > 0.0


def test_mask_of_zeros_on_a_fresh_context_is_delay_and_sum():
    fs, N, F = 48000, 1024, 6
    xs = synth.ULA8
    pcm = nt.scene(xs, fs, N, F, 1)
    bf = api.MvdrBeamformer(fs, xs, N)
    r = bf.process(pcm, 0.4, want_spec=True, update_mask=np.zeros((1, F, N // 2 + 1), dtype=np.float32))
    X = po.stft_frames(pcm.astype(np.float64), N)
    for t in range(F):
        ref = po.beamformer_process_frame(fs, xs, X[t], float(np.float32(0.4)))
        refc = ref[0::2] + 1j * ref[1::2]
        assert np.abs(r["spec"][0, t] - refc).max() <= 2e-5 * np.abs(refc).max(), t
    assert not bf.covariance(0).any()


@pytest.mark.parametrize("M,S,gain,pf", [(16, 1, 0.0, None), (11, 3, 10.0, None), (8, 2, 0.0, "pf")])
@pytest.mark.parametrize("agree", ["every_other_bin", "bins_0_63"])
def test_mask_column_independence(agree, M, S, gain, pf):
    """two masks that agree on a set of bins and differ at random elsewhere: the spectra and covariance bytes of the agreeing bins
    are equal, whatever the other quads of their waves did"""
    fs, N, F, A = 16000, 256, 12, 2
    xs = _irregular(M)
    K = N // 2 + 1
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    doa = nt.drifting_doa(A, F, S)
    keep = (np.arange(K) % 2 == 0) if agree == "every_other_bin" else (np.arange(K) < 64)
    m1 = mt.parity_mask(A, F)
    m2 = np.random.default_rng(3).choice(np.array([0, 0, 1, .5], dtype=np.float32), size=m1.shape)
    m2[:, :, keep] = m1[:, :, keep]
    res = []
    for m in (m1, m2):
        bf = _bf(fs, xs, N, A, S, gain, pt.PARITY_PF if pf else None)
        r = bf.process_sources(pcm, doa, update_mask=m)
        res.append((r, [bf.covariance(a) for a in range(A)]))
        bf.close()
    (r1, c1), (r2, c2) = res
    assert np.array_equal(np.ascontiguousarray(r1["spec"][..., keep]).view(np.float32), np.ascontiguousarray(r2["spec"][..., keep]).view(np.float32))
    assert not np.array_equal(r1["spec"][..., ~keep], r2["spec"][..., ~keep])
    for a in range(A):
        assert np.array_equal(c1[a][keep], c2[a][keep]) and not np.array_equal(c1[a][~keep], c2[a][~keep])


@pytest.mark.parametrize("M,S,gain", [(16, 1, 0.0), (12, 3, 0.0), (8, 4, 10.0)])
def test_mask_cut_invariance(M, S, gain):
    """12 frames in one call, as 5 + 7 and as 12 calls of one frame: the same bytes"""
    fs, N, F, A = 16000, 256, 12, 2
    xs = _irregular(M)
    hop = N // 2
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    doa = nt.drifting_doa(A, F, S)
    mask = mt.parity_mask(A, F)
    one_bf = _bf(fs, xs, N, A, S, gain)
    one = one_bf.process_sources(pcm, doa, update_mask=mask)
    for cuts in ([0, 5, 12], list(range(13))):
        bf = _bf(fs, xs, N, A, S, gain)
        rs = [bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy(), update_mask=mask[:, t0:t1])
              for t0, t1 in zip(cuts[:-1], cuts[1:])]
        _same(_cat(rs, 2), one, "%d calls" % (len(cuts) - 1))
        for a in range(A):
            assert np.array_equal(bf.covariance(a), one_bf.covariance(a)), a
        bf.close()


def test_mask_pieced_tail_launch():
    """256 streams x 129 bins = 516 solve workgroups: the 4 behind the last whole round go in a second launch cut along the frames
    into pieces; two calls of 8 frames cut theirs differently.  The frames before a piece's own run the same masked recursion."""
    fs, N, F, A, M = 16000, 256, 16, 256, 4
    xs = _irregular(M)
    hop, K = N // 2, N // 2 + 1
    base = np.stack([nt.scene(xs, fs, N, F, a) for a in range(3)])
    pick = np.arange(A) % 3
    pick[255] = 0
    pcm = base[pick]
    doa = nt.drifting_doa(3, F, 1)[pick][:, :, 0].copy()
    mask = np.random.default_rng(7).choice(np.array([0, 0, 1, 1, .5, .125], dtype=np.float32), size=(A, F, K))
    mask[0] = mt.parity_mask(1, F)[0]
    mask[3] = mask[0]
    mask[255, 3:, ::2] = 0
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A)
    one = bf.process(pcm, doa, want_spec=True, update_mask=mask)
    worst = [0.0, 0.0, 0.0]
    for a in (0, 255):
        tw = mt.mvdr_mask_stream(fs, N, xs, pcm[a].astype(np.float64), doa[a], 0.0, mask[a])
        _check_against_twin(dict(spec=one["spec"][:, None], out=one["out"][:, None]), tw, a, "256 streams", worst)
        _check_covariance(bf, tw, a, "256 streams", worst)
    # the same input and mask give the same bytes wherever the stream sits (stream 3: the main launch)
    assert np.array_equal(one["spec"][0], one["spec"][3]) and np.array_equal(bf.covariance(0), bf.covariance(3))
    two_bf = api.MvdrBeamformer(fs, xs, N, max_streams=A)
    r1 = two_bf.process(pcm[:, :, :(8 + 1) * hop].copy(), doa[:, :8].copy(), want_spec=True, update_mask=mask[:, :8])
    r2 = two_bf.process(pcm[:, :, 8 * hop:].copy(), doa[:, 8:].copy(), want_spec=True, update_mask=mask[:, 8:])
    _same(_cat([r1, r2], 1), one, "two calls of 8 frames")
    for a in (0, 1, 2, 254, 255):
        assert np.array_equal(two_bf.covariance(a), bf.covariance(a)), a


def test_mask_sparse_target_scene():
    """the scene of tests/test_mvdr_mask_twin.py from the mixture alone, over the last 24 frames: the twin has the open cells 12.84 dB
    under the delay-and-sum (a frozen fresh context; all ones: 6.41 dB) and the closed cells at 0.866 of it (all ones: 0.095); the
    bars, 9 dB, 0.6 and 4 times the all-ones closed-cell power, are mvdr_mask_twin.assert_mixture_bars"""
    sc = mt.sparse_target_scene()
    bf = api.MvdrBeamformer(mt.SCENE_FS, sc["xs"], mt.SCENE_N)

    def run(u):
        bf.reset()
        return bf.process(sc["pcm"], mt.SCENE_LOOK, want_spec=True, update_mask=u)["spec"][0]
    # the masked run against the twin at the parity bars: the margin of the bars below need not cover fp32
    bf.reset()
    r = bf.process(sc["pcm"], mt.SCENE_LOOK, want_spec=True, update_mask=sc["mask"])
    tw = mt.mvdr_mask_stream(mt.SCENE_FS, mt.SCENE_N, sc["xs"], sc["pcm"].astype(np.float64), np.full(mt.SCENE_F, mt.SCENE_LOOK), 0.0, sc["mask"])
    worst = [0.0, 0.0, 0.0]
    _check_against_twin(dict(spec=r["spec"][:, None], out=r["out"][:, None]), tw, 0, "scene", worst)
    _check_covariance(bf, tw, 0, "scene", worst)
    print("scene: worst spectra %.2e audio %.2e covariance %.2e" % tuple(worst))
    f = mt.mixture_figures(run, sc["mask"])
    print("open cells: masked %.2f dB under the delay-and-sum, all ones %.2f dB; closed cells: masked %.3f of it, all ones %.3f" % f)
    mt.assert_mixture_bars(f)


@pytest.mark.parametrize("S,gain", [(1, 0.0), (3, 100.0)])
def test_mask_dev_entry_under_a_padded_offset_stride(S, gain):
    """the _dev entry with PCM at padded, offset strides in a poisoned allocation equals the contiguous call bit for bit"""
    import torch
    from dev_layout_helpers import guarded, strided_pcm
    fs, N, F, A = 48000, 1024, 6, 2
    xs = synth.ULA8
    hop, K = N // 2, N // 2 + 1
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    doa = nt.drifting_doa(A, F, S)
    mask = mt.mask_for(K, A, F)
    ref_bf = _bf(fs, xs, N, A, S, gain)
    ref = ref_bf.process_sources(pcm, doa, update_mask=mask)
    bf = _bf(fs, xs, N, A, S, gain)
    view, whole = strided_pcm(pcm)
    t_doa, t_m = torch.from_numpy(doa).cuda(), torch.from_numpy(mask).cuda()
    g_out, g_spec = guarded((A, S, F * hop), torch.float32), guarded((A, S, F, K, 2), torch.float32)
    if S == 1:
        bf.process_dev(view, F, t_doa[:, :, 0].contiguous(), out_pcm=g_out.t, out_spec=g_spec.t, update_mask=t_m)
    else:
        bf.process_sources_dev(view, F, t_doa, out_pcm=g_out.t, out_spec=g_spec.t, update_mask=t_m)
    torch.cuda.synchronize()
    g_out.assert_guards_intact("out"); g_spec.assert_guards_intact("spec")
    spec = g_spec.t.cpu().numpy()
    assert np.array_equal(spec.reshape(ref["spec"].shape + (2,)), ref["spec"].view(np.float32).reshape(ref["spec"].shape + (2,)))
    assert np.array_equal(g_out.t.cpu().numpy(), ref["out"])
    for a in range(A):
        assert np.array_equal(bf.covariance(a), ref_bf.covariance(a)), a
    blob = bf.state_save()
    for bad in (t_m[:, :F - 1].contiguous(), t_m[:, :, :K - 1].contiguous(), t_m[:, :, ::2], t_m.double()):
        with pytest.raises(api.MCArrayHipError, match="update_mask"):
            bf.process_sources_dev(view, F, t_doa, out_pcm=g_out.t, update_mask=bad)
    with pytest.raises(api.MCArrayHipError, match="not combined"):
        bf.process_sources_dev(view, F, t_doa, out_pcm=g_out.t, update_mask=t_m, update=t_m[:, :, 0].contiguous())
    assert bf.state_save() == blob


def test_mask_refusals_leave_the_state():
    fs, N, F, A = 16000, 256, 4, 2
    xs = synth.REEM_C
    K = N // 2 + 1
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    m = mt.parity_mask(A, F)
    bf = _bf(fs, xs, N, A, 2, 0.0, pt.PARITY_PF)
    bf.process_sources(pcm, nt.drifting_doa(A, F, 2), update_mask=m)
    before, blob = [bf.covariance(a) for a in range(A)], bf.state_save()
    with pytest.raises(api.MCArrayHipError, match="n_sources"):
        bf.process_sources(pcm, nt.drifting_doa(A, F, 3), update_mask=m)          # above the context's maximum
    with pytest.raises(api.MCArrayHipError, match="both NULL"):
        bf.process_sources(pcm, nt.drifting_doa(A, F, 2), want_audio=False, want_spec=False, update_mask=m)
    with pytest.raises(api.MCArrayHipError, match="update_mask"):
        bf.process_sources(pcm, nt.drifting_doa(A, F, 2), update_mask=np.ones((A, F, K + 1), dtype=np.float32))
    with pytest.raises(api.MCArrayHipError, match="update_mask"):
        bf.process(pcm, 0.3, update_mask=np.ones((A, F + 1, K), dtype=np.float32))
    with pytest.raises(api.MCArrayHipError, match="not combined"):
        bf.process_sources(pcm, nt.drifting_doa(A, F, 2), update=np.ones((A, F), dtype=np.float32), update_mask=m)
    with pytest.raises(api.MCArrayHipError, match="not combined"):
        bf.process(pcm, 0.3, update=1.0, update_mask=m)
    for a in range(A):
        assert np.array_equal(bf.covariance(a), before[a]), a
    assert bf.state_save() == blob


def test_mask_results_do_not_move_beside_a_matrix_core_neighbour():
    """the masked solve kernel beside the neighbour of tests/test_gpu_coresidency.py (the procedure of its module test, as
    tests/test_gpu_mvdr_gate.py runs it): 16 microphones, a mask whose quads diverge"""
    import ctypes as C
    import time
    import torch
    import test_gpu_coresidency as tc
    nb = tc._neighbour()
    dev = torch.device("cuda:0")
    F, A, N, xs = 60, 16, 1024, synth.ULA16
    pcm = np.stack([synth.noise_source_stream(xs, np.deg2rad(20.0 - 7 * a), 48000, (F + 1) * N // 2, 80 + a) for a in range(A)]).astype(np.float32)
    doa = (np.deg2rad(20.0 - 7 * np.arange(A))[:, None] + 0.01 * np.arange(F)[None, :]).astype(np.float32)
    mask = np.ascontiguousarray(np.tile(mt.mask_for(N // 2 + 1, 2, 12), (A // 2, F // 12, 1)))

    def fn():
        bf = api.MvdrBeamformer(48000, xs, N, max_streams=A)
        r = bf.process(pcm, doa, want_spec=True, update_mask=mask)
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
