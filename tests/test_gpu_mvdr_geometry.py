"""GPU: the XYZ geometry of the MVDR context (mca_hip_mvdr_set_geometry) against tests/mvdr_geometry_twin.py.

Bars: the module's own -- 5e-4 of the peak for spectra and audio, 5e-6 for the covariance, 5e-4 of the row's maximum for the Capon
spectrum and the own spectrum of a track.  The float32 half of the tracks is compared with array_equal.  Every test prints its worst
figure.  On an MI355X the parity cases stay under 1.24e-4 (spectra), 1.04e-4 (audio) and 2.94e-7 (covariance) of the peak, the
spectrum rows under 2.5e-6 and the own spectra under 1e-7 of the row's maximum (DESIGN.md 4.12 has the table)."""
import numpy as np
import pytest

from mcarray_amd import api, synth
from oracle import np_twin

import mvdr_estmask_twin as et
import mvdr_geometry_twin as gt
import mvdr_mask_twin as mt
import mvdr_nulls_twin as nt
import mvdr_rtf_twin as rt
import mvdr_spectrum_twin as sp
import mvdr_tracks_twin as tt

pytestmark = pytest.mark.gpu

SPEC_TOL, AUDIO_TOL, COV_TOL, ROW_TOL = 5e-4, 5e-4, 5e-6, 5e-4
FS, N = 16000, 256
F32 = np.float32


def _torch():
    import torch
    return torch


def _pcm(xyz, fs, n_fft, F, A=2, elevation=0.0):
    """[A][M][(F+1) hop]: two talkers per stream, in front of and behind the array"""
    return np.stack([gt.two_sources_xyz(xyz, fs, n_fft, F, 2.6 - 1.7 * a, -0.9 + 2.2 * a, seed=a, elevation=elevation) for a in range(A)])


def _same(r, q, what):
    assert np.array_equal(r["spec"].view(F32), q["spec"].view(F32), equal_nan=True), what
    assert np.array_equal(r["out"], q["out"], equal_nan=True), what


# ---- 1. bytes: XYZ on the x axis is LINEAR_X ----
@pytest.mark.parametrize("M", [3, 8, 16])
def test_xyz_on_the_x_axis_has_the_bytes_of_linear_x(M):
    """microphones at negative, zero and positive x, look directions over the whole circle and beyond: a sources call with three
    directions and null gain 10, the auto call with RTF, mask estimator and RTF nulls, covariance() and steering()"""
    xs = (np.asarray(synth.ULA16[:M]) - 0.02).tolist()
    assert min(xs) < 0 < max(xs) and 0.0 in xs
    A, S, F, hop = 2, 3, 6, N // 2
    pcm = np.stack([nt.scene(xs, FS, N, 2 * F, a) for a in range(A)])
    doa = gt.drifting_azimuths(A, 2 * F, S)
    res = []
    for mode in ("linear_x", "xyz"):
        bf = api.MvdrBeamformer(FS, xs, N, max_streams=A, max_sources=S, null_gain=10.0, geometry=mode)
        assert bf.get_geometry() == dict(mode=mode, elevation_rad=0.0)
        r1 = bf.process_sources(pcm[:, :, :(F + 1) * hop].copy(), doa[:, :F].copy())
        cov1 = np.stack([bf.covariance(a) for a in range(A)])
        bf.set_rtf(True, **rt.parity_config(M))
        bf.set_mask_estimator(True, **et.parity_config(N, S, 1))
        bf.set_rtf_nulls(True)
        r2 = bf.process_sources(pcm[:, :, F * hop:].copy(), doa[:, F:].copy(), estimate_masks=True)
        cov2 = np.stack([bf.covariance(a) for a in range(A)])
        steer = [bf.steering(th, a, s) for a in range(A) for s in range(S) for th in (0.3, 2.9, -4.0)]
        res.append((r1, cov1, r2, cov2, steer))
        bf.close()
    lin, xyz = res
    _same(lin[0], xyz[0], "sources call")
    _same(lin[2], xyz[2], "auto call")
    assert np.array_equal(lin[2]["update_mask"], xyz[2]["update_mask"]) and np.array_equal(lin[2]["target_mask"], xyz[2]["target_mask"])
    assert np.array_equal(lin[1], xyz[1]) and np.array_equal(lin[3], xyz[3])
    n_est = 0
    for (d0, e0), (d1, e1) in zip(lin[4], xyz[4]):
        assert np.array_equal(d0, d1) and np.array_equal(e0, e1)
        n_est += int(e0.sum())
    assert n_est > 0 and np.abs(lin[0]["out"]).max() > 0
    print("M %d: sources call, auto call, covariance and steering() byte-identical; %d estimated steering cells" % (M, n_est))


# ---- 2. parity with the twin on planar and 3-D arrays ----
def _err(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def _check(r, tw, a, what, worst):
    es, ea = _err(r["spec"][a], tw["spec"]), _err(r["out"][a], tw["out"])
    worst[0], worst[1] = max(worst[0], es), max(worst[1], ea)
    assert np.all(np.isfinite(r["spec"][a])) and np.all(np.isfinite(r["out"][a]))
    assert es <= SPEC_TOL and ea <= AUDIO_TOL, (what, a, es, ea)


ARRAYS = {"uca4": (lambda: synth.uca(4, 0.045), 0.0), "uca6": (lambda: synth.uca(6, 0.045), 0.0), "uca11": (lambda: synth.uca(11, 0.045), 0.0),
          "uca16": (lambda: synth.uca(16, 0.045), 0.0), "cube7_el0.4": (lambda: gt.array_3d(7), 0.4)}


@pytest.mark.parametrize("name", list(ARRAYS))
def test_parity_on_planar_and_3d_arrays(name):
    """look directions that drift per frame round the whole circle, values outside [-pi, pi] among them: the single look, three
    directions with null gain 10, the masked call and the RTF call (two calls, the second continuing the first)"""
    from test_gpu_mvdr_rtf import _check_call
    xyz, el = ARRAYS[name][0](), ARRAYS[name][1]
    M, A, S, F, hop, K = len(xyz), 2, 3, rt.PARITY_F, N // 2, N // 2 + 1
    pcm = _pcm(xyz, FS, N, 2 * F, A, el)
    doa = gt.drifting_azimuths(A, 2 * F, S)
    assert doa.max() > np.pi and doa.min() < -np.pi
    pcm64 = pcm.astype(np.float64)
    worst = {}
    # single look and S = 3 with nulls
    for label, s_n, gain in (("single", 1, 0.0), ("nulls", 3, 10.0)):
        w = worst[label] = [0.0, 0.0, 0.0]
        bf = api.MvdrBeamformer(FS, xyz, N, max_streams=A, max_sources=s_n, null_gain=gain, geometry="xyz", elevation_rad=el)
        r = bf.process_sources(pcm[:, :, :(F + 1) * hop].copy(), doa[:, :F, :s_n].copy())
        for a in range(A):
            with gt.xyz_mode(el):
                tw = nt.mvdr_nulls_stream(FS, N, xyz, pcm64[a, :, :(F + 1) * hop], doa[a, :F, :s_n], gain)
            _check(r, tw, a, (name, label), w)
            w[2] = max(w[2], _err(bf.covariance(a), tw["phi"]))
        assert w[2] <= COV_TOL, (name, label, w)
        bf.close()
    # the masked call
    w = worst["masked"] = [0.0, 0.0, 0.0]
    upd = np.ascontiguousarray(mt.mask_for(K, A, 12)[:, :F])
    bf = api.MvdrBeamformer(FS, xyz, N, max_streams=A, max_sources=2, null_gain=10.0, geometry="xyz", elevation_rad=el)
    r = bf.process_sources(pcm[:, :, :(F + 1) * hop].copy(), doa[:, :F, :2].copy(), update_mask=upd)
    for a in range(A):
        with gt.xyz_mode(el):
            tw = mt.mvdr_mask_stream(FS, N, xyz, pcm64[a, :, :(F + 1) * hop], doa[a, :F, :2], 10.0, upd[a])
        _check(r, tw, a, (name, "masked"), w)
        w[2] = max(w[2], _err(bf.covariance(a), tw["phi"]))
    assert w[2] <= COV_TOL, (name, "masked", w)
    bf.close()
    # the RTF call: cells at a decision edge of the twin's estimator are left out, as in tests/test_gpu_mvdr_rtf.py
    w = worst["rtf"] = [0.0, 0.0, 0.0, 0.0]
    cfg = rt.parity_config(M)
    upd2 = np.ascontiguousarray(np.concatenate([mt.mask_for(K, A, 12)[:, :F], mt.mask_for(K, A, 12)[:, 6:6 + F]], axis=1))
    tm = rt.target_parity_mask(2, A, 12, K)
    tmask = np.ascontiguousarray(np.concatenate([tm[:, :, :F], tm[:, :, 6:6 + F]], axis=2))
    bf = api.MvdrBeamformer(FS, xyz, N, max_streams=A, max_sources=2, geometry="xyz", elevation_rad=el)
    bf.set_rtf(True, **cfg)
    prev, st, shares = [np.zeros((2, hop)) for _ in range(A)], [None] * A, []
    for i, (t0, t1) in enumerate(((0, F), (F, 2 * F))):
        r = bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1, :2].copy(), update_mask=upd2[:, t0:t1], target_mask=tmask[:, :, t0:t1])
        for a in range(A):
            with gt.xyz_mode(el):
                st[a] = rt.mvdr_rtf_stream(FS, N, xyz, pcm64[a, :, t0 * hop:(t1 + 1) * hop], doa[a, t0:t1, :2], upd2[a, t0:t1], tmask[a, :, t0:t1],
                                           state=st[a], **cfg)
            prev[a] = _check_call(r, st[a], a, "%s rtf call %d" % (name, i), w, prev[a], None)
            w[2] = max(w[2], _err(bf.covariance(a), st[a]["phi"]))
            shares.append(float(rt.edges_of(st[a]).mean()))
            assert st[a]["est"].any()
    assert w[2] <= COV_TOL and max(shares) <= 0.01, (name, "rtf", w, shares)
    bf.close()
    for label, w in worst.items():
        print("%s %s: spectra %.2e audio %.2e of the peak, covariance %.2e" % (name, label, w[0], w[1], w[2]))


@pytest.mark.parametrize("n_fft", [512, 1024])
def test_parity_long_frames(n_fft):
    """k_mvdr_analyse_512 and k_mvdr_analyse_1024 form an XYZ table: three directions with null gain 10, four frames"""
    fs, xyz, A, S, F, hop = 48000, synth.uca(8, 0.05), 2, 3, 4, n_fft // 2
    pcm = _pcm(xyz, fs, n_fft, F, A)
    doa = gt.drifting_azimuths(A, F, S)
    bf = api.MvdrBeamformer(fs, xyz, n_fft, max_streams=A, max_sources=S, null_gain=10.0, geometry="xyz")
    r = bf.process_sources(pcm, doa)
    w = [0.0, 0.0, 0.0]
    for a in range(A):
        with gt.xyz_mode():
            tw = nt.mvdr_nulls_stream(fs, n_fft, xyz, pcm[a].astype(np.float64), doa[a], 10.0)
        _check(r, tw, a, n_fft, w)
        w[2] = max(w[2], _err(bf.covariance(a), tw["phi"]))
    bf.close()
    print("uca8 N %d nulls: spectra %.2e audio %.2e of the peak, covariance %.2e" % (n_fft, w[0], w[1], w[2]))
    assert w[2] <= COV_TOL


# ---- 3. the spectrum on the periodic grid ----
def _scene_context(sc, n_peaks=gt.SCENE_PEAKS, D=gt.SCENE_D):
    bf = api.MvdrBeamformer(gt.SCENE_FS, sc["xyz"], gt.SCENE_N, max_streams=1, geometry="xyz")
    bf.process(sc["pcm"][None], np.zeros((1, gt.SCENE_F), dtype=F32))
    bf.configure_spectrum(D, gt.SCENE_BAND[0], gt.SCENE_BAND[1], n_peaks=n_peaks)
    return bf


@pytest.mark.parametrize("D", [3, 64, 65, 360])
def test_spectrum_rows_and_grid(D):
    sc = gt.named_scene("back")
    bf = _scene_context(sc, 1, D)
    assert np.array_equal(bf.spectrum_grid(), gt.grid_xyz(D).astype(F32))
    worst = 0.0
    for weighting, kind in (("normalised", sp.NORMALISED), ("power", sp.POWER)):
        bf.configure_spectrum(D, gt.SCENE_BAND[0], gt.SCENE_BAND[1], weighting=weighting)
        got = bf.spectrum()["spectrum"][0]
        with gt.xyz_mode():
            P = sp.spectrum(bf.covariance(0), gt.SCENE_FS, gt.SCENE_N, sc["xyz"], D, gt.SCENE_BAND[0], gt.SCENE_BAND[1], kind)
        e = float(np.abs(got - P).max() / P.max())
        worst = max(worst, e)
        assert e <= ROW_TOL, (D, weighting, e)
    bf.close()
    print("D %d: spectrum rows %.2e of the row's maximum" % (D, worst))


@pytest.mark.parametrize("name", ["seam_last", "seam_first", "back"])
def test_spectrum_peaks_across_the_seam(name):
    """the scenes of tests/test_mvdr_geometry_twin.py, whose three compared peaks clear ten times the bar: peak_doa is the twin's grid
    point in every slot, peak_val within the bar"""
    sc = gt.named_scene(name)
    bf = _scene_context(sc)
    got = bf.spectrum()
    idx, doa, val = gt.peaks_circular(sc["P"], gt.SCENE_PEAKS)
    e = float(np.abs(got["spectrum"][0] - sc["P"]).max() / sc["P"].max())
    ev = float(np.abs(got["peak_val"][0] - val).max() / sc["P"].max())
    print("%s: peaks at grid points %s; row %.2e, peak values %.2e of the row's maximum" % (name, idx.tolist(), e, ev))
    assert np.array_equal(got["peak_doa"][0], doa), (got["peak_doa"][0], doa)
    assert e <= ROW_TOL and ev <= ROW_TOL
    bf.close()


# ---- 4. the tracks on the circle ----
def _pad(tr):
    out = {}
    for k, v in tr.items():
        out[k] = np.zeros((v.shape[0], tt.MAX_SLOTS), dtype=v.dtype)
        out[k][:, :v.shape[1]] = v
    return out


def _track_context(A, n_tracks, n_own, cfg, D=72):
    bf = api.MvdrBeamformer(FS, synth.uca(4, 0.045), 64, max_streams=A, max_sources=4, geometry="xyz")
    bf.set_rtf(True)
    bf.configure_spectrum(D, 1, 30)
    bf.configure_tracks(n_tracks, n_own, **cfg)
    return bf


def test_association_seam_cases():
    """the cases of tests/test_mvdr_geometry_twin.py, one per stream"""
    torch = _torch()
    cfg = dict(max_step_rad=0.2, min_sep_rad=0.1, hold=3)
    nan = np.nan
    # (seeds [2], own_doa [1], candidate, n_own)
    cases = [([3.10, nan], [nan], -3.10, 0), ([3.12, nan], [3.62], 0.0, 1), ([3.12, nan], [3.62 - 2 * np.pi], 0.0, 1), ([3.12, nan], [nan], -3.13, 1),
             ([7.0, -4.0], [nan], 7.1, 0), ([-3.12, nan], [-3.5], 0.0, 1)]
    for n_own in (0, 1):
        sel = [c for c in cases if c[3] == n_own]
        A = len(sel)
        bf = _track_context(A, 2, n_own, cfg)
        seeds = np.array([c[0] for c in sel], dtype=F32)
        own = np.array([c[1] for c in sel], dtype=F32)
        cd = np.array([[c[2]] for c in sel], dtype=F32)
        cv = np.array([[1.0 if c[2] != 0.0 else 0.0] for c in sel], dtype=F32)
        bf.seed_tracks(seeds)
        sts = [gt.seed_circular(tt.new_state(), seeds[a]) for a in range(A)]
        bf.associate_tracks_dev(A, torch.from_numpy(own).cuda() if n_own else None, torch.from_numpy(cd).cuda(), torch.from_numpy(cv).cuda())
        for a in range(A):
            gt.associate_circular(sts[a], own[a, :n_own], cd[a], cv[a], 2, n_own, **cfg)
        got = _pad(bf.tracks())
        for k in ("theta", "alive", "miss", "gen"):
            assert np.array_equal(got[k], np.stack([st[k] for st in sts])), (n_own, k, got[k])
        assert np.all(np.abs(got["theta"]) <= gt.PI_F)
        print("n_own %d: theta %s alive %s" % (n_own, got["theta"][:, :2].tolist(), got["alive"][:, :2].tolist()))
        bf.close()


@pytest.mark.parametrize("n_tracks,n_own", [(2, 1), (4, 0), (4, 2)])
def test_association_against_the_twin_on_the_circle(n_tracks, n_own):
    """associate_dev on 300 random streams, three rounds: angles from a grid of 1/16 rad over +-4.5 rad (ties in distance and at the gates
    are common, both sides of the seam and beyond it), NaNs and zeros as in tests/test_gpu_mvdr_tracks.py"""
    torch = _torch()
    A = 300
    rng = np.random.default_rng(10 * n_tracks + n_own)
    cfg = dict(max_step_rad=0.25, min_sep_rad=0.125, hold=1)
    bf = _track_context(A, n_tracks, n_own, cfg)

    def angles(shape, p_nan):
        v = (rng.integers(-72, 73, shape) / 16.0).astype(F32)
        v[rng.random(shape) < p_nan] = np.nan
        return v
    seeds = angles((A, n_tracks), 0.3)
    bf.seed_tracks(seeds)
    sts = [gt.seed_circular(tt.new_state(), seeds[a]) for a in range(A)]
    lin = [gt.seed_circular(tt.new_state(), seeds[a]) for a in range(A)]      # the association that does not wrap, on the same inputs
    for rnd, n_cand in enumerate((8, 2, 3)):
        own = angles((A, max(n_own, 1)), 0.2)[:, :n_own]
        cd = angles((A, n_cand), 0.1)
        cv = rng.choice(F32([1.0, 0.5, 0.0, np.nan, 2.0]), (A, n_cand), p=[0.4, 0.3, 0.1, 0.05, 0.15]).astype(F32)
        t_own = torch.from_numpy(np.ascontiguousarray(own)).cuda() if n_own else None
        bf.associate_tracks_dev(A, t_own, torch.from_numpy(cd).cuda(), torch.from_numpy(cv).cuda())
        for a in range(A):
            gt.associate_circular(sts[a], own[a], cd[a], cv[a], n_tracks, n_own, **cfg)
            gt.associate_circular(lin[a], own[a], cd[a], cv[a], n_tracks, n_own, circular=False, **cfg)
        got = _pad(bf.tracks())
        for k in ("theta", "alive", "miss", "gen"):
            want = np.stack([st[k] for st in sts])
            assert np.array_equal(got[k], want, equal_nan=True), (rnd, k, np.flatnonzero((got[k] != want).any(axis=1))[:5])
        assert np.all(np.abs(got["theta"]) <= gt.PI_F)
    # the wrap matters on these inputs: the association that does not wrap ends elsewhere
    n_diff = sum(int(not np.array_equal(lin[a]["alive"], sts[a]["alive"]) or not np.array_equal(lin[a]["gen"], sts[a]["gen"])) for a in range(A))
    print("n_tracks %d n_own %d: the association that does not wrap ends with other slots alive or born in %d of %d streams" % (n_tracks, n_own, n_diff, A))
    assert n_diff > 0
    bf.close()


def test_update_with_an_own_window_across_the_seam_and_a_loop_over_it():
    """uca(8, 0.05), a talker that crosses theta = pi over three chunks and an interferer.  Per chunk: the auto call with the look
    directions the tracks fill in, then one update.  The own spectrum is the twin's on the state the GPU holds, within the bar; the
    own track (whose search window straddles the seam from the first chunk on) moves to the twin's window maximum wherever that stands
    5e-3 clear, by the twin's circular association; it ends on the other side of the seam.  (On the float64 twin alone the three window
    maxima stand 3.0e-2 ... 4.0e-2 clear and the track goes 3.054 -> 3.1416 -> -3.054 rad.)"""
    torch = _torch()
    xyz, M, A, S, F, D, hop, K = synth.uca(8, 0.05), 8, 1, 2, 12, 72, N // 2, N // 2 + 1
    truth, itf = [3.05, -3.05, -2.85], -1.0
    n = (F + 1) * hop
    chunks = []
    for c, th in enumerate(truth):
        full = (synth.noise_source_stream_xyz(xyz, th, FS, 3 * F * hop + hop, 4, sigma=0.3).astype(np.float64)
                + synth.noise_source_stream_xyz(xyz, itf, FS, 3 * F * hop + hop, 3, snr_db=60).astype(np.float64))
        chunks.append(full[:, c * F * hop:c * F * hop + n].astype(F32))
    rtf = dict(target_alpha=0.5, iterations=2, ref_mic=0, min_share=0.05)
    em = et.parity_config(N, S, 1)
    trk = dict(n_tracks=2, n_own=1, max_step_rad=0.3, min_sep_rad=0.2, hold=3)
    band = (4, 124)
    bf = api.MvdrBeamformer(FS, xyz, N, max_streams=A, max_sources=S, geometry="xyz")
    bf.set_rtf(True, **rtf)
    bf.set_mask_estimator(True, **em)
    bf.configure_spectrum(D, band[0], band[1], n_peaks=2)
    bf.configure_tracks(**trk)
    seeds = F32([[truth[0] - 0.1, itf]])
    bf.seed_tracks(seeds)
    st = gt.seed_circular(tt.new_state(), seeds[0])
    g32 = gt.grid_xyz(D).astype(F32)
    kw = dict(iterations=rtf["iterations"], ref_mic=rtf["ref_mic"], min_share=rtf["min_share"])
    worst, n_cmp, thetas = 0.0, 0, []
    for c in range(3):
        doa = torch.empty((A, F, S), dtype=torch.float32, device="cuda")
        bf.fill_tracks_dev(A, F, doa)
        torch.cuda.synchronize()
        rows = doa.cpu().numpy()
        assert np.array_equal(rows[0], np.repeat(tt.fill(st, 2)[None], F, axis=0))
        bf.process_sources(chunks[c][None], rows, estimate_masks=True)
        theta0 = st["theta"][0]
        assert abs(gt.wrap32(F32(theta0 - gt.reduce32(truth[c])))) <= trk["max_step_rad"] + 0.1
        r = bf.update_tracks(want_spectrum=True)
        psi, cpsi = bf.target_covariance(0, 0)
        cphi = np.frombuffer(bf.state_save()[-A * K * 4:], dtype=F32).reshape(A, K).astype(np.float64)[0]
        with gt.xyz_mode():
            args = (FS, N, xyz, D) + band + (psi, cpsi, bf.covariance(0), cphi, theta0)
            tw = tt.own_spectrum(*args, **kw)
            gu, gs = r["own_used"][0, 0], r["own_spectrum"][0, 0]
            assert np.array_equal(gu[~tw["edge"]], tw["used"][~tw["edge"]])
            if (gu != tw["used"]).any():
                tw = tt.own_spectrum(*args, used=np.where(tw["edge"], gu, tw["used"]), **kw)
            P = sp.spectrum(bf.covariance(0), FS, N, xyz, D, band[0], band[1], sp.NORMALISED)
        top = tw["T"].max()
        assert top > 0
        e = float(np.abs(gs - tw["T"]).max() / top)
        worst = max(worst, e)
        assert e <= ROW_TOL, (c, e)
        pk = bf.spectrum()
        assert float(np.abs(pk["spectrum"][0] - P).max() / P.max()) <= ROW_TOL
        win = np.array([abs(gt.wrap32(F32(g - theta0))) <= F32(trk["max_step_rad"]) for g in g32])
        assert win[0] or win[-1] or c == 0, "the window straddles the seam"
        v = np.sort(tw["T"][win])[::-1]
        clear = (v[0] - v[1]) / top
        phi_tw = gt.window_argmax_circular(tw["T"], g32, theta0, trk["max_step_rad"])[0]
        got = _pad(bf.tracks())
        if clear >= 5e-3:
            gt.associate_circular(st, [phi_tw], pk["peak_doa"][0], pk["peak_val"][0], **trk)
            for k in ("theta", "alive", "miss", "gen"):
                assert np.array_equal(got[k][0], st[k]), (c, k, got[k][0], st[k])
            n_cmp += 1
        else:                                              # (not compared: the twin goes on from what the GPU holds)
            for k in ("theta", "alive", "miss", "gen"):
                st[k][:] = got[k][0]
        thetas.append(float(got["theta"][0, 0]))
        assert abs(got["theta"][0, 0]) <= gt.PI_F
    bf.close()
    print("own track per chunk %s (truth %s); own spectra %.2e of the row's maximum; %d of 3 updates compared" % (np.round(thetas, 3).tolist(), truth, worst, n_cmp))
    assert n_cmp > 0
    # (the track lags the talker by Psi's memory, as in DESIGN.md 4.11: it is on the talker's side of the seam, within a step of it)
    assert thetas[0] > 0 > thetas[-1] and abs(gt.wrap32(F32(thetas[-1]) - F32(truth[-1]))) <= trk["max_step_rad"]


# ---- 5. behaviour of the setter ----
def test_setter_refusals_changes_and_state_blobs():
    xyz, A, S, F, hop = synth.uca(6, 0.045), 2, 2, 4, N // 2
    pcm = _pcm(xyz, FS, N, 2 * F, A)
    doa = gt.drifting_azimuths(A, 2 * F, S)
    first, second = (pcm[:, :, :(F + 1) * hop].copy(), doa[:, :F].copy()), (pcm[:, :, F * hop:].copy(), doa[:, F:].copy())

    def fresh(mode, el=0.0):
        bf = api.MvdrBeamformer(FS, xyz, N, max_streams=A, max_sources=S, geometry=mode, elevation_rad=el)
        bf.set_rtf(True)
        return bf
    ref = fresh("xyz", 0.3)
    ref.process_sources(*first)
    want = ref.process_sources(*second)
    bf = fresh("xyz", 0.3)
    bf.process_sources(*first)
    blob1 = bf.state_save()
    assert bf.get_geometry() == dict(mode="xyz", elevation_rad=0.3)
    # refusals leave get_geometry and the next call's bytes as they were
    import ctypes as C
    from mcarray_amd import _lib
    bad = [(2, 0.0, 16), (-1, 0.0, 16), (1, np.nan, 16), (1, np.inf, 16), (1, -np.inf, 16), (1, 1.6, 16), (1, -1.6, 16), (0, np.nan, 16), (1, 0.1, 12), (1, 0.1, 24)]
    for mode, el, size in bad:
        cfg = _lib.MvdrGeometryConfig(size, mode, el)
        assert bf._lib.mca_hip_mvdr_set_geometry(bf.h, C.byref(cfg)) == -1, (mode, el, size)
        assert bf.get_geometry() == dict(mode="xyz", elevation_rad=0.3)
    with pytest.raises(api.MCArrayHipError):
        bf.set_geometry(2)
    assert bf._lib.mca_hip_mvdr_set_geometry(bf.h, None) == -1
    _same(bf.process_sources(*second), want, "after the refusals")
    # a change un-configures the spectrum and disables the tracks; the same values twice change nothing
    bf.configure_spectrum(72, 1, 127, n_peaks=2)
    bf.configure_tracks(2, 1)
    bf.set_geometry("xyz", 0.3)
    assert bf.spectrum_config is not None and bf.get_tracks_config()["enable"] and bf.spectrum()["spectrum"].shape == (A, 72)
    cov = [bf.covariance(a) for a in range(A)]
    blob = bf.state_save()
    bf.set_geometry("xyz", 0.2)
    assert bf.get_geometry() == dict(mode="xyz", elevation_rad=0.2)
    assert bf.spectrum_config is None and not bf.get_tracks_config()["enable"]
    for call in (bf.spectrum, bf.tracks, bf.update_tracks, lambda: bf.seed_tracks([[0.0, 0.0]] * A), bf.spectrum_grid):
        with pytest.raises(api.MCArrayHipError):
            call()
    assert all(np.array_equal(bf.covariance(a), cov[a]) for a in range(A)) and bf.state_save() == blob
    bf.configure_spectrum(72, 1, 127, n_peaks=2)
    bf.configure_tracks(2, 1)
    assert bf.spectrum()["spectrum"].shape == (A, 72)
    bf.set_geometry("linear_x", 0.9)                   # LINEAR_X ignores the elevation
    assert bf.get_geometry() == dict(mode="linear_x", elevation_rad=0.0) and bf.spectrum_config is None
    bf.configure_spectrum(61, 1, 127)
    assert np.array_equal(bf.spectrum_grid(), sp.grid(61).astype(F32))
    bf.set_geometry("linear_x", -0.4)                  # nothing changes: the spectrum stays configured
    assert bf.spectrum_config is not None and bf.spectrum()["spectrum"].shape == (A, 61)
    bf.set_geometry("xyz")
    with pytest.raises(api.MCArrayHipError):
        bf.configure_spectrum(2, 1, 127)               # the periodic grid needs three angles
    bf.configure_spectrum(3, 1, 127)
    bf.close()
    # a state blob saved in one mode loads in the other, and the stream goes on with the other mode's bytes
    other = fresh("linear_x")
    other.state_load(blob1)
    other.set_geometry("xyz", 0.3)
    assert other.state_save() == blob1
    _same(other.process_sources(*second), want, "blob across the modes")
    other.close()
    ref.close()
    print("refusals (%d), no-ops, un-configuring and state blobs across the modes: as specified" % len(bad))
