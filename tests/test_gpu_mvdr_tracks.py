"""GPU: the tracks of the look directions of the MVDR context (mca_hip_mvdr_tracks_*) against tests/mvdr_tracks_twin.py.

The association is float32 on both sides, operation for operation: theta, alive, miss and gen are compared with array_equal.  The own
spectrum is compared with the float64 twin evaluated on the state the GPU holds (covariance(), target_covariance(), cphi from the
state blob), at the module's bar of 5e-4 of the row's maximum; at the bins the twin flags as decision edges of the estimator
(mvdr_rtf_twin.edge_cells; at most 1 % of the cells, tests/test_mvdr_tracks_twin.py) the twin takes the GPU's flags."""
import ctypes as C

import numpy as np
import pytest

from mcarray_amd import _lib, api, synth

import mvdr_estmask_twin as et
import mvdr_tracks_twin as tt

pytestmark = pytest.mark.gpu

SPEC_TOL = 5e-4
SCENE_SHARE_BAR = 5e-4      # the module's parity, of the twin's share
FS, N = tt.FS, tt.N
K, HOP = N // 2 + 1, N // 2


def _torch():
    import torch
    return torch


def _pad(tr):
    """tracks() [A][n_tracks] -> the twin's [A][4] layout"""
    out = {}
    for k, v in tr.items():
        out[k] = np.zeros((v.shape[0], tt.MAX_SLOTS), dtype=v.dtype)
        out[k][:, :v.shape[1]] = v
    return out


def _cphi(bf, A):
    """cphi [A][K] of an RTF context: the last part of its state blob"""
    return np.frombuffer(bf.state_save()[-A * bf.K * 4:], dtype=np.float32).reshape(A, bf.K).astype(np.float64)


@pytest.mark.parametrize("n_tracks,n_own", [(1, 0), (1, 1), (2, 1), (3, 0), (3, 2), (4, 0), (4, 1), (4, 2)])
def test_association_against_the_twin(n_tracks, n_own):
    """associate_dev on 300 random streams, three rounds with 1 ... 8 candidates: angles from a grid of 1/16 rad (ties in distance and at
    the gates are common), NaNs among the seeds, the own directions, the candidates and their values, values of 0"""
    torch = _torch()
    A = 300
    rng = np.random.default_rng(100 * n_tracks + n_own)
    bf = api.MvdrBeamformer(FS, synth.ULA8[:4], 64, max_streams=A, max_sources=4)
    bf.set_rtf(True)
    bf.configure_spectrum(31, 1, 30)
    cfg = dict(max_step_rad=0.25, min_sep_rad=0.125, hold=1)
    bf.configure_tracks(n_tracks, n_own, **cfg)
    assert bf.get_tracks_config() == dict(enable=True, n_tracks=n_tracks, n_own=n_own, **cfg)
    z = bf.tracks()
    assert all(not z[k].any() for k in z)

    def angles(shape, p_nan):
        v = (rng.integers(-24, 25, shape) / 16.0).astype(np.float32)
        v[rng.random(shape) < p_nan] = np.nan
        return v
    seeds = angles((A, n_tracks), 0.3)
    bf.seed_tracks(seeds)
    sts = [tt.seed(tt.new_state(), seeds[a]) for a in range(A)]
    for rnd, n_cand in enumerate((8, 1 + (n_tracks + n_own) % 7, 3)):
        own = angles((A, max(n_own, 1)), 0.2)[:, :n_own]
        cd = angles((A, n_cand), 0.1)
        cv = rng.choice(np.float32([1.0, 0.5, 0.0, np.nan, 2.0]), (A, n_cand), p=[0.4, 0.3, 0.1, 0.05, 0.15]).astype(np.float32)
        t_own = torch.from_numpy(np.ascontiguousarray(own)).cuda() if n_own else None
        bf.associate_tracks_dev(A, t_own, torch.from_numpy(cd).cuda(), torch.from_numpy(cv).cuda())
        for a in range(A):
            tt.associate(sts[a], own[a], cd[a], cv[a], n_tracks, n_own, **cfg)
        got = _pad(bf.tracks())
        for k in ("theta", "alive", "miss", "gen"):
            want = np.stack([st[k] for st in sts])
            assert np.array_equal(got[k], want, equal_nan=True), (rnd, k, np.flatnonzero((got[k] != want).any(axis=1))[:5])
    n_born = int(sum(int(st["gen"].sum()) for st in sts) - np.isfinite(seeds).sum())
    n_dead = int(sum(int((st["alive"][:n_tracks] == 0).sum()) for st in sts))
    print("n_tracks %d n_own %d: %d births, %d dead slots at the end over %d streams" % (n_tracks, n_own, n_born, n_dead, A))
    assert n_tracks == n_own or n_born > 0
    # fill: every frame carries the row of the twin
    d = torch.empty((A, 5, n_tracks), dtype=torch.float32, device="cuda")
    bf.fill_tracks_dev(A, 5, d)
    torch.cuda.synchronize()
    want = np.stack([tt.fill(st, n_tracks) for st in sts])
    assert np.array_equal(d.cpu().numpy(), np.repeat(want[:, None, :], 5, axis=1))
    bf.close()


def _parity_context(M):
    """the context after the two auto calls on the parity inputs, and what the twin needs of its state"""
    p = tt.parity_setup(M)
    A = p["pcm"].shape[0]
    bf = api.MvdrBeamformer(FS, p["xs"], N, max_streams=A, max_sources=tt.PARITY_S)
    bf.set_rtf(True, **p["rtf"])
    bf.set_mask_estimator(True, **p["estmask"])
    F = et.PARITY_F
    for t0, t1 in ((0, F), (F, 2 * F)):
        bf.process_sources(p["pcm"][:, :, t0 * HOP:(t1 + 1) * HOP].copy(), p["doa"][:, t0:t1].copy(), estimate_masks=True)
    cphi = _cphi(bf, A)
    state = [dict(phi=bf.covariance(a), cphi=cphi[a], psi=[bf.target_covariance(a, s) for s in range(tt.PARITY_S)]) for a in range(A)]
    return p, bf, state


@pytest.mark.parametrize("D", tt.PARITY_D)
@pytest.mark.parametrize("M", tt.PARITY_M)
def test_own_spectrum_parity(M, D):
    """after two auto calls on the parity inputs: every number of row slots and M < 4 Q, one scan pass and two, a band whose chunks are
    cut at both ends, n_own = 1 and 2.  own_used is the twin's outside its edge bins; own_spectrum is within 5e-4 of the row's maximum
    of the twin evaluated with the GPU's flags at the edge bins; the track moves to the twin's window argmax wherever that stands
    5e-3 of the row's maximum clear of the next angle (the rule of tests/test_gpu_mvdr_spectrum.py)"""
    p, bf, state = _parity_context(M)
    A = len(state)
    kw = dict(iterations=p["rtf"]["iterations"], ref_mic=p["rtf"]["ref_mic"], min_share=p["rtf"]["min_share"])
    bf.configure_spectrum(D, tt.PARITY_BAND[0], tt.PARITY_BAND[1], n_peaks=2)
    grid = bf.spectrum_grid()
    assert np.array_equal(grid, tt.grid64(D).astype(np.float32))
    seeds = tt.parity_seed(p["doa"])
    before = bf.state_save()
    worst, n_edge, n_cells, n_cmp = 0.0, 0, 0, 0
    for n_own in (1, 2):
        bf.configure_tracks(tt.PARITY_S, n_own, max_step_rad=tt.PARITY_STEP, min_sep_rad=0.1, hold=1000)
        bf.seed_tracks(seeds)
        r = bf.update_tracks(want_spectrum=True)
        tr = bf.tracks()
        assert r["own_spectrum"].shape == (A, n_own, D) and r["own_used"].shape == (A, n_own, K)
        assert np.all(np.isfinite(r["own_spectrum"])) and np.all(r["own_spectrum"] >= 0)
        for a in range(A):
            for s in range(n_own):
                psi, cpsi = state[a]["psi"][s]
                args = (FS, N, p["xs"], D) + tt.PARITY_BAND + (psi, cpsi, state[a]["phi"], state[a]["cphi"], seeds[a, s])
                tw = tt.own_spectrum(*args, **kw)
                gu, gs = r["own_used"][a, s], r["own_spectrum"][a, s]
                assert np.array_equal(gu[~tw["edge"]], tw["used"][~tw["edge"]]), (M, D, n_own, a, s, np.flatnonzero((gu != tw["used"]) & ~tw["edge"]))
                assert not gu[:tt.PARITY_BAND[0]].any() and not gu[tt.PARITY_BAND[1] + 1:].any()
                n_edge, n_cells = n_edge + int(tw["edge"].sum()), n_cells + tt.PARITY_BAND[1] - tt.PARITY_BAND[0] + 1
                if (gu != tw["used"]).any():
                    tw = tt.own_spectrum(*args, used=np.where(tw["edge"], gu, tw["used"]), **kw)
                top = tw["T"].max()
                if top > 0:
                    e = float(np.abs(gs - tw["T"]).max() / top)
                    worst = max(worst, e)
                    assert e <= SPEC_TOL, (M, D, n_own, a, s, e)
                else:
                    assert not gs.any()
                # the track: where the twin's window maximum stands clear, the GPU moved to it (by at most max_step)
                phi_tw = tt.window_argmax(tw["T"], grid, seeds[a, s], tt.PARITY_STEP)[0]
                if not top > 0:
                    assert tr["theta"][a, s] == seeds[a, s] and tr["miss"][a, s] == 1
                elif tt.clear_margin(tw["T"], grid, seeds[a, s], tt.PARITY_STEP) >= 5e-3:
                    st = tt.seed(tt.new_state(), seeds[a])
                    own = np.full(n_own, np.nan, dtype=np.float32)
                    own[s] = phi_tw
                    tt.associate(st, own, [], [], tt.PARITY_S, n_own, tt.PARITY_STEP, 0.1, 1000)
                    assert tr["theta"][a, s] == st["theta"][s] and tr["miss"][a, s] == 0, (M, D, n_own, a, s, tr["theta"][a, s], phi_tw)
                    n_cmp += 1
        assert np.array_equal(tr["alive"], np.ones((A, tt.PARITY_S), dtype=np.int32)) and np.array_equal(tr["gen"], tr["alive"])
    assert bf.state_save() == before                   # update and get read the stream state, they write none of it
    bf.close()
    print("M %d D %d: own spectra %.2e of the row's maximum; %d of %d cells (%.2f %%) at a decision edge; %d window maxima compared"
          % (M, D, worst, n_edge, n_cells, 100.0 * n_edge / n_cells, n_cmp))
    # (three microphones over the 17-degree window: the own spectrum is too flat for any maximum to stand 5e-3 clear on the finer grid)
    assert n_edge <= 0.01 * n_cells and (n_cmp > 0 or (M, D) == (3, 181))


def test_capon_half_is_the_spectrum_call_and_state_is_untouched_but_at_a_birth():
    """n_own = 0: the tracks of an update are the association twin fed the output of spectrum(), exactly; update, fill and get change no
    byte of the state blob (Phi, tr, tails, Psi, cpsi, cphi), except Psi and cpsi of a slot at its birth, which read 0"""
    torch = _torch()
    p, bf, _ = _parity_context(8)
    A, T = 2, tt.PARITY_S
    bf.configure_spectrum(181, 5, 100, n_peaks=2)
    cfg = dict(max_step_rad=0.2, min_sep_rad=0.1, hold=0)
    bf.configure_tracks(T, 0, **cfg)
    pk = bf.spectrum(A)
    assert (pk["peak_val"][:, 0] > 0).all()
    before = bf.state_save()
    psi_before = [[bf.target_covariance(a, s) for s in range(T)] for a in range(A)]
    assert all(np.abs(psi_before[a][s][0]).max() > 0 for a in range(A) for s in range(T))
    # slot 0 seeded on the strongest peak of stream 0 and far from every peak of stream 1; slot 1 dead
    seeds = np.float32([[pk["peak_doa"][0, 0], np.nan], [1.5, np.nan]])
    bf.seed_tracks(seeds)
    sts = [tt.seed(tt.new_state(), seeds[a]) for a in range(A)]
    born = []
    for rnd in range(2):
        assert bf.update_tracks() is None
        born.append([tt.associate(sts[a], None, pk["peak_doa"][a], pk["peak_val"][a], T, 0, **cfg) for a in range(A)])
        got = _pad(bf.tracks())
        for k in ("theta", "alive", "miss", "gen"):
            assert np.array_equal(got[k], np.stack([st[k] for st in sts])), (rnd, k, got[k])
    d = torch.empty((A, 3, T), dtype=torch.float32, device="cuda")
    bf.fill_tracks_dev(A, 3, d)
    torch.cuda.synchronize()
    print("births per round and stream:", born, "tracks", np.rad2deg(got["theta"][:, :T]).round(1).tolist())
    assert any(b for rb in born for b in rb)
    after = bf.state_save()
    assert len(after) == len(before)
    # the blob: header, Phi, tr, tails | Psi [A][T][K][tri], cpsi [A][T][K], cphi [A][K]
    tri = bf.M * (bf.M + 1) // 2
    n_psi, n_cpsi, n_cphi = A * T * K * tri * 8, A * T * K * 4, A * K * 4
    cut = len(before) - n_psi - n_cpsi - n_cphi
    assert after[:cut] == before[:cut] and after[-n_cphi:] == before[-n_cphi:]
    was_born = np.zeros((A, T), dtype=bool)
    for rb in born:
        for a, b in enumerate(rb):
            was_born[a, b] = True
    pb = np.frombuffer(before[cut:cut + n_psi], dtype=np.float32).reshape(A, T, -1)
    pa = np.frombuffer(after[cut:cut + n_psi], dtype=np.float32).reshape(A, T, -1)
    cb = np.frombuffer(before[cut + n_psi:cut + n_psi + n_cpsi], dtype=np.float32).reshape(A, T, -1)
    ca = np.frombuffer(after[cut + n_psi:cut + n_psi + n_cpsi], dtype=np.float32).reshape(A, T, -1)
    for a in range(A):
        for s in range(T):
            if was_born[a, s]:
                psi, cpsi = bf.target_covariance(a, s)
                assert not psi.any() and not cpsi.any() and not pa[a, s].any() and not ca[a, s].any()
            else:
                assert np.array_equal(pa[a, s], pb[a, s]) and np.array_equal(ca[a, s], cb[a, s])
    bf.close()


def test_no_host_step():
    """a four-chunk loop of auto_dev + tracks_update_dev + tracks_fill_dev gives the bytes of the same loop with the tracks read back by
    tracks(), the doa_rad array built on the host and uploaded: audio, spectra and covariance"""
    torch = _torch()
    p = tt.parity_setup(8)
    A, S, F = 2, tt.PARITY_S, 3
    pcm = torch.from_numpy(p["pcm"]).cuda()
    seeds = tt.parity_seed(p["doa"][:, :1])
    res = []
    for on_device in (True, False):
        bf = api.MvdrBeamformer(FS, p["xs"], N, max_streams=A, max_sources=S)
        bf.set_rtf(True, **p["rtf"])
        bf.set_mask_estimator(True, **p["estmask"])
        bf.configure_spectrum(61, 5, 100, n_peaks=2)
        bf.configure_tracks(S, 1, max_step_rad=0.1, min_sep_rad=0.1, hold=1)
        bf.seed_tracks(seeds)
        bf.follow_tracks(on_device)
        outs, specs, thetas = [], [], []
        for c in range(4):
            chunk = pcm[:, :, c * F * HOP:((c + 1) * F + 1) * HOP]
            out = torch.empty((A, S, F * HOP), dtype=torch.float32, device="cuda")
            spec = torch.empty((A, S, F, K, 2), dtype=torch.float32, device="cuda")
            if on_device:
                doa = None
            else:
                tr = bf.tracks()
                rows = np.stack([tt.fill(dict(theta=tr["theta"][a], alive=tr["alive"][a]), S) for a in range(A)])
                doa = torch.from_numpy(np.ascontiguousarray(np.repeat(rows[:, None, :], F, axis=1))).cuda()
            bf.process_sources_dev(chunk, F, doa, out_pcm=out, out_spec=spec, estimate_masks=True)
            bf.update_tracks_dev(A)
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy()); specs.append(spec.cpu().numpy()); thetas.append(bf.tracks()["theta"])
        res.append(dict(out=np.stack(outs), spec=np.stack(specs), theta=np.stack(thetas), cov=np.stack([bf.covariance(a) for a in range(A)]),
                        blob=bf.state_save()))
        bf.close()
    dev, host = res
    print("tracks per chunk (degrees):", np.rad2deg(dev["theta"]).round(1).tolist())
    assert np.all(np.isfinite(dev["out"])) and np.abs(dev["out"]).max() > 0
    for k in ("out", "spec", "theta", "cov"):
        assert dev[k].tobytes() == host[k].tobytes(), k
    assert dev["blob"] == host["blob"]


def test_repeatable_and_independent_of_the_place_in_the_batch():
    p, bf, _ = _parity_context(13)
    A = 2
    bf.configure_spectrum(181, 5, 100, n_peaks=2)
    seeds = tt.parity_seed(p["doa"])
    runs = []
    for _ in range(2):
        bf.configure_tracks(tt.PARITY_S, 2, max_step_rad=tt.PARITY_STEP, min_sep_rad=0.1, hold=3)
        bf.seed_tracks(seeds)
        r = bf.update_tracks(want_spectrum=True)
        runs.append((r["own_spectrum"], r["own_used"], bf.tracks()))
    assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32)) and np.array_equal(runs[0][1], runs[1][1])
    assert all(np.array_equal(runs[0][2][k], runs[1][2][k]) for k in runs[0][2])
    blob = bf.state_save()
    bf.close()
    # the same two streams in the other order, among four
    bf2 = api.MvdrBeamformer(FS, p["xs"], N, max_streams=4, max_sources=tt.PARITY_S)
    bf2.set_rtf(True, **p["rtf"])
    bf2.set_mask_estimator(True, **p["estmask"])
    F = et.PARITY_F
    order = [1, 0, 1, 0]
    for t0, t1 in ((0, F), (F, 2 * F)):
        bf2.process_sources(p["pcm"][order][:, :, t0 * HOP:(t1 + 1) * HOP].copy(), p["doa"][order][:, t0:t1].copy(), estimate_masks=True)
    bf2.configure_spectrum(181, 5, 100, n_peaks=2)
    bf2.configure_tracks(tt.PARITY_S, 2, max_step_rad=tt.PARITY_STEP, min_sep_rad=0.1, hold=3)
    bf2.seed_tracks(seeds[order])
    r2 = bf2.update_tracks(want_spectrum=True)
    t2 = bf2.tracks()
    for i, a in enumerate(order):
        assert np.array_equal(r2["own_spectrum"][i].view(np.uint32), runs[0][0][a].view(np.uint32)), (i, a)
        assert np.array_equal(r2["own_used"][i], runs[0][1][a])
        assert all(np.array_equal(t2[k][i], runs[0][2][k][a]) for k in t2)
    assert len(blob) > 0
    bf2.close()


def test_refusals_and_timing_slot():
    """the refusals of the header; none of them faults, the configuration and the state stay as they were"""
    torch = _torch()
    bf = api.MvdrBeamformer(FS, synth.ULA8, 64, max_streams=2, max_sources=3)
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    with pytest.raises(api.MCArrayHipError):
        bf.configure_tracks(2)                                             # the spectrum first
    with pytest.raises(api.MCArrayHipError):
        bf.get_timing(api.MvdrBeamformer.K_TRACKS)                          # the slot does not exist yet
    bf.configure_spectrum(31, 1, 30, n_peaks=2)
    for call in (lambda: bf.update_tracks(), lambda: bf.tracks(), lambda: bf.fill_tracks_dev(1, 2, buf), lambda: bf.seed_tracks([0.1, 0.2]),
                 lambda: bf.associate_tracks_dev(1, None, buf[:2], buf[2:4])):
        with pytest.raises(api.MCArrayHipError):
            call()                                                         # before configure
    with pytest.raises(api.MCArrayHipError):
        bf.configure_tracks(2, 1)                                          # n_own > 0 without RTF
    bf.configure_tracks(2, 0, max_step_rad=0.3, min_sep_rad=0.05, hold=4)
    good = bf.get_tracks_config()
    bf.seed_tracks([[0.5, np.nan], [np.nan, -0.5]])
    held = bf.tracks()
    for bad in (dict(n_tracks=0), dict(n_tracks=4), dict(n_own=-1), dict(n_own=3), dict(max_step_rad=0.0), dict(max_step_rad=3.2),
                dict(max_step_rad=np.nan), dict(min_sep_rad=-0.1), dict(min_sep_rad=3.2), dict(min_sep_rad=np.inf), dict(hold=-1), dict(hold=1001)):
        with pytest.raises(api.MCArrayHipError):
            bf.configure_tracks(**dict(dict(n_tracks=2, n_own=0, max_step_rad=0.3, min_sep_rad=0.05, hold=4), **bad))
        assert bf.get_tracks_config() == good
    wrong = _lib.MvdrTracksConfig(C.sizeof(_lib.MvdrTracksConfig) - 4, 1, 1, 0, 0.3, 0.05, 4)      # a struct of another size
    assert bf._lib.mca_hip_mvdr_tracks_configure(bf.h, C.byref(wrong)) == -1 and bf.get_tracks_config() == good
    for call in (lambda: bf.update_tracks(0), lambda: bf.update_tracks(3), lambda: bf.tracks(3), lambda: bf.fill_tracks_dev(3, 2, buf),
                 lambda: bf.fill_tracks_dev(1, 0, buf), lambda: bf.associate_tracks_dev(1, None, buf[:9].reshape(1, 9), buf[9:18].reshape(1, 9))):
        with pytest.raises(api.MCArrayHipError):
            call()
    now = bf.tracks()
    assert all(np.array_equal(held[k], now[k], equal_nan=True) for k in held)
    assert held["alive"].tolist() == [[1, 0], [0, 1]] and held["gen"].tolist() == [[1, 0], [0, 1]]
    # the timing slot exists now and counts the track launches
    bf.set_timing(True)
    bf.update_tracks()
    n, ms = bf.get_timing(api.MvdrBeamformer.K_TRACKS)
    assert n == 1 and ms >= 0.0
    assert bf.get_timing(api.MvdrBeamformer.K_SPECTRUM)[0] == 1            # the Capon kernels of the update
    bf.set_timing(False)
    # reset clears the tracks; fewer slots than tracks and disabling RTF under own tracks disable them
    bf.reset()
    z = bf.tracks()
    assert all(not z[k].any() for k in z)
    bf.set_max_sources(1)
    assert bf.get_tracks_config()["enable"] is False
    with pytest.raises(api.MCArrayHipError):
        bf.update_tracks()
    bf.set_max_sources(2)
    bf.set_rtf(True)
    bf.configure_tracks(2, 1)
    bf.set_rtf(False)
    assert bf.get_tracks_config()["enable"] is False
    bf.set_rtf(True)
    bf.configure_tracks(2, 0)
    bf.set_rtf(False)                                                      # whatever n_own is
    assert bf.get_tracks_config()["enable"] is False
    bf.close()


def test_scene_on_the_gpu():
    """the scene of tests/test_mvdr_tracks_twin.py through the GPU: the auto call and update_tracks() per chunk.  Measured once on the
    MI355X: the own track 19, 20, 21, 23, 24, 25, 26, 28 degrees after the chunks, the twin's in every chunk (0.00 grid steps apart), 7.0
    degrees off the truth at the worst; the share 0.51790 against the twin's 0.51790.  Bars: the own track within one grid step (1 degree) of the twin's after every chunk -- a float32
    near-tie can move an argmax by one sample, and the window pulls it back; the last chunk's share of the target, formed from the
    GPU's held covariance() and steering() after the last frame, against the twin's formed the same way, within the module's 5e-4 of it.  The GPU hands out no weights,
    so that share covers the end state only; the weights the kernels used over the last chunk are covered by its output spectra, which
    are within 5e-4 of the twin's peak (measured: 1.0e-5 and 1.7e-5 for the two outputs, over all cells; 0.84 % of the cells at an edge) --
    with equal inputs and equal outputs per cell, the twin's share under per-frame weights, 0.497, is the GPU's."""
    import mvdr_rtf_twin as rt
    runs = tt.scene_runs()
    sc, tw = runs["sc"], runs["tracked"]
    fs, n_fft, hop = rt.SCENE_FS, rt.SCENE_N, rt.SCENE_N // 2
    bf = api.MvdrBeamformer(fs, sc["xs"], n_fft, max_streams=1, max_sources=2)
    bf.set_rtf(True, **et.SCENE_RTF)
    bf.set_mask_estimator(True, **et.SCENE_CFG)
    bf.configure_spectrum(tt.SCENE_D, tt.SCENE_BAND[0], tt.SCENE_BAND[1], n_peaks=2)
    bf.configure_tracks(**tt.SCENE_TRACKS)
    bf.seed_tracks(np.float32([[tt.SCENE_TRUTH[0], tt.SCENE_ITF]]))
    thetas = []
    for c in range(tt.SCENE_CHUNKS):
        tr = bf.tracks()
        row = tt.fill(dict(theta=tr["theta"][0], alive=tr["alive"][0]), 2)
        f0, f1 = c * tt.SCENE_CF, (c + 1) * tt.SCENE_CF
        r = bf.process_sources(sc["pcm"][None, :, f0 * hop:(f1 + 1) * hop].copy(), np.tile(row, (1, tt.SCENE_CF, 1)), estimate_masks=True)
        bf.update_tracks()
        thetas.append(float(bf.tracks()["theta"][0, 0]))
    thetas = np.array(thetas)
    step = np.pi / (tt.SCENE_D - 1)
    dist = np.abs(thetas - tw["theta"]) / step

    def frozen_share(phi, d):
        """the share of the target over the last chunk under the weights of the last frame"""
        M = phi.shape[1]
        trc = np.real(np.trace(phi, axis1=1, axis2=2))
        PL = phi + (1e-3 * trc / M)[:, None, None] * np.eye(M)
        h = np.linalg.solve(PL, d[:, :, None])[:, :, 0]
        w = h / np.einsum("km,km->k", np.conj(d), h)[:, None]
        return tt.target_share(np.broadcast_to(w, (tt.SCENE_CF,) + w.shape), sc, (tt.SCENE_CHUNKS - 1) * tt.SCENE_CF, tt.SCENE_CHUNKS * tt.SCENE_CF)
    last = tw["run"]
    # the weights the kernels used over the last chunk: its output spectra against the twin's, outside the cells at a decision edge of
    # the RTF estimator or of the mask estimator (the module's rule)
    m32 = et.masks(fs, n_fft, sc["xs"], sc["pcm"][:, f0 * hop:(f1 + 1) * hop], np.tile(row.astype(np.float64), (tt.SCENE_CF, 1)), dtype=np.float32, **et.SCENE_CFG)
    edge = np.swapaxes(rt.edges_of(last), 0, 1) | et.edge_cells(last["masks"], m32)[1][None]
    d = np.abs(r["spec"][0].astype(np.complex128) - last["spec"])
    peak = np.abs(last["spec"]).max(axis=(1, 2))
    e_spec, e_all = (d * ~edge).max(axis=(1, 2)) / peak, d.max(axis=(1, 2)) / peak
    print("last chunk's output spectra against the twin's: %s of the peak outside %.2f %% edge cells (%s over all cells)"
          % (["%.2e" % v for v in e_spec], 100.0 * edge.mean(), ["%.2e" % v for v in e_all]))
    g_d = bf.steering(float(row[0]), 0, 0)[0]
    share_gpu = frozen_share(bf.covariance(0), g_d)
    share_tw = frozen_share(last["phi"], last["d"][-1, 0])
    print("own track per chunk: GPU %s twin %s degrees (%.2f grid steps apart at most); truth %s; worst error %.2f degrees; "
          "share over the last chunk under the last frame's weights: GPU %.5f twin %.5f"
          % (np.rad2deg(thetas).round(1).tolist(), np.rad2deg(tw["theta"]).round(1).tolist(), dist.max(), np.rad2deg(tt.SCENE_TRUTH).round(1).tolist(),
             np.rad2deg(np.abs(thetas - tt.SCENE_TRUTH)).max(), share_gpu, share_tw))
    bf.close()
    assert dist.max() <= 1.0 + 1e-3
    assert abs(share_gpu - share_tw) <= SCENE_SHARE_BAR * share_tw
    assert e_spec.max() <= SPEC_TOL and edge.mean() <= 0.01
