"""GPU: the map mode of the tracks of the MVDR context (mca_hip_mvdr_tracks_*_map) against
tests/mvdr_tracks_map_twin.py.

The association is float32 on both sides, operation for operation: theta, eps, alive, miss and gen are compared with array_equal.  The
own map is compared with the float64 twin evaluated on the state the GPU holds (covariance(), target_covariance(), cphi from the state
blob), at the module's bar of 5e-4 of the map's maximum; at the bins the twin flags as decision edges of the estimator
(mvdr_rtf_twin.edge_cells; at most 1 % of the cells, tests/test_mvdr_tracks_map_twin.py) the twin takes the GPU's flags."""
import ctypes as C

import numpy as np
import pytest

from mcarray_amd import _lib, api, synth

import mvdr_estmask_twin as et
import mvdr_geometry_twin as gt
import mvdr_map_twin as mp
import mvdr_tracks_map_twin as tm
import mvdr_tracks_twin as tt

pytestmark = pytest.mark.gpu

MAP_TOL = 5e-4              # the project's bar for a spectrum row, of the map's maximum
CLEAR = 5e-3                # mvdr_tracks_twin.clear_margin's rule
F32 = np.float32
FS, N = tm.FS, tm.N
K, HOP = N // 2 + 1, N // 2
KEYS = ("theta", "eps", "alive", "miss", "gen")


def _torch():
    import torch
    return torch


def _pad(tr):
    """tracks_map() [A][n_tracks] -> the twin's [A][4] layout"""
    out = {}
    for k, v in tr.items():
        out[k] = np.zeros((v.shape[0], tm.MAX_SLOTS), dtype=v.dtype)
        out[k][:, :v.shape[1]] = v
    return out


def _cphi(bf, A):
    """cphi [A][K] of an RTF context: the last part of its state blob"""
    return np.frombuffer(bf.state_save()[-A * bf.K * 4:], dtype=F32).reshape(A, bf.K).astype(np.float64)


def _small_context(A, n_tracks, n_own, cfg, el_cfg, n_az=12, n_el=3):
    bf = api.MvdrBeamformer(FS, gt.array_3d(4, 4), 64, max_streams=A, max_sources=4, geometry="xyz")
    bf.set_rtf(True)
    bf.configure_spectrum(n_az, 1, 30)
    bf.map_configure(n_az, n_el, 0.0, 1.0, 1, 30, n_peaks=2)
    bf.configure_tracks(n_tracks, n_own, **cfg)
    bf.configure_tracks_map(**el_cfg)
    return bf


@pytest.mark.parametrize("n_tracks,n_own", [(1, 0), (1, 1), (2, 1), (3, 0), (3, 2), (4, 0), (4, 1), (4, 2)])
def test_association_against_the_twin(n_tracks, n_own):
    """associate_map_dev on 300 random streams, three rounds with 1 ... 8 candidates: angles from a grid of 1/16 rad (ties in distance
    and at the gates are common) beyond +-pi in azimuth and beyond +-pi/2 in elevation, NaNs in either angle among the seeds, the own
    targets and the candidates, values of 0 and NaN.  Then the fill: doa_rad and the elevations of the slots"""
    torch = _torch()
    A = 300
    rng = np.random.default_rng(100 * n_tracks + n_own)
    cfg = dict(max_step_rad=0.25, min_sep_rad=0.125, hold=1)
    el_cfg = dict(max_step_el_rad=0.1875, min_sep_el_rad=0.125)
    bf = _small_context(A, n_tracks, n_own, cfg, el_cfg)
    assert bf.get_tracks_map_config() == dict(enable=True, **el_cfg)
    z = bf.tracks_map()
    assert all(not z[k].any() for k in z)

    def angles(shape, p_nan, span):
        v = (rng.integers(-span, span + 1, shape) / 16.0).astype(F32)
        v[rng.random(shape) < p_nan] = np.nan
        return v
    saz, sel = angles((A, n_tracks), 0.2, 64), angles((A, n_tracks), 0.1, 28)
    bf.seed_tracks_map(saz, sel)
    sts = [tm.seed_map(tm.new_state(), saz[a], sel[a]) for a in range(A)]
    n_born = 0
    for rnd, n_cand in enumerate((8, 1 + (n_tracks + n_own) % 7, 3)):
        oaz, oel = angles((A, max(n_own, 1)), 0.15, 64)[:, :n_own], angles((A, max(n_own, 1)), 0.1, 28)[:, :n_own]
        caz, cel = angles((A, n_cand), 0.1, 64), angles((A, n_cand), 0.05, 28)
        # elevations on few values, so that a candidate often meets a slot's height
        cel = np.where(rng.random((A, n_cand)) < 0.5, (np.round(cel * 4) / 4).astype(F32), cel)
        cv = rng.choice(F32([1.0, 0.5, 0.0, np.nan, 2.0]), (A, n_cand), p=[0.4, 0.3, 0.1, 0.05, 0.15]).astype(F32)
        dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (oaz, oel, caz, cel, cv)]
        bf.associate_tracks_map_dev(A, dev[0] if n_own else None, dev[1] if n_own else None, dev[2], dev[3], dev[4])
        for a in range(A):
            n_born += len(tm.associate_map(sts[a], oaz[a], oel[a], caz[a], cel[a], cv[a], n_tracks, n_own, **cfg, **el_cfg))
        got = _pad(bf.tracks_map())
        for k in KEYS:
            want = np.stack([st[k] for st in sts])
            assert np.array_equal(got[k], want, equal_nan=True), (rnd, k, np.flatnonzero((got[k] != want).any(axis=1))[:5])
        assert np.all(np.abs(got["theta"]) <= gt.PI_F) and np.all(np.abs(got["eps"]) <= tm.HALF_PI_F)
    print("n_tracks %d n_own %d: %d births over %d streams" % (n_tracks, n_own, n_born, A))
    assert n_tracks == n_own or n_born > 0
    # the 1-D get works in both modes
    one = bf.tracks()
    assert all(np.array_equal(one[k], got[k][:, :n_tracks]) for k in one)
    # fill: every frame carries the row of the twin, the slots their elevations; the slots behind n_tracks stay unset
    d = torch.empty((A, 5, n_tracks), dtype=torch.float32, device="cuda")
    bf.fill_tracks_dev(A, 5, d)
    torch.cuda.synchronize()
    want = [tm.fill_map(st, n_tracks) for st in sts]
    assert np.array_equal(d.cpu().numpy(), np.repeat(np.stack([w[0] for w in want])[:, None, :], 5, axis=1))
    el = bf.get_elevations()
    assert np.array_equal(el[:, :n_tracks], np.stack([w[1] for w in want]), equal_nan=True) and np.isnan(el[:, n_tracks:]).all()
    assert bf.get_tracks_config()["enable"] and bf.get_tracks_map_config()["enable"]      # a fill is no set_elevations call
    bf.close()


RTF_KEYS = ("iterations", "ref_mic", "min_share")


def _parity_context(name, elevation=0.0, slot_el=True):
    """the context after the two auto calls on the parity inputs, and what the twin needs of its state"""
    inp = tm.parity_inputs(name)
    A = inp["pcm"].shape[0]
    bf = api.MvdrBeamformer(FS, inp["xyz"], N, max_streams=A, max_sources=tm.PARITY_S, geometry="xyz", elevation_rad=elevation)
    rtf = tm.parity_rtf(name)
    bf.set_rtf(True, **rtf)
    bf.set_mask_estimator(True, **tm.parity_estmask())
    if slot_el:
        bf.set_elevations(inp["el"])
    F = tm.PARITY_F
    for t0, t1 in ((0, F), (F, 2 * F)):
        bf.process_sources(inp["pcm"][:, :, t0 * HOP:(t1 + 1) * HOP].copy(), inp["doa"][:, t0:t1].copy(), estimate_masks=True)
    return inp, bf, {k: rtf[k] for k in RTF_KEYS}


def _held_state(bf, A):
    cphi = _cphi(bf, A)
    return [dict(phi=bf.covariance(a), cphi=cphi[a], psi=[bf.target_covariance(a, s) for s in range(tm.PARITY_S)]) for a in range(A)]


@pytest.mark.parametrize("name", sorted(tm.PARITY_ARRAYS))
def test_own_map_parity(name):
    """after two auto calls on the parity inputs, every look direction at an elevation of its own: Q = 1, 2 and 4 row slots and the
    ring; maps of 120, 180 and 252 directions; a band whose last chunk is partial; n_own = 1 and 2.  own_used is the twin's outside
    its edge bins; own_map is within 5e-4 of the map's maximum of the twin evaluated with the GPU's flags at the edge bins; the track
    moves towards the twin's window argmax wherever that stands 5e-3 of the maximum clear"""
    inp, bf, kw = _parity_context(name)
    A, S = inp["pcm"].shape[0], tm.PARITY_S
    state = _held_state(bf, A)
    bf.configure_spectrum(24, *tm.PARITY_BAND)
    before = bf.state_save()
    worst, n_cmp = 0.0, 0
    for n_az, n_el in tm.PARITY_MAPS:
        els = mp.grid_el(n_el, *tm.PARITY_EL)
        step = float(els[1] - els[0])
        bf.map_configure(n_az, n_el, tm.PARITY_EL[0], tm.PARITY_EL[1], tm.PARITY_BAND[0], tm.PARITY_BAND[1], n_peaks=2)
        az32, el32 = bf.map_grid()
        assert np.array_equal(az32, gt.grid_xyz(n_az).astype(F32)) and np.array_equal(el32, els.astype(F32))
        saz, sel = tm.parity_seeds(inp, step)
        cfg = dict(max_step_rad=tm.PARITY_STEP, min_sep_rad=0.1, hold=1000)
        el_cfg = dict(max_step_el_rad=1.5 * step, min_sep_el_rad=0.5 * step)
        n_edge = n_cells = 0
        for n_own in (1, 2):
            bf.configure_tracks(S, n_own, **cfg)
            bf.configure_tracks_map(**el_cfg)
            bf.seed_tracks_map(saz, sel)
            r = bf.update_tracks_map(want_map=True)
            tr = bf.tracks_map()
            assert r["own_map"].shape == (A, n_own, n_el, n_az) and r["own_used"].shape == (A, n_own, K)
            assert np.all(np.isfinite(r["own_map"])) and np.all(r["own_map"] >= 0)
            for a in range(A):
                for s in range(n_own):
                    psi, cpsi = state[a]["psi"][s]
                    args = (FS, N, inp["xyz"], n_az, els) + tm.PARITY_BAND + (psi, cpsi, state[a]["phi"], state[a]["cphi"], saz[a, s], sel[a, s])
                    tw = tm.own_map(*args, **kw)
                    gu, gm = r["own_used"][a, s], r["own_map"][a, s]
                    assert np.array_equal(gu[~tw["edge"]], tw["used"][~tw["edge"]]), (name, n_az, n_el, n_own, a, s, np.flatnonzero((gu != tw["used"]) & ~tw["edge"]))
                    assert not gu[:tm.PARITY_BAND[0]].any() and not gu[tm.PARITY_BAND[1] + 1:].any()
                    n_edge, n_cells = n_edge + int(tw["edge"].sum()), n_cells + tm.PARITY_BAND[1] - tm.PARITY_BAND[0] + 1
                    if (gu != tw["used"]).any():
                        tw = tm.own_map(*args, used=np.where(tw["edge"], gu, tw["used"]), **kw)
                    top = tw["T"].max()
                    assert top > 0
                    e = float(np.abs(gm - tw["T"]).max() / top)
                    worst = max(worst, e)
                    assert e <= MAP_TOL, (name, n_az, n_el, n_own, a, s, e)
                    if tm.clear_margin_map(tw["T"], az32, el32, saz[a, s], sel[a, s], cfg["max_step_rad"], el_cfg["max_step_el_rad"]) >= CLEAR:
                        paz, pel, _ = tm.window_argmax_map(tw["T"], az32, el32, saz[a, s], sel[a, s], cfg["max_step_rad"], el_cfg["max_step_el_rad"])
                        st = tm.seed_map(tm.new_state(), saz[a], sel[a])
                        oaz, oel = np.full(n_own, np.nan, dtype=F32), np.full(n_own, np.nan, dtype=F32)
                        oaz[s], oel[s] = paz, pel
                        tm.associate_map(st, oaz, oel, [], [], [], S, n_own, **cfg, **el_cfg)
                        assert tr["theta"][a, s] == st["theta"][s] and tr["eps"][a, s] == st["eps"][s] and tr["miss"][a, s] == 0, \
                            (name, n_az, n_el, n_own, a, s, tr["theta"][a, s], tr["eps"][a, s], paz, pel)
                        n_cmp += 1
            assert np.array_equal(tr["alive"], np.ones((A, S), dtype=np.int32)) and np.array_equal(tr["gen"], tr["alive"])
        print("%s %d x %d: %d of %d cells (%.2f %%) at a decision edge" % (name, n_az, n_el, n_edge, n_cells, 100.0 * n_edge / n_cells))
        assert n_edge <= 0.01 * n_cells
    assert bf.state_save() == before                   # update and get read the stream state, they write none of it
    bf.close()
    print("%s: own maps %.2e of the map's maximum; %d window maxima compared" % (name, worst, n_cmp))
    assert n_cmp > 0


def test_one_row_map_is_the_update_on_one_angle():
    """n_el = 1 at the context's elevation, max_step_el = min_sep_el = 0: after an update theta, alive, miss and gen are those of a
    second context updated through the call on one angle -- wherever the own window maximum stands clear and both calls saw the same
    peaks -- and the own map is within 5e-4 of mvdr_tracks_twin.own_spectrum on the state the GPU holds"""
    name, el0, D = "cube7", 0.3, 36
    cfg = dict(max_step_rad=tm.PARITY_STEP, min_sep_rad=0.1, hold=1)
    res = {}
    for mode in ("map", "one"):
        inp, bf, kw = _parity_context(name, elevation=el0, slot_el=False)
        A, S = inp["pcm"].shape[0], tm.PARITY_S
        bf.configure_spectrum(D, tm.PARITY_BAND[0], tm.PARITY_BAND[1], n_peaks=2)
        bf.configure_tracks(S, 1, **cfg)
        saz = tm.parity_seeds(inp, 0.0)[0]
        if mode == "map":
            bf.map_configure(D, 1, el0, el0, tm.PARITY_BAND[0], tm.PARITY_BAND[1], n_peaks=2)
            bf.configure_tracks_map(0.0, 0.0)
            e32 = bf.map_grid()[1]
            assert e32.tolist() == [float(F32(el0))]
            bf.seed_tracks_map(saz, np.full_like(saz, e32[0]))
            pk = bf.map(A)
            r = bf.update_tracks_map(want_map=True)
            tr = bf.tracks_map()
            assert np.array_equal(tr["eps"], np.full((A, S), e32[0]))
            res[mode] = dict(tr=tr, T=r["own_map"][:, :, 0, :], used=r["own_used"], peaks=(pk["peak_az"], pk["peak_val"] > 0))
            state, grid = _held_state(bf, A), bf.map_grid()[0]
        else:
            bf.seed_tracks(saz)
            pk = bf.spectrum(A)
            r = bf.update_tracks(want_spectrum=True)
            res[mode] = dict(tr=bf.tracks(), T=r["own_spectrum"], used=r["own_used"], peaks=(pk["peak_doa"], pk["peak_val"] > 0))
        bf.close()
    n_cmp = 0
    for a in range(A):
        psi, cpsi = state[a]["psi"][0]
        with gt.xyz_mode(float(F32(el0))):
            tw = tt.own_spectrum(FS, N, inp["xyz"], D, tm.PARITY_BAND[0], tm.PARITY_BAND[1], psi, cpsi, state[a]["phi"], state[a]["cphi"], saz[a, 0], **kw)
            gu = res["map"]["used"][a, 0]
            assert np.array_equal(gu[~tw["edge"]], tw["used"][~tw["edge"]])
            if (gu != tw["used"]).any():
                tw = tt.own_spectrum(FS, N, inp["xyz"], D, tm.PARITY_BAND[0], tm.PARITY_BAND[1], psi, cpsi, state[a]["phi"], state[a]["cphi"], saz[a, 0],
                                     used=np.where(tw["edge"], gu, tw["used"]), **kw)
        top = tw["T"].max()
        assert top > 0 and float(np.abs(res["map"]["T"][a, 0] - tw["T"]).max() / top) <= MAP_TOL
        win = np.array([abs(gt.wrap32(F32(g - saz[a, 0]))) <= F32(cfg["max_step_rad"]) for g in grid])
        v = np.sort(tw["T"][win])[::-1]
        same_peaks = all(np.array_equal(p[a], q[a]) for p, q in zip(res["map"]["peaks"], res["one"]["peaks"]))
        if (v[0] - v[1]) / top >= CLEAR and same_peaks:
            for k in ("theta", "alive", "miss", "gen"):
                assert np.array_equal(res["map"]["tr"][k][a], res["one"]["tr"][k][a]), (a, k, res["map"]["tr"][k][a], res["one"]["tr"][k][a])
            n_cmp += 1
    assert n_cmp > 0


def test_tile_skip_purity_batch_place_and_workspace_cap():
    """cube16 on the 36 x 7 map (two tiles), n_own = 1 of 2 with the second slot dead, so that a map peak is born into it.  The update
    without own_map_dev (tiles without a cell of the window are not scanned) leaves the track state of the update with it; a second
    run gives the same bytes; so does a context that holds the streams in another order among four, and a workspace cap of one stream a
    pass.  Update, fill and get change no byte of the state blob but Psi and cpsi of the slot born, which read 0"""
    torch = _torch()
    name = "cube16"
    inp, bf, _ = _parity_context(name)
    A, S = inp["pcm"].shape[0], tm.PARITY_S
    n_az, n_el = tm.PARITY_MAPS[2]
    step = (tm.PARITY_EL[1] - tm.PARITY_EL[0]) / (n_el - 1)
    cfg = dict(max_step_rad=tm.PARITY_STEP, min_sep_rad=0.1, hold=2)
    el_cfg = dict(max_step_el_rad=1.5 * step, min_sep_el_rad=0.5 * step)
    saz, sel = tm.parity_seeds(inp, step)
    saz[:, 1] = np.nan                                                     # the second slot starts dead

    def prepare(b, seeds_az, seeds_el):
        b.configure_spectrum(24, *tm.PARITY_BAND)
        b.map_configure(n_az, n_el, tm.PARITY_EL[0], tm.PARITY_EL[1], tm.PARITY_BAND[0], tm.PARITY_BAND[1], n_peaks=2)
        b.configure_tracks(S, 1, **cfg)
        b.configure_tracks_map(**el_cfg)
        b.seed_tracks_map(seeds_az, seeds_el)

    before = bf.state_save()
    runs = []
    for want_map, cap in ((True, None), (False, None), (True, None), (True, 8)):
        bf.state_load(before)                                              # (a birth cleared Psi of the slot: back to the state compared on)
        if cap is not None:
            bf.set_rtf_workspace(cap)
        prepare(bf, saz, sel)
        r = bf.update_tracks_map(want_map=want_map)
        runs.append((r, bf.tracks_map()))
    bf.set_rtf_workspace(1 << 30)
    ref_r, ref_t = runs[0]
    assert ref_t["gen"][:, 1].tolist() == [1] * A and ref_t["alive"][:, 1].tolist() == [1] * A, "a map peak is born into the dead slot"
    for r, t in runs[1:]:
        assert all(np.array_equal(t[k], ref_t[k]) for k in KEYS)
        if r is not None:
            assert np.array_equal(r["own_map"].view(np.uint32), ref_r["own_map"].view(np.uint32)) and np.array_equal(r["own_used"], ref_r["own_used"])
    # the blob after the last run: only Psi and cpsi of the slot born differ, and read 0
    d = torch.empty((A, 3, S), dtype=torch.float32, device="cuda")
    bf.fill_tracks_dev(A, 3, d)
    torch.cuda.synchronize()
    after = bf.state_save()
    tri = bf.M * (bf.M + 1) // 2
    n_psi, n_cpsi, n_cphi = A * S * K * tri * 8, A * S * K * 4, A * K * 4
    cut = len(before) - n_psi - n_cpsi - n_cphi
    assert len(after) == len(before) and after[:cut] == before[:cut] and after[-n_cphi:] == before[-n_cphi:]
    pb, pa = (np.frombuffer(b[cut:cut + n_psi], dtype=F32).reshape(A, S, -1) for b in (before, after))
    cb, ca = (np.frombuffer(b[cut + n_psi:cut + n_psi + n_cpsi], dtype=F32).reshape(A, S, -1) for b in (before, after))
    assert pb[:, 1].any() and not pa[:, 1].any() and not ca[:, 1].any()
    assert np.array_equal(pa[:, 0], pb[:, 0]) and np.array_equal(ca[:, 0], cb[:, 0])
    bf.close()
    # the same two streams in the other order, among four
    bf2 = api.MvdrBeamformer(FS, inp["xyz"], N, max_streams=4, max_sources=S, geometry="xyz")
    bf2.set_rtf(True, **tm.parity_rtf(name))
    bf2.set_mask_estimator(True, **tm.parity_estmask())
    order = [1, 0, 1, 0]
    bf2.set_elevations(inp["el"][order])
    F = tm.PARITY_F
    for t0, t1 in ((0, F), (F, 2 * F)):
        bf2.process_sources(inp["pcm"][order][:, :, t0 * HOP:(t1 + 1) * HOP].copy(), inp["doa"][order][:, t0:t1].copy(), estimate_masks=True)
    prepare(bf2, saz[order], sel[order])
    r2 = bf2.update_tracks_map(want_map=True)
    t2 = bf2.tracks_map()
    for i, a in enumerate(order):
        assert np.array_equal(r2["own_map"][i].view(np.uint32), ref_r["own_map"][a].view(np.uint32)), (i, a)
        assert np.array_equal(r2["own_used"][i], ref_r["own_used"][a])
        assert all(np.array_equal(t2[k][i], ref_t[k][a]) for k in KEYS)
    bf2.close()


def test_no_host_step():
    """a four-chunk loop of the auto call, update_map_dev and fill_dev (follow_tracks) gives the bytes of the loop that reads the tracks
    back, uploads doa_rad and calls set_elevations_dev with the same angles: audio, spectra, covariance and state blob.  Both slots are
    own tracks, so that no birth clears a Psi the second context keeps"""
    torch = _torch()
    name = "cube7"
    inp = tm.parity_inputs(name)
    A, S, F = inp["pcm"].shape[0], tm.PARITY_S, 3
    n_az, n_el = tm.PARITY_MAPS[1]
    step = (tm.PARITY_EL[1] - tm.PARITY_EL[0]) / (n_el - 1)
    pcm = torch.from_numpy(inp["pcm"]).cuda()
    saz, sel = tm.parity_seeds(inp, step)
    res, angles = [], []
    for on_device in (True, False):
        bf = api.MvdrBeamformer(FS, inp["xyz"], N, max_streams=A, max_sources=S, geometry="xyz")
        bf.set_rtf(True, **tm.parity_rtf(name))
        bf.set_mask_estimator(True, **tm.parity_estmask())
        if on_device:
            bf.configure_spectrum(24, *tm.PARITY_BAND)
            bf.map_configure(n_az, n_el, tm.PARITY_EL[0], tm.PARITY_EL[1], tm.PARITY_BAND[0], tm.PARITY_BAND[1], n_peaks=2)
            bf.configure_tracks(S, S, max_step_rad=0.1, min_sep_rad=0.1, hold=1)
            bf.configure_tracks_map(max_step_el_rad=step, min_sep_el_rad=step)
            bf.seed_tracks_map(saz, sel)
            bf.follow_tracks(True)
        outs, specs = [], []
        for c in range(4):
            chunk = pcm[:, :, c * F * HOP:((c + 1) * F + 1) * HOP]
            out = torch.empty((A, S, F * HOP), dtype=torch.float32, device="cuda")
            spec = torch.empty((A, S, F, K, 2), dtype=torch.float32, device="cuda")
            if on_device:
                tr = bf.tracks_map()
                angles.append([tm.fill_map({k: tr[k][a] for k in KEYS}, S) for a in range(A)])
                bf.process_sources_dev(chunk, F, None, out_pcm=out, out_spec=spec, estimate_masks=True)
                bf.update_tracks_map_dev(A)
            else:
                rows = np.stack([angles[c][a][0] for a in range(A)])
                els = np.stack([angles[c][a][1] for a in range(A)])
                doa = torch.from_numpy(np.ascontiguousarray(np.repeat(rows[:, None, :], F, axis=1))).cuda()
                bf.set_elevations_dev(A, torch.from_numpy(np.ascontiguousarray(els)).cuda())
                bf.process_sources_dev(chunk, F, doa, out_pcm=out, out_spec=spec, estimate_masks=True)
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy()); specs.append(spec.cpu().numpy())
        res.append(dict(out=np.stack(outs), spec=np.stack(specs), cov=np.stack([bf.covariance(a) for a in range(A)]), blob=bf.state_save(),
                        el=bf.get_elevations()))
        bf.close()
    dev, host = res
    moved = np.stack([[angles[c][a][1] for a in range(A)] for c in range(4)])
    print("elevations per chunk (degrees):", np.rad2deg(moved).round(1).tolist())
    assert np.all(np.isfinite(dev["out"])) and np.abs(dev["out"]).max() > 0 and not np.array_equal(moved[0], moved[-1])
    for k in ("out", "spec", "cov"):
        assert dev[k].tobytes() == host[k].tobytes(), k
    assert dev["blob"] == host["blob"]


def test_seam_and_clamp():
    """uca(8, 0.05): a talker that crosses theta = pi while it rises, over three chunks, and an interferer.  Per chunk the auto call at
    the directions the tracks fill in, then one update: the own map is the twin's on the state the GPU holds, and the own track is the
    twin's track wherever the window maximum stands clear.  A seed at eps = 1.6 is stored as 1.57079637f"""
    torch = _torch()
    xyz, A, S, F = np.asarray(synth.uca(8, 0.05)), 1, 2, 12
    truth, itf = [(3.05, 0.2), (-3.05, 0.4), (-2.85, 0.6)], (-1.0, 0.0)
    n = (F + 1) * HOP
    chunks = []
    for c, (th, ep) in enumerate(truth):
        full = (synth.noise_source_stream_xyz(xyz, th, FS, 3 * F * HOP + HOP, 4, sigma=0.3, elevation=ep).astype(np.float64)
                + synth.noise_source_stream_xyz(xyz, itf[0], FS, 3 * F * HOP + HOP, 3, snr_db=60, elevation=itf[1]).astype(np.float64))
        chunks.append(full[:, c * F * HOP:c * F * HOP + n].astype(F32))
    rtf = dict(target_alpha=0.5, iterations=2, ref_mic=0, min_share=0.05)
    kw = {k: rtf[k] for k in RTF_KEYS}
    trk = dict(n_tracks=2, n_own=1, max_step_rad=0.3, min_sep_rad=0.2, hold=3)
    el_cfg = dict(max_step_el_rad=0.25, min_sep_el_rad=0.2)
    band, n_az, n_el, el_hi = (4, 124), 72, 5, 0.8
    bf = api.MvdrBeamformer(FS, xyz, N, max_streams=A, max_sources=S, geometry="xyz")
    bf.set_rtf(True, **rtf)
    bf.set_mask_estimator(True, **et.parity_config(N, S, 1))
    bf.configure_spectrum(n_az, band[0], band[1], n_peaks=2)
    bf.map_configure(n_az, n_el, 0.0, el_hi, band[0], band[1], n_peaks=2)
    bf.configure_tracks(**trk)
    bf.configure_tracks_map(**el_cfg)
    bf.seed_tracks_map(F32([[0.0, 1.0]]), F32([[1.6, -1.6]]))
    z = bf.tracks_map()
    assert z["eps"][0, 0] == F32(1.57079637) and z["eps"][0, 1] == F32(-1.57079637)
    bf.configure_tracks_map(**el_cfg)                                      # (clears the tracks)
    assert not bf.tracks_map()["alive"].any()
    saz, sel = F32([[truth[0][0] - 0.1, itf[0]]]), F32([[truth[0][1], itf[1]]])
    bf.seed_tracks_map(saz, sel)
    st = tm.seed_map(tm.new_state(), saz[0], sel[0])
    az32, el32 = bf.map_grid()
    els = mp.grid_el(n_el, 0.0, el_hi)
    worst, n_cmp, path = 0.0, 0, []
    for c in range(3):
        doa = torch.empty((A, F, S), dtype=torch.float32, device="cuda")
        bf.fill_tracks_dev(A, F, doa)
        torch.cuda.synchronize()
        rows = doa.cpu().numpy()
        want_doa, want_el = tm.fill_map(st, S)
        assert np.array_equal(rows[0], np.repeat(want_doa[None], F, axis=0)) and np.array_equal(bf.get_elevations()[0], want_el)
        # (process_sources takes doa_rad from the host; the elevations are those the fill left on the device)
        bf.process_sources(chunks[c][None], rows, estimate_masks=True)
        th0, ep0 = st["theta"][0], st["eps"][0]
        pk = bf.map(A)
        r = bf.update_tracks_map(want_map=True)
        psi, cpsi = bf.target_covariance(0, 0)
        args = (FS, N, xyz, n_az, els) + band + (psi, cpsi, bf.covariance(0), _cphi(bf, A)[0], th0, ep0)
        tw = tm.own_map(*args, **kw)
        gu, gm = r["own_used"][0, 0], r["own_map"][0, 0]
        assert np.array_equal(gu[~tw["edge"]], tw["used"][~tw["edge"]])
        if (gu != tw["used"]).any():
            tw = tm.own_map(*args, used=np.where(tw["edge"], gu, tw["used"]), **kw)
        top = tw["T"].max()
        assert top > 0
        e = float(np.abs(gm - tw["T"]).max() / top)
        worst = max(worst, e)
        assert e <= MAP_TOL, (c, e)
        win = tm.in_window(az32, el32, th0, ep0, trk["max_step_rad"], el_cfg["max_step_el_rad"])
        assert win[:, 0].any() or win[:, -1].any() or c == 0, "the window straddles the seam"
        got = _pad(bf.tracks_map())
        if tm.clear_margin_map(tw["T"], az32, el32, th0, ep0, trk["max_step_rad"], el_cfg["max_step_el_rad"]) >= CLEAR:
            paz, pel, _ = tm.window_argmax_map(tw["T"], az32, el32, th0, ep0, trk["max_step_rad"], el_cfg["max_step_el_rad"])
            tm.associate_map(st, [paz], [pel], pk["peak_az"][0], pk["peak_el"][0], pk["peak_val"][0], **trk, **el_cfg)
            for k in KEYS:
                assert np.array_equal(got[k][0], st[k]), (c, k, got[k][0], st[k])
            n_cmp += 1
        else:                                              # (not compared: the twin goes on from what the GPU holds)
            for k in KEYS:
                st[k][:] = got[k][0]
        path.append((float(got["theta"][0, 0]), float(got["eps"][0, 0])))
    bf.close()
    print("own track per chunk %s (truth %s); own maps %.2e of the map's maximum; %d of 3 updates compared" % (np.round(path, 3).tolist(), truth, worst, n_cmp))
    assert n_cmp > 0
    # (a ring in the plane z = 0 sees an elevation through cos eps alone: the azimuth is what the last assertion holds the track to)
    assert path[0][0] > 0 > path[-1][0], "across the seam"


def test_refusals_and_timing_slots():
    """every refusal of the header; none of them faults, configuration and state stay as they were.  Slot 9 counts the kernels of the
    mode, slot 8 the map kernels of an update, and an update with n_own == n_tracks adds nothing to 8"""
    torch = _torch()
    T = api.MvdrBeamformer
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    xyz = gt.array_3d(4, 4)
    lin = T(FS, synth.ULA8[:4], 64, max_streams=2, max_sources=3)
    lin.configure_spectrum(31, 1, 30)
    lin.configure_tracks(2, 0)
    with pytest.raises(api.MCArrayHipError):
        lin.configure_tracks_map(0.2, 0.1)                                 # LINEAR_X geometry
    lin.close()
    bf = T(FS, xyz, 64, max_streams=2, max_sources=3, geometry="xyz")
    bf.configure_spectrum(12, 1, 30, n_peaks=2)
    with pytest.raises(api.MCArrayHipError):
        bf.configure_tracks_map(0.2, 0.1)                                  # no tracks
    bf.configure_tracks(2, 0, max_step_rad=0.3, min_sep_rad=0.05, hold=4)
    with pytest.raises(api.MCArrayHipError):
        bf.configure_tracks_map(0.2, 0.1)                                  # no map
    with pytest.raises(api.MCArrayHipError):
        bf.get_timing(T.K_TRACKS_MAP)                                      # the slot does not exist yet
    bf.map_configure(12, 3, 0.0, 1.0, 1, 30, n_peaks=2)
    for call in (lambda: bf.update_tracks_map(), lambda: bf.tracks_map(), lambda: bf.seed_tracks_map([0.1, 0.2], [0.0, 0.0]),
                 lambda: bf.associate_tracks_map_dev(1, None, None, buf[:2], buf[2:4], buf[4:6]), lambda: bf.update_tracks_map_dev(1)):
        with pytest.raises(api.MCArrayHipError):
            call()                                                         # outside map mode the _map calls are refused
    assert bf.get_tracks_map_config()["enable"] is False
    bf.configure_tracks_map(0.2, 0.1)
    good = bf.get_tracks_map_config()
    assert good == dict(enable=True, max_step_el_rad=0.2, min_sep_el_rad=0.1)
    bf.seed_tracks_map([[0.5, np.nan], [np.nan, -0.5]], [[0.3, 0.0], [0.0, np.nan]])
    held = bf.tracks_map()
    assert held["alive"].tolist() == [[1, 0], [0, 0]] and held["gen"].tolist() == [[1, 0], [0, 0]]
    for bad in (dict(max_step_el_rad=-0.1), dict(max_step_el_rad=3.2), dict(max_step_el_rad=np.nan), dict(min_sep_el_rad=-0.1), dict(min_sep_el_rad=3.2),
                dict(min_sep_el_rad=np.inf)):
        with pytest.raises(api.MCArrayHipError):
            bf.configure_tracks_map(**dict(dict(max_step_el_rad=0.2, min_sep_el_rad=0.1), **bad))
        assert bf.get_tracks_map_config() == good
    for size, enable in ((C.sizeof(_lib.MvdrTracksMapConfig) - 4, 1), (C.sizeof(_lib.MvdrTracksMapConfig), 2)):    # a struct of another size; enable
        wrong = _lib.MvdrTracksMapConfig(size, enable, 0.2, 0.1)
        assert bf._lib.mca_hip_mvdr_tracks_set_map(bf.h, C.byref(wrong)) == -1 and bf.get_tracks_map_config() == good
    assert bf._lib.mca_hip_mvdr_tracks_set_map(bf.h, None) == -1
    # in map mode the calls on one angle are refused; the get and the fill work
    for call in (lambda: bf.seed_tracks([0.1, 0.2]), lambda: bf.update_tracks(), lambda: bf.seed_tracks_dev(1, buf), lambda: bf.update_tracks_dev(1),
                 lambda: bf.associate_tracks_dev(1, None, buf[:2], buf[2:4])):
        with pytest.raises(api.MCArrayHipError):
            call()
    for call in (lambda: bf.update_tracks_map(0), lambda: bf.update_tracks_map(3), lambda: bf.tracks_map(3), lambda: bf.seed_tracks_map_dev(3, buf, buf),
                 lambda: bf.associate_tracks_map_dev(1, None, None, buf[:9].reshape(1, 9), buf[9:18].reshape(1, 9), buf[18:27].reshape(1, 9))):
        with pytest.raises(api.MCArrayHipError):
            call()
    assert bf._lib.mca_hip_mvdr_tracks_associate_map_dev(bf.h, 1, None, None, 2, buf.data_ptr(), None, buf.data_ptr(), None) == -1
    assert bf._lib.mca_hip_mvdr_tracks_seed_map_dev(bf.h, 1, buf.data_ptr(), None, None) == -1
    assert bf._lib.mca_hip_mvdr_tracks_get_map(bf.h, 1, None, None, None, None, None) == -1
    now = bf.tracks_map()
    assert all(np.array_equal(held[k], now[k], equal_nan=True) for k in held) and np.array_equal(bf.tracks()["theta"], held["theta"])
    # timing: 9 counts the mode's launches, 8 the map kernels of an update
    bf.set_timing(True)
    bf.update_tracks_map()
    assert bf.get_timing(T.K_TRACKS_MAP)[0] == 1 and bf.get_timing(T.K_MAP)[0] == 1 and bf.get_timing(T.K_TRACKS)[0] == 0
    bf.fill_tracks_dev(1, 2, buf)
    assert bf.get_timing(T.K_TRACKS_MAP)[0] == 2 and bf.get_timing(T.K_TRACKS)[0] == 0
    bf.set_rtf(True)
    bf.configure_tracks(2, 2)
    assert bf.get_tracks_map_config()["enable"] is False                   # tracks_configure leaves map mode
    bf.configure_tracks_map(0.2, 0.1)
    bf.seed_tracks_map([[0.5, 1.0]], [[0.3, 0.0]])
    bf.update_tracks_map(1)
    n9, ms = bf.get_timing(T.K_TRACKS_MAP)
    assert n9 == 4 and ms >= 0.0 and bf.get_timing(T.K_MAP)[0] == 1, "an update with n_own == n_tracks launches no map kernel"
    bf.set_timing(False)
    with pytest.raises(api.MCArrayHipError):
        bf.get_timing(10)
    # reset and state_load zero eps with the rest
    assert bf.tracks_map()["eps"][0].tolist() != [0.0, 0.0]
    blob = bf.state_save()
    bf.reset()
    z = bf.tracks_map()
    assert all(not z[k].any() for k in z)
    bf.seed_tracks_map([[0.5, 1.0]], [[0.3, 0.2]])
    bf.state_load(blob)
    z = bf.tracks_map()
    assert all(not z[k].any() for k in z)
    # everything that disables the tracks leaves map mode
    def enter():
        bf.configure_tracks(2, 0)
        bf.configure_tracks_map(0.2, 0.1)
        assert bf.get_tracks_map_config()["enable"] is True
    for leave in (lambda: bf.set_elevations(np.zeros((2, 3), dtype=F32)), lambda: bf.set_elevations_dev(1, buf[:3]), lambda: bf.set_max_sources(1),
                  lambda: bf.set_rtf(False)):
        enter()
        leave()
        assert bf.get_tracks_map_config()["enable"] is False and bf.get_tracks_config()["enable"] is False
        with pytest.raises(api.MCArrayHipError):
            bf.update_tracks_map()
        bf.set_max_sources(3)
    enter()
    bf.set_geometry("xyz", 0.2)
    assert bf.get_tracks_map_config()["enable"] is False
    with pytest.raises(api.MCArrayHipError):
        bf.configure_tracks_map(0.2, 0.1)                                  # the tracks, the spectrum and the map are configured anew
    # leaving by enable = 0: the calls on one angle work again, every slot is unset
    bf.configure_spectrum(12, 1, 30)
    bf.map_configure(12, 3, 0.0, 1.0, 1, 30)
    enter()
    bf.seed_tracks_map([[0.5, 1.0]], [[0.3, 0.2]])
    bf.fill_tracks_dev(1, 2, buf)
    assert np.array_equal(bf.get_elevations(1)[0, :2], F32([0.3, 0.2]))
    bf.configure_tracks_map(0.2, 0.1, enable=False)
    assert bf.get_tracks_config()["enable"] is True and np.isnan(bf.get_elevations()).all() and not bf.tracks()["alive"].any()
    bf.seed_tracks([0.1, 0.2])
    bf.update_tracks()
    bf.close()


def test_scene_on_the_gpu():
    """the scene of tests/test_mvdr_tracks_map_twin.py through the GPU, once: the auto call at the directions and elevations the fill
    writes, update_tracks_map() per chunk.  Bars: the own track within one grid cell per axis (5 and 10 degrees) of the twin's after
    every chunk -- a float32 near-tie can move an argmax by one cell, and the window pulls it back; the last chunk's output spectra
    within 5e-4 of the twin's peak outside the cells at a decision edge of either estimator (at most 1 % of the cells, which
    tests/test_mvdr_tracks_map_twin.py holds the scene to on the twin alone).  Measured once on the MI355X: the own track 25, 25, 25,
    25, 30, 30, 30, 35 degrees in azimuth and 20, 20, 20, 20, 30, 30, 30, 40 in elevation, the twin's in every chunk; the spectra
    7.3e-6 and 2.0e-5 of the peak over all cells, 0.78 % of them at an edge"""
    import mvdr_rtf_twin as rt
    torch = _torch()
    runs = tm.scene_runs()
    sc, tw = runs["sc"], runs["tracked"]
    fs, n_fft, hop = rt.SCENE_FS, rt.SCENE_N, rt.SCENE_N // 2
    m, trk = tm.SCENE_MAP, tm.SCENE_TRACKS
    bf = api.MvdrBeamformer(fs, sc["xyz"], n_fft, max_streams=1, max_sources=2, geometry="xyz")
    bf.set_rtf(True, **et.SCENE_RTF)
    bf.set_mask_estimator(True, **et.SCENE_CFG)
    bf.configure_spectrum(m["n_az"], tm.SCENE_BAND[0], tm.SCENE_BAND[1], n_peaks=2)
    bf.map_configure(m["n_az"], m["n_el"], m["el_lo"], m["el_hi"], tm.SCENE_BAND[0], tm.SCENE_BAND[1], n_peaks=2)
    bf.configure_tracks(trk["n_tracks"], trk["n_own"], max_step_rad=trk["max_step_rad"], min_sep_rad=trk["min_sep_rad"], hold=trk["hold"])
    bf.configure_tracks_map(trk["max_step_el_rad"], trk["min_sep_el_rad"])
    bf.seed_tracks_map(F32([[tm.SCENE_TRUTH_AZ[0], tm.SCENE_ITF[0]]]), F32([[tm.SCENE_TRUTH_EL[0], tm.SCENE_ITF[1]]]))
    thetas, epss = [], []
    doa = torch.empty((1, tm.SCENE_CF, 2), dtype=torch.float32, device="cuda")
    for c in range(tm.SCENE_CHUNKS):
        bf.fill_tracks_dev(1, tm.SCENE_CF, doa)
        torch.cuda.synchronize()
        rows, el = doa.cpu().numpy(), bf.get_elevations()[0]
        f0, f1 = c * tm.SCENE_CF, (c + 1) * tm.SCENE_CF
        r = bf.process_sources(sc["pcm"][None, :, f0 * hop:(f1 + 1) * hop].copy(), rows, estimate_masks=True)
        bf.update_tracks_map()
        t = bf.tracks_map()
        thetas.append(float(t["theta"][0, 0])); epss.append(float(t["eps"][0, 0]))
    bf.close()
    thetas, epss = np.array(thetas), np.array(epss)
    d_az = np.abs(thetas - tw["theta"]) / (2 * np.pi / m["n_az"])
    d_el = np.abs(epss - tw["eps"]) / ((m["el_hi"] - m["el_lo"]) / (m["n_el"] - 1))
    last = tw["run"]
    want_doa, want_el = tw["last_rows"]
    assert np.array_equal(rows[0, 0], want_doa) and np.array_equal(el, want_el, equal_nan=True)      # the last chunk ran at the twin's directions
    edge = tm.scene_edge_cells(sc, tw)
    d = np.abs(r["spec"][0].astype(np.complex128) - last["spec"])
    peak = np.abs(last["spec"]).max(axis=(1, 2))
    e_spec, e_all = (d * ~edge).max(axis=(1, 2)) / peak, d.max(axis=(1, 2)) / peak
    print("own track per chunk: GPU az %s el %s, twin az %s el %s degrees (%.2f / %.2f grid cells apart at most); last chunk's output spectra against the "
          "twin's: %s of the peak outside %.2f %% edge cells (%s over all cells)"
          % (np.rad2deg(thetas).round(1).tolist(), np.rad2deg(epss).round(1).tolist(), np.rad2deg(tw["theta"]).round(1).tolist(), np.rad2deg(tw["eps"]).round(1).tolist(),
             d_az.max(), d_el.max(), ["%.2e" % v for v in e_spec], 100.0 * edge.mean(), ["%.2e" % v for v in e_all]))
    assert d_az.max() <= 1.0 + 1e-3 and d_el.max() <= 1.0 + 1e-3
    assert e_spec.max() <= MAP_TOL and edge.mean() <= 0.01
