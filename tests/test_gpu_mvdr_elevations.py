"""GPU: an elevation per look-direction slot of the MVDR context (mca_hip_mvdr_set_elevations_*).

Unset slots are the context without the call, byte for byte; the host call with one value everywhere is a context created at that
elevation, byte for byte; the device call and mixed elevations stay within the module's bars (5e-4 of the peak for spectra and audio,
5e-6 for the covariance) of that context and of the per-slot twin (tests/mvdr_map_twin.slot_elevations); the loop
map peaks -> doa_rad + set_elevations_dev -> next chunk runs without a host step.  Every test prints its worst figure."""
import numpy as np
import pytest

from mcarray_amd import api

import mvdr_estmask_twin as et
import mvdr_geometry_twin as gt
import mvdr_map_twin as mp
import mvdr_mask_twin as mt
import mvdr_nulls_twin as nt
import mvdr_rtf_twin as rt

pytestmark = pytest.mark.gpu

SPEC_TOL, AUDIO_TOL, COV_TOL = 5e-4, 5e-4, 5e-6
FS, N, K, HOP = 16000, 256, 129, 128
F = rt.PARITY_F
A, S = 2, 3
F32 = np.float32


def _torch():
    import torch
    return torch


def _cube():
    return gt.array_3d(7)


def _pcm(xyz, frames, elevation=0.0):
    return np.stack([gt.two_sources_xyz(xyz, FS, N, frames, 2.6 - 1.7 * a, -0.9 + 2.2 * a, seed=a, elevation=elevation) for a in range(A)])


def _err(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def _masks():
    upd = np.ascontiguousarray(np.concatenate([mt.mask_for(K, A, 12)[:, :F], mt.mask_for(K, A, 12)[:, 6:6 + F]], axis=1))
    tm = rt.target_parity_mask(S, A, 12, K)
    return upd, np.ascontiguousarray(np.concatenate([tm[:, :, :F], tm[:, :, 6:6 + F]], axis=2))


def _every_call(bf, pcm, doa):
    """every frames call on one context, each continuing the one before: sources with null gain 10, masked, RTF, auto; then the
    covariance and steering() -> list of arrays"""
    upd, tmask = _masks()
    M = pcm.shape[1]
    cut = lambda i: pcm[:, :, i * F * HOP:((i + 1) * F + 1) * HOP].copy()
    res = []
    r = bf.process_sources(cut(0), doa[:, :F].copy())
    res += [r["spec"].view(F32), r["out"]]
    r = bf.process_sources(cut(1), doa[:, F:2 * F].copy(), update_mask=upd[:, :F])
    res += [r["spec"].view(F32), r["out"]]
    bf.set_rtf(True, **rt.parity_config(M))
    bf.set_rtf_nulls(True)
    r = bf.process_sources(cut(2), doa[:, 2 * F:3 * F].copy(), update_mask=upd[:, F:], target_mask=tmask[:, :, F:])
    res += [r["spec"].view(F32), r["out"]]
    bf.set_mask_estimator(True, **et.parity_config(N, S, 1))
    r = bf.process_sources(cut(3), doa[:, 3 * F:].copy(), estimate_masks=True)
    res += [r["spec"].view(F32), r["out"], r["update_mask"], r["target_mask"]]
    res += [np.stack([bf.covariance(a) for a in range(A)])]
    for a in range(A):
        for s in range(S):
            d, e = bf.steering(0.7 - 2.0 * a + s, a, s)
            res += [d, e]
    return res


def _context(el, **kw):
    return api.MvdrBeamformer(FS, _cube(), N, max_streams=A, max_sources=S, null_gain=10.0, geometry="xyz", elevation_rad=el, **kw)


# ---- 1. unset is the context's elevation, byte for byte ----
def test_unset_and_nan_are_the_context_without_the_call():
    el = 0.4
    pcm, doa = _pcm(_cube(), 4 * F, el), gt.drifting_azimuths(A, 4 * F, S)
    runs = []
    for how in ("none", "host", "dev"):
        bf = _context(el)
        if how == "host":
            bf.set_elevations(np.full((A, S), np.nan))
        elif how == "dev":
            torch = _torch()
            bf.set_elevations_dev(A, torch.full((A, S), float("nan"), dtype=torch.float32, device="cuda:0"))
        assert np.isnan(bf.get_elevations()).all()
        runs.append(_every_call(bf, pcm, doa))
        bf.close()
    for how, run in zip(("host", "dev"), runs[1:]):
        assert len(run) == len(runs[0]) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(runs[0], run)), how
    assert np.abs(runs[0][1]).max() > 0
    print("NaN everywhere (host call, device call): sources, masked, RTF and auto calls, covariance and steering() byte-identical")


# ---- 2. one value everywhere is a context created at that elevation ----
def test_one_elevation_everywhere_is_a_context_at_that_elevation():
    el = 0.375
    pcm, doa = _pcm(_cube(), 4 * F, el), gt.drifting_azimuths(A, 4 * F, S)
    ref = _context(el)
    want = _every_call(ref, pcm, doa)
    ref.close()
    # the host call: the bytes
    bf = _context(0.0)
    bf.set_elevations(np.full((A, S), el))
    assert np.array_equal(bf.get_elevations(), np.full((A, S), F32(el)))
    got = _every_call(bf, pcm, doa)
    bf.close()
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(want, got))
    # the device call: the device's cos and sin, within the module's bars
    torch = _torch()
    bf = _context(0.0)
    bf.set_elevations_dev(A, torch.full((A, S), el, dtype=torch.float32, device="cuda:0"))
    assert np.array_equal(bf.get_elevations(), np.full((A, S), F32(el)))
    dev = _every_call(bf, pcm, doa)
    bf.close()
    worst = [0.0, 0.0, 0.0]
    for i in range(4):                                                      # spectra and audio of the four calls
        spec_w, spec_d = want[[0, 2, 4, 6][i]], dev[[0, 2, 4, 6][i]]
        out_w, out_d = want[[1, 3, 5, 7][i]], dev[[1, 3, 5, 7][i]]
        worst[0], worst[1] = max(worst[0], _err(spec_d, spec_w)), max(worst[1], _err(out_d, out_w))
    worst[2] = _err(dev[10], want[10])
    print("0.375 in every slot: host call byte-identical to a context at 0.375; device call spectra %.2e audio %.2e covariance %.2e" % tuple(worst))
    assert worst[0] <= SPEC_TOL and worst[1] <= AUDIO_TOL and worst[2] <= COV_TOL, worst


# ---- 3. mixed elevations against the per-slot twin ----
ELS = np.array([[-0.3, 0.2, 0.9], [0.9, np.nan, 0.2]])                    # per stream and slot; a NaN: the context's 0.1
CTX_EL = 0.1


@pytest.mark.parametrize("how", ["host", "dev"])
def test_mixed_elevations_against_the_per_slot_twin(how):
    from test_gpu_mvdr_rtf import _check_call
    xyz = _cube()
    M = len(xyz)
    pcm, doa = _pcm(xyz, 2 * F, 0.3), gt.drifting_azimuths(A, 2 * F, S)
    pcm64 = pcm.astype(np.float64)
    upd, tmask = _masks()

    def ctx():
        bf = _context(CTX_EL)
        if how == "host":
            bf.set_elevations(ELS)
        else:
            torch = _torch()
            bf.set_elevations_dev(A, torch.tensor(ELS, dtype=torch.float32, device="cuda:0"))
        assert np.array_equal(bf.get_elevations(), ELS.astype(F32), equal_nan=True)
        return bf

    def check(r, tw, a, w):
        es, ea = _err(r["spec"][a], tw["spec"]), _err(r["out"][a], tw["out"])
        w[0], w[1] = max(w[0], es), max(w[1], ea)
        assert np.all(np.isfinite(r["spec"][a])) and es <= SPEC_TOL and ea <= AUDIO_TOL, (a, es, ea)

    worst = {}
    # sources with null gain 10, then the masked call continuing it
    w = worst["sources"], worst["masked"] = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    bf = ctx()
    r1 = bf.process_sources(pcm[:, :, :(F + 1) * HOP].copy(), doa[:, :F].copy())
    cov1 = [bf.covariance(a) for a in range(A)]
    r2 = bf.process_sources(pcm[:, :, F * HOP:].copy(), doa[:, F:].copy(), update_mask=upd[:, F:])
    for a in range(A):
        with mp.slot_elevations(ELS[a], CTX_EL):
            t1 = nt.mvdr_nulls_stream(FS, N, xyz, pcm64[a, :, :(F + 1) * HOP], doa[a, :F], 10.0)
            t2 = mt.mvdr_mask_stream(FS, N, xyz, pcm64[a, :, F * HOP:], doa[a, F:], 10.0, upd[a, F:], state=t1)
        check(r1, t1, a, w[0])
        check(r2, t2, a, w[1])
        w[0][2], w[1][2] = max(w[0][2], _err(cov1[a], t1["phi"])), max(w[1][2], _err(bf.covariance(a), t2["phi"]))
        # the elevation matters: the twin at the context's elevation everywhere is outside the bar tenfold
        with gt.xyz_mode(CTX_EL):
            flat = nt.mvdr_nulls_stream(FS, N, xyz, pcm64[a, :, :(F + 1) * HOP], doa[a, :F], 10.0)
        assert _err(r1["spec"][a], flat["spec"]) > 10 * SPEC_TOL
    assert w[0][2] <= COV_TOL and w[1][2] <= COV_TOL, w
    bf.close()
    # the RTF call, two calls: cells at a decision edge of the twin's estimator are left out, as in tests/test_gpu_mvdr_rtf.py
    w = worst["rtf"] = [0.0, 0.0, 0.0]
    cfg = rt.parity_config(M)
    bf = ctx()
    bf.set_null_gain(0.0)                                                   # (mvdr_rtf_twin has no nulls)
    bf.set_rtf(True, **cfg)
    prev, st, shares = [np.zeros((S, HOP)) for _ in range(A)], [None] * A, []
    for i, (t0, t1) in enumerate(((0, F), (F, 2 * F))):
        r = bf.process_sources(pcm[:, :, t0 * HOP:(t1 + 1) * HOP].copy(), doa[:, t0:t1].copy(), update_mask=upd[:, t0:t1], target_mask=tmask[:, :, t0:t1])
        for a in range(A):
            with mp.slot_elevations(ELS[a], CTX_EL):
                st[a] = rt.mvdr_rtf_stream(FS, N, xyz, pcm64[a, :, t0 * HOP:(t1 + 1) * HOP], doa[a, t0:t1], upd[a, t0:t1], tmask[a, :, t0:t1],
                                           state=st[a], **cfg)
            prev[a] = _check_call(r, st[a], a, "mixed elevations rtf call %d" % i, w, prev[a], None)
            w[2] = max(w[2], _err(bf.covariance(a), st[a]["phi"]))
            shares.append(float(rt.edges_of(st[a]).mean()))
            assert st[a]["est"].any()
    assert w[2] <= COV_TOL and max(shares) <= 0.01, (w, shares)
    bf.close()
    for label, w in worst.items():
        print("mixed elevations (%s call) %s: spectra %.2e audio %.2e of the peak, covariance %.2e" % (how, label, w[0], w[1], w[2]))


@pytest.mark.parametrize("n_fft", [512, 1024])
def test_mixed_elevations_long_frames(n_fft):
    """k_mvdr_analyse_512 and k_mvdr_analyse_1024 read the slot's pair: three directions with null gain 10, four frames"""
    fs, xyz, F4, hop = 48000, gt.array_3d(9, 5), 4, n_fft // 2
    pcm = np.stack([gt.two_sources_xyz(xyz, fs, n_fft, F4, 2.6 - 1.7 * a, -0.9 + 2.2 * a, seed=a, elevation=0.3) for a in range(A)])
    doa = gt.drifting_azimuths(A, F4, S)
    bf = api.MvdrBeamformer(fs, xyz, n_fft, max_streams=A, max_sources=S, null_gain=10.0, geometry="xyz", elevation_rad=CTX_EL)
    bf.set_elevations(ELS)
    r = bf.process_sources(pcm, doa)
    w = [0.0, 0.0, 0.0]
    for a in range(A):
        with mp.slot_elevations(ELS[a], CTX_EL):
            tw = nt.mvdr_nulls_stream(fs, n_fft, xyz, pcm[a].astype(np.float64), doa[a], 10.0)
        w[0], w[1] = max(w[0], _err(r["spec"][a], tw["spec"])), max(w[1], _err(r["out"][a], tw["out"]))
        w[2] = max(w[2], _err(bf.covariance(a), tw["phi"]))
    bf.close()
    print("N %d mixed elevations: spectra %.2e audio %.2e of the peak, covariance %.2e" % (n_fft, w[0], w[1], w[2]))
    assert w[0] <= SPEC_TOL and w[1] <= AUDIO_TOL and w[2] <= COV_TOL


# ---- 4. the loop: map peaks -> doa_rad + set_elevations_dev -> the next chunk, no host step ----
def test_the_loop_from_map_peaks_to_the_next_chunk():
    torch = _torch()
    dev = torch.device("cuda:0")
    sc = [mp.scene("cube7", s) for s in mp.SEEDS]
    xyz, P2 = sc[0]["xyz"], 2
    pcm = np.stack([s["pcm"] for s in sc])                                  # [A][M][(12 + 1) hop]
    F1 = mp.F // 2
    bf = api.MvdrBeamformer(FS, xyz, N, max_streams=A, max_sources=P2, geometry="xyz", elevation_rad=CTX_EL)
    bf.map_configure(mp.N_AZ, mp.N_EL, mp.EL_LO, mp.EL_HI, n_peaks=P2)
    d_pcm = torch.tensor(pcm, device=dev)
    first = gt.drifting_azimuths(A, F1, P2)
    out = [torch.zeros((A, P2, F1 * HOP), dtype=torch.float32, device=dev) for _ in range(2)]
    spec = [torch.zeros((A, P2, F1, K, 2), dtype=torch.float32, device=dev) for _ in range(2)]
    paz, pel = (torch.zeros((A, P2), dtype=torch.float32, device=dev) for _ in range(2))
    # chunk 1 at the context's elevation; the peaks of the map; chunk 2 at the peaks -- one stream of work, nothing read back between
    bf.process_sources_dev(d_pcm[:, :, :(F1 + 1) * HOP], F1, torch.tensor(first, device=dev), out[0], spec[0])
    bf.map_dev(A, peak_az=paz, peak_el=pel)
    bf.set_elevations_dev(A, pel)
    bf.process_sources_dev(d_pcm[:, :, F1 * HOP:], F1, paz[:, None, :].expand(A, F1, P2).contiguous(), out[1], spec[1])
    torch.cuda.synchronize()
    az, el = paz.cpu().numpy(), pel.cpu().numpy()
    assert np.array_equal(bf.get_elevations(), el)
    worst = [0.0, 0.0, 0.0]
    for a in range(A):
        with gt.xyz_mode(CTX_EL):
            t1 = nt.mvdr_nulls_stream(FS, N, xyz, pcm[a, :, :(F1 + 1) * HOP].astype(np.float64), first[a], 0.0)
        # the peaks are the talkers' cells already after six frames?  Not asserted: the twin runs on the peaks the GPU picked
        with mp.slot_elevations(el[a].astype(np.float64), CTX_EL):
            t2 = nt.mvdr_nulls_stream(FS, N, xyz, pcm[a, :, F1 * HOP:].astype(np.float64), np.broadcast_to(az[a], (F1, P2)), 0.0, state=t1)
        for i, tw in enumerate((t1, t2)):
            g = spec[i][a].cpu().numpy()
            worst[0] = max(worst[0], _err(g[..., 0] + 1j * g[..., 1], tw["spec"]))
            worst[1] = max(worst[1], _err(out[i][a].cpu().numpy(), tw["out"]))
        worst[2] = max(worst[2], _err(bf.covariance(a), t2["phi"]))
    bf.close()
    print("loop: peaks az %s el %s; spectra %.2e audio %.2e of the peak, covariance %.2e" % (az.tolist(), el.tolist(), *worst))
    assert len(set(el.reshape(-1).tolist())) > 1                            # the second angle is in use
    assert worst[0] <= SPEC_TOL and worst[1] <= AUDIO_TOL and worst[2] <= COV_TOL, worst


# ---- 5. bookkeeping ----
def test_bookkeeping_tracks_geometry_reset_and_refusals():
    from mcarray_amd import _lib
    xyz = _cube()
    bf = api.MvdrBeamformer(FS, xyz, N, max_streams=A, max_sources=S, geometry="xyz", elevation_rad=CTX_EL)
    lib, fp = bf._lib, _lib.c_fp
    bf.process_sources(_pcm(xyz, F), gt.drifting_azimuths(A, F, S))
    assert np.isnan(bf.get_elevations()).all()                              # the initial state
    bf.set_elevations(ELS)
    # the host call refuses the whole array and changes nothing
    for bad in (1.6, -1.6, np.inf, -np.inf):
        e = ELS.astype(F32).copy()
        e[1, 2] = bad
        assert lib.mca_hip_mvdr_set_elevations_host(bf.h, A, e.ctypes.data_as(fp)) == -1 and lib.mca_hip_mvdr_last_error(bf.h)
    assert lib.mca_hip_mvdr_set_elevations_host(bf.h, A, None) == -1 and lib.mca_hip_mvdr_get_elevations(bf.h, A, None) == -1
    e = ELS.astype(F32).copy()
    for n in (0, A + 1):
        assert lib.mca_hip_mvdr_set_elevations_host(bf.h, n, e.ctypes.data_as(fp)) == -1
        assert lib.mca_hip_mvdr_set_elevations_dev(bf.h, n, e.ctypes.data_as(fp), None) == -1
    assert lib.mca_hip_mvdr_set_elevations_dev(bf.h, A, None, None) == -1
    assert np.array_equal(bf.get_elevations(), ELS.astype(F32), equal_nan=True)
    # the ends of the range are accepted, the float nearest to pi/2 among them; n_streams = 1 leaves stream 1 alone
    bf.set_elevations(np.array([[F32(np.pi / 2), -np.pi / 2, 0.0]]))
    got = bf.get_elevations()
    assert np.array_equal(got[0], np.array([np.pi / 2, -np.pi / 2, 0.0], dtype=F32)) and np.array_equal(got[1], ELS[1].astype(F32), equal_nan=True)
    # the device call clamps; NaN stays unset
    torch = _torch()
    bf.set_elevations_dev(A, torch.tensor([[2.0, -7.0, float("inf")], [float("-inf"), float("nan"), 0.25]], dtype=torch.float32, device="cuda:0"))
    h = F32(np.pi / 2)
    assert np.array_equal(bf.get_elevations(), np.array([[h, -h, h], [-h, np.nan, 0.25]], dtype=F32), equal_nan=True)
    # mca_hip_mvdr_reset keeps them
    bf.set_elevations(ELS)
    bf.reset()
    assert np.array_equal(bf.get_elevations(), ELS.astype(F32), equal_nan=True)
    # setting elevations disables the tracks; configuring the tracks resets the elevations
    bf.configure_spectrum(72, n_peaks=2)
    bf.configure_tracks(2)
    assert bf.get_tracks_config()["enable"] and np.isnan(bf.get_elevations()).all()
    bf.set_elevations(ELS)
    assert not bf.get_tracks_config()["enable"]
    with pytest.raises(api.MCArrayHipError):
        bf.update_tracks()
    bf.configure_tracks(2)
    bf.set_elevations_dev(A, torch.zeros((A, S), dtype=torch.float32, device="cuda:0"))
    assert not bf.get_tracks_config()["enable"]
    bf.configure_tracks(2, enable=False)                                    # a disabled configuration leaves the elevations alone
    assert np.array_equal(bf.get_elevations(), np.zeros((A, S), dtype=F32))
    # a geometry change resets them; one that changes nothing does not
    bf.set_elevations(ELS)
    bf.set_geometry("xyz", CTX_EL)
    assert np.array_equal(bf.get_elevations(), ELS.astype(F32), equal_nan=True)
    bf.set_geometry("xyz", 0.3)
    assert np.isnan(bf.get_elevations()).all()
    # max_sources: the array is [streams][max_sources], and the slots a smaller setting hides keep their values
    bf.set_elevations(ELS)
    bf.set_max_sources(2)
    assert np.array_equal(bf.get_elevations(), ELS[:, :2].astype(F32), equal_nan=True)
    with pytest.raises(api.MCArrayHipError):
        bf.set_elevations(ELS)
    bf.set_max_sources(3)
    assert np.array_equal(bf.get_elevations(), ELS.astype(F32), equal_nan=True)
    bf.close()
