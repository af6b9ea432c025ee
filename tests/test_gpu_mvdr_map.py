"""GPU: the azimuth x elevation Capon map of the MVDR context (mca_hip_mvdr_map_*).

One elevation row at the context's elevation is the 1-D spectrum call byte for byte; the map is the float64 twin
(tests/mvdr_map_twin.py) on the covariance the GPU holds within 5e-4 of the map's maximum, the module's bar for a spectrum row; the
peak kernel is the twin's rule on the GPU's own map exactly, and on the scenes the picked cells are the twin's.  Every test prints its
worst figure."""
import numpy as np
import pytest

from mcarray_amd import api, synth

import mvdr_geometry_twin as gt
import mvdr_map_twin as mt

pytestmark = pytest.mark.gpu

MAP_TOL = 5e-4               # of the map's maximum (the bar of a spectrum row)
FS, N, F = mt.FS, mt.N, mt.F
F32 = np.float32


def _torch():
    import torch
    return torch


def _two(xyz, A, elevation=0.0):
    """[A][M][(F+1) hop]: two talkers per stream, in front of and behind the array"""
    return np.stack([gt.two_sources_xyz(xyz, FS, N, F, 2.6 - 1.7 * a, -0.9 + 2.2 * a, seed=a, elevation=elevation) for a in range(A)])


def _same(r, q):
    return all(np.array_equal(r[k], q[k]) for k in r)


def _rule_on_own_map(r, els, n_peaks, ctx_el):
    """the peak kernel against the twin's rule on the map the GPU wrote: exact"""
    for a in range(r["map"].shape[0]):
        idx, paz, pel, val = mt.peaks(r["map"][a], n_peaks, els, ctx_el=ctx_el)
        assert np.array_equal(r["peak_az"][a], paz) and np.array_equal(r["peak_el"][a], pel), (a, idx, r["peak_az"][a], r["peak_el"][a])
        assert np.array_equal(r["peak_val"][a], val.astype(F32)), (a, idx)


# ---- 1. bytes against the 1-D call ----
TILE = 128                   # directions of a workgroup of the scan (MVDR_MAP_TILE)
ROWS = {"uca6": (lambda: synth.uca(6, 0.045), 0.0), "cube3": (lambda: gt.array_3d(3), 0.375), "cube7": (lambda: gt.array_3d(7), 0.375),
        "cube16": (lambda: gt.array_3d(16), 0.375)}


@pytest.mark.parametrize("name", list(ROWS))
def test_one_row_at_the_contexts_elevation_has_the_bytes_of_the_spectrum_call(name):
    """n_el = 1, el_lo = el_hi = the context's elevation: map, peak azimuths and peak values are those of mca_hip_mvdr_spectrum_* with
    n_angles = n_az -- D below, at and above a wave, D across the direction tile, Q = 1, 2, 4 row slots"""
    xyz, el = ROWS[name][0](), ROWS[name][1]
    A = 2
    bf = api.MvdrBeamformer(FS, xyz, N, max_streams=A, geometry="xyz", elevation_rad=el)
    bf.process(_two(xyz, A, el), 0.0)
    for D in (3, 63, 64, 65, TILE + 72):
        for weighting, band in (("normalised", (1, 127)), ("power", (20, 90))):
            bf.configure_spectrum(D, band[0], band[1], weighting, n_peaks=4)
            bf.map_configure(D, 1, el, el, band[0], band[1], weighting, n_peaks=4)
            s, m = bf.spectrum(), bf.map()
            assert s["spectrum"].max() > 0
            assert np.array_equal(m["map"][:, 0, :], s["spectrum"]), (name, D, weighting)
            assert np.array_equal(m["peak_az"], s["peak_doa"]) and np.array_equal(m["peak_val"], s["peak_val"]), (name, D, weighting)
            assert np.array_equal(m["peak_el"], np.full((A, 4), F32(el)))
            az, e1 = bf.map_grid()
            assert np.array_equal(az, bf.spectrum_grid()) and np.array_equal(e1, [F32(el)])
    bf.close()
    print("%s: map == spectrum, bytes, D = 3, 63, 64, 65, %d" % (name, TILE + 72))


# ---- 2. parity with the twin ----
@pytest.mark.parametrize("name", sorted(mt.SCENES))
def test_parity_with_the_twin_on_the_scenes(name):
    """streams 0 and 1: the scene with seeds 0 and 1; stream 2: digital silence.  The twin runs on the covariance the GPU holds."""
    sc = [mt.scene(name, s) for s in mt.SEEDS]
    xyz, els, ctx_el = sc[0]["xyz"], sc[0]["els"], 0.2
    pcm = np.stack([sc[0]["pcm"], sc[1]["pcm"], np.zeros_like(sc[0]["pcm"])])
    bf = api.MvdrBeamformer(FS, xyz, N, max_streams=3, geometry="xyz", elevation_rad=ctx_el)
    bf.process(pcm, 0.0)
    cov = [bf.covariance(a) for a in range(2)]
    worst = 0.0
    for weighting, band in ((mt.NORMALISED, mt.BAND), (mt.POWER, mt.BAND), (mt.NORMALISED, (30, 99)), (mt.POWER, (64, 64))):
        bf.map_configure(mt.N_AZ, mt.N_EL, mt.EL_LO, mt.EL_HI, band[0], band[1], weighting, n_peaks=3)
        r = bf.map()
        az, el = bf.map_grid()
        assert np.array_equal(az, gt.grid_xyz(mt.N_AZ).astype(F32)) and np.array_equal(el, els.astype(F32))
        _rule_on_own_map(r, els, 3, ctx_el)
        for a in range(2):
            P = mt.capon_map(cov[a], FS, N, xyz, mt.N_AZ, els, band[0], band[1], weighting)
            err = float(np.abs(r["map"][a] - P).max() / P.max())
            worst = max(worst, err)
            assert err <= MAP_TOL, (name, weighting, band, a, err)
            if weighting == mt.NORMALISED and band == mt.BAND:
                idx, paz, pel, val = mt.peaks(P, 3, els, ctx_el=ctx_el)
                assert sorted((int(c) // mt.N_AZ, int(c) % mt.N_AZ) for c in idx[:2]) == sorted(mt.TALKERS)
                assert np.array_equal(r["peak_az"][a, :2], paz[:2]) and np.array_equal(r["peak_el"][a, :2], pel[:2]), (name, a)
                assert np.abs(r["peak_val"][a, :2] - val[:2]).max() <= MAP_TOL * P.max()
        # the silent stream: a zero map, every slot at value 0, azimuth 0 and the context's elevation
        assert not r["map"][2].any() and not r["peak_val"][2].any() and not r["peak_az"][2].any()
        assert np.array_equal(r["peak_el"][2], np.full(3, F32(ctx_el)))
    bf.close()
    print("%s: map within %.3g of its maximum of the twin (bar %.1g); picked cells are the talkers'" % (name, worst, MAP_TOL))


def test_2048_directions():
    """n_az n_el = 2048 at M = 3: every tile, a full last thread cell, the pick's eight cells a thread"""
    xyz, n_az, n_el, lo, hi = gt.array_3d(3), 128, 16, -np.pi / 2, np.pi / 2
    els = mt.grid_el(n_el, lo, hi)
    A = 2
    bf = api.MvdrBeamformer(FS, xyz, N, max_streams=A, geometry="xyz")
    bf.process(_two(xyz, A), 0.0)
    bf.map_configure(n_az, n_el, lo, hi, n_peaks=4)
    r = bf.map()
    _rule_on_own_map(r, els, 4, 0.0)
    worst = 0.0
    for a in range(A):
        P = mt.capon_map(bf.covariance(a), FS, N, xyz, n_az, els, 1, 127, mt.NORMALISED)
        worst = max(worst, float(np.abs(r["map"][a] - P).max() / P.max()))
    assert worst <= MAP_TOL, worst
    bf.close()
    print("2048 directions: within %.3g of the maximum" % worst)


# ---- 3. reproducible, read-only, independent of the batch; the workspace passes ----
def test_reproducible_read_only_and_independent_of_the_batch_and_the_workspace():
    xyz = gt.array_3d(7)
    pcm = _two(xyz, 3)
    bf = api.MvdrBeamformer(FS, xyz, N, max_streams=3, geometry="xyz")
    bf.set_timing(True)
    bf.process(pcm, 0.0)
    bf.map_configure(40, 5, -0.5, 1.0, n_peaks=3)
    blob = bf.state_save()
    r = bf.map()
    assert r["map"].min() > 0 and bf.state_save() == blob                  # reads the state, writes none
    assert _same(r, bf.map())                                              # the same bytes on every run
    for n in (1, 2):                                                       # whatever n_streams is
        q = bf.map(n)
        assert all(np.array_equal(q[k], r[k][:n]) for k in r), n
    launches = bf.get_timing(bf.K_MAP)[0]
    assert launches == 4 and bf.get_timing(bf.K_SPECTRUM)[0] == 0
    # wherever a stream sits in the batch
    other = api.MvdrBeamformer(FS, xyz, N, max_streams=2, geometry="xyz")
    other.process(np.ascontiguousarray(pcm[[2, 0]]), 0.0)
    other.map_configure(40, 5, -0.5, 1.0, n_peaks=3)
    q = other.map()
    assert all(np.array_equal(q[k][0], r[k][2]) and np.array_equal(q[k][1], r[k][0]) for k in r)
    other.close()
    # a workspace cap below the partial sums of one stream: one stream a pass, the same bytes
    bf.set_rtf_workspace(8)
    assert _same(r, bf.map())
    bf.set_rtf_workspace(2 * 2 * 4 * 256 * 4)                              # two streams a pass (2 chunks x 4 waves x 256 directions), then one
    assert _same(r, bf.map())
    # the device-pointer call, any one output alone
    torch = _torch()
    dev = torch.device("cuda:0")
    m = torch.zeros((3, 5, 40), dtype=torch.float32, device=dev)
    pk = [torch.zeros((3, 3), dtype=torch.float32, device=dev) for _ in range(3)]
    bf.map_dev(3, map=m, peak_az=pk[0], peak_el=pk[1], peak_val=pk[2])
    torch.cuda.synchronize()
    assert np.array_equal(m.cpu().numpy(), r["map"])
    assert all(np.array_equal(t.cpu().numpy(), r[k]) for t, k in zip(pk, ("peak_az", "peak_el", "peak_val")))
    only = torch.zeros((3, 3), dtype=torch.float32, device=dev)
    bf.map_dev(3, peak_el=only)
    torch.cuda.synchronize()
    assert np.array_equal(only.cpu().numpy(), r["peak_el"])
    bf.close()


# ---- 4. refusals: each leaves the former configuration in place ----
def test_refusals_leave_the_configuration_in_place():
    from mcarray_amd import _lib
    import ctypes as C
    INVALID = -1
    xyz = gt.array_3d(4)
    bf = api.MvdrBeamformer(FS, xyz, N, max_streams=2)
    bf.process(_two(xyz, 2), 0.0)
    lib, fp = bf._lib, _lib.c_fp
    buf = np.zeros((2, 2048), dtype=np.float32)

    def cfg(n_az=36, n_el=7, lo=-0.5, hi=1.0, bin_lo=1, bin_hi=127, weighting=1, n_peaks=2, size=None):
        return _lib.MvdrMapConfig(C.sizeof(_lib.MvdrMapConfig) if size is None else size, n_az, n_el, lo, hi, bin_lo, bin_hi, weighting, n_peaks)

    # LINEAR_X: the configure call is refused, and so is a call before configure
    assert lib.mca_hip_mvdr_map_configure(bf.h, C.byref(cfg())) == INVALID and b"XYZ" in lib.mca_hip_mvdr_last_error(bf.h)
    bf.set_geometry("xyz", 0.1)
    assert lib.mca_hip_mvdr_map_host(bf.h, 2, buf.ctypes.data_as(fp), None, None, None) == INVALID
    assert lib.mca_hip_mvdr_map_dev(bf.h, 2, None, None, None, None, None) == INVALID
    assert lib.mca_hip_mvdr_map_get_grid(bf.h, buf.ctypes.data_as(fp), None) == INVALID
    with pytest.raises(api.MCArrayHipError):
        bf.map_grid()
    bf.map_configure(36, 7, -0.5, 1.0, n_peaks=2)
    before = bf.map()
    bad = [cfg(size=8), cfg(n_az=2), cfg(n_az=361), cfg(n_el=0), cfg(n_el=92), cfg(n_az=360, n_el=6), cfg(n_az=64, n_el=33),
           cfg(n_el=1), cfg(lo=-1.6), cfg(hi=1.6), cfg(lo=0.5, hi=0.4), cfg(lo=float("nan")), cfg(hi=float("inf")),
           cfg(bin_lo=-1), cfg(bin_lo=90, bin_hi=80), cfg(bin_hi=129), cfg(weighting=2), cfg(n_peaks=0), cfg(n_peaks=5)]
    for c in bad:
        assert lib.mca_hip_mvdr_map_configure(bf.h, C.byref(c)) == INVALID, [getattr(c, f) for f, _ in c._fields_]
        assert lib.mca_hip_mvdr_last_error(bf.h)
    assert lib.mca_hip_mvdr_map_configure(bf.h, None) == INVALID
    for n in (0, 3):
        assert lib.mca_hip_mvdr_map_host(bf.h, n, buf.ctypes.data_as(fp), None, None, None) == INVALID
    assert lib.mca_hip_mvdr_map_host(bf.h, 2, None, None, None, None) == INVALID
    assert lib.mca_hip_mvdr_map_dev(bf.h, 2, None, None, None, None, None) == INVALID
    assert _same(before, bf.map())
    # the limits themselves are accepted: 2048 directions, one row, rows at +-pi/2
    for c in (cfg(n_az=128, n_el=16), cfg(n_az=360, n_el=1, lo=0.3, hi=0.3), cfg(n_az=3, n_el=91, lo=-np.pi / 2, hi=np.pi / 2)):
        assert lib.mca_hip_mvdr_map_configure(bf.h, C.byref(c)) == 0
    # a geometry change un-configures the map, as it does the spectrum
    bf.map_configure(36, 7, -0.5, 1.0, n_peaks=2)
    bf.set_geometry("xyz", 0.1)                                             # no change: still configured
    assert _same(before, bf.map())
    bf.set_geometry("xyz", 0.3)
    assert bf.map_config is None and lib.mca_hip_mvdr_map_host(bf.h, 2, buf.ctypes.data_as(fp), None, None, None) == INVALID
    bf.map_configure(36, 7, -0.5, 1.0, n_peaks=2)
    assert np.array_equal(bf.map()["map"], before["map"])                  # the map does not depend on the context's elevation
    bf.close()
