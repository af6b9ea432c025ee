"""CPU: the float64 twin of the azimuth x elevation Capon map (tests/mvdr_map_twin.py): the kernel's Cholesky route is the dense
definition, one elevation row is the circular spectrum of the geometry twin, the peak rule on crafted maps, and the scenes the GPU
tests compare clear the margin."""
import numpy as np
import pytest

import mvdr_geometry_twin as gt
import mvdr_map_twin as mt
import mvdr_nulls_twin as nt
import mvdr_spectrum_twin as sp

MARGIN = 5e-3                # ten times the GPU bar of a map (5e-4 of its maximum), as tests/test_mvdr_spectrum_twin.py asks


@pytest.mark.parametrize("name", sorted(mt.SCENES))
@pytest.mark.parametrize("weighting", [mt.POWER, mt.NORMALISED])
def test_cholesky_route_is_the_dense_definition(name, weighting):
    s = mt.scene(name)
    args = (s["phi"], mt.FS, mt.N, s["xyz"], mt.N_AZ, s["els"], mt.BAND[0], mt.BAND[1], weighting)
    P, C = mt.capon_map(*args), mt.cholesky_route(*args)
    assert P.shape == (mt.N_EL, mt.N_AZ) and P.min() > 0
    assert np.abs(C - P).max() <= 1e-10 * P.max()


def test_one_elevation_row_is_the_circular_spectrum():
    s = mt.scene("cube7")
    el = 0.375
    P = mt.capon_map(s["phi"], mt.FS, mt.N, s["xyz"], 72, mt.grid_el(1, el, el), 1, 127, mt.NORMALISED)
    with gt.xyz_mode(el):
        row = sp.spectrum(s["phi"], mt.FS, mt.N, s["xyz"], 72, 1, 127, sp.NORMALISED)
    assert P.shape == (1, 72) and np.array_equal(P[0], row)
    idx, paz, pel, val = mt.peaks(P, 4, [el], ctx_el=el)
    i1, d1, v1 = gt.peaks_circular(row, 4)
    assert np.array_equal(idx, i1) and np.array_equal(paz, d1) and np.array_equal(val, v1)
    assert np.array_equal(pel, np.full(4, np.float32(el)))
    # crafted rows, the seam and a plateau across it among them
    for r in ([1, 3, 3, 1, 5, 5, 0, 2], [4, 1, 2, 2, 2, 1, 0, 4], [0, 0, 0, 0], [7, 7, 7, 7], [2, 1, 1, 3]):
        r = np.array(r, dtype=np.float64)
        assert np.array_equal(mt.peaks(r[None], 4, [0.0])[0], gt.peaks_circular(r, 4)[0])


def test_grid():
    e = mt.grid_el(7, mt.EL_LO, mt.EL_HI)
    assert np.allclose(np.rad2deg(e), [-30, -15, 0, 15, 30, 45, 60]) and e[0] == mt.EL_LO
    assert np.array_equal(mt.grid_el(1, 0.3, 0.3), [0.3])


def _map(n_el, n_az, cells, base=1.0):
    P = np.full((n_el, n_az), base)
    for (j, i), v in cells.items():
        P[j, i] = v
    return P


def test_peak_rule_on_crafted_maps():
    els = mt.grid_el(4, -0.3, 0.6)
    az32, el32 = gt.grid_xyz(6).astype(np.float32), els.astype(np.float32)
    # a flat map has no cell strictly above the one before it round the circle: no maximum (as a flat row has none in the circular rule)
    assert mt.local_maxima(_map(4, 6, {})) == []
    # a plateau of equal cells counts once, at its lowest flat index -- along a row, down a column and on a diagonal
    assert mt.local_maxima(_map(4, 6, {(1, 2): 3.0, (1, 3): 3.0}, 0.5)) == [1 * 6 + 2]
    assert mt.local_maxima(_map(4, 6, {(1, 2): 3.0, (2, 2): 3.0}, 0.5)) == [1 * 6 + 2]
    assert mt.local_maxima(_map(4, 6, {(1, 2): 3.0, (2, 3): 3.0}, 0.5)) == [1 * 6 + 2]
    assert mt.local_maxima(_map(4, 6, {(1, 3): 3.0, (2, 2): 3.0}, 0.5)) == [1 * 6 + 3]
    # the azimuth seam: columns 0 and n_az - 1 are neighbours, diagonally too
    assert mt.local_maxima(_map(4, 6, {(1, 5): 3.0, (1, 0): 2.0}, 0.5)) == [1 * 6 + 5]
    assert mt.local_maxima(_map(4, 6, {(1, 5): 2.0, (2, 0): 3.0}, 0.5)) == [2 * 6 + 0]
    assert mt.local_maxima(_map(4, 6, {(1, 0): 3.0, (1, 5): 3.0}, 0.5)) == [1 * 6 + 5]      # (1, 5) is "before" (1, 0) round the seam
    # the elevation edges have no neighbour beyond them: rows 0 and n_el - 1 are not neighbours
    assert mt.local_maxima(_map(4, 6, {(0, 2): 3.0, (3, 2): 2.0}, 0.5)) == [0 * 6 + 2, 3 * 6 + 2]
    # P > 0: a map of zeros has no maximum, and the empty slots are azimuth 0 at the context's elevation
    idx, paz, pel, val = mt.peaks(np.zeros((4, 6)), 3, els, ctx_el=0.25)
    assert np.array_equal(idx, [-1, -1, -1]) and not paz.any() and not val.any() and np.array_equal(pel, np.full(3, np.float32(0.25)))
    # ranking by value, ties to the lower flat index; empty slots repeat slot 0 with value 0
    P = _map(4, 6, {(2, 4): 5.0, (0, 1): 5.0, (3, 1): 7.0}, 0.5)
    idx, paz, pel, val = mt.peaks(P, 4, els)
    assert np.array_equal(idx, [3 * 6 + 1, 0 * 6 + 1, 2 * 6 + 4, -1])
    assert np.array_equal(paz, az32[[1, 1, 4, 1]]) and np.array_equal(pel, el32[[3, 0, 2, 3]]) and np.array_equal(val, [7.0, 5.0, 5.0, 0.0])
    # the margin: the least of a peak above its 8 neighbours and the next-ranked maximum, of the map's maximum
    assert mt.peak_margin(P, mt.peaks(P, 2, els)[0]) == pytest.approx((7.0 - 5.0) / 7.0)
    assert mt.peak_margin(P, mt.peaks(P, 3, els)[0]) == 0.0
    Q = _map(4, 6, {(2, 4): 5.0, (2, 5): 4.9, (0, 1): 3.0}, 0.5)
    assert mt.peak_margin(Q, mt.peaks(Q, 2, els)[0]) == pytest.approx(0.1 / 5.0)


@pytest.mark.parametrize("seed", mt.SEEDS)
@pytest.mark.parametrize("name", sorted(mt.SCENES))
def test_scene_peaks_are_the_talkers_and_clear_the_margin(name, seed):
    """the two top picks are exactly the talkers' cells; each stands 5e-3 of the maximum above its 8 neighbours and the next maximum"""
    s = mt.scene(name, seed)
    idx, paz, pel, _ = mt.peaks(s["P"], 3, s["els"])
    cells = sorted((int(c) // mt.N_AZ, int(c) % mt.N_AZ) for c in idx[:2])
    assert cells == sorted(mt.TALKERS)
    margin = mt.peak_margin(s["P"], idx)
    print(name, seed, "margin", margin, "local maxima", len(mt.local_maxima(s["P"])))
    assert margin >= MARGIN
    if name != "cube4":
        assert idx[2] == -1                                                # no third local maximum
    else:
        assert s["P"].reshape(-1)[idx[2]] <= 0.17 * s["P"].max()


def test_slot_elevations_generalise_xyz_mode():
    """one elevation in every slot is xyz_mode() at that elevation; a NaN is the context's; the exchange ends with the block"""
    s = mt.scene("cube7")
    doa = np.array([0.4, -2.0, 3.3])
    with gt.xyz_mode(0.375):
        want = nt.steering(mt.FS, mt.N, s["xyz"], doa)
        with mt.slot_elevations([np.nan, np.nan, np.nan], 0.375):
            assert np.array_equal(nt.steering(mt.FS, mt.N, s["xyz"], doa), want)
    with mt.slot_elevations([0.375, 0.375, 0.375]):
        assert np.array_equal(nt.steering(mt.FS, mt.N, s["xyz"], doa), want)
        assert np.array_equal(nt.steering(mt.FS, mt.N, s["xyz"], doa[:2]), want[:, :2])
        with pytest.raises(ValueError):
            nt.steering(mt.FS, mt.N, s["xyz"], np.zeros(4))
    with mt.slot_elevations([-0.3, np.nan, 0.9], 0.1):
        d = nt.steering(mt.FS, mt.N, s["xyz"], doa)
    for i, el in enumerate((-0.3, 0.1, 0.9)):
        assert np.array_equal(d[:, i], gt.steering_xyz(mt.FS, mt.N, s["xyz"], doa[i:i + 1], el)[:, 0])
    assert nt.steering(mt.FS, mt.N, [0.0, 0.1], doa).shape == (mt.N // 2 + 1, 3, 2)
    # a frames twin inside the block steers every source at its own elevation: distortionless towards (azimuth, its elevation)
    F = 4
    pcm = gt.two_sources_xyz(s["xyz"], mt.FS, mt.N, F, 0.4, -2.0).astype(np.float64)
    with mt.slot_elevations([-0.3, 0.9]):
        run = nt.mvdr_nulls_stream(mt.FS, mt.N, s["xyz"], pcm, np.broadcast_to(doa[:2], (F, 2)), 0.0, want_weights=True)
    for i, el in enumerate((-0.3, 0.9)):
        d = gt.steering_xyz(mt.FS, mt.N, s["xyz"], doa[i:i + 1], el)[:, 0]
        assert np.abs(np.einsum("fkm,km->fk", np.conj(run["w"][:, i]), d) - 1.0).max() < 1e-9
