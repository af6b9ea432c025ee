"""CPU: the float64 twin of the XYZ geometry (tests/mvdr_geometry_twin.py): it is the existing steering on an array on the x axis, it is
distortionless behind the array, the elevation scales a planar array, the peak rule and the association work across the seam of the
periodic grid, and the scenes the GPU tests compare clear the margin."""
import numpy as np
import pytest

from mcarray_amd import synth

import mvdr_geometry_twin as gt
import mvdr_nulls_twin as nt
import mvdr_spectrum_twin as sp
import mvdr_tracks_twin as tt

F32 = np.float32
MARGIN = 5e-3                # ten times the GPU bar of a spectrum row (5e-4 of its maximum)


@pytest.mark.parametrize("xs", [synth.ULA8, synth.ULA16, synth.REEM_C, [-0.05, 0.0, 0.07]])
def test_on_axis_arrays_are_the_existing_steering_and_streams(xs):
    doa = np.array([0.0, 0.3, -1.2, np.pi / 2, 2.5, -3.0, 7.0])
    xyz = gt._xyz(xs)
    assert np.array_equal(gt.steering_xyz(48000, 256, xyz, doa), nt.steering(48000, 256, xs, doa))
    assert np.array_equal(gt.steering_xyz(16000, 1024, xs, doa), nt.steering(16000, 1024, xs, doa))
    with gt.xyz_mode():
        assert np.array_equal(nt.steering(48000, 256, xyz, doa), gt.steering_xyz(48000, 256, xyz, doa))
    assert nt.steering(48000, 256, xyz, doa).shape == (129, 7, len(xs))            # the exchange ends with the block
    for th in (0.4, -2.0):
        assert np.array_equal(synth.noise_source_stream_xyz(xyz, th, 16000, 1500, 3), synth.noise_source_stream(xs, th, 16000, 1500, 3))
        s = np.random.default_rng(1).standard_normal(512)
        assert np.array_equal(synth.delay_channels_xyz(s, xyz, th, 16000), synth.delay_channels(s, xs, th, 16000))


def test_definition_against_the_unit_vector():
    """d_m = exp(+j 2 pi k fs (r_m . e) / (N c)) on a 3-D array, term by term"""
    xyz, fs, N, el = gt.array_3d(), 16000, 256, 0.4
    doa = np.array([0.0, np.pi / 2, 2.5, -2.0])
    d = gt.steering_xyz(fs, N, xyz, doa, el)
    k = np.arange(N // 2 + 1)
    for s, th in enumerate(doa):
        e = synth.unit_vector(th, el)
        want = np.exp(2j * np.pi * k[:, None] * fs * (xyz @ e)[None, :] / (N * synth.C_SOUND))
        assert np.abs(d[:, s] - want).max() < 1e-12
    assert np.allclose(synth.unit_vector(0.0), [0, 1, 0]) and np.allclose(synth.unit_vector(np.pi / 2), [1, 0, 0])


def test_distortionless_towards_a_direction_behind_the_array():
    xyz, fs, N, F = synth.uca(6, 0.045), 16000, 256, 6
    look = 2.8                                                               # behind: cos(theta) < 0
    pcm = gt.two_sources_xyz(xyz, fs, N, F, look, -0.6).astype(np.float64)
    with gt.xyz_mode():
        run = nt.mvdr_nulls_stream(fs, N, xyz, pcm, np.full((F, 1), look), 0.0, want_weights=True)
    d = gt.steering_xyz(fs, N, xyz, [look])[:, 0]
    resp = np.einsum("fkm,km->fk", np.conj(run["w"][:, 0]), d)
    assert np.abs(resp - 1.0).max() < 1e-9
    # and the front-back mirror image of the look direction is another vector on a planar array
    assert np.abs(gt.steering_xyz(fs, N, xyz, [np.pi - look])[:, 0] - d).max() > 0.5


def test_elevation_on_a_planar_array_scales_the_coordinates():
    xyz, el = synth.uca(11, 0.045), 0.7
    doa = np.linspace(-4.0, 4.0, 9)
    a, b = gt.steering_xyz(16000, 256, xyz, doa, el), gt.steering_xyz(16000, 256, xyz * np.cos(el), doa, 0.0)
    assert np.abs(a - b).max() < 1e-12


def test_periodic_grid():
    for D in (3, 64, 65, 72, 360, 361):
        g = gt.grid_xyz(D)
        assert g[0] == -np.pi and len(g) == D and np.all(np.diff(g) > 0) and g[-1] < np.pi
        assert abs((g[-1] + 2 * np.pi / D) - np.pi) < 1e-14


@pytest.mark.parametrize("name, want, unwrapped", [("seam_last", [24, 71, 13], [24, 71, 0]), ("seam_first", [24, 0, 48], [24, 0, 71])])
def test_peak_rule_across_the_seam(name, want, unwrapped):
    """a talker on the grid point next to the seam: the circular rule returns the two talkers and the true third maximum, a rule that
    does not wrap takes the talker's own flank across the seam for the third"""
    sc = gt.named_scene(name)
    P = sc["P"]
    idx4, doa, val = gt.peaks_circular(P, gt.SCENE_PEAKS + 1)
    assert list(idx4[:3]) == want, idx4
    assert list(gt.peaks_circular(P, 3, circular=False)[0]) == unwrapped
    g = gt.grid_xyz(gt.SCENE_D)
    assert {int(i) for i in idx4[:2]} == {int(np.argmin(np.abs(g - a))) for a in sc["az"]}           # the two talkers, on their grid points
    assert np.array_equal(doa[:3], g.astype(F32)[want]) and np.array_equal(val[:3], P[want])
    m = gt.peak_margin_circular(P, idx4)
    print("%s: margin %.2e of the maximum" % (name, m))
    assert m >= MARGIN


def test_talkers_in_front_and_behind_are_found():
    sc = gt.named_scene("back")
    idx4, doa, _ = gt.peaks_circular(sc["P"], gt.SCENE_PEAKS + 1)
    step = 2 * np.pi / gt.SCENE_D
    found = np.sort(doa[:2].astype(np.float64))
    assert np.all(np.abs(found - np.sort(sc["az"])) <= step), (found, sc["az"])
    m = gt.peak_margin_circular(sc["P"], idx4)
    print("back: margin %.2e of the maximum" % m)
    assert m >= MARGIN


def test_a_line_array_shows_every_talker_twice():
    """front-back ambiguity: P(theta) = P(pi - theta) on an array on the x axis"""
    xs, fs, N, F, D = synth.ULA8, 16000, 256, 8, 72
    pcm = sp.two_sources(xs, fs, N, F, 20.0, -50.0).astype(np.float64)
    phi = nt.mvdr_nulls_stream(fs, N, xs, pcm, np.zeros((F, 1)), 0.0)["phi"]
    with gt.xyz_mode():
        P = sp.spectrum(phi, fs, N, gt._xyz(xs), D, 1, 127, sp.NORMALISED)
    i = np.arange(D)
    assert np.abs(P - P[(D // 2 - i) % D]).max() <= 1e-9 * P.max()          # theta_i -> pi - theta_i is i -> D/2 - i on this grid (D even)


def test_reduce_and_wrap():
    for v in (0.0, 3.0, -3.0, 3.2, -3.2, 7.0, -7.0, 100.0, -1000.5, 3.1415927, -3.1415927):
        r = gt.reduce32(v)
        assert r.dtype == F32 and -gt.PI_F <= r <= gt.PI_F
        assert abs(np.remainder(float(r) - float(F32(v)) + np.pi, 2 * np.pi) - np.pi) < 1e-4 * max(1.0, abs(v))
    assert np.isnan(gt.reduce32(np.nan)) and np.isinf(gt.reduce32(np.inf))
    assert -gt.PI_F <= gt.reduce32(1e30) <= gt.PI_F
    assert gt.wrap32(F32(6.2)) == F32(F32(6.2) - gt.TWO_PI_F) and gt.wrap32(F32(-6.2)) == F32(F32(-6.2) + gt.TWO_PI_F) and gt.wrap32(F32(1.0)) == F32(1.0)


CFG = dict(n_tracks=2, n_own=0, max_step_rad=0.2, min_sep_rad=0.1, hold=3)


def test_association_across_the_seam():
    # an interferer track at 3.10 and a candidate at -3.10: 0.083 rad apart round the seam
    st = tt.seed(tt.new_state(), [3.10, np.nan])
    born = gt.associate_circular(st, None, [-3.10], [1.0], **CFG)
    assert born == [] and st["theta"][0] == F32(-3.10) and list(st["alive"][:2]) == [1, 0] and st["gen"][0] == 1
    st = tt.seed(tt.new_state(), [3.10, np.nan])
    born = gt.associate_circular(st, None, [-3.10], [1.0], circular=False, **CFG)
    assert born == [1] and st["theta"][0] == F32(3.10) and st["theta"][1] == F32(-3.10) and st["miss"][0] == 1      # without the wrap: a birth
    # an own track at 3.12 stepping by +0.2
    own = dict(CFG, n_own=1)
    st = tt.seed(tt.new_state(), [3.12, np.nan])
    gt.associate_circular(st, [3.12 + 0.5], [0.0], [0.0], **own)
    assert st["theta"][0] == F32(F32(F32(3.12) + F32(0.2)) - gt.TWO_PI_F) and abs(float(st["theta"][0]) - (3.12 + 0.2 - 2 * np.pi)) < 1e-6
    # the same target given from the other side of the seam
    st2 = tt.seed(tt.new_state(), [3.12, np.nan])
    gt.associate_circular(st2, [3.12 + 0.5 - 2 * np.pi], [0.0], [0.0], **own)
    assert abs(float(st2["theta"][0]) - float(st["theta"][0])) < 1e-6
    # min_sep across the seam: a peak at -3.13 is the own talker at 3.12 (0.033 rad away), not an interferer
    st = tt.seed(tt.new_state(), [3.12, np.nan])
    born = gt.associate_circular(st, [np.nan], [-3.13], [1.0], **own)
    assert born == [] and list(st["alive"][:2]) == [1, 0]
    st = tt.seed(tt.new_state(), [3.12, np.nan])
    assert gt.associate_circular(st, [np.nan], [-3.13], [1.0], circular=False, **own) == [1]
    # seeds and candidates outside [-pi, pi] are reduced on entry; a stored theta is always in [-pi, pi]
    st = gt.seed_circular(tt.new_state(), [7.0, -4.0])
    assert st["theta"][0] == gt.reduce32(7.0) and st["theta"][1] == gt.reduce32(-4.0) and np.all(np.abs(st["theta"]) <= gt.PI_F)
    gt.associate_circular(st, None, [7.1, 9.0], [1.0, 1.0], **CFG)
    assert st["theta"][0] == gt.reduce32(7.1) and np.all(np.abs(st["theta"]) <= gt.PI_F)


def test_search_window_straddles_the_seam():
    D = 72
    g32 = gt.grid_xyz(D).astype(F32)
    T = np.zeros(D, dtype=F32)
    T[1], T[68] = 2.0, 1.0                         # -3.054 rad (across the seam from a track at 3.10) and 2.79 rad (outside the window)
    th, i = gt.window_argmax_circular(T, g32, F32(3.10), 0.2)
    assert i == 1 and th == g32[1]
    assert tt.window_argmax(T, g32, F32(3.10), 0.2)[1] == -1                 # the window that does not wrap sees neither
