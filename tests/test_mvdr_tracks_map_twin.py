"""CPU: the twin of the tracks' map mode (tests/mvdr_tracks_map_twin.py) against the twins it extends -- the
association on the circle with every elevation equal, the own spectrum of a one-row map -- and against its own dense definition."""
import numpy as np
import pytest

import mvdr_geometry_twin as gt
import mvdr_map_twin as mp
import mvdr_tracks_map_twin as tm
import mvdr_tracks_twin as tt

F32 = np.float32
CASES = [(1, 0), (1, 1), (2, 1), (3, 0), (3, 2), (4, 0), (4, 1), (4, 2)]      # those of tests/test_gpu_mvdr_tracks.py


def _angles(rng, shape, p_nan, span=64):
    """angles from a grid of 1/16 rad over +-span/16 (ties in distance and at the gates are common; beyond +-pi the reduction works),
    NaNs and zeros among them"""
    v = (rng.integers(-span, span + 1, shape) / 16.0).astype(F32)
    v[rng.random(shape) < 0.1] = 0.0
    v[rng.random(shape) < p_nan] = np.nan
    return v


@pytest.mark.parametrize("n_tracks,n_own", CASES)
def test_equal_elevations_give_the_association_on_the_circle(n_tracks, n_own):
    """300 random streams, three rounds: with every elevation equal the distance is |d theta| + 0 and theta, alive, miss and gen are
    those of mvdr_geometry_twin.associate_circular, bit for bit; eps of every slot that ever lived is the one elevation"""
    A, e0 = 300, F32(0.25)
    rng = np.random.default_rng(100 * n_tracks + n_own)
    cfg = dict(max_step_rad=0.25, min_sep_rad=0.125, hold=1)
    seeds = _angles(rng, (A, n_tracks), 0.3)
    one = [gt.seed_circular(tt.new_state(), seeds[a]) for a in range(A)]
    two = [tm.seed_map(tm.new_state(), seeds[a], np.full(n_tracks, e0)) for a in range(A)]
    n_born = 0
    for rnd, n_cand in enumerate((8, 1 + (n_tracks + n_own) % 7, 3)):
        own = _angles(rng, (A, max(n_own, 1)), 0.2)[:, :n_own]
        cd = _angles(rng, (A, n_cand), 0.1)
        cv = rng.choice(F32([1.0, 0.5, 0.0, np.nan, 2.0]), (A, n_cand), p=[0.4, 0.3, 0.1, 0.05, 0.15]).astype(F32)
        for a in range(A):
            gt.associate_circular(one[a], own[a], cd[a], cv[a], n_tracks, n_own, **cfg)
            n_born += len(tm.associate_map(two[a], own[a], np.full(n_own, e0), cd[a], np.full(n_cand, e0), cv[a], n_tracks, n_own,
                                           max_step_el_rad=0.0625 * rnd, min_sep_el_rad=0.125 * (2 - rnd), **cfg))
        for k in ("theta", "alive", "miss", "gen"):
            got, want = np.stack([st[k] for st in two]), np.stack([st[k] for st in one])
            assert np.array_equal(got, want, equal_nan=True), (rnd, k, np.flatnonzero((got != want).any(axis=1))[:5])
    eps, gen = np.stack([st["eps"] for st in two]), np.stack([st["gen"] for st in two])
    assert np.array_equal(eps[gen > 0], np.full(int((gen > 0).sum()), e0)) and not eps[gen == 0].any()
    assert n_tracks == n_own or n_born > 0


def test_the_second_angle_gates_steps_and_clamps():
    """what one angle cannot tell: a peak at the own azimuth but another height is an interferer; a candidate inside the azimuth gate
    and outside the elevation gate is a birth; the nearer slot is the nearer in |d theta| + |d eps|; the own step is clamped per axis
    and eps stays within +-(float) pi/2; an angle that is not finite in either place is a miss or a skip"""
    cfg = dict(n_tracks=4, n_own=1, max_step_rad=0.25, min_sep_rad=0.125, hold=1, max_step_el_rad=0.125, min_sep_el_rad=0.0625)
    st = tm.seed_map(tm.new_state(), [0.5, 1.0, 1.25, np.nan], [0.25, 0.5, 0.5, 0.0])
    assert st["alive"].tolist() == [1, 1, 1, 0] and st["gen"].tolist() == [1, 1, 1, 0]
    born = tm.associate_map(st, [1.5], [1.5], [0.5, 0.5, 1.125, 1.0, 0.1], [0.25, 0.5, 0.4375, 0.75, np.nan], [1.0, 1.0, 1.0, 1.0, 1.0], **cfg)
    # own: both steps clamped
    assert st["theta"][0] == F32(0.75) and st["eps"][0] == F32(0.375) and st["miss"][0] == 0
    # (0.5, 0.25) was the talker's before the step but lies outside the box of (0.75, 0.375) now, and in no gate: born into slot 3;
    # (0.5, 0.5): no gate either, no free slot left;  (1.125, 0.4375): 0.125 + 0.0625 from both slots 1 and 2 -- the lower slot wins;
    # (1.0, 0.75) is outside the elevation gate; the NaN elevation is skipped
    assert born == [3] and st["theta"][3] == F32(0.5) and st["eps"][3] == F32(0.25)
    assert st["theta"][1] == F32(1.125) and st["eps"][1] == F32(0.4375) and st["miss"].tolist() == [0, 0, 1, 0]
    st2 = tm.seed_map(tm.new_state(), [0.0, 7.0], [1.6, -9.0])
    assert st2["eps"][0] == tm.HALF_PI_F == F32(1.57079637) and st2["eps"][1] == -tm.HALF_PI_F and abs(st2["theta"][1]) <= gt.PI_F
    tm.associate_map(st2, [0.0], [np.inf], [], [], [], 2, 1, 0.25, 0.125, 1, 0.125, 0.0625)
    assert st2["miss"][0] == 1 and st2["eps"][0] == tm.HALF_PI_F
    doa, el = tm.fill_map(st, 4)
    assert np.array_equal(doa, st["theta"]) and np.array_equal(el, st["eps"])
    dead = tm.new_state()
    doa, el = tm.fill_map(dead, 2)
    assert not doa.any() and np.isnan(el).all()
    assert tm.fill_map(st2, 2)[1][0] == F32(np.pi / 2)


def test_own_map_is_the_dense_definition_and_the_window_argmax_finds_the_talker():
    fs, N, xyz = 16000, 32, gt.array_3d(5, 2)
    s = tm.synthetic_state(fs, N, xyz, 0.6, 0.4, 1)
    n_az, els = 12, mp.grid_el(4, 0.0, 1.2)
    args = (fs, N, xyz, n_az, els, 2, 14, s["psi"], s["cpsi"], s["phi"], s["cphi"], F32(0.5), F32(0.3))
    r = tm.own_map(*args)
    assert r["T"].shape == (4, 12) and r["used"][2:15].any() and not r["used"][:2].any() and not r["used"][15:].any()
    dense = tm.own_map_dense(*args)
    assert np.abs(r["T"] - dense).max() <= 1e-12 * dense.max()
    az32, el32 = gt.grid_xyz(n_az).astype(F32), els.astype(F32)
    a, e, i = tm.window_argmax_map(r["T"], az32, el32, 0.5, 0.3, 0.6, 0.45)
    win = tm.in_window(az32, el32, 0.5, 0.3, 0.6, 0.45)
    assert 1 < win.sum() < win.size and win.reshape(-1)[i] and r["T"].reshape(-1)[i] == r["T"][win].max()
    assert abs(a - 0.6) <= 2 * np.pi / n_az and abs(e - 0.4) <= 0.4          # the cell next to the talker
    assert tm.window_argmax_map(np.zeros((4, 12)), az32, el32, 0.5, 0.3, 0.6, 0.45)[2] == -1
    assert tm.window_argmax_map(r["T"], az32, el32, 0.5, 0.2, 0.6, 0.0)[2] == -1      # no row at eps = 0.2


@pytest.mark.parametrize("name", sorted(tm.PARITY_ARRAYS))
def test_parity_inputs_leave_few_bins_at_a_decision_edge(name):
    """the inputs tests/test_gpu_mvdr_tracks_map.py compares on: on the twin alone, with the tracks seeded 3 degrees and one elevation
    step behind the look directions, at most 1 % of a case's cells sit at a decision edge of the estimator (DESIGN.md 4.11's cap), every
    own map has a maximum, and at least one window maximum per array stands 5e-3 of it clear"""
    inp, state = tm.parity_inputs(name), tm.parity_state(name)
    rtf = tm.parity_rtf(name)
    kw = dict(iterations=rtf["iterations"], ref_mic=rtf["ref_mic"], min_share=rtf["min_share"])
    n_clear = 0
    for n_az, n_el in tm.PARITY_MAPS:
        els = mp.grid_el(n_el, *tm.PARITY_EL)
        az32, el32 = gt.grid_xyz(n_az).astype(F32), els.astype(F32)
        step = float(els[1] - els[0])
        saz, sel = tm.parity_seeds(inp, step)
        n_edge = n_cells = 0
        for a, s in [(a, s) for n_own in (1, 2) for a in range(len(state)) for s in range(n_own)]:      # the cells the GPU test counts
            st = state[a]
            r = tm.own_map(tm.FS, tm.N, inp["xyz"], n_az, els, tm.PARITY_BAND[0], tm.PARITY_BAND[1], st["psi"][s], st["cpsi"][s], st["phi"], st["cphi"],
                           saz[a, s], sel[a, s], **kw)
            n_edge, n_cells = n_edge + int(r["edge"].sum()), n_cells + tm.PARITY_BAND[1] - tm.PARITY_BAND[0] + 1
            assert r["T"].max() > 0 and r["used"].sum() > 20
            n_clear += tm.clear_margin_map(r["T"], az32, el32, saz[a, s], sel[a, s], tm.PARITY_STEP, 1.5 * step) >= 5e-3
        print("%s %d x %d: %d of %d cells at a decision edge" % (name, n_az, n_el, n_edge, n_cells))
        assert n_edge <= 0.01 * n_cells
    assert n_clear > 0


@pytest.mark.parametrize("elevation", [0.0, 0.35])
def test_one_row_at_the_contexts_elevation_is_the_own_spectrum(elevation):
    """n_el = 1 at the context's eps: the map is mvdr_tracks_twin.own_spectrum in XYZ mode, the window argmax its window argmax"""
    fs, N, xyz, D = 16000, 32, gt.array_3d(6, 3), 24
    s = tm.synthetic_state(fs, N, xyz, -2.9, elevation, 2)
    eps32 = F32(elevation)
    r = tm.own_map(fs, N, xyz, D, [float(eps32)], 1, 15, s["psi"], s["cpsi"], s["phi"], s["cphi"], F32(3.1), eps32)
    with gt.xyz_mode(float(eps32)):
        w = tt.own_spectrum(fs, N, xyz, D, 1, 15, s["psi"], s["cpsi"], s["phi"], s["cphi"], F32(3.1))
        g32 = tt.grid64(D).astype(F32)
        want = tt.window_argmax(w["T"], g32, F32(3.1), 0.6)
    assert np.array_equal(r["used"], w["used"]) and np.abs(r["T"][0] - w["T"]).max() <= 1e-12 * w["T"].max()
    a, e, i = tm.window_argmax_map(r["T"], g32, [eps32], F32(3.1), eps32, 0.6, 0.0)
    assert (a, i) == want and e == eps32 and i >= 0


def test_scene_the_track_follows_the_talker_in_both_angles():
    """the scene of tests/mvdr_tracks_map_twin.py on the twin alone: the tracked run's worst azimuth and elevation errors and its kept
    target share are the recorded figures, within one grid step (5 and 10 degrees) and a tenth; the run that holds the seed direction
    is worse in all three"""
    runs = tm.scene_runs()
    tr, held = runs["tracked"], runs["held"]
    got = (tr["err_az_deg"].max(), tr["err_el_deg"].max(), tr["share"])
    print("tracked: az %s el %s degrees; worst errors %.2f / %.2f degrees, share %.3f; held: %.2f / %.2f, share %.3f"
          % (np.rad2deg(tr["theta"]).round(1).tolist(), np.rad2deg(tr["eps"]).round(1).tolist(), got[0], got[1], got[2], held["err_az_deg"].max(),
             held["err_el_deg"].max(), held["share"]))
    want = tm.SCENE_TWIN["tracked"]
    assert abs(got[0] - want[0]) <= 5.0 and abs(got[1] - want[1]) <= 10.0 and abs(got[2] - want[2]) <= 0.1
    wh = tm.SCENE_TWIN["held"]
    assert abs(held["err_az_deg"].max() - wh[0]) <= 5.0 and abs(held["err_el_deg"].max() - wh[1]) <= 10.0 and abs(held["share"] - wh[2]) <= 0.1
    assert held["err_az_deg"].max() > got[0] and held["err_el_deg"].max() > got[1] and held["share"] < got[2]
    assert tr["tracks"]["alive"][:2].tolist() == [1, 1] and tr["tracks"]["gen"][:2].tolist() == [1, 1]      # both talkers kept their slots
    # what the GPU test compares outside of: the last chunk's cells at a decision edge of either estimator, on the twin alone
    edge = tm.scene_edge_cells(runs["sc"], tr)
    print("%.2f %% of the last chunk's cells at a decision edge" % (100.0 * edge.mean()))
    assert edge.shape == (2, tm.SCENE_CF, 129) and edge.mean() <= 0.01
