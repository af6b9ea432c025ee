"""CPU: the definition of the DOA tracker ("The DOA tracker") as restated in tests/gcc2_tracker_twin.py -- the random
numbers' known answers, the resampling's guarantees, the control-flow table, and that the filter tracks: on the smoothed
correlations of the CPU oracle (oracle.pyoracle.FreqGCC) for the jump16k signal of tests/test_gpu_gcc2_probability.py
(-42 degrees for 75 frames, then +25 degrees; 16 kHz, N = 1024).  tests/test_gpu_gcc2_tracker.py holds the GPU to the same twin, bit
for bit, and to the same tracking thresholds."""
import numpy as np
import pytest

import gcc2_tracker_twin as tw
from mcarray_amd import synth
from oracle import pyoracle as po

SEEDS = tuple(range(1, 11))
# Frames after the jump until the estimate is within one grid step (3 degrees) of +25 degrees FOR GOOD, measured with this twin on
# the oracle's rows, seeds 1..10: 25, 28, 21, 26, 24, 20, 16, 20, 18, 22.  The bar is twice the worst seed's value.
JUMP_L = 56
# (measured at the same time: the mean estimate of frames 30..74 was between -42.045 and -42.400 degrees, no frame of them further
# than 1.142 degrees from -42; from frame 75 + 28 on the estimates average 24.91 .. 25.21 degrees; without injection, seed 1, the
# estimate after 150 frames is -45.95 degrees: the side lobe the filter never leaves)


def test_draw_known_answers():
    assert [int(tw.draw(0, c)) for c in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    # the key of an update depends on every one of its four inputs
    keys = {int(tw.make_key(*k)) for k in [(1, 0, 1, 0), (2, 0, 1, 0), (1, 1, 1, 0), (1, 0, 2, 0), (1, 0, 1, 1), (1, 0xFFFFFFFF, 1, 0)]}
    assert len(keys) == 6


def test_gauss_is_exact_and_standard():
    n = 20000
    g = tw.gauss(tw.make_key(7, 0, 1, 3), np.arange(n))
    assert np.array_equal(g * 131072, np.round(g * 131072)) and np.abs(g).max() <= 6.0
    assert abs(g.mean()) <= 4 / np.sqrt(n), g.mean()
    assert abs(g.var() - 1.0) <= 0.04, g.var()          # 4 standard errors of a variance at kurtosis 2.9: 4 sqrt(1.9 / n)
    u = tw.unif(tw.make_key(7, 0, 1, 3), np.arange(n))
    assert 0.0 <= u.min() and u.max() < 1.0 and abs(u.mean() - 0.5) <= 4 / np.sqrt(12 * n)


@pytest.fixture(scope="module")
def jump_rows():
    fs, N, F = 16000, 1024, 150
    hop = N // 2
    L = (F + 1) * hop
    a = synth.noise_source_stream(synth.BINAURAL, np.deg2rad(-42.0), fs, L, 21)
    b = synth.noise_source_stream(synth.BINAURAL, np.deg2rad(25.0), fs, L, 22)
    h = (F // 2) * hop
    pcm = np.concatenate([a[:, :h], b[:, h:]], axis=1)
    X = po.stft_frames(pcm.astype(np.float64), N)
    og = po.FreqGCC(fs, synth.BINAURAL, N + 2, False, 3.0)
    rows, am = [], []
    for t in range(F):
        voiced, corr, idx, _, _ = og.process(X[t, 0], X[t, 1])
        assert voiced
        rows.append(corr.copy())
        am.append(idx)
    grid, step = tw.reference_grid(3.0)
    assert len(grid) == og.D == 61
    return np.array(rows), np.array(am), grid, step


def _run(jump_rows, **cfg):
    rows, am, grid, step = jump_rows
    return tw.run(rows, np.ones(len(rows), dtype=bool), am, 0, 93, grid, step, **cfg)


@pytest.mark.parametrize("cfg", [dict(seed=3), dict(seed=4, n_particles=64, n_inject=-1), dict(seed=5, n_particles=1000, n_inject=100)])
def test_systematic_resampling_keeps_the_proportions(jump_rows, cfg):
    rows, am, grid, step = jump_rows
    tr = tw.Tracker(grid, step, 0, **cfg)
    N = tr.N
    for t in range(len(rows)):
        tr.row = rows[t]
        if not tr.alive:
            tr._seed(am[t])
        before = tr.x.copy()
        tr.update()
        q = tr.last_q
        Q = int(q.sum(dtype=np.uint64))
        assert Q > 0
        anc = tw.resample_ancestors(q, float(tw.unif(tw.make_key(tr.seed, 0, tr.track, tr.upd), 3 * N)))
        count = np.bincount(anc, minlength=N)
        share = N * q.astype(np.float64) / Q
        assert (count >= np.floor(share) - 1).all() and (count <= np.ceil(share) + 1).all(), t
        assert not count[q == 0].any(), t
        assert (np.diff(anc) >= 0).all()
        # the particles after the update are the predicted ones at those ancestors, then the injected tail
        keep = N - tr.n_inject
        pred = np.minimum(np.maximum(before + tr.sigma_step * tw.gauss(tw.make_key(tr.seed, 0, tr.track, tr.upd), np.arange(N)),
                                     -tw.HALFPI), tw.HALFPI)
        assert np.array_equal(tr.x[:keep], pred[anc][:keep])
        assert (np.abs(tr.x[keep:]) <= tw.HALFPI).all()


def test_no_weight_keeps_the_particles():
    grid, step = tw.reference_grid(3.0)
    tr = tw.Tracker(grid, step, 0, seed=9, n_inject=-1)
    tr.row = np.full(61, 0.25)                    # a flat row: sum - min * D = 0, every weight 0
    tr._seed(30)
    before = tr.x.copy()
    e = tr.update()
    pred = np.minimum(np.maximum(before + tr.sigma_step * tw.gauss(tw.make_key(9, 0, 1, 1), np.arange(500)), -tw.HALFPI), tw.HALFPI)
    assert not tr.last_q.any() and np.array_equal(tr.x, pred)
    assert abs(e - pred.mean()) <= 1e-15 and abs(e - float(grid[30])) < 0.02
    tr2 = tw.Tracker(grid, step, 0, seed=9)      # with injection the tail is still replaced
    tr2.row = tr.row
    tr2._seed(30)
    tr2.update()
    assert np.array_equal(tr2.x[:475], pred[:475]) and not np.array_equal(tr2.x[475:], pred[475:])


def test_control_flow_table():
    grid, step = tw.reference_grid(3.0)
    rng = np.random.default_rng(1)
    D, wtd, f0 = 61, 5, 4
    row = 0.1 + 0.05 * rng.random(D)
    row[40] = 1.0
    #         floor estimation | known, no track | burst | gap 3 | burst | gap 8 > wtd       | burst
    voiced = [0, 0, 0, 0,        0, 0,             1, 1,   0, 0, 0, 1,     0, 0, 0, 0, 0, 0, 0, 0, 1, 1]
    F = len(voiced)
    r = tw.run(np.tile(row, (F, 1)), voiced, np.full(F, 40), f0, wtd, grid, step, seed=2)
    assert r["fired"].tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 2, 1, 2, 2, 2, 2, 2, 0, 0, 0, 1, 1]
    assert r["track"].tolist() == [0] * 6 + [1] * 14 + [2] * 2
    assert r["doa"][:6].tolist() == [0.0] * 6 and r["prob"][:6].tolist() == [-1.0] * 6
    assert r["prob"][6] == tw.prob_at(row, *tw.row_min_sum_adj(row), step, grid, [0.0])[0]      # setProbability of the DOA before
    assert (r["prob"][8:11] == r["prob"][7]).all()                  # coasting leaves prob alone and moves the DOA
    assert len(set(r["doa"][7:12])) == 5
    assert r["doa"][17] == r["doa"][18] == r["doa"][19] == r["doa"][16]      # a dropped track keeps the DOA
    assert (np.abs(r["doa"][6:] - float(grid[40])) < np.deg2rad(3.0)).all()
    # the first update of track 2 is update 1 of a new key: a fresh seeding around the argmax
    t2 = tw.Tracker(grid, step, 0, seed=2)
    t2.track, t2.doa = 1, r["doa"][19]
    t2.voiced_frame(row, 40)
    assert t2.track == 2 and t2.upd == 1 and t2.doa == r["doa"][20]
    # the gap of exactly wtd frames coasts all the way and drops nothing
    v2 = [1] + [0] * wtd + [1]
    r2 = tw.run(np.tile(row, (len(v2), 1)), v2, np.full(len(v2), 40), 0, wtd, grid, step, seed=2)
    assert r2["fired"].tolist() == [1] + [2] * wtd + [1] and r2["track"].tolist() == [1] * len(v2)


def test_it_tracks_the_jump_for_every_seed(jump_rows):
    for seed in SEEDS:
        d = np.rad2deg(_run(jump_rows, seed=seed)["doa"])
        steady = d[30:75].mean()
        late = np.abs(d[75 + JUMP_L:] - 25.0).max()
        assert abs(steady + 42.0) <= 1.0, (seed, steady)         # a third of a grid step
        assert late <= 3.0, (seed, late)                         # one grid step


def test_without_injection_the_filter_stays_on_the_side_lobe(jump_rows):
    d = np.rad2deg(_run(jump_rows, seed=1, n_inject=-1)["doa"])
    assert d[-1] < -40.0, d[-1]
