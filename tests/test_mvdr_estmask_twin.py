"""CPU: the float64 twin of the mask estimator (tests/mvdr_estmask_twin.py) against the properties of the definition
(include/mcarray_hip.h, mca_hip_mvdr_set_mask_estimator), on the scene of the RTF twin with the masks estimated instead of given, and
on the parity inputs of tests/test_gpu_mvdr_estmask.py, whose mask bar it measures.  Every test prints its worst case."""
import numpy as np
import pytest

from mcarray_amd import synth

import mvdr_estmask_twin as et
import mvdr_mask_twin as mt
import mvdr_nulls_twin as nt
import mvdr_rtf_twin as rt

FS, N = 16000, 256
K = N // 2 + 1


def _plane_wave(xs, theta, F, n, seed=9):
    return synth.noise_source_stream(xs, theta, FS, (F + 1) * n // 2, seed, snr_db=60).astype(np.float64)


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("xs", [synth.ULA8, synth.REEM_C], ids=["ula8", "reem_c"])
def test_a_plane_wave_goes_to_its_look_direction(xs, s):
    """a plane wave from look direction s against a second direction 60 degrees away, default thresholds: from the first bin whose
    beam-pattern value between the two directions |g_0^H g_1|^2 / M^2 is under 0.5, target_mask[s] = 1, the other target mask is
    0 and the update mask is 0; outside the band nothing is assigned.  Frames of 1024 samples: a frame of noise is a plane wave only
    as far as the delay across the array (13 samples on the ULA8) is short beside it, and at 256 samples single cells (one of 960) fall
    to a coherence of 0.1 towards their own source"""
    F, N = 8, 1024
    K = N // 2 + 1
    doas = np.deg2rad([-20.0, 40.0])
    g = nt.steering(FS, N, xs, doas)                                       # [K][S][M]
    M = g.shape[2]
    pattern = np.abs(np.sum(np.conj(g[:, 0]) * g[:, 1], axis=1)) ** 2 / M ** 2
    k0 = int(np.flatnonzero(pattern < 0.5)[0])
    pcm = _plane_wave(xs, doas[s], F, N)
    m = et.masks(FS, N, xs, pcm, np.tile(doas, (F, 1)), bin_lo=k0, bin_hi=K - 2)
    band = slice(k0, K - 1)
    worst = float(m["c"][:, band, s].min())
    print("M %d source %d: bins %d ... %d, least coherence towards the source %.4f, largest towards the other direction %.4f"
          % (M, s, k0, K - 2, worst, float(m["c"][:, band, 1 - s].max())))
    assert 0 < k0 < K // 2
    assert np.array_equal(m["target"][s][:, band], np.ones((F, K - 1 - k0)))
    assert not m["target"][1 - s].any()
    assert not m["update"][:, band].any()
    # out of the band: target 0, update 1, whatever the cell holds
    for sl in (slice(0, k0), slice(K - 1, K)):
        assert not m["target"][:, :, sl].any() and np.array_equal(m["update"][:, sl], np.ones_like(m["update"][:, sl]))


def test_silent_and_non_finite_cells():
    """e <= 1e-30: every c is 0, the winner is direction 0 with v = 0 -- target 0, update 1; a NaN cell likewise; with coherence_lo = 0 a
    cell just above silence is assigned as any other (c is a ratio)"""
    F, S, M = 3, 2, 4
    xs = np.arange(M) * 0.03
    g = et.steering_frames(FS, N, xs, np.tile(np.deg2rad([10.0, -50.0]), (F, 1)))
    X = np.zeros((F, M, K), dtype=np.complex128)
    X[1, :, 40] = 1e-16                                                    # e = 4e-32: silent
    X[1, :, 41] = 1e-14 * g[1, 41, 1]                                      # e = 4e-28: live, a plane wave from direction 1
    X[2, 0, 50] = np.nan
    for dt in (np.float64, np.float32):
        m = et.estimate(X, g, dtype=dt)
        assert m["update"][1, 41] == 0.0 and m["target"][1, 1, 41] == 1.0 and m["target"][0, 1, 41] == 0.0
        m["update"][1, 41], m["target"][1, 1, 41] = 1.0, 0.0
        assert not m["target"].any() and np.array_equal(m["update"], np.ones((F, K), dtype=dt))
        assert not m["c"][1, 40].any() and m["w"][1, 41] == 1 and int(m["w"].sum()) == 1


def test_ties_and_nans_stay_with_the_lower_index_and_thresholds_clamp():
    F, M = 1, 4
    xs = np.arange(M) * 0.04
    doa = np.deg2rad([[15.0, 15.0, -30.0]])
    g = et.steering_frames(FS, N, xs, doa)
    X = np.swapaxes(g[:, :, 0, :], 1, 2).copy()                           # every bin a plane wave from direction 0 == direction 1
    m = et.estimate(X, g, coherence_lo=0.5, coherence_hi=0.9)
    assert np.array_equal(m["c"][..., 0], m["c"][..., 1]) and not m["w"][:, 8:].any()
    assert np.allclose(m["target"][0][:, 8:], 1.0) and not m["target"][1:].any()
    # between the thresholds the mask is linear in c, under coherence_lo it is 0
    half = X + np.swapaxes(g[:, :, 2, :], 1, 2)
    m = et.estimate(half, g, coherence_lo=0.2, coherence_hi=0.999)
    c = m["c"].max(axis=2)
    inner = (c > 0.2) & (c < 0.999)
    assert inner.any()
    assert np.allclose(m["target"].max(axis=0)[inner], (c[inner] - 0.2) / 0.799, rtol=0, atol=1e-12)
    m = et.estimate(half, g, coherence_lo=0.9995, coherence_hi=1.0)
    assert not m["target"][:, inner].any() and np.array_equal(m["update"][inner], np.ones(int(inner.sum())))


def test_a_competitor_takes_cells_and_leaves_the_update_mask_open():
    """S = 2 with n_protected = 1: where direction 1 wins, its target mask holds v and the update mask stays 1; with both protected
    the same cells are closed.  n_protected above S counts as all."""
    xs = synth.ULA8
    F = 8
    pcm = nt.scene(xs, FS, N, F, 0).astype(np.float64)
    doa = nt.drifting_doa(1, F, 2)[0]
    one = et.masks(FS, N, xs, pcm, doa, n_protected=1)
    both = et.masks(FS, N, xs, pcm, doa, n_protected=0)
    over = et.masks(FS, N, xs, pcm, doa, n_protected=4)
    comp = one["w"] == 1
    print("competitor wins %d of %d cells" % (int(comp.sum()), comp.size))
    assert comp.any() and not comp.all()
    assert np.array_equal(one["target"], both["target"])
    assert np.array_equal(one["update"][comp], np.ones(int(comp.sum()))) and one["target"][1][comp].min() > 0.0
    assert np.array_equal(one["update"][~comp], 1.0 - one["target"][0][~comp])
    assert np.array_equal(both["update"], 1.0 - both["target"].max(axis=0)) and both["update"][comp].max() < 1.0
    assert np.array_equal(over["update"], both["update"])


def test_the_auto_stream_is_the_stream_under_its_own_masks():
    """the auto call is the masked (without RTF) or the RTF call fed the masks it returns, and the masks of a stream cut into calls
    are the masks of the whole stream (the estimator holds no state)"""
    xs = synth.REEM_C
    F, S = 12, 2
    hop = N // 2
    pcm = nt.scene(xs, FS, N, F, 1).astype(np.float64)
    doa = nt.drifting_doa(2, F, S)[1].astype(np.float64)
    cfg = et.parity_config(N, S)
    a = et.auto_stream(FS, N, xs, pcm, doa, cfg)
    q = mt.mvdr_mask_stream(FS, N, xs, pcm, doa, 0.0, a["update_mask"])
    assert np.array_equal(a["spec"], q["spec"]) and np.array_equal(a["phi"], q["phi"])
    r = et.auto_stream(FS, N, xs, pcm, doa, cfg, rtf=et.SCENE_RTF)
    q = rt.mvdr_rtf_stream(FS, N, xs, pcm, doa, r["update_mask"], r["target_mask"], **et.SCENE_RTF)
    assert np.array_equal(r["spec"], q["spec"]) and np.array_equal(r["psi"], q["psi"]) and r["est"].any()
    st, um, tm = None, [], []
    for t0, t1 in ((0, 5), (5, 12)):
        st = et.auto_stream(FS, N, xs, pcm[:, t0 * hop:(t1 + 1) * hop], doa[t0:t1], cfg, rtf=et.SCENE_RTF, state=st)
        um.append(st["update_mask"]); tm.append(st["target_mask"])
    assert np.array_equal(np.concatenate(um), r["update_mask"]) and np.array_equal(np.concatenate(tm, axis=1), r["target_mask"])
    assert np.array_equal(st["phi"], r["phi"]) and np.array_equal(st["psi"], r["psi"])


SCENE_TWIN = et.SCENE_TWIN   # the twin's recorded figures of the scene, held to what the test below recomputes


def test_the_scene_without_masks_and_with_estimated_ones():
    """rtf_scene() (ULA8 at 16 kHz, N = 256, gains and positions the beamformer does not know, interferer at -40 degrees, sparse target
    at +20 degrees, look direction 24 degrees), RTF steering with two iterations, last 24 frames, output 0.  Without masks (update
    all 1, no target mask) the twin keeps 0.009 of the target's power at the reference microphone (interferer 17.21 dB down); with
    the masks estimated for the look directions (+24, -40 degrees), the first one protected, thresholds 0 / 0.05, whole band: 0.982
    and 12.54 dB (oracle masks: 0.998 and 19.52 dB, tests/test_mvdr_rtf_twin.py).  Bars: the project's rt.SCENE_BARS -- share within
    [0.85, 1.15], the share without masks below geometric_below."""
    r = et.scene_runs()
    print("no masks: target share %.3f, interferer %.2f dB under the reference microphone; estimated masks: %.3f, %.2f dB; estimated cells of "
          "the last frames %.1f %%" % (r["none"] + r["estimated"] + (100.0 * r["run"]["est"][-rt.SCENE_LAST:, 0].mean(),)))
    b = rt.SCENE_BARS
    assert r["none"][0] < b["geometric_below"]
    assert b["share_lo"] <= r["estimated"][0] <= b["share_hi"]
    # the recorded figures are the twin's (the GPU test's suppression bar is the recorded figure less 3 dB)
    for key in ("none", "estimated"):
        assert abs(r[key][0] - SCENE_TWIN[key][0]) <= 2e-3 and abs(r[key][1] - SCENE_TWIN[key][1]) <= 0.02, (key, r[key])


@pytest.mark.parametrize("case", et.PARITY_CASES, ids=[c[0] for c in et.PARITY_CASES])
def test_parity_cases_keep_clear_of_the_decision_edges(case):
    """the cases of the GPU parity test on the twin alone: at most 1 % of the cells are edge cells (two largest c within 1e-4, e under
    1e-6 of the frame's largest, or another winner in float32), every look direction wins cells, the masks take values inside (0, 1),
    and the float32 variant stays within MASK_F32_MEASURED = 1.031e-6 of the float64 twin outside edge cells (the largest, M8_S1) -- the GPU's bar is four times that"""
    share, wt, wu = et.parity_distance(case)
    p = et.parity(case)
    S = case[4]
    wins = np.bincount(np.concatenate([d["w"][:, d["band"]].ravel() for d in p["d64"]]), minlength=S)
    tm = np.concatenate([d["target"].ravel() for d in p["d64"]])
    print("%s: %.3f %% edge cells; float32 variant: target masks %.2e, update mask %.2e; wins %s; %.1f %% of the target cells inside (0, 1)"
          % (case[0], 100.0 * share, wt, wu, wins, 100.0 * ((tm > 0) & (tm < 1)).mean()))
    assert share <= 0.01
    assert wins.min() > 0 and ((tm > 0) & (tm < 1)).any() and (tm == 1).any()
    assert wt <= et.MASK_F32_MEASURED and wu <= et.MASK_F32_MEASURED


def test_the_recorded_distance_is_the_measured_one():
    worst = max(max(et.parity_distance(c)[1:]) for c in et.PARITY_CASES)
    print("largest float32 distance over the parity cases: %.3e (recorded %.3e, bar %.3e)" % (worst, et.MASK_F32_MEASURED, et.MASK_BAR))
    assert 0.9 * et.MASK_F32_MEASURED <= worst <= et.MASK_F32_MEASURED
    assert et.MASK_BAR == 4.0 * et.MASK_F32_MEASURED
