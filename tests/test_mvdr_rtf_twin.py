"""CPU: the float64 twin of the MVDR call that steers with an estimated relative transfer function (tests/mvdr_rtf_twin.py) against
the mask twin, against the properties of the definition (include/mcarray_hip.h, mca_hip_mvdr_set_rtf) and on the scene in which the
geometric vector distorts the target."""
import numpy as np
import pytest

from mcarray_amd import synth

import mvdr_mask_twin as mt
import mvdr_nulls_twin as nt
import mvdr_postfilter_twin as pt
import mvdr_rtf_twin as rt

# (xs, fs, N, S, pf) of tests/test_gpu_mvdr_rtf.py::test_rtf_parity
PARITY_CASES = [(pt.irregular(M), 16000, 256, S, None) for M in (2, 3, 4, 5, 8, 11, 13, 16) for S in (1, 2, 4)]
PARITY_CASES += [(pt.irregular(11), 16000, 256, 3, pt.PARITY_PF), (synth.ULA16, 48000, 1024, 3, None)]


@pytest.mark.parametrize("pf", [None, pt.PARITY_PF])
def test_a_target_mask_of_zeros_on_fresh_state_is_the_mask_twin(pf):
    """nothing learned: every cell falls back to the geometric vector, and the run is mvdr_mask_twin's exactly"""
    fs, N, F, S = 16000, 256, 12, 2
    xs = synth.REEM_C
    pcm = nt.scene(xs, fs, N, F, 0).astype(np.float64)
    doa = nt.drifting_doa(1, F, S)[0].astype(np.float64)
    upd = mt.parity_mask()[0]
    for tm in (None, np.zeros((S, F, N // 2 + 1)), np.full((S, F, N // 2 + 1), np.nan), -1.0):
        r = rt.mvdr_rtf_stream(fs, N, xs, pcm, doa, upd, tm, pf=pf)
        q = mt.mvdr_mask_stream(fs, N, xs, pcm, doa, 0.0, upd) if pf is None else mt.mvdr_mask_postfilter_stream(fs, N, xs, pcm, doa, 0.0, upd, **pf)
        for key in ("spec", "out", "phi", "tail") + (("A", "p") if pf else ()):
            assert np.array_equal(r[key], q[key]), key
        assert not r["est"].any() and not r["psi"].any() and not r["cpsi"].any()
        # cphi counts the weights in Phi: 0 where the update mask never opened, else 1 - prod(a_tk)
        u = np.nan_to_num(np.clip(upd.astype(np.float64), 0.0, 1.0), nan=0.0)
        assert np.allclose(r["cphi"], 1.0 - np.prod(1.0 - 0.05 * u, axis=0), rtol=0, atol=1e-12)


@pytest.mark.parametrize("M,ref", [(2, 1), (5, 0), (8, 3), (16, 9)])
def test_a_rank_one_target_covariance_returns_the_transfer_function(M, ref):
    """Psi = p h h^H, Phi = 0: one iteration from any start that is not orthogonal to h gives h / h_ref; further iterations change
    nothing; a start orthogonal to h, a zero Psi and a zero reference entry fall back to the start"""
    rng = np.random.default_rng(M)
    K = 7
    h = rng.standard_normal((K, M)) + 1j * rng.standard_normal((K, M))
    p = 10.0 ** rng.uniform(-12, 3, K)
    psi = p[:, None, None] * h[:, :, None] * np.conj(h[:, None, :])
    cpsi = rng.uniform(0.1, 1.0, K)
    g0 = rng.standard_normal((K, M)) + 1j * rng.standard_normal((K, M))
    zero = np.zeros_like(psi)
    for it in (1, 2, 4):
        # (min_share 0 for the single iteration: its rho is the start's share of h, anything above 0 here; from the second on rho = 1)
        d, est, dg = rt.estimate(psi, cpsi, zero, np.zeros(K), g0, iterations=it, ref_mic=ref, min_share=0.0 if it == 1 else 0.05)
        assert est.all()
        assert np.abs(d - h / h[:, ref][:, None]).max() <= 1e-12 * np.abs(d).max()
        assert np.array_equal(d[:, ref], np.ones(K))
        assert np.allclose(dg["rho"], 1.0, atol=1e-12) if it > 1 else np.all(dg["rho"] > 0)      # tr(Delta) = 1: the share of the dominant direction
    # orthogonal start: g = 0
    orth = g0 - h * (np.sum(np.conj(h) * g0, axis=1) / np.sum(np.abs(h) ** 2, axis=1))[:, None]
    d, est, _ = rt.estimate(psi, cpsi, zero, np.zeros(K), orth, iterations=1, ref_mic=ref)
    assert not est.any() and np.array_equal(d, orth)
    d, est, _ = rt.estimate(zero, np.zeros(K), zero, np.zeros(K), g0, ref_mic=ref)
    assert not est.any() and np.array_equal(d, g0)
    h0 = h.copy()
    h0[:, ref] = 0.0
    d, est, _ = rt.estimate(p[:, None, None] * h0[:, :, None] * np.conj(h0[:, None, :]), cpsi, zero, np.zeros(K), g0, ref_mic=ref)
    assert not est.any() and np.array_equal(d, g0)


def test_the_noise_covariance_is_subtracted():
    """Psi = target + noise with the noise covariance in Phi: the estimate is the target's transfer function, which the dominant
    direction of Psi alone is not when the noise is as loud"""
    rng = np.random.default_rng(1)
    K, M = 5, 8
    h = np.exp(1j * rng.uniform(0, 6.28, (K, M)))
    q = np.exp(1j * rng.uniform(0, 6.28, (K, M)))
    noise = 2.0 * q[:, :, None] * np.conj(q[:, None, :]) + 0.1 * np.eye(M)
    psi = 0.6 * (h[:, :, None] * np.conj(h[:, None, :]) + noise)
    d, est, _ = rt.estimate(psi, np.full(K, 0.6), 0.9 * noise, np.full(K, 0.9), h + 0.3 * q, iterations=2)
    assert est.all() and np.abs(d - h / h[:, :1]).max() <= 1e-9
    d, _, _ = rt.estimate(psi, np.full(K, 0.6), np.zeros_like(noise), np.zeros(K), h + 0.3 * q, iterations=2)
    assert np.abs(d - h / h[:, :1]).max() > 0.3


@pytest.mark.parametrize("pf", [None, pt.PARITY_PF])
def test_state_is_carried_across_calls(pf):
    fs, N, F, S = 16000, 256, 12, 2
    xs = pt.irregular(5)
    hop = N // 2
    pcm, doa, _, _ = rt.parity_inputs(xs, fs, N, S, A=1)
    pcm, doa = pcm[0].astype(np.float64), doa[0]
    upd, tm = mt.parity_mask(1, F)[0], rt.target_parity_mask(S, 1, F)[0]
    cfg = rt.parity_config(5)
    one = rt.mvdr_rtf_stream(fs, N, xs, pcm, doa, upd, tm, pf=pf, **cfg)
    assert one["est"].any() and not one["est"].all()
    for cuts in ([0, 5, 12], list(range(13))):
        st, specs = None, []
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            st = rt.mvdr_rtf_stream(fs, N, xs, pcm[:, t0 * hop:(t1 + 1) * hop], doa[t0:t1], upd[t0:t1], tm[:, t0:t1], pf=pf, state=st, **cfg)
            specs.append(st["spec"])
        assert np.array_equal(np.concatenate(specs, axis=1), one["spec"])
        for key in ("phi", "psi", "cpsi", "cphi", "tail") + (("A",) if pf else ()):
            assert np.array_equal(st[key], one[key]), key


def test_closed_target_cells_leave_psi():
    fs, N, F = 16000, 256, 6
    xs = synth.REEM_C
    K = N // 2 + 1
    pcm = nt.scene(xs, fs, N, 2 * F, 0).astype(np.float64)
    hop = N // 2
    lead = rt.mvdr_rtf_stream(fs, N, xs, pcm[:, :(F + 1) * hop], np.full(F, 0.3), None, 1.0)
    tm = np.ones((1, F, K))
    tm[0, :, 1::2] = np.random.default_rng(0).choice([0.0, np.nan, -1.0, -0.0], size=(F, K // 2))
    r = rt.mvdr_rtf_stream(fs, N, xs, pcm[:, F * hop:], np.full(F, 0.3), None, tm, state=lead)
    assert np.array_equal(r["psi"][0, 1::2], lead["psi"][0, 1::2]) and np.array_equal(r["cpsi"][0, 1::2], lead["cpsi"][0, 1::2])
    assert all(not np.array_equal(r["psi"][0, k], lead["psi"][0, k]) for k in range(0, K, 2))


# the twin's figures on the scene (printed by the test below): target share and interferer suppression in dB
SCENE_TWIN = dict(geometric=(0.462, 23.14), rtf=(0.998, 19.52))


def test_the_scene_shows_the_need_and_the_cure():
    """rtf_scene(): ULA8 at 16 kHz, N = 256, gains +-2 dB and position errors of about 8 mm the beamformer does not know, interferer at
    -40 degrees, sparse target at +20 degrees 10 dB above it in its cells, look direction 24 degrees, oracle masks.  Over the last
    24 frames the twin keeps 0.462 of the target's power at the reference microphone with the geometric vector (interferer 23.14 dB
    down) and 0.998 with the estimated one (19.52 dB down; one iteration: 1.002, 19.52).  Bars: RTF share within [0.85, 1.15],
    geometric share below 0.8.  The scene's perturbation seed was chosen among 15 for a reference microphone of about nominal gain;
    the bars and the rest of the scene are as first written."""
    sc = rt.rtf_scene()
    doa = np.full((rt.SCENE_F, 1), rt.SCENE_LOOK)
    pcm = sc["pcm"].astype(np.float64)
    g = mt.mvdr_mask_stream(rt.SCENE_FS, rt.SCENE_N, sc["xs"], pcm, doa, 0.0, sc["update"], want_weights=True)
    fg = rt.scene_figures(g["w"][:, 0], sc)
    print("geometric: target share %.3f, interferer %.2f dB under the reference microphone" % fg)
    figs = {}
    for it in (1, 2):
        r = rt.mvdr_rtf_stream(rt.SCENE_FS, rt.SCENE_N, sc["xs"], pcm, doa, sc["update"], sc["tmask"], iterations=it, want_weights=True)
        figs[it] = rt.scene_figures(r["w"][:, 0], sc)
        print("RTF, %d iteration(s): target share %.3f, interferer %.2f dB under; estimated cells of the last frames %.1f %%"
              % ((it,) + figs[it] + (100.0 * r["est"][-rt.SCENE_LAST:].mean(),)))
    b = rt.SCENE_BARS
    assert fg[0] < b["geometric_below"]
    for it in (1, 2):
        assert b["share_lo"] <= figs[it][0] <= b["share_hi"]
    # the recorded figures are the twin's (the GPU test's suppression bar is the recorded figure less 3 dB)
    assert abs(fg[0] - SCENE_TWIN["geometric"][0]) <= 2e-3 and abs(fg[1] - SCENE_TWIN["geometric"][1]) <= 0.02
    assert abs(figs[2][0] - SCENE_TWIN["rtf"][0]) <= 2e-3 and abs(figs[2][1] - SCENE_TWIN["rtf"][1]) <= 0.02
    # without the subtraction the estimate is pulled towards the interferer
    e, _, _ = rt.estimate(r["psi"][0], r["cpsi"][0], np.zeros_like(r["phi"]), np.zeros_like(r["cphi"]), r["d"][-1, 0])
    d = r["d"][-1, 0]
    assert np.abs(e - d).max() > 0.05


@pytest.mark.parametrize("case", range(len(PARITY_CASES)))
def test_parity_cases_keep_clear_of_the_decision_edges(case):
    """the cases of the GPU parity test on the twin alone: at most 1 % of the cells sit at a decision edge (and are left out of the
    comparison there), estimated and fallback cells both occur, and the estimator evaluated in float32 on the same float64 state
    stays within 1.25e-4 of the peak in spectra and steering vectors -- measured 2.4e-5 and 2.8e-5 at the most -- so the module's 5e-4
    bars hold for the GPU test"""
    xs, fs, N, S, pf = PARITY_CASES[case]
    t64, t32 = rt.parity_twin(xs, fs, N, S, pf), rt.parity_twin(xs, fs, N, S, pf, est_dtype=np.float32)
    n_edge = n_all = 0
    ws = wd = 0.0
    for a in range(2):
        for c in range(2):
            r, q = t64[a][c], t32[a][c]
            e = rt.edges_of(r)
            assert r["est"].any() and not r["est"].all(), (a, c)
            n_edge, n_all = n_edge + int(e.sum()), n_all + e.size
            ws = max(ws, (np.abs(r["spec"] - q["spec"]) * ~np.swapaxes(e, 0, 1)).max() / np.abs(r["raw" if pf else "spec"]).max())
            wd = max(wd, (np.abs(r["d"] - q["d"]) * ~e[..., None]).max() / np.abs(r["d"]).max())
    print("M %d N %d S %d: %.3f %% edge cells; float32 estimator: spectra %.2e, steering %.2e of the peak" % (len(xs), N, S, 100.0 * n_edge / n_all, ws, wd))
    assert n_edge <= 0.01 * n_all
    assert ws <= 1.25e-4 and wd <= 1.25e-4
