"""CPU: the float64 twin of the MVDR call with the decision-directed Wiener post-filter (tests/mvdr_postfilter_twin.py) against
the twin without it, against the properties of the definition (include/mcarray_hip.h, mca_hip_mvdr_set_postfilter), on the
self-cancellation scene with a noise-only covariance, and on every parity scene of tests/test_gpu_mvdr_postfilter.py: there the
filtered spectra are far from the unfiltered ones, so a kernel that ignores the filter cannot pass."""
import numpy as np
import pytest

from mcarray_amd import synth

import mvdr_gate_twin as gt
import mvdr_nulls_twin as nt
import mvdr_postfilter_twin as pt

WEIGHTS = np.array([1, 1, .5, 0, 0, 1, .25, 0, 0, 0, 1, .75])


@pytest.mark.parametrize("S,gain", [(1, 0.0), (3, 0.0), (3, 10.0)])
def test_gain_floor_one_is_the_gate_twin(S, gain):
    fs, N, F = 16000, 256, 12
    xs = synth.REEM_C
    pcm = nt.scene(xs, fs, N, F, 0).astype(np.float64)
    doa = nt.drifting_doa(1, F, S)[0].astype(np.float64)
    g = gt.mvdr_gate_stream(fs, N, xs, pcm, doa, gain, WEIGHTS)
    r = pt.mvdr_postfilter_stream(fs, N, xs, pcm, doa, gain, WEIGHTS, gain_floor=1.0)
    for key in ("spec", "out", "phi", "tail"):
        assert np.abs(r[key] - g[key]).max() <= 1e-12 * np.abs(g[key]).max(), key
    assert np.all(r["gain"] == 1.0)
    # and the unfiltered spectra a filtered run reports are the gate twin's, whatever the filter does
    f = pt.mvdr_postfilter_stream(fs, N, xs, pcm, doa, gain, WEIGHTS)
    assert np.abs(f["raw"] - g["spec"]).max() <= 1e-12 * np.abs(g["spec"]).max()
    assert np.abs(f["raw_out"] - g["out"]).max() <= 1e-12 * np.abs(g["out"]).max()
    assert np.array_equal(f["phi"], r["phi"])


def test_gain_range_and_silent_bins():
    """G lies in [floor, 1]; G = 1 exactly where the bin is digitally silent so far (p = 0), also behind a filtered lead-in"""
    fs, N, F, S = 16000, 256, 8, 2
    xs = synth.REEM_C
    hop = N // 2
    pcm = nt.scene(xs, fs, N, F, 0).astype(np.float64)
    pcm[:, :4 * hop] = 0.0                                                   # frames 0 ... 2 see nothing at all
    doa = nt.drifting_doa(1, F, S)[0].astype(np.float64)
    for floor in (0.0, 0.1, 0.7):
        r = pt.mvdr_postfilter_stream(fs, N, xs, pcm, doa, 0.0, None, gain_floor=floor)
        assert r["gain"].min() >= floor and r["gain"].max() <= 1.0
        assert np.all(r["p"][:, :3] == 0.0) and np.all(r["gain"][:, :3] == 1.0)
        assert np.array_equal(r["spec"][:, :3], r["raw"][:, :3])
        assert np.all(r["p"][:, 4:] > 0.0) and r["gain"][:, 4:].min() < 1.0
        assert np.array_equal(r["spec"], r["gain"] * r["raw"])
    # the floor is reached and left
    r = pt.mvdr_postfilter_stream(fs, N, xs, pcm, doa, 0.0, None, gain_floor=0.1)
    assert (r["gain"] == 0.1).any() and ((r["gain"] > 0.1) & (r["gain"] < 1.0)).any()


def test_state_is_carried_across_calls():
    fs, N, F, S = 16000, 256, 12, 2
    xs = synth.REEM_C
    hop = N // 2
    pcm = nt.scene(xs, fs, N, F, 0).astype(np.float64)
    doa = nt.drifting_doa(1, F, S)[0].astype(np.float64)
    one = pt.mvdr_postfilter_stream(fs, N, xs, pcm, doa, 10.0, WEIGHTS, **pt.PARITY_PF)
    for cuts in ([0, 5, 12], list(range(13))):
        st, outs, specs = None, [], []
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            st = pt.mvdr_postfilter_stream(fs, N, xs, pcm[:, t0 * hop:(t1 + 1) * hop], doa[t0:t1], 10.0, WEIGHTS[t0:t1], state=st, **pt.PARITY_PF)
            outs.append(st["out"]); specs.append(st["spec"])
        assert np.abs(np.concatenate(outs, axis=1) - one["out"]).max() <= 1e-12 * np.abs(one["out"]).max()
        assert np.abs(np.concatenate(specs, axis=1) - one["spec"]).max() <= 1e-12 * np.abs(one["spec"]).max()
        assert np.abs(st["A"] - one["A"]).max() <= 1e-12 * np.abs(one["A"]).max()
        assert np.abs(st["phi"] - one["phi"]).max() <= 1e-12 * np.abs(one["phi"]).max()
    # a state of two slots continued with one and with two again: slot 1 restarts from silence
    r2 = pt.mvdr_postfilter_stream(fs, N, xs, pcm[:, :5 * hop], doa[:4], 0.0, None)
    r1 = pt.mvdr_postfilter_stream(fs, N, xs, pcm[:, 4 * hop:9 * hop], doa[4:8, :1], 0.0, None, state=r2)
    assert r1["A"].shape == (1, N // 2 + 1) and r1["tail"].shape == (1, hop)
    r3 = pt.mvdr_postfilter_stream(fs, N, xs, pcm[:, 8 * hop:], doa[8:], 0.0, None, state=r1)
    z = dict(r1, A=np.concatenate([r1["A"], np.zeros_like(r1["A"])]), tail=np.concatenate([r1["tail"], np.zeros_like(r1["tail"])]),
             raw_tail=np.concatenate([r1["raw_tail"], np.zeros_like(r1["raw_tail"])]))
    r3z = pt.mvdr_postfilter_stream(fs, N, xs, pcm[:, 8 * hop:], doa[8:], 0.0, None, state=z)
    assert np.array_equal(r3["spec"], r3z["spec"]) and np.array_equal(r3["out"], r3z["out"])


def test_scene_interferer_down_target_kept():
    """the self-cancellation scene with a noise-only covariance (weights 1 before the target's onset, 0 from it on), look direction
    20 degrees, the defaults (smoothing 0.98, floor 0.1, noise scale 1), powers over the frames 36 ... 47: the interferer alone
    comes out at < 0.03 of its unfiltered power (measured 0.0146: a factor of two of margin), the scene with the target at > 0.95
    (measured 0.9685: a third of the way to 1)"""
    look = np.full(gt.CANCEL_F, np.deg2rad(20.0))
    ratio = {}
    for target in (False, True):
        xs, pcm, update = gt.cancellation_scene(target=target)
        r = pt.mvdr_postfilter_stream(gt.CANCEL_FS, gt.CANCEL_N, xs, pcm.astype(np.float64), look, 0.0, update)
        pu, pf = gt.last_frames_power(r["raw"][0]), gt.last_frames_power(r["spec"][0])
        ratio[target] = pf / pu
        print("target %s: unfiltered %.4g filtered %.4g ratio %.4f" % (target, pu, pf, pf / pu))
    assert ratio[False] < 0.03
    assert ratio[True] > 0.95


@pytest.mark.parametrize("case", pt.parity_cases(), ids=lambda c: c[0])
def test_the_filter_matters_on_the_parity_scenes(case):
    """filtered and unfiltered twin spectra (and audio) differ by at least 20 times the parity bar of the peak of the unfiltered
    ones, in every call, stream and source of the case"""
    p = pt.parity(case)
    worst_s = worst_a = np.inf
    for call in p["calls"]:
        for tw in call:
            for s in range(tw["spec"].shape[0]):
                ds = np.abs(tw["spec"][s] - tw["raw"][s]).max() / np.abs(tw["raw"][s]).max()
                da = np.abs(tw["out"][s] - tw["raw_out"][s]).max() / np.abs(tw["raw_out"][s]).max()
                worst_s, worst_a = min(worst_s, ds), min(worst_a, da)
    g = np.concatenate([tw["gain"].ravel() for call in p["calls"] for tw in call])
    print("%s: filtered against unfiltered, the least over calls, streams and sources: spectra %.3f audio %.3f of the peak; gains %.3f ... %.3f, %.0f %% at the floor"
          % (case[0], worst_s, worst_a, g.min(), g.max(), 100.0 * np.mean(g == pt.PARITY_PF["gain_floor"])))
    assert worst_s >= 20 * pt.PARITY_BAR and worst_a >= 20 * pt.PARITY_BAR
