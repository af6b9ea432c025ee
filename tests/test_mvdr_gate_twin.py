"""CPU: the float64 twin of the MVDR call with per-frame covariance update weights (tests/mvdr_gate_twin.py) against the existing
oracles, against the properties of the definition (include/mcarray_hip.h, mca_hip_mvdr_sources_frames_weighted_*) and on the scene
in which the unweighted recursion cancels its own target."""
import numpy as np
import pytest

from mcarray_amd import synth
from oracle import np_twin
from oracle import pyoracle as po

import mvdr_gate_twin as gt
import mvdr_nulls_twin as nt

WEIGHTS = np.array([1, 1, .5, 0, 0, 1, .25, 0, 0, 0, 1, .75])


def _irregular(M):
    return np.sort(np.random.default_rng(M).uniform(0.0, 0.04 * M, M))


def test_all_ones_is_the_existing_oracle():
    """update all 1 (and None) with gain 0: oracle.np_twin.mvdr_stream and the C oracle, in spectra, audio and covariance"""
    fs, N, F, S = 16000, 256, 8, 3
    xs = synth.REEM_C
    pcm = nt.scene(xs, fs, N, F, 0).astype(np.float64)
    doa = nt.drifting_doa(1, F, S)[0].astype(np.float64)
    r = gt.mvdr_gate_stream(fs, N, xs, pcm, doa, 0.0, np.ones(F))
    none = gt.mvdr_gate_stream(fs, N, xs, pcm, doa, 0.0, None)
    assert np.array_equal(r["spec"], none["spec"]) and np.array_equal(r["phi"], none["phi"])
    for s in range(S):
        o = np_twin.mvdr_stream(fs, N, xs, pcm, doa[:, s])
        m = po.MVDR(fs, N, xs)
        c = m.stream(pcm, doa[:, s], want_spec=True)
        cspec = c["spec"][:, 0::2] + 1j * c["spec"][:, 1::2]
        for name, spec, out, phi in (("np_twin", o["spec"], o["out"], o["phi"]), ("C oracle", cspec, c["out"], m.covariance())):
            es = np.abs(r["spec"][s] - spec).max() / np.abs(spec).max()
            ea = np.abs(r["out"][s] - out).max() / np.abs(out).max()
            ec = np.abs(r["phi"] - phi).max() / np.abs(phi).max()
            print("source %d against %s: spectra %.2e audio %.2e covariance %.2e of the peak" % (s, name, es, ea, ec))
            assert es <= 1e-10 and ea <= 1e-10 and ec <= 1e-10, (s, name)
    # the nulls twin at a gain, too
    g = gt.mvdr_gate_stream(fs, N, xs, pcm, doa, 10.0, np.ones(F))
    n = nt.mvdr_nulls_stream(fs, N, xs, pcm, doa, 10.0)
    assert np.abs(g["spec"] - n["spec"]).max() <= 1e-10 * np.abs(n["spec"]).max()
    assert np.abs(g["out"] - n["out"]).max() <= 1e-10 * np.abs(n["out"]).max()


def test_state_is_carried_across_calls():
    fs, N, F, S = 16000, 256, 12, 2
    xs = synth.REEM_C
    hop = N // 2
    pcm = nt.scene(xs, fs, N, F, 0).astype(np.float64)
    doa = nt.drifting_doa(1, F, S)[0].astype(np.float64)
    one = gt.mvdr_gate_stream(fs, N, xs, pcm, doa, 10.0, WEIGHTS)
    r1 = gt.mvdr_gate_stream(fs, N, xs, pcm[:, :(5 + 1) * hop], doa[:5], 10.0, WEIGHTS[:5])
    r2 = gt.mvdr_gate_stream(fs, N, xs, pcm[:, 5 * hop:], doa[5:], 10.0, WEIGHTS[5:], state=r1)
    assert np.abs(np.concatenate([r1["out"], r2["out"]], axis=1) - one["out"]).max() <= 1e-12 * np.abs(one["out"]).max()
    assert np.abs(r2["phi"] - one["phi"]).max() <= 1e-12 * np.abs(one["phi"]).max()


@pytest.mark.parametrize("geo", ["four_irregular", "sixteen_irregular"])
def test_the_weights_matter(geo):
    """the scene and the weights of the GPU tests: the weighted spectra and covariance are far from the unweighted ones, so a
    kernel that ignores the weights cannot pass the 5e-4 / 5e-6 bars there"""
    fs, N, F, S = 16000, 256, 12, 2
    xs = _irregular(4) if geo == "four_irregular" else _irregular(16)
    pcm = nt.scene(xs, fs, N, F, 0).astype(np.float64)
    doa = nt.drifting_doa(1, F, S)[0].astype(np.float64)
    w = gt.mvdr_gate_stream(fs, N, xs, pcm, doa, 0.0, WEIGHTS)
    p = gt.mvdr_gate_stream(fs, N, xs, pcm, doa, 0.0, None)
    ds = max(np.abs(w["spec"][s] - p["spec"][s]).max() / np.abs(p["spec"][s]).max() for s in range(S))
    dc = np.abs(w["phi"] - p["phi"]).max() / np.abs(p["phi"]).max()
    print("%s: weighted against unweighted: spectra %.2f covariance %.2f of the peak" % (geo, ds, dc))
    assert ds >= 0.1 and dc >= 0.1


def test_noise_only_covariance_keeps_the_target():
    """the self-cancellation scene: with the covariance frozen from the target's onset on, the last 12 frames carry at least four
    times the power the all-ones run leaves of the target (measured: 13 times; the 4 leaves 5 dB for fp32 and seeds)"""
    xs, pcm, update = gt.cancellation_scene()
    pcm = pcm.astype(np.float64)
    doa = np.full(gt.CANCEL_F, gt.CANCEL_LOOK)
    ones = gt.mvdr_gate_stream(gt.CANCEL_FS, gt.CANCEL_N, xs, pcm, doa, 0.0, None)
    gated = gt.mvdr_gate_stream(gt.CANCEL_FS, gt.CANCEL_N, xs, pcm, doa, 0.0, update)
    p1, pg = gt.last_frames_power(ones["spec"][0]), gt.last_frames_power(gated["spec"][0])
    target = gt.mvdr_gate_stream(gt.CANCEL_FS, gt.CANCEL_N, xs, pcm - gt.cancellation_scene(target=False)[1], doa, 0.0, np.zeros(gt.CANCEL_F))
    print("last 12 frames: all ones %.1f, frozen from the onset %.1f: %.1f times; the target alone through delay-and-sum %.1f"
          % (p1, pg, pg / p1, gt.last_frames_power(target["spec"][0])))
    assert pg >= 4.0 * p1


def test_exact_points():
    fs, N, F = 16000, 256, 6
    xs = synth.REEM_C
    hop = N // 2
    pcm = nt.scene(xs, fs, N, F, 0).astype(np.float64)
    doa = nt.drifting_doa(1, F, 1)[0].astype(np.float64)
    lead = gt.mvdr_gate_stream(fs, N, xs, pcm[:, :(3 + 1) * hop], doa[:3], 0.0, None)
    # a weight of 0 leaves phi bit-identical, and the frames are still beamformed
    froz = gt.mvdr_gate_stream(fs, N, xs, pcm[:, 3 * hop:], doa[3:], 0.0, np.zeros(3), state=lead)
    assert np.array_equal(froz["phi"], lead["phi"])
    assert np.abs(froz["spec"]).min(axis=2).max() > 0.0
    # NaN, -3 and 7 behave as 0, 0 and 1
    assert np.array_equal(gt.clamp([np.nan, -3.0, 7.0, 0.25]), [0.0, 0.0, 1.0, 0.25])
    odd = gt.mvdr_gate_stream(fs, N, xs, pcm[:, 3 * hop:], doa[3:], 0.0, [np.nan, -3.0, 7.0], state=lead)
    ref = gt.mvdr_gate_stream(fs, N, xs, pcm[:, 3 * hop:], doa[3:], 0.0, [0.0, 0.0, 1.0], state=lead)
    assert np.array_equal(odd["spec"], ref["spec"]) and np.array_equal(odd["phi"], ref["phi"])
    assert not np.array_equal(odd["phi"], lead["phi"])
    # a frozen fresh stream is the delay-and-sum
    fresh = gt.mvdr_gate_stream(fs, N, xs, pcm, doa, 0.0, np.zeros(F))
    d = np.stack([nt.steering(fs, N, xs, doa[t])[:, 0] for t in range(F)])            # [F][K][M]
    X = np_twin.stft_frames(pcm, N)                                                  # [F][M][K]
    das = np.einsum("fkm,fmk->fk", np.conj(d), X) / len(xs)
    assert np.abs(fresh["spec"][0] - das).max() <= 1e-12 * np.abs(das).max()
    assert not fresh["phi"].any()
