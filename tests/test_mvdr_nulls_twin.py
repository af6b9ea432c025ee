"""CPU: the float64 twin of the MVDR call with soft nulls (tests/mvdr_nulls_twin.py) against oracle.np_twin.mvdr_stream, against the
Gram route the kernel evaluates, and against the properties of the definition (include/mcarray_hip.h, mca_hip_mvdr_set_null_gain)."""
import numpy as np
import pytest

from mcarray_amd import synth
from oracle import np_twin

import mvdr_nulls_twin as nt

GAINS = [0.0, 10.0, 100.0, 1000.0]


def _loaded(fs, N, xs, F, a=0, loading=1e-3):
    """the loaded covariances [K][M][M] and the last frame's spectra [K][M] after F frames of scene a"""
    pcm = nt.scene(xs, fs, N, F, a).astype(np.float64)
    X = np_twin.stft_frames(pcm, N)
    M, K = X.shape[1], X.shape[2]
    Phi = np.zeros((K, M, M), dtype=np.complex128)
    for t in range(F):
        Xc = X[t].T
        Phi = 0.95 * Phi + 0.05 * Xc[:, :, None] * np.conj(Xc[:, None, :])
    tr = np.real(np.trace(Phi, axis1=1, axis2=2))
    return Phi + (loading * tr / M)[:, None, None] * np.eye(M), X[F - 1].T


CASES = {
    "ula16_s2": (synth.ULA16, 48000, 256, [0.35, -0.15]),
    "ula16_s4": (synth.ULA16, 48000, 256, [0.35, -0.15, 0.8, -0.45]),
    "reemc_s3": (synth.REEM_C, 16000, 256, [0.35, -0.6, 1.1]),
    "five_s4": ([0.0, 0.03, 0.07, 0.10, 0.20], 8000, 256, [0.3, -0.7, 0.9, 0.2]),
    "coincident_pair": (synth.ULA8, 48000, 256, [0.35, 0.35]),
    "coincident_two_of_three": (synth.ULA8, 48000, 256, [0.35, -0.4, 0.35]),
    "four_on_two_microphones": (synth.BINAURAL, 16000, 256, [0.3, -0.7, 0.9, 0.2]),
}


def test_gain_zero_is_the_plain_mvdr_of_np_twin():
    fs, N, F, S = 16000, 256, 8, 3
    xs = synth.REEM_C
    pcm = nt.scene(xs, fs, N, F, 0).astype(np.float64)
    doa = nt.drifting_doa(1, F, S)[0].astype(np.float64)
    r = nt.mvdr_nulls_stream(fs, N, xs, pcm, doa, 0.0)
    for s in range(S):
        o = np_twin.mvdr_stream(fs, N, xs, pcm, doa[:, s])
        es = np.abs(r["spec"][s] - o["spec"]).max() / np.abs(o["spec"]).max()
        ea = np.abs(r["out"][s] - o["out"]).max() / np.abs(o["out"]).max()
        print("source %d: spectra %.2e audio %.2e of the peak" % (s, es, ea))
        assert es <= 1e-12 and ea <= 1e-12, s
        assert np.abs(r["phi"] - o["phi"]).max() <= 1e-12 * np.abs(o["phi"]).max()
    # a second call that continues from the state equals one call
    h = (F // 2) * (N // 2)
    r1 = nt.mvdr_nulls_stream(fs, N, xs, pcm[:, :h + N // 2], doa[:F // 2], 10.0)
    r2 = nt.mvdr_nulls_stream(fs, N, xs, pcm[:, h:], doa[F // 2:], 10.0, state=r1)
    one = nt.mvdr_nulls_stream(fs, N, xs, pcm, doa, 10.0)
    assert np.abs(np.concatenate([r1["out"], r2["out"]], axis=1) - one["out"]).max() <= 1e-12 * np.abs(one["out"]).max()


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_own_direction_is_distortionless(case, gain):
    xs, fs, N, doa = CASES[case]
    PL, _ = _loaded(fs, N, xs, 6)
    d = nt.steering(fs, N, xs, np.array(doa))
    w = nt.null_weights(PL, d, gain)
    resp = np.einsum("ksm,ksm->ks", np.conj(w), d)
    e = np.abs(resp - 1.0).max()
    print("%s gain %g: |w_s^H d_s - 1| <= %.2e" % (case, gain, e))
    assert e <= 1e-9


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_gram_route_equals_the_dense_definition(case, gain):
    xs, fs, N, doa = CASES[case]
    PL, x = _loaded(fs, N, xs, 6)
    d = nt.steering(fs, N, xs, np.array(doa))
    dense = np.einsum("ksm,km->ks", np.conj(nt.null_weights(PL, d, gain)), x)
    gram = nt.gram_route(PL, d, x, gain)
    e = np.abs(gram - dense).max() / np.abs(dense).max()
    print("%s gain %g: Gram route against the dense definition %.2e of the peak" % (case, gain, e))
    assert e <= 1e-9


@pytest.mark.parametrize("gain", GAINS)
def test_two_directions_closed_form_of_the_leak(gain):
    """|w_s^H d_r| = (|G_sr| / G_ss) / (1 + g (1 - |G_sr|^2 / (G_ss G_rr))) with G = D^H PhiL^-1 D"""
    xs, fs, N, doa = CASES["ula16_s2"]
    PL, _ = _loaded(fs, N, xs, 6)
    d = nt.steering(fs, N, xs, np.array(doa))
    w = nt.null_weights(PL, d, gain)
    G = np.einsum("ksm,kmr->ksr", np.conj(d), np.linalg.solve(PL, np.swapaxes(d, 1, 2)))
    for s, r in ((0, 1), (1, 0)):
        leak = np.abs(np.einsum("km,km->k", np.conj(w[:, s]), d[:, r]))
        gss, grr, gsr = np.real(G[:, s, s]), np.real(G[:, r, r]), np.abs(G[:, s, r])
        form = (gsr / gss) / (1.0 + gain * (1.0 - gsr ** 2 / (gss * grr)))
        assert np.abs(leak - form).max() <= 1e-9, (s, r)


def test_the_null_is_deep_and_changes_the_output():
    """the 16-microphone scene of tests/test_gpu_mvdr_sources.py, a fresh stream: at the sixth frame the covariance has not yet
    learnt the other talker; the gain puts the null there at once -- and moves the spectra by far more than the parity bar of the
    GPU tests, so a kernel that ignores the gain cannot pass them"""
    fs, N, F, S, gain = 48000, 256, 6, 2, 100.0
    xs = synth.ULA16
    pcm = nt.scene(xs, fs, N, F, 0).astype(np.float64)
    doa = nt.drifting_doa(1, F, S)[0].astype(np.float64)
    plain = nt.mvdr_nulls_stream(fs, N, xs, pcm, doa, 0.0, want_weights=True)
    nulls = nt.mvdr_nulls_stream(fs, N, xs, pcm, doa, gain, want_weights=True)
    d = nt.steering(fs, N, xs, doa[F - 1])
    leak = lambda r: np.median(np.abs(np.einsum("km,km->k", np.conj(r["w"][F - 1, 0]), d[:, 1])))
    print("median |w_0^H d_1| at frame %d: plain %.4f, null_gain %g: %.4f" % (F, leak(plain), gain, leak(nulls)))
    assert leak(nulls) < leak(plain) / 20.0
    for s in range(S):
        diff = np.abs(nulls["spec"][s] - plain["spec"][s]).max() / np.abs(plain["spec"][s]).max()
        print("source %d: spectra differ from plain MVDR's by %.2f of the peak" % (s, diff))
        assert diff > 0.1
    assert np.array_equal(nulls["phi"], plain["phi"])


def test_coincident_directions_in_the_twin():
    """two equal directions and nothing else: each output is the plain MVDR output (a virtual interferer along the own direction
    scales Phi_s^-1 d_s and leaves w_s).  Two equal directions beside a third: the pair's outputs are those of the call without
    the duplicate -- they null the third direction -- and not plain MVDR's."""
    fs, N, F, gain = 48000, 256, 8, 100.0
    xs = synth.ULA8
    pcm = nt.scene(xs, fs, N, F, 0).astype(np.float64)
    doa = nt.drifting_doa(1, F, 2)[0].astype(np.float64)
    plain = nt.mvdr_nulls_stream(fs, N, xs, pcm, doa, 0.0)["spec"]
    peak = np.abs(plain[0]).max()
    pair = nt.mvdr_nulls_stream(fs, N, xs, pcm, doa[:, [0, 0]], gain)["spec"]
    assert np.abs(pair[0] - plain[0]).max() <= 1e-9 * peak and np.abs(pair[1] - plain[0]).max() <= 1e-9 * peak
    two = nt.mvdr_nulls_stream(fs, N, xs, pcm, doa, gain)["spec"]
    three = nt.mvdr_nulls_stream(fs, N, xs, pcm, doa[:, [0, 1, 0]], gain)["spec"]
    assert np.abs(three[0] - two[0]).max() <= 1e-9 * peak and np.abs(three[2] - two[0]).max() <= 1e-9 * peak
    print("the equal pair of three against plain MVDR: %.2f of the peak" % (np.abs(three[0] - plain[0]).max() / peak))
    assert np.abs(three[0] - plain[0]).max() > 0.1 * peak
