"""CPU: the float64 twin of the Capon spatial spectrum (tests/mvdr_spectrum_twin.py) -- its two routes agree, the closed forms
hold, the peak rule does what include/mcarray_hip.h says, the spectrum finds the sources of the scenes the GPU tests use, and
every peak those tests compare stands clear of its neighbours and of the next-ranked peak by ten times their tolerance."""
import numpy as np
import pytest

from mcarray_amd import synth
from oracle import np_twin

import mvdr_spectrum_twin as st

GPU_TOL = 5e-4                 # tests/test_gpu_mvdr_spectrum.py
MARGIN = 10 * GPU_TOL

_phi = {}


def _named_phi(name):
    if name not in _phi:
        sc = st.named_scene(name)
        _phi[name] = (sc, np_twin.mvdr_stream(sc["fs"], sc["N"], sc["xs"], sc["pcm"].astype(np.float64), 0.0)["phi"])
    return _phi[name]


@pytest.mark.parametrize("weighting", [st.POWER, st.NORMALISED])
@pytest.mark.parametrize("name", sorted(st.NAMED))
def test_dense_and_cholesky_routes_agree(name, weighting):
    sc, phi = _named_phi(name)
    for band in [sc["band"], (0, sc["N"] // 2), (17, 17)]:
        a = st.spectrum(phi, sc["fs"], sc["N"], sc["xs"], sc["D"], band[0], band[1], weighting)
        b = st.cholesky_route(phi, sc["fs"], sc["N"], sc["xs"], sc["D"], band[0], band[1], weighting)
        assert np.abs(a - b).max() <= 1e-10 * a.max(), (name, band)


@pytest.mark.parametrize("M", [2, 5, 16])
def test_white_covariance_is_flat(M):
    N, K, D, loading = 256, 129, 61, 1e-3
    xs = np.sort(np.random.default_rng(M).uniform(0, 0.3, M))
    level = np.random.default_rng(1).uniform(1e-6, 10.0, K)
    phi = level[:, None, None] * np.eye(M)[None].astype(np.complex128)
    P = st.spectrum(phi, 16000, N, xs, D, 3, 40, st.NORMALISED, loading)
    assert np.allclose(P, 38 * (1 + loading) / M, rtol=1e-12, atol=0)
    Pp = st.spectrum(phi, 16000, N, xs, D, 3, 40, st.POWER, loading)
    assert np.allclose(Pp, level[3:41].sum() * (1 + loading) / M, rtol=1e-12, atol=0)
    # an exactly flat row: index 0 is its only local maximum (P[0] >= P[1]; no later sample exceeds its left neighbour)
    idx, doa, val = st.peaks(np.full(D, 0.25), 3)
    assert idx.tolist() == [0, -1, -1] and val.tolist() == [0.25, 0.0, 0.0]
    assert np.all(doa == np.float32(-np.pi / 2))


def test_zero_state_gives_the_zero_row():
    phi = np.zeros((129, 4, 4), dtype=np.complex128)
    for w in (st.POWER, st.NORMALISED):
        P = st.spectrum(phi, 16000, 256, synth.REEM_C, 61, 0, 128, w)
        assert np.all(P == 0.0)
        assert np.all(st.cholesky_route(phi, 16000, 256, synth.REEM_C, 61, 0, 128, w) == 0.0)
        idx, doa, val = st.peaks(P, 4)
        assert np.all(idx == -1) and np.all(doa == 0.0) and np.all(val == 0.0)
    # a band of silent bins beside live ones: the silent ones add nothing
    phi[10:20] = np.eye(4)
    a = st.spectrum(phi, 16000, 256, synth.REEM_C, 61, 0, 128, st.POWER)
    b = st.spectrum(phi, 16000, 256, synth.REEM_C, 61, 10, 19, st.POWER)
    assert np.array_equal(a, b) and a.min() > 0


def test_peak_rule_on_hand_made_rows():
    g = lambda D: st.grid(D).astype(np.float32)
    # ties go to the lower index
    idx, doa, val = st.peaks(np.array([0.0, 2.0, 1.0, 2.0, 0.0, 3.0, 1.0]), 4)
    assert idx.tolist() == [5, 1, 3, -1] and val.tolist() == [3.0, 2.0, 2.0, 0.0]
    assert doa.tolist() == [g(7)[5], g(7)[1], g(7)[3], g(7)[5]]          # the empty slot repeats slot 0
    # a plateau counts once, at its first sample; a plateau on a rising flank is a local maximum by the rule as well
    idx, _, _ = st.peaks(np.array([1.0, 2.0, 2.0, 1.0]), 2)
    assert idx.tolist() == [1, -1]
    idx, _, _ = st.peaks(np.array([1.0, 2.0, 2.0, 3.0]), 3)
    assert idx.tolist() == [3, 1, -1]
    # the ends: index 0 needs P[0] >= P[1], the last index P[D-1] > P[D-2]
    idx, _, _ = st.peaks(np.array([3.0, 1.0, 2.0]), 2)
    assert idx.tolist() == [0, 2]
    idx, _, _ = st.peaks(np.array([1.0, 1.0]), 2)
    assert idx.tolist() == [0, -1]
    # zeros are no maxima; fewer slots than maxima keeps the highest
    idx, doa, val = st.peaks(np.array([0.0, 0.0, 5.0, 0.0, 0.0, 6.0, 0.0, 4.0]), 2)
    assert idx.tolist() == [5, 2] and val.tolist() == [6.0, 5.0]
    idx, doa, val = st.peaks(np.zeros(9), 3)
    assert idx.tolist() == [-1, -1, -1] and doa.tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("weighting", [st.POWER, st.NORMALISED])
def test_ula16_two_sources_property(weighting):
    """sources at 20 and 32 degrees, D = 181 (1 degree), bins 1 ... 127: the two highest peaks lie on the grid points of the
    sources, the third peak is below 0.1 of the maximum"""
    sc, phi = _named_phi("ula16_20_32")
    P = st.spectrum(phi, sc["fs"], sc["N"], sc["xs"], 181, 1, 127, weighting)
    idx, doa, val = st.peaks(P, 3)
    print("weighting %d: peaks at %s, values %s of the maximum" % (weighting, idx.tolist(), (val / P.max()).tolist()))
    assert sorted(idx[:2].tolist()) == [90 + 20, 90 + 32]
    assert val[2] < 0.1 * P.max()


@pytest.mark.parametrize("name", sorted(st.NAMED))
def test_margins_of_the_peaks_the_gpu_tests_compare(name):
    sc, phi = _named_phi(name)
    P = st.spectrum(phi, sc["fs"], sc["N"], sc["xs"], sc["D"], sc["band"][0], sc["band"][1], sc["weighting"])
    idx, doa, val = st.peaks(P, sc["slots"] + 1)
    m = st.peak_margin(P, idx)
    print("%s: peaks %s values %s of the maximum, margin %.3g" % (name, idx.tolist(), (val / P.max()).tolist(), m))
    assert idx[0] >= 0 and m >= MARGIN, (name, m)


def test_margins_of_the_loop():
    pcm, res = st.loop_twin()
    for j, r in enumerate(res):
        m = st.peak_margin(r["P"], r["idx"])
        print("chunk %d: peaks %s, margin %.3g" % (j, r["idx"].tolist(), m))
        assert np.all(r["idx"][:2] >= 0) and m >= MARGIN, (j, m)
    # by the last chunk the loop has found the sources
    assert sorted(res[-1]["idx"][:2].tolist()) == [110, 122]
