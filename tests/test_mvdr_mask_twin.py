"""CPU: the float64 twin of the MVDR call with a covariance update weight per frame and bin (tests/mvdr_mask_twin.py) against the
per-frame twin, against the properties of the definition (include/mcarray_hip.h, mca_hip_mvdr_sources_frames_masked_*) and on the
scene whose target is sparse in time and frequency."""
import numpy as np
import pytest

from mcarray_amd import synth
from oracle import np_twin

import mvdr_gate_twin as gt
import mvdr_mask_twin as mt
import mvdr_nulls_twin as nt
import mvdr_postfilter_twin as pt

WEIGHTS = np.array([1, 1, .5, 0, 0, 1, .25, 0, 0, 0, 1, .75])


def _irregular(M):
    return np.sort(np.random.default_rng(M).uniform(0.0, 0.04 * M, M))


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("gain", [0.0, 10.0])
def test_a_per_frame_constant_mask_is_the_per_frame_twin(gain):
    fs, N, F, S = 16000, 256, 12, 3
    xs = synth.REEM_C
    K = N // 2 + 1
    pcm = nt.scene(xs, fs, N, F, 0).astype(np.float64)
    doa = nt.drifting_doa(1, F, S)[0].astype(np.float64)
    g = gt.mvdr_gate_stream(fs, N, xs, pcm, doa, gain, WEIGHTS)
    for form, u in (("[F][K]", np.repeat(WEIGHTS[:, None], K, axis=1)), ("[F][1]", WEIGHTS[:, None])):
        m = mt.mvdr_mask_stream(fs, N, xs, pcm, doa, gain, u)
        es, ea, ec = _rel(m["spec"], g["spec"]), _rel(m["out"], g["out"]), _rel(m["phi"], g["phi"])
        print("gain %g, mask %s against the per-frame twin: spectra %.1e audio %.1e covariance %.1e" % (gain, form, es, ea, ec))
        assert es <= 1e-12 and ea <= 1e-12 and ec <= 1e-12
    none, ones = mt.mvdr_mask_stream(fs, N, xs, pcm, doa, gain, None), gt.mvdr_gate_stream(fs, N, xs, pcm, doa, gain, None)
    assert _rel(none["spec"], ones["spec"]) <= 1e-12 and _rel(none["phi"], ones["phi"]) <= 1e-12
    # ... and the post-filter form is the post-filter twin
    p = pt.mvdr_postfilter_stream(fs, N, xs, pcm, doa, gain, WEIGHTS, **pt.PARITY_PF)
    q = mt.mvdr_mask_postfilter_stream(fs, N, xs, pcm, doa, gain, WEIGHTS[:, None], **pt.PARITY_PF)
    for key in ("spec", "out", "raw", "gain", "p", "A", "phi"):
        assert _rel(q[key], p[key]) <= 1e-12, key


def test_state_is_carried_across_calls():
    fs, N, F, S = 16000, 256, 12, 2
    xs = synth.REEM_C
    hop = N // 2
    pcm = nt.scene(xs, fs, N, F, 0).astype(np.float64)
    doa = nt.drifting_doa(1, F, S)[0].astype(np.float64)
    mask = mt.parity_mask()[0]
    for stream in (mt.mvdr_mask_stream, lambda *a, **k: mt.mvdr_mask_postfilter_stream(*a, **pt.PARITY_PF, **k)):
        one = stream(fs, N, xs, pcm, doa, 10.0, mask)
        r1 = stream(fs, N, xs, pcm[:, :(5 + 1) * hop], doa[:5], 10.0, mask[:5])
        r2 = stream(fs, N, xs, pcm[:, 5 * hop:], doa[5:], 10.0, mask[5:], state=r1)
        assert np.array_equal(np.concatenate([r1["spec"], r2["spec"]], axis=1), one["spec"])
        assert np.array_equal(np.concatenate([r1["out"], r2["out"]], axis=1), one["out"])
        assert np.array_equal(r2["phi"], one["phi"])


def test_exact_points():
    fs, N, F = 16000, 256, 6
    xs = synth.REEM_C
    hop, K = N // 2, N // 2 + 1
    pcm = nt.scene(xs, fs, N, F, 0).astype(np.float64)
    doa = nt.drifting_doa(1, F, 1)[0].astype(np.float64)
    lead = mt.mvdr_mask_stream(fs, N, xs, pcm[:, :(3 + 1) * hop], doa[:3], 0.0, None)
    rest = pcm[:, 3 * hop:]
    # the clamp: NaN, -3 and 7 behave as 0, 0 and 1, cell by cell
    odd = np.ones((3, K))
    odd[0, 5], odd[1, 9], odd[2, 11], odd[1, 20] = np.nan, -3.0, 7.0, 0.25
    ref = odd.copy()
    ref[0, 5], ref[1, 9], ref[2, 11] = 0.0, 0.0, 1.0
    a, b = mt.mvdr_mask_stream(fs, N, xs, rest, doa[3:], 0.0, odd, state=lead), mt.mvdr_mask_stream(fs, N, xs, rest, doa[3:], 0.0, ref, state=lead)
    assert np.array_equal(a["spec"], b["spec"]) and np.array_equal(a["phi"], b["phi"])
    # closed cells: a column of zeros leaves Phi[k] bit for bit and is still beamformed; the other bins of the frames update
    mask = np.ones((3, K))
    closed = np.arange(K) % 3 == 1
    mask[:, closed] = 0.0
    froz = mt.mvdr_mask_stream(fs, N, xs, rest, doa[3:], 0.0, mask, state=lead)
    assert np.array_equal(froz["phi"][closed], lead["phi"][closed])
    assert all(not np.array_equal(froz["phi"][k], lead["phi"][k]) for k in np.flatnonzero(~closed))
    assert np.abs(froz["spec"][0][:, closed]).min() > 0.0
    # a bin closed since the reset is the delay-and-sum while its neighbours are MVDR
    fresh = mt.mvdr_mask_stream(fs, N, xs, pcm, doa, 0.0, np.repeat((~closed).astype(float)[None], F, axis=0))
    d = np.stack([nt.steering(fs, N, xs, doa[t])[:, 0] for t in range(F)])            # [F][K][M]
    das = np.einsum("fkm,fmk->fk", np.conj(d), np_twin.stft_frames(pcm, N)) / len(xs)
    assert np.abs(fresh["spec"][0][:, closed] - das[:, closed]).max() <= 1e-12 * np.abs(das).max()
    assert np.abs(fresh["spec"][0][:, ~closed] - das[:, ~closed])[:, 2:-2].min() > 1e-6 * np.abs(das).max()
    assert not fresh["phi"][closed].any() and fresh["phi"][~closed].any(axis=(1, 2)).all()


def test_column_independence():
    """bin k of the spectra and of the covariance depends on column k of the mask alone"""
    fs, N, F, S = 16000, 256, 12, 2
    xs = _irregular(5)
    K = N // 2 + 1
    pcm = nt.scene(xs, fs, N, F, 1).astype(np.float64)
    doa = nt.drifting_doa(1, F, S)[0].astype(np.float64)
    m1 = mt.parity_mask()[0]
    for agree in (np.arange(K) % 2 == 0, np.arange(K) < 64):
        m2 = np.random.default_rng(3).choice(np.array([0, 1, .5], dtype=np.float32), size=m1.shape)
        m2[:, agree] = m1[:, agree]
        a, b = mt.mvdr_mask_stream(fs, N, xs, pcm, doa, 10.0, m1), mt.mvdr_mask_stream(fs, N, xs, pcm, doa, 10.0, m2)
        assert np.array_equal(a["spec"][:, :, agree], b["spec"][:, :, agree]) and np.array_equal(a["phi"][agree], b["phi"][agree])
        assert not np.array_equal(a["spec"][:, :, ~agree], b["spec"][:, :, ~agree])


@pytest.mark.parametrize("geo", ["four_irregular", "sixteen_irregular"])
def test_the_bin_index_matters(geo):
    """the scene and the mask of the GPU parity tests: the masked spectra and covariance are far from those of the all-ones run and of
    the per-frame run at the mask's mean over the bins, so a kernel that ignores the bin index cannot pass the 5e-4 / 5e-6 bars"""
    fs, N, F, S = 16000, 256, 12, 2
    xs = _irregular(4) if geo == "four_irregular" else _irregular(16)
    pcm = nt.scene(xs, fs, N, F, 0).astype(np.float64)
    doa = nt.drifting_doa(1, F, S)[0].astype(np.float64)
    mask = mt.parity_mask()[0]
    m = mt.mvdr_mask_stream(fs, N, xs, pcm, doa, 0.0, mask)
    for name, other in (("all ones", gt.mvdr_gate_stream(fs, N, xs, pcm, doa, 0.0, None)),
                        ("per-frame mean", gt.mvdr_gate_stream(fs, N, xs, pcm, doa, 0.0, gt.clamp(mask).mean(axis=1)))):
        ds = max(_rel(m["spec"][s], other["spec"][s]) for s in range(S))
        dc = _rel(m["phi"], other["phi"])
        print("%s: masked against %s: spectra %.2f covariance %.2f of the peak" % (geo, name, ds, dc))
        assert ds >= 0.1 and dc >= 0.1


def test_sparse_target_scene():
    """The scene of DESIGN.md 4.7 (8-microphone ULA, white interferer at -40 degrees, a target at +20 degrees gated by blocks of 4
    frames x 16 bins, look direction 24 degrees), figures over the last 24 of 48 frames, measured with this twin:

        covariance update rule                          target kept (of delay-and-sum)   interferer under delay-and-sum
        all ones                                        0.165                            6.19 dB
        per frame, only if every bin is target-free     1.000                            0.00 dB  (never learns)
        per frame, if more than half are target-free    0.343                            3.76 dB
        per bin                                         1.041                            9.48 dB

    41.8 % of the cells are open, no frame is fully open, none fully closed.  The bars sit under these figures by the margin a
    re-implementation of the resynthesis may need, not the kernel."""
    sc = mt.sparse_target_scene()
    m = sc["mask"]
    print("open cells %.1f %%, fully open frames %d, fully closed %d" % (100 * m.mean(), int(m.all(axis=1).sum()), int((~m.any(axis=1)).sum())))
    assert 0.35 <= m.mean() <= 0.5 and not m.all(axis=1).any() and m.any(axis=1).all()
    K = m.shape[1]
    doa = np.full(mt.SCENE_F, mt.SCENE_LOOK)
    pcm = sc["pcm"].astype(np.float64)
    fig = {}
    for name, u in (("ones", None), ("every", np.repeat(m.min(axis=1)[:, None], K, axis=1)),
                    ("half", np.repeat((m.mean(axis=1) > 0.5).astype(float)[:, None], K, axis=1)), ("mask", m)):
        r = mt.mvdr_mask_stream(mt.SCENE_FS, mt.SCENE_N, sc["xs"], pcm, doa, 0.0, u, want_weights=True)
        fig[name] = mt.scene_figures(r["w"][:, 0], sc)
        print("%-5s target kept %.3f of delay-and-sum, interferer %.2f dB under delay-and-sum" % ((name,) + fig[name]))
    assert fig["mask"][0] >= 0.8 and fig["mask"][1] >= 6.0
    assert fig["ones"][0] <= 0.3
    assert abs(fig["every"][1]) <= 0.1
    # no per-frame rule has both columns
    assert all(fig[n][0] < 0.8 or fig[n][1] < 6.0 for n in ("ones", "every", "half"))


def test_scene_from_the_mixture_alone():
    """what tests/test_gpu_mvdr_mask.py measures on the GPU, here on the twin (last 24 frames): output power in the open cells 12.84
    dB under the delay-and-sum's (all ones: 6.41), in the closed cells 0.866 of the delay-and-sum's (all ones: 0.095).  The bars of
    both files: 9 dB, 0.6, and 4 times the all-ones closed-cell power -- 3 dB and a factor 0.7 under the figures."""
    sc = mt.sparse_target_scene()
    f = mt.mixture_figures(lambda u: mt.mvdr_mask_stream(mt.SCENE_FS, mt.SCENE_N, sc["xs"], sc["pcm"].astype(np.float64),
                                                         np.full(mt.SCENE_F, mt.SCENE_LOOK), 0.0, u)["spec"][0], sc["mask"])
    print("open cells: masked %.2f dB under the delay-and-sum, all ones %.2f dB; closed cells: masked %.3f of it, all ones %.3f" % f)
    mt.assert_mixture_bars(f)
