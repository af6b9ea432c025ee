"""GPU parity for the stream API at frame lengths other than 1024 (kernels_generic.hip), through
the C ABI, against the CPU oracle.  The reference derives the frame length from the sample rate
(calculateOrderFromSampleRate): 8 kHz -> 256, 16 kHz -> 512, 96 kHz -> 2048, 192 kHz -> 4096.

Tolerances as in test_gpu_parity.py: DOA bins exact (flagged ties +-1), energy map
<= TOL_E * max|E|, audio <= 2e-5 * max|out| + 1e-7.
"""
import os

import numpy as np
import pytest

from mcarray_amd import api, synth
from oracle import pyoracle as po
from test_gpu_parity import TOL_E, _assert_bins

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("prec", [api.SRP_FP32, api.SRP_FP16X3])
@pytest.mark.parametrize("fs,N,step", [(8000, 256, 5.0), (16000, 512, 5.0), (96000, 2048, 0.5), (192000, 4096, 5.0)])
def test_stream_other_frame_lengths_ula8(fs, N, step, prec):
    xs, F, A = synth.ULA8, 24, 2
    pcm = np.stack([synth.noise_source_stream(xs, np.deg2rad(-50.0 + 75.0 * a), fs, (F + 1) * N // 2, 31 + a) for a in range(A)])
    ctx = api.Context(fs, xs, N, step, 1, srp_precision=prec, max_arrays=A)
    assert ctx.G == 7
    r = ctx.process_frames_host(pcm, want_energy=True)
    for a in range(A):
        o = po.ssl_stream(fs, N, xs, pcm[a].astype(np.float64), 1, step, want_map=True)
        _assert_bins(r["bin"][a], o["bin"], o["energy"], ctx.P, max_ties=2)
        assert np.abs(r["energy"][a] - o["energy"]).max() <= TOL_E[prec] * np.abs(o["energy"]).max()
        assert np.abs(r["out"][a] - o["out"]).max() <= 2e-5 * np.abs(o["out"]).max() + 1e-7
    ctx.close()


def test_other_frame_length_irregular_array_two_sources_and_state():
    # Reem-C (no delay-group merging), 2 sources, N = 512; then the same stream in two calls
    fs, N, F = 16000, 512, 30
    xs = synth.REEM_C
    pcm = synth.noise_source_stream(xs, np.deg2rad(35.0), fs, (F + 1) * N // 2, 12)
    ctx = api.Context(fs, xs, N, 5.0, 2)
    assert ctx.G == ctx.P == 6
    r = ctx.process_frames_host(pcm[None], want_energy=True)
    o = po.ssl_stream(fs, N, xs, pcm.astype(np.float64), 2, 5.0, want_map=True)
    _assert_bins(r["bin"][0], o["bin"], o["energy"], 6, max_ties=1)
    assert np.abs(r["energy"][0] - o["energy"]).max() <= 2e-5 * np.abs(o["energy"]).max()
    assert np.abs(r["out"][0] - o["out"]).max() <= 2e-5 * np.abs(o["out"]).max() + 1e-7
    ctx.close()
    ctx = api.Context(fs, xs, N, 5.0, 2)
    h, hop = 13, N // 2
    ra = ctx.process_frames_host(pcm[None, :, :(h + 1) * hop], want_energy=True)
    rb = ctx.process_frames_host(pcm[None, :, h * hop:], want_energy=True)
    assert np.array_equal(np.concatenate([ra["bin"], rb["bin"]], axis=1), r["bin"])
    np.testing.assert_allclose(np.concatenate([ra["energy"], rb["energy"]], axis=1), r["energy"], rtol=0, atol=1e-6 * np.abs(r["energy"]).max())
    np.testing.assert_allclose(np.concatenate([ra["out"], rb["out"]], axis=2), r["out"], rtol=0, atol=1e-6 * np.abs(r["out"]).max())
    ctx.close()


def test_other_frame_length_power_gate():
    # the gate's floor estimation counts fft_size samples per frame (BeamformingSeparationAndLocalisation.cpp:58-66):
    # 3 s at 16 kHz = 94 frames of 512 samples
    fs, N, F = 16000, 512, 200
    xs, hop = synth.ULA8, N // 2
    rng = np.random.default_rng(3)
    L = (F + 1) * hop
    src = synth.noise_source_stream(xs, np.deg2rad(20.0), fs, L, 21).astype(np.float64)
    env = np.zeros(L)
    for a, b in ((105, 125), (131, 140), (150, F - 1)):
        env[a * hop:b * hop] = 1.0
    pcm = (rng.standard_normal((len(xs), L)) * 0.001 + src * env).astype(np.float32)
    o = po.ssl_stream_gated(fs, N, xs, pcm.astype(np.float64), 1, 5.0, True)
    assert 0 < o["fired"].sum() < F and o["fired"][:94].sum() == 0
    ctx = api.Context(fs, xs, N, 5.0, 1, use_power_floor=True)
    r = ctx.process_frames_host(pcm[None], want_energy=True)
    assert np.array_equal(r["voiced"][0], o["fired"])
    np.testing.assert_allclose(r["power"][0][94:], o["power"][94:], rtol=0, atol=2e-3)          # dB
    np.testing.assert_allclose(r["power"][0][:93], o["power"][:93], rtol=2e-5)                  # running sum (linear)
    assert np.array_equal(r["bin"][0], o["bin"])
    assert np.abs(r["energy"][0] - o["energy"]).max() <= 2e-5 * np.abs(o["energy"]).max()
    assert np.abs(r["out"][0] - o["out"]).max() <= 2e-5 * np.abs(o["out"]).max() + 1e-7
    ctx.close()


IRR5 = [0.0, 0.028, 0.071, 0.102, 0.155]


@pytest.mark.parametrize("prec", [api.SRP_FP32, api.SRP_FP16X3, api.SRP_FP16])
@pytest.mark.parametrize("name,xs,S,step", [("ULA8", synth.ULA8, 1, 0.5), ("REEMC", synth.REEM_C, 2, 5.0), ("IRR5", IRR5, 1, 1.0), ("ULA3", [0.0, 0.05, 0.1], 1, 3.0),
                                             ("ULA16", synth.ULA16, 1, 1.0)])
def test_2048_sample_frames_on_the_wave_level_transform(name, xs, S, step, prec):
    """Round 6 (kernels_2048.hip): a 2048-sample frame is ONE 1024-point complex transform of (even, odd) samples per channel plus a split
    step -- k_stft_phat_2048 (3 ... 8 microphones: compile-time 8 / 4, run-time others; 16 keep the any-length analysis) and
    k_beamform_wave_2048 (any M).  The reference's own beamformer test runs this frame length (test/test_mcarray.cpp:660-662, fftOrder 11).
    Against the oracle in two calls (the overlap-add carries and the energy state), and against the any-length kernels
    (MCA_HIP_NO_N2048) on the same input."""
    fs, N, hop, F, cut, A = 96000, 2048, 1024, 45, 19, 2
    pcm = np.stack([sum(synth.noise_source_stream(xs, np.deg2rad(th + 31.0 * a), fs, (F + 1) * hop, 90 + 7 * a + i) for i, th in enumerate((-48.0, 22.0)[:S]))
                    for a in range(A)]).astype(np.float32)
    ctx = api.Context(fs, xs, N, step, S, srp_precision=prec, max_arrays=A)
    ra = ctx.process_frames_host(pcm[:, :, :(cut + 1) * hop], want_energy=True)
    rb = ctx.process_frames_host(pcm[:, :, cut * hop:], want_energy=True)
    r = {k: np.concatenate([ra[k], rb[k]], axis=2 if k == "out" else 1) for k in ("bin", "energy", "out")}
    tol_e = {api.SRP_FP32: 2e-5, api.SRP_FP16X3: 2e-5, api.SRP_FP16: 2e-4}[prec]
    from parity_helpers import assert_audio_where_bins_agree
    for a in range(A):
        o = po.ssl_stream(fs, N, xs, pcm[a].astype(np.float64), S, step, want_map=True)
        _assert_bins(r["bin"][a], o["bin"], o["energy"], ctx.P, max_ties=3)
        assert np.abs(r["energy"][a] - o["energy"]).max() <= tol_e * np.abs(o["energy"]).max()
        assert_audio_where_bins_agree(r["out"][a][:o["out"].shape[0]], o["out"], r["bin"][a], o["bin"], hop)
    ctx.close()
    os.environ["MCA_HIP_NO_N2048"] = "1"
    try:
        ctx = api.Context(fs, xs, N, step, S, srp_precision=prec, max_arrays=A)
    finally:
        del os.environ["MCA_HIP_NO_N2048"]
    g = ctx.process_frames_host(pcm, want_energy=True)
    ctx.close()
    assert np.mean(g["bin"] != r["bin"]) <= 0.02
    assert np.abs(g["energy"] - r["energy"]).max() <= (4e-6 if prec != api.SRP_FP16 else 2e-4) * np.abs(r["energy"]).max()


def test_2048_merged_rows_are_the_same_bits_every_run():
    """Round 6: the one-plane rows of an 8-microphone ULA at 2048-sample frames are stored on the merged index (k_stft_phat_2048<..., MERGE>):
    512 threads add their PHAT sums into one LDS region per frame with integer atomics (2^26 fixed point), so the result does not depend
    on the order the waves arrive in -- the energies of three runs over the same stream (fresh state each time) are bit-identical, and so
    are those of a second context."""
    fs, N, hop, F, A = 96000, 2048, 1024, 96, 4
    xs = synth.ULA8
    pcm = np.stack([synth.noise_source_stream(xs, np.deg2rad(-65.0 + 40.0 * a), fs, (F + 1) * hop, 400 + a, snr_db=12.0) for a in range(A)]).astype(np.float32)
    runs = []
    for rep in range(2):
        ctx = api.Context(fs, xs, N, 0.5, 1, srp_precision=api.SRP_FP16, max_arrays=A)
        for _ in range(3 if rep == 0 else 1):
            ctx.reset()
            r = ctx.process_frames_host(pcm, want_energy=True)
            runs.append((r["energy"].copy(), r["bin"].copy()))
        ctx.close()
    for e, b in runs[1:]:
        assert np.array_equal(e.view(np.uint32), runs[0][0].view(np.uint32)) and np.array_equal(b, runs[0][1])


def test_2048_sample_frames_power_gate():
    """the gate on the 2048-sample analysis (FFTPower from the spectra in LDS; 3 s at 96 kHz = 141 frames of 2048 samples)"""
    fs, N, F = 96000, 2048, 230
    xs, hop = synth.ULA8, N // 2
    rng = np.random.default_rng(4)
    L = (F + 1) * hop
    src = synth.noise_source_stream(xs, np.deg2rad(-33.0), fs, L, 23).astype(np.float64)
    env = np.zeros(L)
    for a, b in ((150, 170), (176, 181), (195, F - 1)):
        env[a * hop:b * hop] = 1.0
    pcm = (rng.standard_normal((len(xs), L)) * 0.001 + src * env).astype(np.float32)
    o = po.ssl_stream_gated(fs, N, xs, pcm.astype(np.float64), 1, 5.0, True)
    assert 0 < o["fired"].sum() < F and o["fired"][:141].sum() == 0
    ctx = api.Context(fs, xs, N, 5.0, 1, use_power_floor=True)
    r = ctx.process_frames_host(pcm[None], want_energy=True)
    assert np.array_equal(r["voiced"][0], o["fired"])
    np.testing.assert_allclose(r["power"][0][141:], o["power"][141:], rtol=0, atol=2e-3)          # dB
    assert np.array_equal(r["bin"][0], o["bin"])
    assert np.abs(r["energy"][0] - o["energy"]).max() <= 2e-5 * np.abs(o["energy"]).max()
    assert np.abs(r["out"][0] - o["out"]).max() <= 2e-5 * np.abs(o["out"]).max() + 1e-7
    ctx.close()


def test_2048_sample_frames_at_full_size_properties():
    """8 arrays x 2 048 frames of 2048 samples (the shape of profiles/r06_shapes.log; the oracle cannot reach it): size-independent
    properties of the path on the round-6 kernels -- (1) every array's DOA settles on its source; (2) one call and the same stream
    in two calls return the same bins (up to exact-level ties) and the same audio; (3) STFT -> delay-and-sum -> ISTFT is
    the identity for identical channels steered broadside (grid bin of 0 degrees: k_beamform_wave_2048 with its per-channel rows)."""
    torch = pytest.importorskip("torch")
    fs, N, hop, A, F = 96000, 2048, 1024, 8, 2048
    xs = synth.ULA8
    dev = torch.device("cuda:0")
    thetas = [-70.0 + 20.0 * a for a in range(A)]
    pcm = torch.from_numpy(np.stack([synth.noise_source_stream(xs, np.deg2rad(th), fs, (F + 1) * hop, 300 + a) for a, th in enumerate(thetas)]).astype(np.float32)).to(dev)
    ctx = api.Context(fs, xs, N, 0.5, 1, srp_precision=api.SRP_FP16X3, max_arrays=A)

    def run(x, Fc):
        b = torch.empty(A, Fc, 1, dtype=torch.int32, device=dev); r = torch.empty(A, Fc, 1, dtype=torch.float32, device=dev)
        q = torch.empty(A, Fc, 1, dtype=torch.float32, device=dev); o = torch.empty(A, 1, Fc * hop, dtype=torch.float32, device=dev)
        ctx.process_frames_dev(x.contiguous(), Fc, b, r, q, None, o)
        torch.cuda.synchronize()
        return b, r, o
    b, r, o = run(pcm, F)
    deg = np.rad2deg(r[:, 64:, 0].cpu().numpy())
    for a, th in enumerate(thetas):
        assert abs(np.median(deg[a]) - th) <= 0.75, (a, th, float(np.median(deg[a])))
    ctx.reset()
    cut = 777
    b1, _, o1 = run(pcm[:, :, :(cut + 1) * hop], cut)
    b2, _, o2 = run(pcm[:, :, cut * hop:], F - cut)
    # (the two-plane contraction of 6 216 rows and of 16 384 rows run on different tile kernels: a pick that is an exact-level tie may
    # resolve differently; the audio is compared on every hop whose steering is the same)
    diff = (torch.cat([b1, b2], dim=1) != b)[:, :, 0]
    assert int(diff.sum()) <= 4, int(diff.sum())
    same_hops = (~diff).repeat_interleave(hop, dim=1)
    same_hops[:, hop:] &= same_hops[:, :-hop].clone()
    o12 = torch.cat([o1, o2], dim=2)
    assert float((o12[:, 0][same_hops] - o[:, 0][same_hops]).abs().max()) <= 1e-6 * float(o.abs().max())
    # identity
    same = pcm[0:1, 0:1, :].expand(A, 8, (F + 1) * hop).contiguous()
    grid = ctx.doa_grid()
    b0 = int(np.argmin(np.abs(grid)))
    assert abs(grid[b0]) < 1e-6
    bins = torch.full((A, F, 1), b0, dtype=torch.int32, device=dev)
    rad = torch.zeros(A, F, 1, dtype=torch.float32, device=dev)
    oid = torch.empty(A, 1, F * hop, dtype=torch.float32, device=dev)
    ctx.reset()
    ctx.process_frames_dev(same, F, bins, rad, None, None, oid, localise=False, separate=True, bins_are_grid=True)
    torch.cuda.synchronize()
    assert torch.allclose(oid[3, 0, hop:], same[3, 0, hop:F * hop], rtol=0, atol=2e-6)
    ctx.close()


def test_any_length_kernels_agree_with_tuned_kernels_at_1024():
    # MCA_HIP_FORCE_GENERIC routes N = 1024 through kernels_generic.hip: same A layout, same contraction
    fs, N, F, A = 48000, 1024, 40, 2
    xs = synth.ULA8
    pcm = np.stack([synth.noise_source_stream(xs, np.deg2rad(-20.0 + 60 * a), fs, (F + 1) * N // 2, 70 + a) for a in range(A)])
    ctx = api.Context(fs, xs, N, 0.5, 1, srp_precision=api.SRP_FP32, max_arrays=A)
    r = ctx.process_frames_host(pcm, want_energy=True)
    ctx.close()
    os.environ["MCA_HIP_FORCE_GENERIC"] = "1"
    try:
        ctx = api.Context(fs, xs, N, 0.5, 1, srp_precision=api.SRP_FP32, max_arrays=A)
    finally:
        del os.environ["MCA_HIP_FORCE_GENERIC"]
    g = ctx.process_frames_host(pcm, want_energy=True)
    ctx.close()
    assert (g["bin"] != r["bin"]).sum() <= 1
    assert np.abs(g["energy"] - r["energy"]).max() <= 4e-6 * np.abs(r["energy"]).max()
    assert np.abs(g["out"] - r["out"]).max() <= 4e-6 * np.abs(r["out"]).max()


def check_gcc2_against_oracle(r, a, pcm, fs, xs, N, step=3.0):
    """array a of an ungated gcc2_frames_* result r (argmax, doa, corr) against the oracle on pcm [2][(F+1)*hop]: the smoothed
    correlation within 2e-5 of its peak, the pick exact or one tie the oracle itself holds within 1e-5, the DOA recursion"""
    F = r["argmax"].shape[1]
    og = po.FreqGCC(fs, xs, N + 2, False, step)
    X = po.stft_frames(pcm.astype(np.float64), N)
    nbad = 0
    for t in range(F):
        voiced, corr, idx, doa, power = og.process(X[t, 0], X[t, 1])
        if idx != r["argmax"][a, t]:
            assert abs(corr[idx] - corr[r["argmax"][a, t]]) < 1e-5 * np.abs(corr).max()
            nbad += 1
        assert np.abs(r["corr"][a, t] - corr).max() <= 2e-5 * np.abs(corr).max()
        assert abs(r["doa"][a, t] - doa) <= 2e-5 + 0.06 * nbad
    assert nbad <= 1


@pytest.mark.parametrize("fs,N,F", [(16000, 512, 90), (32000, 2048, 40), (48000, 4096, 21)])
def test_two_microphone_gcc_other_frame_lengths(fs, N, F):
    """512: the any-M tuned kernel; 2048 / 4096 (FreqGCC's 0.075 s frames at 32 / 48 kHz): 512-sample sub-sequences per channel"""
    pcm = synth.noise_source_stream(synth.BINAURAL, np.deg2rad(33.0), fs, (F + 1) * N // 2, 4)
    ctx = api.Context(fs, synth.BINAURAL, N, 3.0, 1)
    r = ctx.gcc2_frames_host(pcm[None], want_corr=True)
    check_gcc2_against_oracle(r, 0, pcm, fs, synth.BINAURAL, N)
    ctx.close()


def test_freqgcc_reference_test_configuration_44k1():
    """The configuration of the reference's own FreqGCC test (test/test_mcarray.cpp:276-301): 44.1 kHz, microphones 0.089 m
    apart, usePowerFloor = true, sources at -60 ... 60 degrees, mean reported DOA within 35 degrees.  0.075 s at 44.1 kHz
    gives 4096-sample frames (the any-length kernels); the recordings are not in the reference's tree, so the source is a
    far-field broadband one after 3 s of quiet for the floor estimation.  One angle is also compared frame by frame
    with the oracle."""
    fs, tol = 44100, 35.0
    xs = [0.0, 0.089]
    loc = None
    for doa_deg in (-60, -30, 0, 20, 60):
        loc = api.FreqGCCBinauralLocalisation(fs, xs, True)             # grid 3 degrees, N from the sample rate
        N = loc.ctx.N
        assert N == 4096 and loc.ctx.D == 61
        hop, F = N // 2, 70
        pcm = synth.noise_source_stream(xs, np.deg2rad(float(doa_deg)), fs, (F + 1) * hop, 100 + doa_deg)
        env = np.repeat(np.where(np.arange(F + 1) < 36, 0.01, 1.0), hop)
        pcm = (pcm * env[None, :]).astype(np.float32)
        got = []
        loc.set_callback(lambda deg, prob, power, n: got.append(float(deg[0])))
        r = loc.process(pcm, want_corr=True)
        assert len(got) == int(r["voiced"].sum()) and len(got) >= 25
        assert abs(np.mean(got) - doa_deg) <= tol, (doa_deg, np.mean(got))
        assert abs(np.mean(got[5:]) - doa_deg) <= 8.0, (doa_deg, np.mean(got[5:]))     # what this build actually achieves
        if doa_deg == 20:
            og = po.FreqGCC(fs, xs, N + 2, True, 3.0)
            X = po.stft_frames(pcm.astype(np.float64), N)
            nbad = 0
            for t in range(F):
                voiced, corr, idx, doa, power = og.process(X[t, 0], X[t, 1])
                assert bool(r["voiced"][0, t]) == voiced, t
                if not voiced:
                    continue
                if idx != r["argmax"][0, t]:
                    assert abs(corr[idx] - corr[r["argmax"][0, t]]) < 1e-5 * np.abs(corr).max()
                    nbad += 1
                assert np.abs(r["corr"][0, t] - corr).max() <= 2e-5 * np.abs(corr).max(), t
                assert abs(r["doa"][0, t] - doa) <= 2e-5 + 0.06 * nbad, t
            assert nbad <= 1
        loc.ctx.close()


MASK_MAX_CELLS, MASK_AUDIO_REL, MASK_AUDIO_ABS = 2, 2e-5, 1e-7      # decision cells that may differ per stream; audio of the peak + absolute


def check_masking_against_oracle(out, dec, pcm, fs, N, d, flo, fhi, method, alg):
    """one stream of FastBinauralMasking (out [2][F*hop], dec [F][45]) against the oracle on pcm [2][(F+1)*hop]: decisions exact
    except at most 2 cells, audio within 2e-5 of the peak + 1e-7 when the decisions agree"""
    F = dec.shape[0]
    o = po.Masking(fs, N, d, flo, fhi, method, alg)
    ol, orr = o.stream(pcm[0].astype(np.float64), pcm[1].astype(np.float64))
    o2 = po.Masking(fs, N, d, flo, fhi, method, alg)
    X = po.stft_frames(pcm.astype(np.float64), N)
    odec = np.array([o2.process(X[t, 0], X[t, 1])[2] for t in range(F)])
    ndiff = int((dec != odec).sum())
    assert ndiff <= MASK_MAX_CELLS, "decisions differ in %d (frame, band) cells" % ndiff
    ref = np.stack([ol, orr])
    if ndiff == 0:
        assert np.abs(out - ref).max() <= MASK_AUDIO_REL * np.abs(ref).max() + MASK_AUDIO_ABS
    return ndiff, odec, ref


def assert_masking_audio_where_decisions_agree(out, ref, dec, odec, hop):
    """the same audio bar on every hop whose own frame and the frame before it (a hop carries that one's second half) have the
    oracle's decisions in all bands (the pattern of parity_helpers.assert_audio_where_bins_agree); returns the hops compared"""
    agree = (dec == odec).all(axis=1)
    ok = agree.copy()
    ok[1:] &= agree[:-1]
    F = dec.shape[0]
    err = np.abs(out.astype(np.float64) - ref).reshape(2, F, hop).max(axis=(0, 2))
    assert err[ok].max() <= MASK_AUDIO_REL * np.abs(ref).max() + MASK_AUDIO_ABS, (int(np.argmax(np.where(ok, err, 0))), err[ok].max())
    return int(ok.sum())


@pytest.mark.parametrize("fs,N", [(48000, 2048), (44100, 2048), (8000, 512), (96000, 4096)])
@pytest.mark.parametrize("method,alg", [(api.RELATIVE, api.BOTH), (api.FULL, api.BOTH), (api.FACTOR, api.TEMPORAL), (api.NOISY, api.SPATIAL)])
def test_masking_stream_other_frame_lengths(fs, N, method, alg):
    """FastBinauralMasking takes N = 2^round(log2(0.050 fs)) (FastBinauralMasking.h:112): 2048 at 44.1 / 48 kHz, 512 at 8 kHz.
    Any-length stream kernel against the oracle; long enough to cross its runs (warm-up of the Q recursion, overlap-add
    carry) and split over two calls.  Decisions exact except cells the oracle itself puts within 1e-4 of a threshold."""
    assert N == 1 << api.calculate_order_from_sample_rate(fs, 0.050)
    hop, F, d = N // 2, 70, 0.086
    rng = np.random.default_rng(N + method)
    n = (F + 1) * hop
    src = rng.standard_normal(n) * 0.1
    left = src + rng.standard_normal(n) * 0.003
    right = np.roll(src, 1) * 0.9 + rng.standard_normal(n) * 0.003
    env = np.repeat(rng.choice([1.0, 0.2, 0.05, 0.6], F + 1), hop)                    # level steps exercise the temporal mask
    pcm = np.stack([left * env, right * env]).astype(np.float32)
    flo, fhi = 300.0, min(5000.0, 0.45 * fs)
    m = api.FastBinauralMasking(fs, d, flo, fhi, method, alg, fft_size=N)
    h = 33
    oa, da = m.process(pcm[:, :(h + 1) * hop])
    ob, db = m.process(pcm[:, h * hop:])
    out = np.concatenate([oa[0], ob[0]], axis=1)
    dec = np.concatenate([da[0], db[0]], axis=0)
    check_masking_against_oracle(out, dec, pcm, fs, N, d, flo, fhi, method, alg)
    m.close()


def test_sixteen_microphones_2048_sample_frames_several_sources_in_passes():
    """M + S spectra of 1 025 bins do not fit the 160 KiB of a CU for S >= 3: the any-length beamformer then takes the sources
    two at a time (the shapes the round-4 fuzz runs listed as refused).  Bins, energies and every source's audio against the
    oracle; then the same stream in two calls (the per-source overlap-add carries go through the passes too)."""
    fs, N, F, S = 96000, 2048, 14, 3
    xs = synth.ULA16
    pcm = sum(synth.noise_source_stream(xs, np.deg2rad(th), fs, (F + 1) * N // 2, 50 + i) for i, th in enumerate((-48.0, 7.0, 52.0)))
    ctx = api.Context(fs, xs, N, 5.0, S)
    r = ctx.process_frames_host(pcm[None], want_energy=True)
    o = po.ssl_stream(fs, N, xs, pcm.astype(np.float64), S, 5.0, want_map=True)
    _assert_bins(r["bin"][0], o["bin"], o["energy"], ctx.P, max_ties=2)
    assert np.abs(r["energy"][0] - o["energy"]).max() <= 2e-5 * np.abs(o["energy"]).max()
    if np.array_equal(r["bin"][0], o["bin"]):
        assert np.abs(r["out"][0] - o["out"]).max() <= 2e-5 * np.abs(o["out"]).max() + 1e-7
    ctx.close()
    ctx = api.Context(fs, xs, N, 5.0, S)
    h, hop = 6, N // 2
    ra = ctx.process_frames_host(pcm[None, :, :(h + 1) * hop]); rb = ctx.process_frames_host(pcm[None, :, h * hop:])
    assert np.array_equal(np.concatenate([ra["bin"], rb["bin"]], axis=1), r["bin"])
    np.testing.assert_allclose(np.concatenate([ra["out"], rb["out"]], axis=2), r["out"], rtol=0, atol=1e-6 * np.abs(r["out"]).max())
    ctx.close()


def test_unsupported_stream_sizes_say_why():
    ctx = api.Context(48000, synth.ULA8, 1000, 5.0, 1)             # even but not a power of two: frame API only
    with pytest.raises(api.MCArrayHipError, match="power-of-two"):
        ctx.process_frames_host(np.zeros((1, 8, 3 * 500), np.float32))
    ctx.close()
    ctx = api.Context(48000, synth.ULA16, 4096, 5.0, 1)            # 16 spectra of 2049 bins exceed the LDS
    with pytest.raises(api.MCArrayHipError, match="LDS"):
        ctx.process_frames_host(np.zeros((1, 16, 3 * 2048), np.float32))
    ctx.close()
