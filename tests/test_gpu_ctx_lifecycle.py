"""GPU: the life of the workspaces of the main context (mca_hip_ctx) and of the multiband, temporal-GCC, mask and bmask contexts.

A buffer's capacity enters no arithmetic.  A context that grows its workspaces call by call must therefore return, call for call,
the bytes of a twin that had the largest shape before its first call (mca_hip_reserve where it covers the path, else one throw-away
call of the largest shape and a state restore), and leave the same state blob.  Every comparison is on bytes (torch.equal /
np.array_equal / bytes ==).

Shapes: 2 arrays of max_arrays = 3 (a size taken from max_arrays where n_arrays was meant shows), calls of 64, 160, 64 and 160 frames
(64 = 2 x SCAN_CHUNK is the shortest call the adaptive path takes), MCA_HIP_ADAPT_MIN_ROWS at 64 so that these small batches run
coarse + repair.  The adaptive cases pin the mode (adaptive_fallback OFF, candidate columns wherever a lazy call allows): what a
call does then depends on the calls before it and their content only, never on when a report of the back-off policy lands, and the
two contexts of a pair take the same path.

The double frame API takes one frame length only (ccs_len == fft_size + 2 is checked), so its two workspaces grow once, from
nothing: that case compares a context whose buffers exist already (a throw-away round and a reset) with a fresh one."""
import numpy as np
import pytest

from mcarray_amd import api, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

A_MAX, A = 3, 2
CALLS = (64, 160, 64, 160)
F_MAX = max(CALLS)
XS4 = [0.05 * m for m in range(4)]


@pytest.fixture
def pinned_adaptive(monkeypatch):
    monkeypatch.setenv("MCA_HIP_ADAPT_MIN_ROWS", "64")          # read by mca_hip_create
    monkeypatch.setenv("MCA_HIP_ADAPT_CAND", "1")
    monkeypatch.delenv("MCA_HIP_ADAPT_FALLBACK", raising=False)


def _pcm(xs, fs, hop, quiet_frames=0):
    total = sum(CALLS)
    pcm = np.stack([synth.noise_source_stream(xs, np.deg2rad(-35.0 + 50 * a), fs, (total + 1) * hop, 4100 + a, snr_db=12.0) for a in range(A)])
    pcm[:, :, :quiet_frames * hop] *= 1e-3                      # a quiet lead-in: the power floor is estimated on it
    return pcm.astype(np.float32)


def _stream(ctx, pcm, hop, energy=True):
    """the four calls through process_frames_dev -> per call the tuple of result tensors"""
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    got, t0 = [], 0
    for F in CALLS:
        chunk = torch.from_numpy(pcm[:, :, t0 * hop:(t0 + F + 1) * hop].copy()).to(dev)
        r = dict(bin=torch.zeros((A, F, ctx.S), dtype=torch.int32, device=dev), rad=torch.zeros((A, F, ctx.S), device=dev),
                 prob=torch.zeros((A, F, ctx.S), device=dev), out=torch.zeros((A, ctx.S, F * hop), device=dev))
        r["energy"] = torch.zeros((A, F, ctx.D), device=dev) if energy else None
        ctx.process_frames_dev(chunk, F, r["bin"], r["rad"], r["prob"], r["energy"], r["out"], stream=st)
        torch.cuda.synchronize()
        got.append(r)
        t0 += F
    return got


def _same_calls(grown, twin, what):
    assert len(grown) == len(twin)
    for i, (g, t) in enumerate(zip(grown, twin)):
        for key in g:
            if g[key] is not None:
                assert torch.equal(g[key], t[key]), (what, "call %d" % i, key)


STREAM_CASES = {
    # (a) the steered path, lazy tails, candidate columns: d_steer_Y, d_steer_mlist and every adaptive list
    "ULA8 adaptive": dict(xs=synth.ULA8, prec=api.SRP_ADAPTIVE, floor=False, n_arrays_max=A_MAX),
    # (b) + the power gate: the gate buffers, eager tails
    "ULA8 adaptive, gated": dict(xs=synth.ULA8, prec=api.SRP_ADAPTIVE, floor=True, n_arrays_max=A_MAX),
    # (c) 16 microphones: the unsure frames
    "ULA16 adaptive": dict(xs=synth.ULA16, prec=api.SRP_ADAPTIVE, floor=False, n_arrays_max=A_MAX),
    # (d) the one- and the two-plane A rows without the adaptive lists
    "4 microphones FP32": dict(xs=XS4, prec=api.SRP_FP32, floor=False, n_arrays_max=A_MAX),
    "4 microphones FP16X3": dict(xs=XS4, prec=api.SRP_FP16X3, floor=False, n_arrays_max=A_MAX),
}


@pytest.mark.parametrize("name", list(STREAM_CASES))
def test_stream_calls_of_a_growing_context_equal_a_reserved_twin(pinned_adaptive, name):
    """cases (a) to (d): small, large, small, large through mca_hip_process_frames_dev; the twin reserved the large shape first"""
    case = STREAM_CASES[name]
    fs, N = 48000, 1024
    hop = N // 2
    pcm = _pcm(case["xs"], fs, hop, quiet_frames=290 if case["floor"] else 0)      # (3 s of floor estimation = 282 frames: known in the last call)
    new = lambda: api.Context(fs, case["xs"], N, 0.5, 1, use_power_floor=case["floor"], srp_precision=case["prec"],
                              max_arrays=case["n_arrays_max"], adaptive_fallback=False)
    grown, twin = new(), new()
    try:
        twin.reserve(A, F_MAX)
        rg, rt = _stream(grown, pcm, hop), _stream(twin, pcm, hop)
        _same_calls(rg, rt, name)
        assert rg[-1]["bin"].max().item() >= 0 and rg[-1]["out"].abs().max().item() > 0.0      # not a comparison of nothing
        if case["prec"] == api.SRP_ADAPTIVE:
            sg, st = grown.repair_stats(), twin.repair_stats()
            assert sg == st and sg["frames"] == A * sum(CALLS), (sg, st)                       # every call ran coarse + repair
        if name == "ULA8 adaptive":
            assert grown.steer_stats() == twin.steer_stats() and grown.steer_stats()["frames"] == A * sum(CALLS)      # ... and steered on the half spectrum
        assert grown.state_save() == twin.state_save(), name
    finally:
        grown.close()
        twin.close()


def test_create_run_destroy_three_times_over(pinned_adaptive):
    """create / two calls / destroy, three times: every round returns the bytes and the state blob of the first"""
    fs, N = 48000, 1024
    hop = N // 2
    pcm = _pcm(synth.ULA8, fs, hop)
    first = None
    for n in range(3):
        ctx = api.Context(fs, synth.ULA8, N, 0.5, 1, srp_precision=api.SRP_ADAPTIVE, max_arrays=A_MAX, adaptive_fallback=False)
        try:
            r = _stream(ctx, pcm, hop)[:2]
            blob = ctx.state_save()
        finally:
            ctx.close()
        if first is None:
            first = (r, blob)
        _same_calls(first[0], r, "round %d" % n)
        assert first[1] == blob, n


def test_gated_two_microphone_tracked_calls_of_a_growing_context():
    """case (e): the gated 2-microphone GCC path with a tracker; the larger calls pass no row / argmax outputs, so the context's own
    (d_trk_corr, d_trk_idx) grow beside d_g2_*.  The twin took a throw-away call of the large shape; its state was restored."""
    fs, N = 16000, 1024
    hop = N // 2
    dev = torch.device("cuda:0")
    pcm = _pcm(synth.BINAURAL, fs, hop, quiet_frames=100)       # (3 s of floor estimation = 94 frames)

    def new():
        ctx = api.Context(fs, synth.BINAURAL, N, 3.0, 1, True, max_arrays=A_MAX)
        ctx.gcc2_tracker_attach(seed=0x5EED0001)
        return ctx

    def run(ctx):
        got, t0 = [], 0
        for F in CALLS:
            chunk = torch.from_numpy(pcm[:, :, t0 * hop:(t0 + F + 1) * hop].copy()).to(dev)
            r = dict(doa=torch.zeros((A, F), device=dev), prob=torch.zeros((A, F), device=dev),
                     fired=torch.zeros((A, F), dtype=torch.uint8, device=dev), track=torch.zeros((A, F), dtype=torch.int32, device=dev))
            if F != F_MAX:
                r["argmax"] = torch.zeros((A, F), dtype=torch.int32, device=dev)
                r["corr"] = torch.zeros((A, F, ctx.D), device=dev)
            ctx.gcc2_tracked_frames_dev(chunk, F, r["doa"], r.get("argmax"), r["prob"], r["fired"], r["track"], r.get("corr"))
            torch.cuda.synchronize()
            got.append(r)
            t0 += F
        return got

    grown, twin = new(), new()
    try:
        blob = twin.state_save()
        big = torch.from_numpy(pcm[:, :, :(F_MAX + 1) * hop].copy()).to(dev)
        twin.gcc2_tracked_frames_dev(big, F_MAX, torch.zeros((A, F_MAX), device=dev))
        torch.cuda.synchronize()
        twin.state_load(blob)
        rg, rt = run(grown), run(twin)
        _same_calls(rg, rt, "tracked gcc2")
        assert rg[-1]["fired"].any().item()
        assert grown.state_save() == twin.state_save()
    finally:
        grown.close()
        twin.close()


def test_double_frame_api_on_fresh_and_on_existing_workspaces():
    """case (f): steering_process_frame / beamformer_process_frame, frame by frame"""
    fs, N, n = 16000, 256, 4
    xs = XS4
    rng = np.random.default_rng(77)
    frames = rng.standard_normal((n, len(xs), N + 2))
    frames[:, :, 1] = 0.0
    frames[:, :, N + 1] = 0.0                                    # CCS: DC and Nyquist are real

    def run(ctx):
        got = []
        for f in frames:
            doa, prob, bins = ctx.steering_process_frame(f)
            got += [doa, prob, bins, ctx.beamformer_process_frame(f, float(doa[0])), ctx.energy()]
        return got

    fresh, used = api.Context(fs, xs, N, 5.0, 1), api.Context(fs, xs, N, 5.0, 1)
    try:
        run(used)
        used.reset()
        for i, (x, y) in enumerate(zip(run(fresh), run(used))):
            assert np.array_equal(x, y), i
        assert fresh.state_save() == used.state_save()
    finally:
        fresh.close()
        used.close()


def _module_twins(new, run, sizes):
    """small, large, small on a fresh module context against a twin that took the large call first and was reset"""
    grown, twin = new(), new()
    try:
        run(twin, max(sizes))
        twin.reset()
        for i, F in enumerate(sizes):
            rg, rt = run(grown, F), run(twin, F)
            for j, (x, y) in enumerate(zip(rg, rt)):
                assert np.array_equal(x, y), (i, j)
            assert all(np.asarray(x).any() for x in rg), i               # (every output is written)
        assert grown.state_save() == twin.state_save()
    finally:
        grown.close()
        twin.close()


MODULE_FRAMES = (6, 40, 6)


def _two_channel_noise(n_samples, seed, fs=16000):
    return np.stack([synth.noise_source_stream(synth.BINAURAL, np.deg2rad(20.0 - 45 * a), fs, n_samples, seed + a) for a in range(A)]).astype(np.float32)


def test_multiband_workspaces():
    fs = 16000
    new = lambda: api.MultibandBinarualLocalisation(fs, synth.BINAURAL, nbins=5, use_power_floor=False, max_arrays=A_MAX)
    probe = new()
    hop = probe.hop
    probe.close()
    pcm = _two_channel_noise((max(MODULE_FRAMES) + 1) * hop, 300)

    def run(m, F):
        r = m.process(pcm[:, :, :(F + 1) * hop], want_bands=True)
        return [r[k] for k in ("doa", "prob", "voiced", "power", "band_idx", "energy_in_doa", "band_corr")]
    _module_twins(new, run, MODULE_FRAMES)


def test_temporal_gcc_workspaces():
    fs = 16000
    new = lambda: api.TemporalGCCBinauralLocalisation(fs, synth.BINAURAL, use_power_floor=False, max_arrays=A_MAX)
    probe = new()
    W, hop = probe.W, probe.hop
    probe.close()
    pcm = _two_channel_noise((max(MODULE_FRAMES) - 1) * hop + W, 310)

    def run(m, F):
        r = m.process(pcm[:, :, :(F - 1) * hop + W], want_index=True)
        return [r[k] for k in ("doa", "prob", "voiced", "power", "delay_idx", "index")]
    _module_twins(new, run, MODULE_FRAMES)


def test_mask_workspaces():
    fs, N = 16000, 512
    new = lambda: api.FastBinauralMasking(fs, 0.086, 100.0, 7000.0, fft_size=N, max_streams=A_MAX)
    pcm = _two_channel_noise((max(MODULE_FRAMES) + 1) * (N // 2), 320)
    _module_twins(new, lambda m, F: list(m.process(pcm[:, :, :(F + 1) * (N // 2)])), MODULE_FRAMES)


def test_bmask_workspaces():
    fs = 16000
    new = lambda: api.BinauralMaskingImpl(fs, 0.086, 100.0, 7000.0, max_streams=A_MAX)
    probe = new()
    hop = probe.hop
    probe.close()
    pcm = _two_channel_noise((max(MODULE_FRAMES) + 1) * hop, 330)
    _module_twins(new, lambda m, F: list(m.process(pcm[:, :, :(F + 1) * hop])), MODULE_FRAMES)
