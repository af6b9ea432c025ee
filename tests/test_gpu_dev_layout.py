"""GPU: the device-pointer ABI under a layout the header allows and no other test uses.

Every *_frames_dev entry point promises "sample n of channel c of array a at pcm[a*array_stride + c*ch_stride + n], 8-byte
aligned, even strides".  Each case here drives two fresh contexts of one configuration with the same samples:

  X  the contiguous call the module's own tests use (the host wrapper: a fresh, 512-byte aligned, densely packed upload);
  Y  the device call on tests/dev_layout_helpers.strided_pcm: rows 6 floats further apart than they are long (a pitch of
     2 mod 4: every other row is 8-byte aligned only), arrays another 10 floats apart, the first sample 2 floats into a
     NaN-filled allocation; every output carved out of a buffer with guard margins; enqueued on a non-default stream.

Both make two consecutive calls (13 + 8 frames, no multiple of any block size; Y without a synchronisation in between), so the
carried state is under the layout too.  3 arrays, so that a = 2 exists: a kernel that formed `a * M * mic_stride` would read
poison.  Asserted: Y's outputs are X's bit for bit (the launch shapes depend on the counts only), no NaN anywhere (an over-read
of a row lands in NaN), the guards are intact (an over-write lands in them), and X agrees with the module's reference under the
module's own bar, imported from its test file.

Where the device call and the host call of a configuration take different routes on purpose, the bit partner of Y is the
contiguous DEVICE call of a third context, and Y itself goes against the reference (said at the case)."""
import ctypes as C

import numpy as np
import pytest

from mcarray_amd import api, synth
from oracle import pyoracle as po

import dev_layout_helpers as dl
from parity_helpers import assert_audio_where_bins_agree

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

A, F1, F2 = 3, 13, 8
F = F1 + F2
INVALID = -1          # MCA_HIP_ERR_INVALID_ARGUMENT (include/mcarray_hip.h)


# ---------------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------------
def _cuts(hop, tail=None):
    """sample ranges of the two calls: frames [0, F1) and [F1, F)"""
    tail = hop if tail is None else tail
    return [(0, (F1 - 1) * hop + hop + tail, F1), (F1 * hop, (F - 1) * hop + hop + tail, F2)]


def _views(pcm, hop, tail=None):
    """one poisoned allocation per call (so that the row of the first call ends in NaN as well, not in the second call's samples)"""
    return [dl.strided_pcm(pcm[:, :, s0:s1]) + (n,) for (s0, s1, n) in _cuts(hop, tail)]


def _guards(spec):
    return {k: dl.guarded(shape, dtype) for k, (shape, dtype) in spec.items()}


def _collect(calls, what):
    """after the synchronisation: guards, NaN, and the numpy form of every output of every call, concatenated along the frames"""
    res = []
    for i, g in enumerate(calls):
        r = {}
        for k, gd in g.items():
            gd.assert_guards_intact("%s call %d output %s" % (what, i, k))
            r[k] = gd.t.cpu().numpy()
            if r[k].dtype.kind == "f":
                assert np.isfinite(r[k]).all(), "%s call %d: %d non-finite values in %s" % (what, i, int((~np.isfinite(r[k])).sum()), k)
        res.append(r)
    return res


def _assert_same_bits(got, want, what):
    bad = []
    for k in got:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if g.tobytes() != w.tobytes():
            d = np.argwhere((g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8)).reshape(g.shape + (g.itemsize,)).any(axis=-1))
            bad.append("%s: %d of %d values differ, the first at %s (%r against %r)" % (k, len(d), g.size, d[0].tolist(), g[tuple(d[0])], w[tuple(d[0])]))
    assert not bad, "%s: the strided device call differs from the contiguous call -- %s" % (what, "; ".join(bad))


def _stream():
    torch.cuda.synchronize()          # the buffers above were filled on the default stream
    return torch.cuda.Stream()


# ---------------------------------------------------------------------------------------------------------------------------
# the main context
# ---------------------------------------------------------------------------------------------------------------------------
from test_gpu_parity import TOL_E, _assert_bins                    # noqa: E402  (the project's bars)

E_TOL = dict(TOL_E)
E_TOL[api.SRP_ADAPTIVE] = TOL_E[api.SRP_FP16]      # fp16-level map on the frames the repair leaves alone (tests/test_gpu_adaptive.py)


def _main_spec(ctx, n, energy=True):
    hop = ctx.hop
    s = dict(bin=((A, n, ctx.S), torch.int32), doa=((A, n, ctx.S), torch.float32), prob=((A, n, ctx.S), torch.float32),
             out=((A, ctx.S, n * hop), torch.float32))
    if energy:
        s["energy"] = ((A, n, ctx.D), torch.float32)
    return s


def _main_dev(ctx, views, graph=False):
    """the two calls on `views` [(view, whole, n_frames)], every output guarded, on a side stream, nothing in between"""
    calls = [_guards(_main_spec(ctx, n)) for (_, _, n) in views]
    st = _stream()
    for (v, _, n), g in zip(views, calls):
        ctx.process_frames_dev(v, n, g["bin"].t, g["doa"].t, g["prob"].t, g["energy"].t, g["out"].t, stream=st.cuda_stream)
    st.synchronize()
    torch.cuda.synchronize()
    return calls


def _cat(parts, keys=("bin", "doa", "prob", "energy", "out")):
    return {k: np.concatenate([p[k] for p in parts], axis=2 if k == "out" else 1) for k in keys if k in parts[0] and parts[0][k] is not None}


def _main_against_oracle(r, pcm, fs, N, xs, S, step, prec, P, max_ties=3):
    hop = N // 2
    for a in range(A):
        o = po.ssl_stream(fs, N, xs, pcm[a].astype(np.float64), S, step, want_map=True)
        _assert_bins(r["bin"][a], o["bin"], o["energy"], P, max_ties=max_ties)
        assert np.abs(r["energy"][a] - o["energy"]).max() <= E_TOL[prec] * np.abs(o["energy"]).max(), a
        assert_audio_where_bins_agree(r["out"][a][:o["out"].shape[0]], o["out"], r["bin"][a], o["bin"], hop)


def _scene(xs, fs, N, S, seed, frames=F):
    hop = N // 2
    return np.stack([sum(synth.noise_source_stream(xs, np.deg2rad(th + 29.0 * a), fs, (frames + 1) * hop, seed + 7 * a + i)
                         for i, th in enumerate((-48.0, 22.0)[:S])) for a in range(A)]).astype(np.float32)


IRR5 = [0.0, 0.028, 0.071, 0.102, 0.155]
MAIN_CASES = [
    # id, microphones, fs, N, step, S, precision, groups G expected, the route
    ("ula8_fp32", synth.ULA8, 48000, 1024, 0.5, 1, "FP32", 7),           # k_stft_phat<8, merged>, k_beamform_wave
    ("ula16", synth.ULA16, 48000, 1024, 1.0, 1, "FP32", 15),             # the 16-channel template
    ("irr5_s2", IRR5, 48000, 1024, 1.0, 2, "FP32", 10),                  # run-time M, un-merged, odd pair rows, two sources
    ("reemc", synth.REEM_C, 48000, 1024, 5.0, 1, "FP32", 6),             # 4 microphones, G == P
    ("reemc_512_s2", synth.REEM_C, 16000, 512, 5.0, 2, "FP32", 6),       # k_stft_phat_512 / the 512 transforms
    ("ula8_2048", synth.ULA8, 96000, 2048, 0.5, 1, "FP32", 7),           # kernels_2048.hip
    ("ula8_256", synth.ULA8, 8000, 256, 5.0, 1, "FP32", 7),              # kernels_generic.hip (any length)
]


@pytest.mark.parametrize("name,xs,fs,N,step,S,prec,G", MAIN_CASES, ids=[c[0] for c in MAIN_CASES])
def test_main_context_strided_equals_contiguous(name, xs, fs, N, step, S, prec, G):
    """mca_hip_process_frames_dev against mca_hip_process_frames_host in FP32: both run the localiser, then the delay-and-sum
    at the localiser's grid bins (the host wrapper calls the same two stages on its staging copy), so every output is the same
    bits.  ctx.G pins the analysis variant (merged ULA rows: G = M - 1; irregular arrays: G == P)."""
    prec = getattr(api, "SRP_" + prec)
    hop = N // 2
    pcm = _scene(xs, fs, N, S, 700)
    mk = lambda: api.Context(fs, xs, N, step, S, srp_precision=prec, max_arrays=A)
    X, Y = mk(), mk()
    assert X.G == G and (G == X.P) == (name in ("irr5_s2", "reemc", "reemc_512_s2"))
    xr = [X.process_frames_host(pcm[:, :, s0:s1], want_energy=True) for (s0, s1, _) in _cuts(hop)]
    yr = _collect(_main_dev(Y, _views(pcm, hop)), name)
    for i in range(2):
        _assert_same_bits(yr[i], {k: xr[i][k] for k in yr[i]}, "%s call %d" % (name, i))
    _main_against_oracle(_cat(xr), pcm, fs, N, xs, S, step, prec, X.P)
    X.close(); Y.close()


def test_main_context_adaptive_strided_equals_contiguous_device_call():
    """The 8-microphone ULA at 1024 samples in ADAPTIVE: the flagship route.  Its DEVICE call differs from the host call on
    purpose -- it steers the delay-and-sum on the half spectrum at the predicted bin (k_steer_*; tests/test_gpu_steer.py) and
    keeps the last 16 frames of PCM as history instead of repairing its last rows (lazy tails) -- so the bit partner of the
    strided call is the contiguous device call of a third context, and the strided call itself goes against the oracle under
    the adaptive bar (bins up to oracle-fragile frames, fp16-level energies, audio where the bins agree).  A call runs coarse +
    repair from 64 frames on (two scan chunks), so this case alone is longer: 77 + 67 frames, with adaptive_min_rows = 16 and the
    back-off off; the repair pass, the history copy and the patch pass of the steering all read the PCM."""
    fs, N, xs, step, prec = 48000, 1024, synth.ULA8, 0.5, api.SRP_ADAPTIVE
    hop, n1, n2 = N // 2, 77, 67
    pcm = _scene(xs, fs, N, 1, 800, frames=n1 + n2)
    mk = lambda: api.Context(fs, xs, N, step, 1, srp_precision=prec, max_arrays=A, adaptive_fallback=False, adaptive_min_rows=16)
    Y, Z = mk(), mk()
    Y.reset_timing()
    cuts = [(0, (n1 + 1) * hop, n1), (n1 * hop, (n1 + n2 + 1) * hop, n2)]
    yr = _collect(_main_dev(Y, [dl.strided_pcm(pcm[:, :, s0:s1]) + (n,) for (s0, s1, n) in cuts]), "adaptive strided")
    zv = [(torch.from_numpy(np.ascontiguousarray(pcm[:, :, s0:s1])).cuda(), None, n) for (s0, s1, n) in cuts]
    zr = _collect(_main_dev(Z, zv), "adaptive contiguous")
    for i in range(2):
        _assert_same_bits(yr[i], zr[i], "adaptive call %d" % i)
    assert Y.repair_stats()["frames"] == A * (n1 + n2), Y.repair_stats()        # both calls ran coarse + repair ...
    assert Y.steer_stats()["frames"] == A * (n1 + n2), Y.steer_stats()          # ... and steered on the half spectrum
    _main_against_oracle(_cat(yr), pcm, fs, N, xs, 1, step, prec, Y.P)
    Y.close(); Z.close()


def test_main_context_power_gate_strided_equals_contiguous():
    """use_power_floor: the floor estimate takes 3 s = 94 frames of 512 samples at 16 kHz (tests/test_gpu_fft_sizes.py,
    test_other_frame_length_power_gate); the calls are 109 and 96 frames, so the first one finishes it and both hold bursts.
    The gate flags of the second call are read back from both contexts (mca_hip_copy_gate serves the last call)."""
    fs, N, xs, step = 16000, 512, synth.ULA8, 5.0
    hop, n1, n2 = N // 2, 109, 96
    Ft = n1 + n2
    L = (Ft + 1) * hop
    rng = np.random.default_rng(3)
    env = np.zeros(L)
    for a, b in ((98, 107), (112, 125), (131, 140), (150, Ft - 1)):
        env[a * hop:b * hop] = 1.0
    pcm = np.stack([(rng.standard_normal((8, L)) * 0.001 + synth.noise_source_stream(xs, np.deg2rad(20.0 - 35.0 * a), fs, L, 21 + a) * env)
                    for a in range(A)]).astype(np.float32)
    mk = lambda: api.Context(fs, xs, N, step, 1, use_power_floor=True, max_arrays=A)
    X, Y = mk(), mk()
    cuts = [(0, (n1 + 1) * hop, n1), (n1 * hop, L, n2)]
    xr = [X.process_frames_host(pcm[:, :, s0:s1], want_energy=True) for (s0, s1, _) in cuts]
    views = [dl.strided_pcm(pcm[:, :, s0:s1]) + (n,) for (s0, s1, n) in cuts]
    yr = _collect(_main_dev(Y, views), "gate")
    voiced, power = np.empty((A, n2), dtype=np.uint8), np.empty((A, n2), dtype=np.float32)
    Y._check(Y._lib.mca_hip_copy_gate(Y.h, voiced.ctypes.data_as(C.c_void_p), power.ctypes.data_as(api._lib.c_fp)))
    for i in range(2):
        _assert_same_bits(yr[i], {k: xr[i][k] for k in yr[i]}, "gate call %d" % i)
    _assert_same_bits(dict(voiced=voiced, power=power), dict(voiced=xr[1]["voiced"], power=xr[1]["power"]), "gate flags of the second call")
    r = _cat(xr, ("bin", "energy", "out", "voiced"))
    assert 0 < r["voiced"][:, :n1].sum() and 0 < r["voiced"][:, n1:].sum() < A * n2 and r["voiced"][:, :94].sum() == 0
    for a in range(A):
        o = po.ssl_stream_gated(fs, N, xs, pcm[a].astype(np.float64), 1, step, True)
        assert np.array_equal(r["voiced"][a], o["fired"]), a
        assert np.array_equal(r["bin"][a], o["bin"]), a
        assert np.abs(r["energy"][a] - o["energy"]).max() <= E_TOL[api.SRP_FP32] * np.abs(o["energy"]).max()
        assert_audio_where_bins_agree(r["out"][a][:o["out"].shape[0]], o["out"], r["bin"][a], o["bin"], hop)
    X.close(); Y.close()


def test_main_context_graph_on_the_strided_view():
    """mca_hip_graph_create on the strided view; two launches of 13 frames, the view refilled in between on the same stream
    (a recording replays on whatever the buffer holds).  X: two host calls of 13 frames."""
    fs, N, xs, step = 48000, 1024, synth.ULA8, 0.5
    hop, n = N // 2, F1
    pcm = _scene(xs, fs, N, 1, 900, frames=2 * n)
    mk = lambda: api.Context(fs, xs, N, step, 1, max_arrays=A)
    X, Y = mk(), mk()
    parts = [pcm[:, :, :(n + 1) * hop], pcm[:, :, n * hop:(2 * n + 1) * hop]]
    xr = [X.process_frames_host(p, want_energy=True) for p in parts]
    view, whole = dl.strided_pcm(parts[0])
    second = torch.from_numpy(np.ascontiguousarray(parts[1])).cuda()
    g = _guards(_main_spec(Y, n))
    st = _stream()
    gr = Y.graph_create(view, n, g["bin"].t, g["doa"].t, g["prob"].t, g["energy"].t, g["out"].t)
    keep = []
    with torch.cuda.stream(st):
        gr.launch(st.cuda_stream)
        keep.append({k: v.t.clone() for k, v in g.items()})
        view.copy_(second)
        gr.launch(st.cuda_stream)
    st.synchronize()
    torch.cuda.synchronize()
    last = _collect([g], "graph")[0]
    first = {k: v.cpu().numpy() for k, v in keep[0].items()}
    assert all(np.isfinite(v).all() for v in first.values() if v.dtype.kind == "f")
    assert torch.isnan(whole).sum().item() == whole.numel() - view.numel()        # the refill touched the view only
    _assert_same_bits(first, {k: xr[0][k] for k in first}, "graph launch 0")
    _assert_same_bits(last, {k: xr[1][k] for k in last}, "graph launch 1")
    r = _cat(xr)
    for a in range(A):
        o = po.ssl_stream(fs, N, xs, pcm[a].astype(np.float64), 1, step, want_map=True)
        _assert_bins(r["bin"][a], o["bin"], o["energy"], X.P, max_ties=3)
        assert np.abs(r["energy"][a] - o["energy"]).max() <= E_TOL[api.SRP_FP32] * np.abs(o["energy"]).max()
        assert_audio_where_bins_agree(r["out"][a], o["out"], r["bin"][a], o["bin"], hop)
    gr.close(); X.close(); Y.close()


@pytest.mark.parametrize("grid", [False, True], ids=["angles", "grid_bins"])
def test_separation_only_strided_equals_contiguous(grid):
    """mca_hip_separate_frames_dev (angles off the grid: k_beamform_ola) and mca_hip_separate_frames_bins_dev (grid bins:
    k_beamform_wave and its per-angle rows).  There is no host form of these calls; X is the contiguous device call
    tests/test_gpu_das_stream.py makes, and goes against the oracle's delay-and-sum stream under that file's bar."""
    from test_gpu_das_stream import _err, _oracle_das
    fs, N, xs = 48000, 1024, synth.ULA8
    hop = N // 2
    pcm = _scene(xs, fs, N, 1, 1000)
    mk = lambda: api.Context(fs, xs, N, 0.5, 1, srp_precision=api.SRP_FP16, max_arrays=A)
    X, Y = mk(), mk()
    rng = np.random.default_rng(5)
    if grid:
        bins = np.where(np.arange(F)[None, :] % 5 == 0, rng.integers(1, X.D - 1, (A, F)), 261 - 40 * np.arange(A)[:, None]).astype(np.int32)
        ang = X.doa_grid()[bins].astype(np.float32)
    else:
        bins = None
        ang = np.deg2rad(np.linspace(-71.3, 66.7, A * F)).reshape(A, F).astype(np.float32)

    def run(ctx, views, guard):
        calls, keep, t0 = [], [], 0
        st = _stream()
        for (v, _, n) in views:
            out = dl.guarded((A, 1, n * hop), torch.float32) if guard else None
            o = out.t if guard else torch.full((A, 1, n * hop), float("nan"), device="cuda")
            rad = torch.from_numpy(np.ascontiguousarray(ang[:, t0:t0 + n, None])).cuda()
            b = torch.from_numpy(np.ascontiguousarray(bins[:, t0:t0 + n, None])).cuda() if grid else None
            keep.append((rad, b))
            torch.cuda.synchronize()
            ctx.process_frames_dev(v, n, b, rad, None, None, o, stream=st.cuda_stream, localise=False, separate=True, bins_are_grid=grid)
            calls.append(dict(out=out) if guard else dict(out=o))
            t0 += n
        st.synchronize()
        torch.cuda.synchronize()
        return calls
    xv = [(torch.from_numpy(np.ascontiguousarray(pcm[:, :, s0:s1])).cuda(), None, n) for (s0, s1, n) in _cuts(hop)]
    xr = [dict(out=c["out"].cpu().numpy()) for c in run(X, xv, False)]
    yr = _collect(run(Y, _views(pcm, hop), True), "separate")
    for i in range(2):
        _assert_same_bits(yr[i], xr[i], "separate call %d" % i)
    got = np.concatenate([x["out"] for x in xr], axis=2)
    for a in range(A):
        ref = _oracle_das(fs, N, xs, pcm[a], ang[a], (F1, F2))
        e, tol = _err(got[a, 0], ref)
        assert e <= tol, (a, e, tol)
    X.close(); Y.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the 2-microphone calls
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,N", [(16000, 1024), (16000, 512), (48000, 4096)])
def test_gcc2_strided_equals_contiguous(fs, N):
    """mca_hip_gcc2_frames_dev: 1024 = k_stft_phat_few<2>, 512 = the any-M 512 kernel, 4096 = 512-sample sub-sequences per channel"""
    from test_gpu_fft_sizes import check_gcc2_against_oracle
    hop, xs = N // 2, synth.BINAURAL
    pcm = np.stack([synth.noise_source_stream(xs, np.deg2rad(33.0 - 40.0 * a), fs, (F + 1) * hop, 4 + a) for a in range(A)]).astype(np.float32)
    mk = lambda: api.Context(fs, xs, N, 3.0, 1, max_arrays=A)
    X, Y = mk(), mk()
    xr = [X.gcc2_frames_host(pcm[:, :, s0:s1], want_corr=True) for (s0, s1, _) in _cuts(hop)]
    views = _views(pcm, hop)
    calls = [_guards(dict(argmax=((A, n), torch.int32), doa=((A, n), torch.float32), prob=((A, n), torch.float32),
                          corr=((A, n, Y.D), torch.float32))) for (_, _, n) in views]
    st = _stream()
    for (v, _, n), g in zip(views, calls):
        Y.gcc2_frames_dev(v, n, g["argmax"].t, g["doa"].t, g["prob"].t, g["corr"].t, stream=st.cuda_stream)
    st.synchronize()
    yr = _collect(calls, "gcc2 %d" % N)
    for i in range(2):
        _assert_same_bits(yr[i], {k: xr[i][k] for k in yr[i]}, "gcc2 N %d call %d" % (N, i))
    r = {k: np.concatenate([x[k] for x in xr], axis=1) for k in ("argmax", "doa", "corr")}
    for a in range(A):
        check_gcc2_against_oracle(r, a, pcm[a], fs, xs, N)
    X.close(); Y.close()


def test_gcc2_tracked_strided_equals_contiguous():
    """mca_hip_gcc2_tracked_frames_dev at N = 1024: the particle filter runs on the rows the analysis leaves, so the twin of
    tests/test_gpu_gcc2_tracker.py (bit for bit on the GPU's own rows) ties X down; the particles of both contexts are compared too."""
    import test_gpu_gcc2_tracker as tk
    fs, xs, N, gated, pcm, _ = tk._batch("jump16k", A)
    hop = N // 2
    pcm = np.ascontiguousarray(pcm[:, :, :(F + 1) * hop]).astype(np.float32)
    X, Y = tk._ctx(fs, xs, N, gated, max_arrays=A), tk._ctx(fs, xs, N, gated, max_arrays=A)
    grid = X.doa_grid()
    xr = [X.gcc2_tracked_frames_host(pcm[:, :, s0:s1], want_corr=True) for (s0, s1, _) in _cuts(hop)]
    views = _views(pcm, hop)
    calls = [_guards(dict(argmax=((A, n), torch.int32), doa=((A, n), torch.float32), prob=((A, n), torch.float32), fired=((A, n), torch.uint8),
                          track=((A, n), torch.int32), corr=((A, n, Y.D), torch.float32))) for (_, _, n) in views]
    st = _stream()
    for (v, _, n), g in zip(views, calls):
        Y.gcc2_tracked_frames_dev(v, n, g["doa"].t, g["argmax"].t, g["prob"].t, g["fired"].t, g["track"].t, g["corr"].t, stream=st.cuda_stream)
    st.synchronize()
    yr = _collect(calls, "tracked")
    for i in range(2):
        _assert_same_bits(yr[i], {k: xr[i][k] for k in yr[i]}, "tracked call %d" % i)
    r = {k: np.concatenate([x[k] for x in xr], axis=1) for k in ("argmax", "doa", "prob", "fired", "track", "corr")}
    n_bad = 0
    for a in range(A):
        px, py = X.gcc2_tracker_particles(a), Y.gcc2_tracker_particles(a)
        assert px["particles"].tobytes() == py["particles"].tobytes() and px["alive"] == py["alive"] and px["track"] == py["track"], a
        t = tk._twin_of(r, a, gated, fs, N, grid)
        n_bad += tk._report("tracked[%d] doa" % a, r["doa"][a], t["doa"].astype(np.float32))
        n_bad += tk._report("tracked[%d] prob" % a, r["prob"][a], t["prob"].astype(np.float32))
        n_bad += tk._report("tracked[%d] particles" % a, px["particles"], t["particles"])
        assert np.array_equal(r["fired"][a], t["fired"]) and np.array_equal(r["track"][a], t["track"]), a
    assert n_bad == 0
    X.close(); Y.close()


def test_temporal_gcc_strided_equals_contiguous():
    """mca_hip_tgcc_frames_dev (kernels_tgcc.hip) in its own window and hop: W = 2400, hop = 1200 at 16 kHz, 13 + 8 frames"""
    import test_gpu_temporal_gcc as tg
    import tgcc_twin as tt
    fs, d = 16000, 0.086
    W, hop, nd = tt.geometry(fs, d)
    L = (F - 1) * hop + W
    pcm = np.stack([(synth.noise_source_stream([0.0, d], np.deg2rad(40.0 - 45.0 * a), fs, L, 60 + a) * 1000.0) for a in range(A)]).astype(np.float32)
    X, Y = tg._module(fs, d, False, max_arrays=A), tg._module(fs, d, False, max_arrays=A)
    assert (X.W, X.hop, X.nd) == (W, hop, nd)
    cuts = _cuts(hop, tail=W - hop)
    xr = [X.process(pcm[:, :, s0:s1], want_index=True) for (s0, s1, _) in cuts]
    views = _views(pcm, hop, tail=W - hop)
    calls = [_guards(dict(doa=((A, n), torch.float32), prob=((A, n), torch.float32), voiced=((A, n), torch.uint8), power=((A, n), torch.float32),
                          delay_idx=((A, n), torch.int32), index=((A, n, nd), torch.float64))) for (_, _, n) in views]
    st = _stream()
    for (v, _, n), g in zip(views, calls):
        Y.process_dev(v, stream=st.cuda_stream, want_index=True, n_frames=n, out={k: x.t for k, x in g.items()})
    st.synchronize()
    yr = _collect(calls, "tgcc")
    for i in range(2):
        _assert_same_bits(yr[i], {k: xr[i][k] for k in yr[i]}, "tgcc call %d" % i)
    r = tg._concat(xr)
    for a in range(A):
        tg._compare(r, a, pcm[a], fs, d, False, "layout stream %d" % a)
    X.close(); Y.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the masking modules and the multiband localiser
# ---------------------------------------------------------------------------------------------------------------------------
def _binaural_input(N, seed):
    hop = N // 2
    n = (F + 1) * hop
    rows = []
    for a in range(A):
        rng = np.random.default_rng(seed + a)
        src = rng.standard_normal(n) * 0.1
        left = src + rng.standard_normal(n) * 0.003
        right = np.roll(src, 1 + a) * 0.9 + rng.standard_normal(n) * 0.003
        env = np.repeat(rng.choice([1.0, 0.2, 0.05, 0.6], F + 1), hop)
        rows.append(np.stack([left * env, right * env]))
    return np.stack(rows).astype(np.float32)


def _mask_dev(m, views, hop):
    calls = [_guards(dict(out=((A, 2, n * hop), torch.float32), dec=((A, n, 45), torch.int32))) for (_, _, n) in views]
    st = _stream()
    for (v, _, n), g in zip(views, calls):
        m.process_dev(v, n, g["out"].t, g["dec"].t, stream=st.cuda_stream)
    st.synchronize()
    return calls


@pytest.mark.parametrize("fs,N,method,alg", [(16000, 1024, "RELATIVE", "BOTH"), (48000, 2048, "RELATIVE", "BOTH"), (8000, 512, "RELATIVE", "BOTH"),
                                             (16000, 1024, "NOISY", "SPATIAL")])
def test_fast_binaural_masking_strided_equals_contiguous(fs, N, method, alg):
    """mca_hip_mask_frames_dev: 1024 = k_mask_stream, 2048 = k_mask_stream_2048 (512-sample sub-sequences), 512 = the any-length
    k_mask_stream_gen; NOISY runs its first call as a single chunk (ft = n_frames, api_mask.hip).  The bar is the one of test_masking_stream_other_frame_lengths."""
    from test_gpu_fft_sizes import check_masking_against_oracle
    method, alg = getattr(api, method), getattr(api, alg)
    hop, d = N // 2, 0.086
    flo, fhi = 300.0, min(5000.0, 0.45 * fs)
    pcm = _binaural_input(N, N + method)
    mk = lambda: api.FastBinauralMasking(fs, d, flo, fhi, method, alg, fft_size=N, max_streams=A)
    X, Y = mk(), mk()
    xr = [dict(zip(("out", "dec"), X.process(pcm[:, :, s0:s1]))) for (s0, s1, _) in _cuts(hop)]
    yr = _collect(_mask_dev(Y, _views(pcm, hop), hop), "mask")
    for i in range(2):
        _assert_same_bits(yr[i], xr[i], "mask N %d call %d" % (N, i))
    out = np.concatenate([x["out"] for x in xr], axis=2)
    dec = np.concatenate([x["dec"] for x in xr], axis=1)
    for a in range(A):
        check_masking_against_oracle(out[a], dec[a], pcm[a], fs, N, d, flo, fhi, method, alg)
    X.close(); Y.close()


def test_binaural_masking_impl_strided_equals_contiguous():
    """mca_hip_bmask_frames_dev at its 16 kHz shape (W = 1024) against the twin under tests/test_gpu_bmask.py's bar"""
    import bmask_twin as bt
    import test_gpu_bmask as tb
    fs = tb.FS
    X, Y = (api.BinauralMaskingImpl(fs, tb.D, tb.LO, tb.HI, bt.RELATIVE, max_streams=A) for _ in range(2))
    hop = X.hop
    pcm = np.stack([bt.parity_input(seed, fs, F) for seed in sorted(bt.PARITY)])
    assert pcm.shape == (A, 2, (F + 1) * hop)
    xr = [dict(zip(("out", "dec"), X.process(pcm[:, :, s0:s1]))) for (s0, s1, _) in _cuts(hop)]
    yr = _collect(_mask_dev(Y, _views(pcm, hop), hop), "bmask")
    for i in range(2):
        _assert_same_bits(yr[i], xr[i], "bmask call %d" % i)
    out = np.concatenate([x["out"] for x in xr], axis=2)
    dec = np.concatenate([x["dec"] for x in xr], axis=1)
    for a in range(A):
        tb._check_stream("layout stream %d" % a, out[a], dec[a], bt.Twin(fs, tb.D, tb.LO, tb.HI, bt.RELATIVE).stream(pcm[a]))
    X.close(); Y.close()


@pytest.mark.parametrize("fs,N", [(48000, 1024), (16000, 512), (96000, 2048)])
def test_multiband_strided_equals_contiguous(fs, N):
    """mca_hip_mb_frames_dev: k_mb_analyse_1024, k_mb_analyse_512 and the any-length analysis (2048)"""
    import test_gpu_multiband as tm
    hop, xs, nbins = N // 2, synth.BINAURAL, 15
    pcm = np.stack([synth.noise_source_stream(xs, np.deg2rad(-55.0 + 45.0 * a), fs, (F + 1) * hop, 40 + a) for a in range(A)]).astype(np.float32)
    mk = lambda: api.MultibandBinarualLocalisation(fs, xs, nbins, False, fft_size=N, max_arrays=A)
    X, Y = mk(), mk()
    xr = [X.process(pcm[:, :, s0:s1], want_bands=True) for (s0, s1, _) in _cuts(hop)]
    views = _views(pcm, hop)
    calls = [_guards(dict(doa=((A, n), torch.float32), prob=((A, n), torch.float32), voiced=((A, n), torch.uint8), power=((A, n), torch.float32),
                          band_idx=((A, n, nbins), torch.int32), energy_in_doa=((A, n, Y.D), torch.float32),
                          band_corr=((A, n, nbins, Y.D), torch.float32))) for (_, _, n) in views]
    st = _stream()
    for (v, _, n), g in zip(views, calls):
        Y.process_dev(v, n, g["doa"].t, g["prob"].t, g["voiced"].t, g["power"].t, g["band_idx"].t, g["energy_in_doa"].t, g["band_corr"].t,
                      stream=st.cuda_stream)
    st.synchronize()
    yr = _collect(calls, "multiband")
    for i in range(2):
        _assert_same_bits(yr[i], {k: xr[i][k] for k in yr[i]}, "multiband N %d call %d" % (N, i))
    r = {k: np.concatenate([x[k] for x in xr], axis=1) for k in yr[0]}
    flagged = 0
    for a in range(A):
        flagged += tm._compare(X, po.Multiband(fs, xs, N + 2, nbins, False), pcm[a], N, r, a)
    assert flagged <= 0.1 * A * F, flagged
    X.close(); Y.close()


# ---------------------------------------------------------------------------------------------------------------------------
# MVDR
# ---------------------------------------------------------------------------------------------------------------------------
import test_gpu_mvdr as tv                    # noqa: E402


def _mvdr_dev(bf, views, doa, S, K, hop):
    """doa [A][F] (single look, S = 0) or [A][F][S]"""
    calls, keep, t0 = [], [], 0
    for (_, _, n) in views:
        lead = (A, S) if S else (A,)
        calls.append(_guards(dict(out=(lead + (n * hop,), torch.float32), spec=(lead + (n, K, 2), torch.float32))))
        keep.append(torch.from_numpy(np.ascontiguousarray(doa[:, t0:t0 + n])).cuda())
        t0 += n
    st = _stream()
    for (v, _, n), g, dd in zip(views, calls, keep):
        (bf.process_sources_dev if S else bf.process_dev)(v, n, dd, g["out"].t, g["spec"].t, stream=st.cuda_stream)
    st.synchronize()
    return calls


def _c64(x):
    return np.ascontiguousarray(x).view(np.float32).reshape(x.shape + (2,))


@pytest.mark.parametrize("xs,fs,N", [(synth.ULA8, 48000, 1024), (synth.REEM_C, 16000, 512), (IRR5, 8000, 256)], ids=["1024", "512", "256"])
def test_mvdr_strided_equals_contiguous(xs, fs, N):
    """mca_hip_mvdr_frames_dev: k_mvdr_analyse_1024, k_mvdr_analyse_512 and the any-length k_mvdr_analyse"""
    hop, K = N // 2, N // 2 + 1
    pcm = np.stack([tv._scene(xs, fs, N, F, a) for a in range(A)])
    doa = (np.deg2rad(20.0 - 30 * np.arange(A))[:, None] + 0.01 * np.arange(F)[None, :]).astype(np.float32)
    X, Y = (api.MvdrBeamformer(fs, xs, N, max_streams=A) for _ in range(2))
    xr, t0 = [], 0
    ogs = [po.MVDR(fs, N, xs) for _ in range(A)]
    for i, (s0, s1, n) in enumerate(_cuts(hop)):
        r = X.process(pcm[:, :, s0:s1], doa[:, t0:t0 + n], want_spec=True)
        for a in range(A):
            o = ogs[a].stream(pcm[a, :, s0:s1].astype(np.float64), doa[a, t0:t0 + n].astype(np.float64), want_spec=True)
            sp = tv._ospec(o)
            assert np.abs(r["spec"][a] - sp).max() <= tv.SPEC_TOL * np.abs(sp).max(), (i, a)
            h = hop if i else 0           # (the oracle's stream() restarts its overlap-add tail per call)
            assert np.abs(r["out"][a, h:] - o["out"][h:]).max() <= tv.AUDIO_TOL * np.abs(o["out"]).max(), (i, a)
            assert np.abs(X.covariance(a) - ogs[a].covariance()).max() <= tv.COV_TOL * np.abs(ogs[a].covariance()).max(), (i, a)
        xr.append(dict(out=r["out"], spec=_c64(r["spec"])))
        t0 += n
    yr = _collect(_mvdr_dev(Y, _views(pcm, hop), doa, 0, K, hop), "mvdr")
    for i in range(2):
        _assert_same_bits(yr[i], xr[i], "mvdr N %d call %d" % (N, i))
    for a in range(A):
        assert np.array_equal(X.covariance(a), Y.covariance(a)), a
    X.close(); Y.close()


@pytest.mark.parametrize("gain", [0.0, 100.0])
def test_mvdr_sources_strided_equals_contiguous(gain):
    """mca_hip_mvdr_sources_frames_dev, S = 3: k_mvdr_solve_t (gain 0, against po.MVDR per look direction) and its NULLS form
    (gain 100, against tests/mvdr_nulls_twin.py under the bar of tests/test_gpu_mvdr_nulls.py)"""
    import mvdr_nulls_twin as nt
    import test_gpu_mvdr_nulls as tn
    import test_gpu_mvdr_sources as ts
    fs, N, xs, S = 48000, 1024, synth.ULA8, 3
    hop, K = N // 2, N // 2 + 1
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    doa = nt.drifting_doa(A, F, S)
    X, Y = (api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=gain) for _ in range(2))
    xr, t0 = [], 0
    state = [None] * A
    ogs = [[po.MVDR(fs, N, xs) for _ in range(S)] for _ in range(A)]
    for i, (s0, s1, n) in enumerate(_cuts(hop)):
        r = X.process_sources(pcm[:, :, s0:s1], doa[:, t0:t0 + n])
        for a in range(A):
            if gain:
                state[a] = nt.mvdr_nulls_stream(fs, N, xs, pcm[a, :, s0:s1].astype(np.float64), doa[a, t0:t0 + n], gain, state=state[a])
                tn._check_against_twin(r, state[a], a, "layout call %d" % i)
                tn._check_covariance(X, state[a], a)
            else:
                ts._check_against_oracle(r, ogs[a], pcm[a, :, s0:s1], doa[a, t0:t0 + n], a, skip_first_hop=bool(i))
                cov = ogs[a][0].covariance()
                assert np.abs(X.covariance(a) - cov).max() <= ts.COV_TOL * np.abs(cov).max(), (i, a)
        xr.append(dict(out=r["out"], spec=_c64(r["spec"])))
        t0 += n
    yr = _collect(_mvdr_dev(Y, _views(pcm, hop), doa, S, K, hop), "mvdr sources")
    for i in range(2):
        _assert_same_bits(yr[i], xr[i], "mvdr sources gain %g call %d" % (gain, i))
    for a in range(A):
        assert np.array_equal(X.covariance(a), Y.covariance(a)), a
    X.close(); Y.close()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: a layout the header rules out returns INVALID_ARGUMENT and touches no state
# ---------------------------------------------------------------------------------------------------------------------------
def _entry_points():
    """name -> (make context, call(ctx, ptr, array_stride, ch_stride, n_arrays, outs) -> rc, outputs spec, channels, samples a row needs,
    aligned: does the header document the alignment rule).  Every call is the raw C entry point, 2 arrays x 4 frames."""
    lib = api._lib.load()
    n = 4
    P = lambda g, k: C.c_void_p(g[k].t.data_ptr())
    eps = {}

    def main(fn_name, S=1):
        mk = lambda: api.Context(48000, synth.REEM_C, 1024, 5.0, S, max_arrays=2)
        spec = dict(bin=((2, n, S), torch.int32), doa=((2, n, S), torch.float32), prob=((2, n, S), torch.float32), out=((2, S, n * 512), torch.float32))
        fn = getattr(lib, fn_name)

        def call(ctx, p, sa, sc, na, g):
            if fn_name == "mca_hip_process_frames_dev":
                return fn(ctx.h, p, sa, sc, na, n, P(g, "bin"), P(g, "doa"), P(g, "prob"), None, P(g, "out"), None)
            if fn_name == "mca_hip_localise_frames_dev":
                return fn(ctx.h, p, sa, sc, na, n, P(g, "bin"), P(g, "doa"), P(g, "prob"), None, None)
            g["doa"].t.fill_(0.3); g["bin"].t.fill_(20)
            torch.cuda.synchronize()
            if fn_name == "mca_hip_separate_frames_dev":
                return fn(ctx.h, p, sa, sc, na, n, P(g, "doa"), P(g, "out"), None)
            return fn(ctx.h, p, sa, sc, na, n, P(g, "bin"), P(g, "doa"), P(g, "out"), None)
        return mk, call, spec, 4, (n + 1) * 512, True
    for name in ("process", "localise", "separate", "separate_frames_bins"):
        full = "mca_hip_%s_frames_dev" % name if name != "separate_frames_bins" else "mca_hip_separate_frames_bins_dev"
        eps[full] = main(full)

    def graph():
        mk = lambda: api.Context(48000, synth.REEM_C, 1024, 5.0, 1, max_arrays=2)
        spec = dict(bin=((2, n, 1), torch.int32), doa=((2, n, 1), torch.float32), prob=((2, n, 1), torch.float32), out=((2, 1, n * 512), torch.float32))

        def call(ctx, p, sa, sc, na, g):
            h = C.c_void_p()
            rc = lib.mca_hip_graph_create(ctx.h, p, sa, sc, na, n, P(g, "bin"), P(g, "doa"), P(g, "prob"), None, P(g, "out"), C.byref(h))
            if rc == 0:
                rc = lib.mca_hip_graph_launch(h, None)
                torch.cuda.synchronize()
                lib.mca_hip_graph_destroy(h)
            else:
                assert not h.value
            return rc
        return mk, call, spec, 4, (n + 1) * 512, True
    eps["mca_hip_graph_create"] = graph()

    def gcc2(tracked):
        def mk():
            ctx = api.Context(16000, synth.BINAURAL, 1024, 3.0, 1, max_arrays=2)
            if tracked:
                ctx.gcc2_tracker_attach(seed=7)
            return ctx
        spec = dict(argmax=((2, n), torch.int32), doa=((2, n), torch.float32), prob=((2, n), torch.float32))

        def call(ctx, p, sa, sc, na, g):
            if tracked:
                return lib.mca_hip_gcc2_tracked_frames_dev(ctx.h, p, sa, sc, na, n, P(g, "argmax"), P(g, "doa"), P(g, "prob"), None, None, None, None)
            return lib.mca_hip_gcc2_frames_dev(ctx.h, p, sa, sc, na, n, P(g, "argmax"), P(g, "doa"), P(g, "prob"), None, None)
        return mk, call, spec, 2, (n + 1) * 512, True
    eps["mca_hip_gcc2_frames_dev"] = gcc2(False)
    eps["mca_hip_gcc2_tracked_frames_dev"] = gcc2(True)

    def masks(kind):
        if kind == "mask":
            mk = lambda: api.FastBinauralMasking(16000, 0.086, 300.0, 5000.0, api.RELATIVE, api.BOTH, fft_size=1024, max_streams=2)
        else:
            mk = lambda: api.BinauralMaskingImpl(16000, 0.086, 500, 5000, api.RELATIVE, max_streams=2)
        spec = dict(out=((2, 2, n * 512), torch.float32), dec=((2, n, 45), torch.int32))
        fn = getattr(lib, "mca_hip_%s_frames_dev" % kind)
        return mk, (lambda ctx, p, sa, sc, na, g: fn(ctx.h, p, sa, sc, na, n, P(g, "out"), P(g, "dec"), None)), spec, 2, (n + 1) * 512, True
    eps["mca_hip_mask_frames_dev"] = masks("mask")
    eps["mca_hip_bmask_frames_dev"] = masks("bmask")

    def mb():
        mk = lambda: api.MultibandBinarualLocalisation(48000, synth.BINAURAL, 15, False, fft_size=1024, max_arrays=2)
        spec = dict(doa=((2, n), torch.float32), prob=((2, n), torch.float32))
        return mk, (lambda ctx, p, sa, sc, na, g: lib.mca_hip_mb_frames_dev(ctx.h, p, sa, sc, na, n, P(g, "doa"), P(g, "prob"), None, None, None, None,
                                                                           None, None)), spec, 2, (n + 1) * 512, True
    eps["mca_hip_mb_frames_dev"] = mb()

    def tgcc():
        mk = lambda: api.TemporalGCCBinauralLocalisation(16000, [0.0, 0.086], use_power_floor=False, max_arrays=2)
        spec = dict(doa=((2, n), torch.float32), prob=((2, n), torch.float32), voiced=((2, n), torch.uint8), power=((2, n), torch.float32),
                    delay_idx=((2, n), torch.int32))
        return mk, (lambda ctx, p, sa, sc, na, g: lib.mca_hip_tgcc_frames_dev(ctx.h, p, sa, sc, na, n, P(g, "doa"), P(g, "prob"), P(g, "voiced"),
                                                                             P(g, "power"), P(g, "delay_idx"), None, None)), spec, 2, 3 * 1200 + 2400, False
    eps["mca_hip_tgcc_frames_dev"] = tgcc()

    def mvdr(sources):
        S = 2 if sources else 1
        mk = lambda: api.MvdrBeamformer(16000, synth.REEM_C, 512, max_streams=2, max_sources=S)
        lead = (2, S) if sources else (2,)
        spec = dict(doa=((2, n, S) if sources else (2, n), torch.float32), out=(lead + (n * 256,), torch.float32))

        def call(ctx, p, sa, sc, na, g):
            g["doa"].t.fill_(0.3)
            torch.cuda.synchronize()
            if sources:
                return lib.mca_hip_mvdr_sources_frames_dev(ctx.h, p, sa, sc, na, n, S, P(g, "doa"), P(g, "out"), None, None)
            return lib.mca_hip_mvdr_frames_dev(ctx.h, p, sa, sc, na, n, P(g, "doa"), P(g, "out"), None, None)
        return mk, call, spec, 4, (n + 1) * 256, True
    eps["mca_hip_mvdr_frames_dev"] = mvdr(False)
    eps["mca_hip_mvdr_sources_frames_dev"] = mvdr(True)
    return eps


ENTRY_POINTS = ["mca_hip_process_frames_dev", "mca_hip_localise_frames_dev", "mca_hip_separate_frames_dev", "mca_hip_separate_frames_bins_dev",
                "mca_hip_graph_create", "mca_hip_gcc2_frames_dev", "mca_hip_gcc2_tracked_frames_dev", "mca_hip_mask_frames_dev",
                "mca_hip_bmask_frames_dev", "mca_hip_mb_frames_dev", "mca_hip_tgcc_frames_dev", "mca_hip_mvdr_frames_dev",
                "mca_hip_mvdr_sources_frames_dev"]


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_layouts_the_header_rules_out_are_refused_and_touch_no_state(entry):
    """an odd channel stride, an odd array stride, a pointer one float off 8-byte alignment (where the header documents the rule:
    mca_hip_tgcc_frames_dev documents none), a channel stride and -- with 2 arrays -- an array stride two samples short: each is
    MCA_HIP_ERR_INVALID_ARGUMENT, and the valid call behind them gives the bits of a fresh context's first call"""
    mk, call, spec, ch, need, aligned = _entry_points()[entry]
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((2, ch, need + 8)) * 0.1).astype(np.float32)
    view, whole = dl.strided_pcm(x)
    p0, sa, sc = view.data_ptr(), view.stride(0), view.stride(1)
    bad = [("a channel stride two samples short", p0, sa, need - 2, 2),
           ("an array stride two samples short", p0, (ch - 1) * sc + need - 2, sc, 2)]
    if aligned:
        bad += [("an odd channel stride", p0, sa, sc + 1, 2), ("an odd array stride", p0, sa + 1, sc, 2),
                ("a pointer one float off 8-byte alignment", p0 + 4, sa, sc, 2)]
    ctx, fresh = mk(), mk()
    g = _guards(spec)
    untouched = {k: v.raw.clone() for k, v in g.items()}
    torch.cuda.synchronize()
    for what, p, a_, c_, na in bad:
        rc = call(ctx, C.c_void_p(p), a_, c_, na, g)
        assert rc == INVALID, "%s: %s gave %d" % (entry, what, rc)
    torch.cuda.synchronize()
    inputs = ("doa", "bin") if ("separate" in entry or "mvdr" in entry) else ()
    for k, v in g.items():
        if k not in inputs:
            assert torch.equal(v.raw, untouched[k]), "%s: a refused call wrote output %s" % (entry, k)
    assert call(ctx, C.c_void_p(p0), sa, sc, 2, g) == 0
    torch.cuda.synchronize()
    g2 = _guards(spec)
    assert call(fresh, C.c_void_p(p0), sa, sc, 2, g2) == 0
    torch.cuda.synchronize()
    a_res, b_res = _collect([g], entry)[0], _collect([g2], entry + " fresh")[0]
    _assert_same_bits(a_res, b_res, entry + " after the refusals")
    ctx.close(); fresh.close()
