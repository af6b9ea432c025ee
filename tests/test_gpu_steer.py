"""Delay-and-sum on the half spectrum of the separated channels (csrc/steer.h): device-pointer calls of a
one-source, ungated 8-microphone ULA at 1024-sample frames (ADAPTIVE, FP16).  The analysis kernel steers every frame at the
array's PREDICTED bin -- its last pick of the previous call -- while it holds the separated spectra, k_steer_patch redoes the
frames whose pick came out different through the same routine, k_steer_synth turns the rows into audio.

What is asked here: the audio equals the oracle's delay-and-sum stream at the GPU's own picks on EVERY hop (2e-5 of the peak +
1e-7, the project's bar), whatever share of the frames missed; picks and audio BITS do not depend on how a stream is cut into
calls, on whether a call's analysis steered ahead (fused) or every frame was steered after the picks (the guard, a workspace
budget too small for the whole call), on a state blob taken in between, or on what runs beside the kernels; the guard
switches off and back on at calls that the calls' content fixes."""
import ctypes as C
import os

import numpy as np
import pytest

from mcarray_amd import api, synth
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FS, N, HOP = 48000, 1024, 512
XS = synth.ULA8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _calls(ctx, pcm, sizes, drain=True):
    """pcm [A][M][(F + 1) * hop] through mca_hip_process_frames_dev in consecutive calls of sizes[i] frames (drain: the device is
    synchronised behind every call; else the calls are fired back to back): bins [A][F], angles [A][F], audio [A][F * hop]"""
    dev = torch.device("cuda:0")
    A = pcm.shape[0]
    keep, t0 = [], 0
    for Fi in sizes:
        x = torch.from_numpy(np.ascontiguousarray(pcm[:, :, t0 * HOP:(t0 + Fi + 1) * HOP])).to(dev)
        b = torch.empty(A, Fi, 1, dtype=torch.int32, device=dev)
        r = torch.empty(A, Fi, 1, dtype=torch.float32, device=dev)
        q = torch.empty(A, Fi, 1, dtype=torch.float32, device=dev)
        o = torch.full((A, 1, Fi * HOP), float("nan"), dtype=torch.float32, device=dev)
        ctx.process_frames_dev(x, Fi, b, r, q, None, o)
        if drain:
            torch.cuda.synchronize()
        keep.append((x, b, r, q, o))
        t0 += Fi
    torch.cuda.synchronize()
    return (np.concatenate([k[1].cpu().numpy()[:, :, 0] for k in keep], axis=1), np.concatenate([k[2].cpu().numpy()[:, :, 0] for k in keep], axis=1),
            np.concatenate([k[4].cpu().numpy()[:, 0] for k in keep], axis=1))


def _ctx(A, precision=api.SRP_FP16, **kw):
    return api.Context(FS, XS, N, 0.5, 1, srp_precision=precision, max_arrays=A, adaptive_fallback=False, **kw)


def _stationary(F, A, seed, base=23.0):
    return np.stack([synth.noise_source_stream(XS, np.deg2rad(base - 41 * a), FS, (F + 1) * HOP, seed + a) for a in range(A)]).astype(np.float32)


def _moving(F, seed, every=5):
    """one array whose source jumps to another angle every few frames (hard cuts: the pick changes every few frames)"""
    rng = np.random.default_rng(seed)
    parts, n = [], 0
    while n < (F + 1) * HOP:
        ln = int(rng.integers(every - 2, every + 3)) * HOP
        parts.append(synth.noise_source_stream(XS, np.deg2rad(float(rng.uniform(-70, 70))), FS, ln, int(rng.integers(1 << 30))))
        n += ln
    return np.concatenate(parts, axis=1)[None, :, :(F + 1) * HOP].astype(np.float32)


def _against_oracle(bins, rad, audio, pcm, min_same=0.0):
    """EVERY hop against the oracle's delay-and-sum stream (mca_or_das_stream: Beamformer.cpp:51-71 in double, inverse transform,
    overlap-add) steered at the GPU's own picks -- complete whatever the picks are, in particular across the boundaries between frames
    the analysis steered ahead and frames the patch pass redid; min_same: the share of the picks that equal the localiser oracle's."""
    for a in range(pcm.shape[0]):
        assert np.isfinite(audio[a]).all()
        ref = po.das_stream(FS, N, XS, pcm[a].astype(np.float64), rad[a].astype(np.float64))
        err = float(np.abs(audio[a] - ref).max())
        print("array %d: audio error %.3e of the peak (%.3e)" % (a, err / np.abs(ref).max(), np.abs(ref).max()))
        assert err <= 2e-5 * np.abs(ref).max() + 1e-7, (a, err, np.abs(ref).max())
        if min_same > 0:
            o = po.ssl_stream(FS, N, XS, pcm[a].astype(np.float64), 1, 0.5, want_audio=False)
            assert (bins[a] == o["bin"][:, 0]).mean() >= min_same


@pytest.mark.parametrize("precision", ["FP16", "ADAPTIVE"])
def test_a_stationary_source_is_steered_ahead_of_its_picks_and_matches_the_oracle(precision):
    F, A = 96, 2
    pcm = _stationary(3 * F, A, 9100)
    ctx = _ctx(A, getattr(api, "SRP_" + precision), adaptive_min_rows=64)
    bins, rad, audio = _calls(ctx, pcm, [F, F, F])
    st = ctx.steer_stats()
    ctx.close()
    assert st["frames"] == 3 * F * A and st["fused_calls"] == 3, st     # (the first call's misses -- bin -1 predicted -- do not count for the guard)
    assert st["missed"] <= A * F + 0.2 * 2 * A * F, (st, [np.unique(bins[a, F:]).tolist() for a in range(A)])
    _against_oracle(bins, rad, audio, pcm, 0.95)


@pytest.mark.parametrize("F", [61, 63, 64, 75, 76, 77, 130])
def test_a_moving_source_matches_the_oracle_on_every_hop(F):
    """the pick changes every few frames: most frames go through the patch pass, next to frames the analysis steered; the lengths
    end around the 16-frame runs and the spans of the synthesis kernel's workgroups"""
    pcm = _moving(2 * F, 7000 + F)
    ctx = _ctx(1)
    bins, rad, audio = _calls(ctx, pcm, [F, F])
    st = ctx.steer_stats()
    ctx.close()
    assert st["fused_calls"] == 2 and F <= st["missed"] <= 2 * F, st
    assert len(np.unique(bins[0, F:])) >= 3
    _against_oracle(bins, rad, audio, pcm)


def test_the_audio_bits_do_not_depend_on_how_the_stream_is_cut_into_calls():
    """one call, two calls and ragged calls give the same picks and the same audio BITS on every hop; a stationary source (no misses
    behind the first call) and one that jumps at the boundary of the two-call form (every frame behind the jump misses there)"""
    F, A = 384, 2
    still = _stationary(F, A, 9200)
    jump = np.concatenate([_stationary(F // 2, A, 9300)[:, :, :F // 2 * HOP], _stationary(F // 2, A, 9400, base=-30.0)], axis=2)
    assert jump.shape == still.shape
    for pcm in (still, jump):
        res = []
        for sizes in ([F], [F // 2, F // 2], [67, 130, 1, 16, 170]):
            ctx = _ctx(A)
            res.append(_calls(ctx, pcm, sizes))
            ctx.close()
        _against_oracle(*res[0], pcm)
        for b, r, o in res[1:]:
            assert np.array_equal(b, res[0][0])
            assert np.array_equal(o, res[0][2])


def test_a_small_workspace_budget_steers_after_the_picks_with_the_same_bits(monkeypatch):
    """MCA_HIP_WS_MAX_MB below the rows of Y a call needs: the analysis does not steer, the patch pass takes every frame, in passes"""
    F, A = 300, 2
    pcm = _stationary(2 * F, A, 9500)
    ctx = _ctx(A)
    b0, r0, o0 = _calls(ctx, pcm, [F, F])
    s0 = ctx.steer_stats()
    ctx.close()
    monkeypatch.setenv("MCA_HIP_WS_MAX_MB", "1")               # 252 rows of Y: passes of 126 frames
    ctx = _ctx(A)
    b1, r1, o1 = _calls(ctx, pcm, [F, F])
    s1 = ctx.steer_stats()
    ctx.close()
    assert s0["fused_calls"] == 2 and s1["fused_calls"] == 0 and s1["frames"] == s0["frames"], (s0, s1)
    assert np.array_equal(b0, b1)
    assert np.array_equal(o0, o1)


def _guard_input(F, A):
    """two calls of a stationary source, three of one that moves every few frames, four stationary again"""
    rows = []
    for a in range(A):
        s1 = synth.noise_source_stream(XS, np.deg2rad(31.0 - 9 * a), FS, 2 * F * HOP, 9950 + a)
        mv = _moving(3 * F, 9960 + a)[0][:, :3 * F * HOP]
        s2 = synth.noise_source_stream(XS, np.deg2rad(-12.0 + 7 * a), FS, (4 * F + 1) * HOP, 9970 + a)
        rows.append(np.concatenate([s1, mv, s2], axis=1))
    return np.stack(rows).astype(np.float32)


def test_the_guard_switches_off_on_moving_content_and_back_and_is_reproducible():
    """the bench's configuration (ADAPTIVE, adaptive_fallback AUTO) at a size the adaptive mode takes.  A call steers ahead of its picks
    unless the call TWO calls before it missed on more than a third of its frames (a report slot at a fixed lag, as the AUTO policy's;
    arrays without a pick yet do not count): calls 1 ... 4 steer ahead, 5 ... 8 do not (calls 3 ... 5 move, call 6 starts from a moving
    call's last pick), 9 does.  Fired back to back or with the device drained behind every call: the same calls switch,
    the same bits come out -- and the audio does not depend on the guard's state: every hop against the oracle's stream."""
    F, A = 512, 8
    pcm = _guard_input(F, A)
    res = []
    for drain in (True, False):
        ctx = api.Context(FS, XS, N, 0.5, 1, srp_precision=api.SRP_ADAPTIVE, max_arrays=A)
        if drain:
            out, fused = [[], [], []], []
            for i in range(9):
                part = _calls(ctx, pcm[:, :, i * F * HOP:((i + 1) * F + 1) * HOP], [F])
                for k in range(3):
                    out[k].append(part[k])
                fused.append(ctx.steer_stats()["fused_calls"])
            got = tuple(np.concatenate(o, axis=1) for o in out)
            assert np.diff([0] + fused).tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 1], fused
        else:
            got = _calls(ctx, pcm, [F] * 9, drain=False)
        res.append((got, ctx.steer_stats()))
        ctx.close()
    (d, sd), (bb, sb) = res
    assert sd == sb, (sd, sb)
    for k in range(3):
        assert np.array_equal(d[k], bb[k])
    _against_oracle(d[0][:2], d[1][:2], d[2][:2], pcm[:2])


@pytest.mark.parametrize("case", ["60 dB down", "80 dB down", "100 dB down", "exact zeros"])
def test_channels_of_very_different_level_are_steered_at_their_own_scale(case):
    """the weaker channel of a pair goes through the shared transform scaled by a power of two (pair_balance.h): the steering sum takes
    it back at its own scale, and a channel of exact zeros as zeros"""
    F = 96
    pcm = _stationary(2 * F, 1, 9600)
    g = {"60 dB down": 1e-3, "80 dB down": 1e-4, "100 dB down": 1e-5, "exact zeros": 0.0}[case]
    pcm[:, 3] *= np.float32(g)
    pcm[:, 6, 40 * HOP + 137:] *= np.float32(g)                # ... and an edge that is not hop-aligned
    ctx = _ctx(1)
    bins, rad, audio = _calls(ctx, pcm, [F, F])
    ctx.close()
    _against_oracle(bins, rad, audio, pcm, 0.95)


def test_a_state_blob_taken_between_two_calls_continues_with_the_same_bits():
    """the prediction is not part of the blob: a loaded context predicts bin -1, misses everywhere and produces the same audio"""
    F, A = 128, 2
    pcm = _stationary(2 * F, A, 9700)
    ctx = _ctx(A)
    b0, _, o0 = _calls(ctx, pcm, [F, F])
    ctx.close()
    ctx = _ctx(A)
    b1, _, o1 = _calls(ctx, pcm[:, :, :(F + 1) * HOP], [F])
    blob = ctx.state_save()
    ctx.close()
    ctx = _ctx(A)
    ctx.state_load(blob)
    b2, _, o2 = _calls(ctx, pcm[:, :, F * HOP:], [F])
    st = ctx.steer_stats()
    ctx.close()
    assert st["missed"] == A * F, st
    assert np.array_equal(np.concatenate([b1, b2], axis=1), b0)
    assert np.array_equal(np.concatenate([o1, o2], axis=1), o0)


def test_the_steering_kernels_do_not_move_beside_a_matrix_core_neighbour():
    """tests/test_gpu_coresidency.py's question for the fused analysis, the patch pass and the synthesis kernel"""
    path = os.path.join(ROOT, "tests", "cxx", "libneighbour.so")
    assert os.path.exists(path), "tests/cxx/libneighbour.so is missing: run __graft_entry__.build() (make -C tests/cxx)"
    nb = C.CDLL(path)
    nb.neighbour_launch.argtypes = [C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]
    dev = torch.device("cuda:0")
    F, A = 512, 9
    pcm = torch.from_numpy(np.concatenate([_stationary(F, A - 1, 9800), _moving(F, 9900)], axis=0)).to(dev)
    side = torch.cuda.Stream(device=dev)
    sink = torch.zeros(1024 * 256, dtype=torch.float32, device=dev)
    main = torch.cuda.current_stream().cuda_stream
    cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def run(with_neighbour):
        ctx = _ctx(A, api.SRP_ADAPTIVE)
        b = torch.empty(A, F, 1, dtype=torch.int32, device=dev); r = torch.empty(A, F, 1, dtype=torch.float32, device=dev)
        q = torch.empty(A, F, 1, dtype=torch.float32, device=dev); o = torch.zeros(A, 1, F * HOP, dtype=torch.float32, device=dev)
        ctx.process_frames_dev(pcm, F, b, r, q, None, o, stream=main)       # tables; the prediction of the second call
        torch.cuda.synchronize()
        if with_neighbour:
            assert nb.neighbour_launch(cus, 20000, C.c_void_p(sink.data_ptr()), C.c_void_p(side.cuda_stream)) == 0
        ctx.process_frames_dev(pcm, F, b, r, q, None, o, stream=main)
        still_running = with_neighbour and not side.query()
        torch.cuda.synchronize()
        res = (b.cpu().numpy().copy(), o.cpu().numpy().copy())
        st = ctx.steer_stats()
        ctx.close()
        return res, still_running, st

    ref, _, st = run(False)
    assert st["fused_calls"] == 2 and 0 < st["missed"] < 2 * A * F, st
    got, overlapped, _ = run(True)
    assert overlapped, "the neighbour had finished before the call did: nothing ran beside it"
    assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])
