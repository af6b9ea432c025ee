"""The steered tail of an ADAPTIVE call (DESIGN.md sections 0 and 4): the frames whose final pick is not the bin the analysis steered them at
are patched inside the second pick's launch (k_scan_repick<PL, true>) -- by the workgroup that re-picks their chunk when the chunk
holds a flagged frame, else from the miss list k_scan_pick leaves -- and no k_steer_patch is launched.

What is asked here: the audio equals the oracle's delay-and-sum stream at the GPU's own picks on every hop; picks and audio BITS are
those of the stand-alone patch kernel (a workspace budget too small to steer ahead sends every frame through it); the miss count is
exact; both roles of the launch really had frames to patch; calls fired back to back give what drained calls give."""
import os

import numpy as np
import pytest

from mcarray_amd import api, synth
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FS, N, HOP = 48000, 1024, 512
XS = synth.ULA8
CHUNK = 32                     # frames per chunk of the scan (SCAN_CHUNK)


# ---- helpers, as in tests/test_gpu_steer.py ----
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


def _ctx(A):
    return api.Context(FS, XS, N, 0.5, 1, srp_precision=api.SRP_ADAPTIVE, max_arrays=A, adaptive_fallback=False, adaptive_min_rows=64)


def _stationary(F, A, seed, base=23.0, step=-41.0):
    return np.stack([synth.noise_source_stream(XS, np.deg2rad(base + step * a), FS, (F + 1) * HOP, seed + a) for a in range(A)]).astype(np.float32)


def _moving(F, seed, every=5):
    """one array whose source jumps to another angle every few frames (hard cuts: the pick changes every few frames)"""
    rng = np.random.default_rng(seed)
    parts, n = [], 0
    while n < (F + 1) * HOP:
        ln = int(rng.integers(every - 2, every + 3)) * HOP
        parts.append(synth.noise_source_stream(XS, np.deg2rad(float(rng.uniform(-70, 70))), FS, ln, int(rng.integers(1 << 30))))
        n += ln
    return np.concatenate(parts, axis=1)[None, :, :(F + 1) * HOP].astype(np.float32)


def _against_oracle(bins, rad, audio, pcm):
    """EVERY hop against the oracle's delay-and-sum stream steered at the GPU's own picks: 2e-5 of the peak + 1e-7, the project's bar"""
    for a in range(pcm.shape[0]):
        assert np.isfinite(audio[a]).all()
        ref = po.das_stream(FS, N, XS, pcm[a].astype(np.float64), rad[a].astype(np.float64))
        err = float(np.abs(audio[a] - ref).max())
        print("array %d: audio error %.3e of the peak (%.3e)" % (a, err / np.abs(ref).max(), np.abs(ref).max()))
        assert err <= 2e-5 * np.abs(ref).max() + 1e-7, (a, err, np.abs(ref).max())


# ---- inputs and runs, each made once ----
def _steps(F, calls, seed, base):
    """one array whose source stands still inside a call of F frames and stands somewhere else in the next one: behind the first frames
    of a call every frame misses the predicted bin, and few frames are flagged"""
    parts = [synth.noise_source_stream(XS, np.deg2rad(base + 30.0 * ((i * 2) % 5 - 2)), FS, F * HOP, seed + i) for i in range(calls)]
    parts.append(synth.noise_source_stream(XS, np.deg2rad(base), FS, HOP, seed + calls))
    return np.concatenate(parts, axis=1)[None].astype(np.float32)


def _excursions(F, seed, home, call=256):
    """one array, _moving's hard cuts, whose source leaves its home angle for two to four frames every six to ten: every 32-frame chunk
    holds frames that miss, yet under a third of a call's frames do (the guard of the steered path stays quiet over any number of calls);
    the last twelve frames of every `call` frames are at home, where the next call's prediction then sits"""
    rng = np.random.default_rng(seed)
    parts = []
    for c0 in range(0, F + 1, call):
        left = min(call, F + 1 - c0)
        while left > 0:
            at_home = int(rng.integers(6, 11))
            away = int(rng.integers(2, 5))
            if left < at_home + away + 12:
                at_home, away = left, 0
            parts.append(synth.noise_source_stream(XS, np.deg2rad(home), FS, at_home * HOP, int(rng.integers(1 << 30))))
            if away:
                parts.append(synth.noise_source_stream(XS, np.deg2rad(float(rng.uniform(-70, 70))), FS, away * HOP, int(rng.integers(1 << 30))))
            left -= at_home + away
    return np.concatenate(parts, axis=1)[None, :, :(F + 1) * HOP].astype(np.float32)


_INPUTS, _RUNS = {}, {}


def _input(kind):
    if kind not in _INPUTS:
        if kind == "mixed":            # A = 3: two arrays whose source jumps every few frames, one stationary near end-fire; four calls of 256 frames
            _INPUTS[kind] = np.concatenate([_excursions(1024, 8101, 17.0), _excursions(1024, 8102, -38.0), _stationary(1024, 1, 8103, base=84.0)], axis=0)
        elif kind == "four":           # ... and a second stationary array: with four arrays no call of the ragged case fits one megabyte of Y
            _INPUTS[kind] = np.concatenate([_input("mixed")[:, :, :(461 + 1) * HOP], _stationary(461, 1, 8104, base=-52.0)], axis=0)
        elif kind == "nine":           # A = 9, calls of 64 frames: seven stationary arrays, two moving ones
            _INPUTS[kind] = np.concatenate([_stationary(192, 7, 8200, base=60.0, step=-19.0), _moving(192, 8207), _moving(192, 8208)], axis=0)
        elif kind == "cuts":           # the two moving arrays alone: every chunk misses, frames are flagged where the source jumps
            _INPUTS[kind] = np.concatenate([_moving(768, 8401), _moving(768, 8402)], axis=0)
        elif kind == "steps":          # two arrays that move between the calls only
            _INPUTS[kind] = np.concatenate([_steps(256, 3, 8300, 11.0), _steps(256, 3, 8310, -23.0)], axis=0)
    return _INPUTS[kind]


def _run(kind, sizes, drain=True, budget_mb=None):
    """(bins, rad, audio, steer_stats, repair_stats) of the calls `sizes` over the input `kind`; budget_mb: MCA_HIP_WS_MAX_MB"""
    key = (kind, tuple(sizes), drain, budget_mb)
    if key not in _RUNS:
        pcm = _input(kind)[:, :, :(sum(sizes) + 1) * HOP]
        old = os.environ.get("MCA_HIP_WS_MAX_MB")
        if budget_mb is not None:
            os.environ["MCA_HIP_WS_MAX_MB"] = str(budget_mb)
        try:
            ctx = _ctx(pcm.shape[0])
            res = _calls(ctx, pcm, sizes, drain)
            _RUNS[key] = res + (ctx.steer_stats(), ctx.repair_stats())
            ctx.close()
        finally:
            if budget_mb is not None:
                if old is None:
                    del os.environ["MCA_HIP_WS_MAX_MB"]
                else:
                    os.environ["MCA_HIP_WS_MAX_MB"] = old
    return _RUNS[key]


def _host_misses(bins, sizes):
    """per call and array: the frames whose pick is not the array's last pick of the call before (-1 before the first)"""
    n, t0 = 0, 0
    pred = np.full(bins.shape[0], -1)
    for Fi in sizes:
        part = bins[:, t0:t0 + Fi]
        n += int((part != pred[:, None]).sum())
        pred = part[:, -1].copy()
        t0 += Fi
    return n


def _chunk_misses(bins, sizes):
    """misses per (call, array, 32-frame chunk of the call), as one flat list"""
    out, t0 = [], 0
    pred = np.full(bins.shape[0], -1)
    for Fi in sizes:
        part = bins[:, t0:t0 + Fi]
        for a in range(bins.shape[0]):
            for c0 in range(0, Fi, CHUNK):
                out.append(int((part[a, c0:c0 + CHUNK] != pred[a]).sum()))
        pred = part[:, -1].copy()
        t0 += Fi
    return out


CASES = {"mixed": ("mixed", [256, 256, 256, 256]), "ragged": ("four", [256, 75, 130]), "nine": ("nine", [64, 64, 64])}


@pytest.mark.parametrize("case", list(CASES))
def test_every_hop_matches_the_oracle_at_the_picks(case):
    kind, sizes = CASES[case]
    bins, rad, audio, st, _ = _run(kind, sizes)
    assert st["fused_calls"] == len(sizes), st
    _against_oracle(bins, rad, audio, _input(kind)[:, :, :(sum(sizes) + 1) * HOP])


@pytest.mark.parametrize("case", list(CASES))
def test_the_bits_are_those_of_the_stand_alone_patch_kernel(case):
    """MCA_HIP_WS_MAX_MB = 1: Y does not hold a call, nothing steers ahead, k_steer_patch takes every frame in passes.  (One megabyte is
    252 rows of Y: 84 frames of three arrays, 63 of the ragged case's four, 28 of nine -- less than the shortest call of each case.)"""
    kind, sizes = CASES[case]
    b0, _, o0, s0, _ = _run(kind, sizes)
    b1, _, o1, s1, _ = _run(kind, sizes, budget_mb=1)
    assert min(sizes) > (1 << 20) // (b0.shape[0] * 520 * 8)    # rows of Y: 520 float2 words
    assert s0["fused_calls"] == len(sizes) and s1["fused_calls"] == 0 and s1["frames"] == s0["frames"], (s0, s1)
    assert s0["missed"] == s1["missed"], (s0, s1)
    assert np.array_equal(b0, b1)
    assert np.array_equal(o0, o1)


@pytest.mark.parametrize("case", list(CASES))
def test_the_miss_count_is_exact(case):
    kind, sizes = CASES[case]
    bins, _, _, st, _ = _run(kind, sizes)
    want = _host_misses(bins, sizes)
    print("missed", st["missed"], "of", st["frames"], "host", want)
    assert st["missed"] == want, (st, want)
    assert 0 < want < st["frames"]


def test_the_workgroup_that_re_picks_a_chunk_patched_frames():
    """every chunk holds a miss and some frame is flagged: the chunk of that frame is patched by the workgroup that re-picks it"""
    sizes = [256, 256, 256]
    bins, rad, audio, st, rs = _run("cuts", sizes)
    # (three calls at the most: the guard reads the report of the call two calls back, and the first call -- no prediction yet -- reports
    # no miss; a fourth call behind two that missed nearly everywhere would not steer ahead and would go through k_steer_patch)
    assert st["fused_calls"] == len(sizes), st
    per_chunk = _chunk_misses(bins, sizes)
    print("chunks", len(per_chunk), "fewest misses in a chunk", min(per_chunk), "flagged", rs["flagged"])
    assert min(per_chunk) >= 1
    assert rs["flagged"] > 0, rs
    assert st["missed"] == _host_misses(bins, sizes)
    _against_oracle(bins, rad, audio, _input("cuts"))


def test_the_workgroups_that_walk_the_miss_list_patched_frames():
    """every chunk holds a miss and fewer frames are flagged than there are chunks: a chunk without a flagged frame held misses, which
    only the miss list carries"""
    sizes = [256, 256, 256]
    bins, rad, audio, st, rs = _run("steps", sizes)
    assert st["fused_calls"] == len(sizes), st                   # (three calls at the most: see the test above)
    per_chunk = _chunk_misses(bins, sizes)
    print("chunks", len(per_chunk), "fewest misses in a chunk", min(per_chunk), "flagged", rs["flagged"])
    assert min(per_chunk) >= 1
    assert rs["flagged"] < len(per_chunk), (rs, len(per_chunk))
    assert st["missed"] == _host_misses(bins, sizes)
    _against_oracle(bins, rad, audio, _input("steps"))


def test_calls_fired_back_to_back_give_what_drained_calls_give():
    kind, sizes = CASES["mixed"]
    b0, r0, o0, s0, p0 = _run(kind, sizes)
    b1, r1, o1, s1, p1 = _run(kind, sizes, drain=False)
    assert s0 == s1, (s0, s1)
    assert p0["flagged"] == p1["flagged"], (p0, p1)
    assert np.array_equal(b0, b1) and np.array_equal(r0, r1) and np.array_equal(o0, o1)
