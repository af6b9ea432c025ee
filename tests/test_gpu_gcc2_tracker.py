"""GPU: the particle-filter DOA tracker of FreqGCCBinauralLocalisation (mca_hip_gcc2_tracker_attach, mca_hip_gcc2_tracked_frames_*,
the frame hook after attach, the C++ class with useParticleFilter) against its numpy restatement tests/gcc2_tracker_twin.py.

The definition ("The DOA tracker") has no transcendental function and no order-dependent sum that the twin does not
restate in the same order, so every comparison with the twin is on bits: the twin is fed the GPU's own smoothed rows, argmaxes and
gate flags, and doa / prob / fired / track of every frame and the particles at the end must be equal.  No frame is excluded."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import gcc2_tracker_twin as tw
from mcarray_amd import api, synth
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 3.0
STEP_F32 = np.float32(STEP * np.pi / 180.0)
XS44 = [0.0, 0.089]
SEED = 0x5EED0001
HOOK = 0xFFFFFFFF
BURSTS = [(60, 100), (110, 112), (215, 260), (300, 331)]       # the envelope of gated16k (tests/test_gpu_gcc2_probability.py)


def _signal(name, a=0):
    """array a of signal `name` -> fs, xs, N, use_power_floor, pcm float32 [2][(F+1)*hop], F.  a = 0 is the signal of that name in
    tests/test_gpu_gcc2_probability.py; other arrays have other angles and noise."""
    if name == "jump16k":
        fs, N, F = 16000, 1024, 150
        hop = N // 2
        L = (F + 1) * hop
        th0, th1 = [(-42.0, 25.0), (30.0, -10.0), (-60.0, 50.0)][a % 3]
        x = synth.noise_source_stream(synth.BINAURAL, np.deg2rad(th0), fs, L, 21 + 10 * a)
        y = synth.noise_source_stream(synth.BINAURAL, np.deg2rad(th1), fs, L, 22 + 10 * a)
        h = (F // 2) * hop
        return fs, synth.BINAURAL, N, False, np.concatenate([x[:, :h], y[:, h:]], axis=1), F
    if name == "gated16k":
        fs, N, F = 16000, 1024, 330
        hop = N // 2
        pcm = synth.noise_source_stream(synth.BINAURAL, np.deg2rad(30.0 - 25.0 * a), fs, (F + 1) * hop, 23 + 10 * a)
        env = np.full(F + 1, 0.01)
        for (b0, b1) in BURSTS:
            env[b0:b1] = 1.0
        return fs, synth.BINAURAL, N, True, (pcm * np.repeat(env, hop)[None, :]).astype(np.float32), F
    assert name == "ref44k"
    fs, N, F = 44100, 4096, 20
    return fs, XS44, N, False, synth.noise_source_stream(XS44, np.deg2rad(-20.0 + 15.0 * a), fs, (F + 1) * N // 2, 24 + 10 * a), F


def _batch(name, A):
    sig = [_signal(name, a) for a in range(A)]
    fs, xs, N, gated, _, F = sig[0]
    return fs, xs, N, gated, np.stack([s[4] for s in sig]), F


def _floor_from(fs, N):
    """the frame that completes the 3 s of floor estimation (BinauralLocalisation.cpp:387-404): the floor is known from it on"""
    return -(-int(3.0 * fs) // N) - 1


def _ctx(fs, xs, N, gated, max_arrays=1, **trk):
    ctx = api.Context(fs, xs, N, STEP, 1, gated, max_arrays=max_arrays)
    trk.setdefault("seed", SEED)
    ctx.gcc2_tracker_attach(**trk)
    return ctx


def _expected_fired_and_track(voiced, wtd):
    """the table of DESIGN.md from the gate flags alone (every silent frame here comes after the floor estimation or before any
    track): voiced frames fire 1; the first wtd frames of a gap after a voiced frame fire 2; a gap of more than wtd frames drops the
    track, and the next voiced frame starts a new one"""
    fired, track = np.zeros(len(voiced), dtype=np.int64), np.zeros(len(voiced), dtype=np.int64)
    alive, k, sil = False, 0, 0
    for t, v in enumerate(voiced):
        if v:
            if not alive:
                alive, k = True, k + 1
            fired[t], sil = 1, 0
        elif k > 0:
            if sil < wtd:
                fired[t] = 2 if alive else 0
            else:
                alive = False
            sil += 1
        track[t] = k
    return fired, track


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _twin_of(r, a, gated, fs, N, grid, **cfg):
    """the twin on the GPU's own rows / argmaxes / gate flags of array a"""
    F = r["doa"].shape[1]
    voiced = r["voiced"][a] if gated else np.ones(F, dtype=np.uint8)
    cfg.setdefault("seed", SEED)
    return tw.run(r["corr"][a].astype(np.float64), voiced, r["argmax"][a], _floor_from(fs, N), 3 * fs // (N // 2), grid, STEP_F32,
                  a_index=a, **cfg)


def _report(what, got, want):
    bad = np.flatnonzero(_bits(got) != _bits(want))
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    print("%s: %d of %d differ as bits, max |diff| %.3e, first at %s" % (what, len(bad), got.size, d.max() if d.size else 0.0, bad[:5]))
    return len(bad)


# ---------------------------------------------------------------------------------------------------------------------------
# 1: the stream call = the twin, exactly
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jump16k", "ref44k", "gated16k"])
def test_tracked_stream_call_is_the_twin_bit_for_bit(name):
    A = 3
    fs, xs, N, gated, pcm, F = _batch(name, A)
    ctx = _ctx(fs, xs, N, gated, max_arrays=A)
    grid = ctx.doa_grid()
    assert ctx.D == 61
    r = ctx.gcc2_tracked_frames_host(pcm, want_corr=True)
    n_bad = 0
    for a in range(A):
        t = _twin_of(r, a, gated, fs, N, grid)
        n_bad += _report("%s[%d] doa" % (name, a), r["doa"][a], t["doa"].astype(np.float32))
        n_bad += _report("%s[%d] prob" % (name, a), r["prob"][a], t["prob"].astype(np.float32))
        got = ctx.gcc2_tracker_particles(a)
        n_bad += _report("%s[%d] particles" % (name, a), got["particles"], t["particles"])
        print("fired", np.bincount(r["fired"][a], minlength=3), "tracks", int(r["track"][a].max()))
        assert np.array_equal(r["fired"][a], t["fired"]), (a, np.flatnonzero(r["fired"][a] != t["fired"])[:8])
        assert np.array_equal(r["track"][a], t["track"]), a
        assert got["alive"] == t["alive"] and got["track"] == t["track"][-1]
    assert n_bad == 0
    if gated:
        # two short gaps coast; the long one drops the track at its 94th frame; the burst after it starts track 2
        for a in range(A):
            v = r["voiced"][a] != 0
            assert _floor_from(fs, N) == 46 and not v[:47].any()
            ef, ek = _expected_fired_and_track(v, 93)
            assert np.array_equal(r["fired"][a], ef) and np.array_equal(r["track"][a], ek), a
            gaps = np.diff(np.flatnonzero(v)) - 1
            assert sorted(gaps[gaps > 0] > 93) == [False, False, True], gaps[gaps > 0]
            assert (ef == 2).sum() == gaps[(gaps > 0) & (gaps <= 93)].sum() + 93 and ek[-1] == 2
    else:
        assert (r["fired"] == 1).all() and (r["track"] == 1).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 2: the result does not depend on the shape of the calls
# ---------------------------------------------------------------------------------------------------------------------------
KEYS = ("doa", "prob", "fired", "track", "argmax")


def _same_outputs(ra, rb, a=slice(None), b=slice(None)):
    for k in KEYS:
        x, y = ra[k][a], rb[k][b]
        assert np.array_equal(_bits(x) if x.dtype.itemsize >= 4 else x, _bits(y) if y.dtype.itemsize >= 4 else y), k


def _cat(parts):
    return {k: np.concatenate([p[k] for p in parts], axis=1) for k in KEYS}


def test_one_call_three_calls_and_a_checkpoint_give_the_same_bits():
    A = 3
    fs, xs, N, gated, pcm, F = _batch("gated16k", A)
    hop = N // 2
    whole_ctx = _ctx(fs, xs, N, gated, max_arrays=A)
    whole = whole_ctx.gcc2_tracked_frames_host(pcm)
    # three calls with uneven cuts: inside the first burst, inside the long gap (the track is coasting), then the rest
    ctx = _ctx(fs, xs, N, gated, max_arrays=A)
    cuts = [0, 77, 170, F]
    parts = [ctx.gcc2_tracked_frames_host(pcm[:, :, c0 * hop:(c1 + 1) * hop]) for c0, c1 in zip(cuts[:-1], cuts[1:])]
    _same_outputs(_cat(parts), whole)
    for a in range(A):
        assert np.array_equal(_bits(ctx.gcc2_tracker_particles(a)["particles"]), _bits(whole_ctx.gcc2_tracker_particles(a)["particles"]))
    # state_save in the long gap -> state_load into a fresh tracked context -> continue
    c1 = _ctx(fs, xs, N, gated, max_arrays=A)
    k = 170
    assert (whole["fired"][0, k - 20:k] == 2).all()                     # the track is coasting there
    p0 = c1.gcc2_tracked_frames_host(pcm[:, :, :(k + 1) * hop])
    blob = c1.state_save()
    assert struct.unpack_from("<i", blob, 4)[0] == 4
    c2 = _ctx(fs, xs, N, gated, max_arrays=A)
    c2.state_load(blob)
    p1 = c2.gcc2_tracked_frames_host(pcm[:, :, k * hop:])
    _same_outputs(_cat([p0, p1]), whole)
    for a in range(A):
        assert np.array_equal(_bits(c2.gcc2_tracker_particles(a)["particles"]), _bits(whole_ctx.gcc2_tracker_particles(a)["particles"]))
    # a blob of another tracker configuration is refused before anything is loaded
    c3 = _ctx(fs, xs, N, gated, max_arrays=A, seed=SEED + 1)
    with pytest.raises(api.MCArrayHipError, match="different DOA tracker configuration"):
        c3.state_load(blob)


def test_an_array_alone_and_as_one_of_64_give_the_same_bits():
    fs, xs, N, gated, pcm, F = _batch("gated16k", 3)
    big = np.concatenate([pcm] + [pcm[(1 + i) % 3:(1 + i) % 3 + 1] * np.float32(1.0 + 0.01 * i) for i in range(61)], axis=0)
    assert big.shape[0] == 64
    r64 = _ctx(fs, xs, N, gated, max_arrays=64).gcc2_tracked_frames_host(big)
    r1 = _ctx(fs, xs, N, gated, max_arrays=1).gcc2_tracked_frames_host(pcm[:1])
    _same_outputs(r1, r64, slice(0, 1), slice(0, 1))
    assert (r64["fired"] == 2).any() and r64["track"].max() == 2


# ---------------------------------------------------------------------------------------------------------------------------
# 3: the frame hook after attach = the twin on the hook's own double rows; the C++ class with useParticleFilter
# ---------------------------------------------------------------------------------------------------------------------------
def _hook_run(ctx, X, fs, N, grid):
    """frame by frame: the hook's outputs and the twin's on the hook's own rows -> rows (t, degrees, prob, power) of the frames that
    fire by the twin, tracks per frame; asserts equality on every frame"""
    tr = tw.Tracker(grid, STEP_F32, HOOK, seed=SEED)
    f0, wtd = _floor_from(fs, N), 3 * fs // (N // 2)
    rows, tracks, kinds = [], [], np.zeros(3, dtype=int)
    for t in range(len(X)):
        r = ctx.gcc2_process_frame(X[t])
        fired = tr.voiced_frame(r["corr"], r["argmax"]) if r["fired"] == 1 else tr.silent_frame(t >= f0, wtd)
        assert r["fired"] == fired, (t, r["fired"], fired)
        assert struct.pack("<d", r["doa"]) == struct.pack("<d", tr.doa), (t, r["doa"], tr.doa)
        assert struct.pack("<d", r["prob"]) == struct.pack("<d", tr.prob), (t, r["prob"], tr.prob)
        assert r["track"] == tr.track, t
        kinds[fired] += 1
        tracks.append(tr.track)
        if fired:
            rows.append((t, (180 / np.pi) * tr.doa, tr.prob, r["power"]))
    got = ctx.gcc2_tracker_particles(-1)
    assert np.array_equal(_bits(got["particles"]), _bits(tr.x)) and got["alive"] == tr.alive
    return np.array(rows), np.array(tracks, dtype=np.float64), kinds


def test_frame_hook_is_the_twin_bit_for_bit():
    fs, xs, N, gated, pcm, F = _signal("gated16k")
    X = po.stft_frames(pcm.astype(np.float64), N)
    ctx = _ctx(fs, xs, N, gated)
    rows, tracks, kinds = _hook_run(ctx, X, fs, N, ctx.doa_grid())
    print("hook frames by fired value", kinds)
    assert kinds[1] > 100 and kinds[2] >= 93 + 20 and tracks[-1] == 2
    # reset forgets the track: the same frames again give the same outputs, track numbers from 1
    ctx.reset()
    rows2, tracks2, _ = _hook_run(ctx, X[:120], fs, N, ctx.doa_grid())
    assert np.array_equal(rows2, rows[rows[:, 0] < 120]) and tracks2.max() == 1


def test_cxx_class_with_particle_filter_end_to_end(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "test_gcc2_tracker"
    lib_dir = os.path.join(ROOT, "mcarray_amd")
    subprocess.check_call([cxx, "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "test_gcc2_tracker.cpp"), "-o", str(exe), "-L" + lib_dir, "-lmcarray_hip",
                           "-Wl,-rpath," + lib_dir], timeout=300)
    fs, xs, N, gated, pcm, F = _signal("gated16k")
    hop = N // 2
    X = po.stft_frames(pcm.astype(np.float64), N)
    pcm.astype(np.float64).tofile(str(tmp_path / "pcm.bin"))
    np.ascontiguousarray(X).tofile(str(tmp_path / "ccs.bin"))
    r = subprocess.run([str(exe), str(tmp_path), str((F + 1) * hop), str(F), str(SEED)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout + r.stderr
    # process(): the twin on the rows of the same stream through the Python binding (array 0 of a one-array context, as the class's)
    ctx = _ctx(fs, xs, N, gated)
    g = ctx.gcc2_tracked_frames_host(pcm[None], want_corr=True)
    t = _twin_of(g, 0, gated, fs, N, ctx.doa_grid())
    fr = np.flatnonzero(t["fired"])
    want = np.stack([fr.astype(np.float64), (180 / np.pi) * t["doa"][fr].astype(np.float32).astype(np.float64),
                     t["prob"][fr].astype(np.float32).astype(np.float64), g["power"][0, fr].astype(np.float64)], axis=1)
    got = np.fromfile(str(tmp_path / "cb_stream.bin")).reshape(-1, 4)
    assert (t["fired"] == 2).sum() >= 93 + 20
    assert got.shape == want.shape and np.array_equal(got, want), (got.shape, want.shape)
    assert np.array_equal(np.fromfile(str(tmp_path / "tracks_stream.bin")), t["track"].astype(np.float64))
    # processParametrisation: the twin on the hook's rows
    hctx = _ctx(fs, xs, N, gated)
    rows, tracks, _ = _hook_run(hctx, X, fs, N, hctx.doa_grid())
    got = np.fromfile(str(tmp_path / "cb_hook.bin")).reshape(-1, 4)
    assert got.shape == rows.shape and np.array_equal(got, rows), (got.shape, rows.shape)
    assert np.array_equal(np.fromfile(str(tmp_path / "tracks_hook.bin")), tracks)


# ---------------------------------------------------------------------------------------------------------------------------
# 4: it tracks (the thresholds of tests/test_gcc2_tracker_twin.py)
# ---------------------------------------------------------------------------------------------------------------------------
def test_it_tracks_the_jump_for_every_seed():
    from test_gcc2_tracker_twin import JUMP_L, SEEDS
    fs, xs, N, gated, pcm, F = _signal("jump16k")
    for seed in SEEDS:
        loc = api.FreqGCCBinauralLocalisation(fs, xs, gated, STEP, fft_size=N, particle_filter=dict(seed=seed))
        d = np.rad2deg(loc.process(pcm)["doa"][0].astype(np.float64))
        steady = d[30:75].mean()
        late = np.abs(d[75 + JUMP_L:] - 25.0).max()
        print("seed %d: mean of frames 30..74 %.3f deg, worst of frames %d.. %.3f deg off +25" % (seed, steady, 75 + JUMP_L, late))
        assert abs(steady + 42.0) <= 1.0, (seed, steady)
        assert late <= 3.0, (seed, late)


# ---------------------------------------------------------------------------------------------------------------------------
# 5: nothing else moved
# ---------------------------------------------------------------------------------------------------------------------------
def test_without_a_tracker_nothing_changes_and_misuse_is_refused():
    fs, xs, N, gated, pcm, F = _signal("gated16k")
    hop = N // 2
    plain = api.Context(fs, xs, N, STEP, 1, gated)
    D, H, na, S, MAXS = plain.D, hop, 1, 1, 4
    v3 = plain.state_save()
    old_size = 48 + na * D * 4 + na * S * H * 4 + na * 32 + 3 * na * MAXS * 4 + na * 4 + D * 8 + na * 8 + na * 4 + D * 8 + 64
    print("untracked blob: version", struct.unpack_from("<i", v3, 4)[0], "bytes", len(v3), "expected", old_size)
    assert struct.unpack_from("<i", v3, 4)[0] == 3 and len(v3) == old_size
    with pytest.raises(api.MCArrayHipError, match="no DOA tracker attached"):
        plain.gcc2_tracked_frames_host(pcm[None])
    ctx = _ctx(fs, xs, N, gated)
    v4 = ctx.state_save()
    assert struct.unpack_from("<i", v4, 4)[0] == 4 and len(v4) == old_size + 32 + 2 * (16 + 16 + 500 * 8)
    with pytest.raises(api.MCArrayHipError, match="mca_hip_gcc2_tracked_frames"):
        ctx.gcc2_frames_host(pcm[None])
    with pytest.raises(api.MCArrayHipError, match="already attached"):
        ctx.gcc2_tracker_attach(seed=1)
    with pytest.raises(api.MCArrayHipError, match="saved by a context with a DOA tracker"):
        plain.state_load(v4)
    c4 = api.Context(fs, synth.REEM_C, N, 5.0, 1, False)
    with pytest.raises(api.MCArrayHipError, match="n_mics == 2"):
        c4.gcc2_tracker_attach()
    for bad in (dict(n_particles=15), dict(n_particles=1025), dict(n_particles=64, n_inject=64), dict(n_inject=500), dict(n_inject=-2)):
        with pytest.raises(api.MCArrayHipError, match="n_particles|n_inject"):
            api.Context(fs, xs, N, STEP, 1, gated).gcc2_tracker_attach(**bad)
    # a version-3 blob of a stream in progress loads into a tracked context and leaves every track unstarted
    plain.gcc2_frames_host(pcm[None, :, :(100 + 1) * hop])
    ctx.gcc2_tracked_frames_host(pcm[None, :, :(100 + 1) * hop])
    assert ctx.gcc2_tracker_particles(0)["alive"]
    ctx.state_load(plain.state_save())
    p = ctx.gcc2_tracker_particles(0)
    assert not p["alive"] and p["track"] == 0 and not p["particles"].any()
    first = _ctx(fs, xs, N, gated).gcc2_tracked_frames_host(pcm[None])
    r = ctx.gcc2_tracked_frames_host(pcm[None, :, 100 * hop:])
    t1 = 100 + int(np.argmax(first["voiced"][0, 100:]))              # the first frame that fires after the cut starts track 1
    assert 100 < t1 < 112 and (r["track"][0, :t1 - 100] == 0).all() and (r["fired"][0, :t1 - 100] == 0).all() and r["track"][0, t1 - 100] == 1
    # mca_hip_reset forgets every track: the stream again from its start, track numbers from 1
    ctx.reset()
    again = ctx.gcc2_tracked_frames_host(pcm[None])
    _same_outputs(again, first)
    assert again["track"].max() == 2
    # other particle counts run (two register layouts: up to 512 and up to 1024 particles) and match the twin
    for n, inj in ((16, -1), (1024, 0)):
        c = _ctx(fs, xs, N, gated, n_particles=n, n_inject=inj)
        g = c.gcc2_tracked_frames_host(pcm[None], want_corr=True)
        t = _twin_of(g, 0, gated, fs, N, c.doa_grid(), n_particles=n, n_inject=inj)
        assert _report("N = %d doa" % n, g["doa"][0], t["doa"].astype(np.float32)) == 0
        assert np.array_equal(_bits(c.gcc2_tracker_particles(0)["particles"]), _bits(t["particles"]))
