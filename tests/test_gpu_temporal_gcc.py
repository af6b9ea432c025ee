"""GPU: TemporalGCCBinauralLocalisation (mca_hip_tgcc_*) against the numpy restatement tests/tgcc_twin.py on every frame:
stream parity at three geometries with the gate on and off, bit-identical results across call splits / batch positions /
state blobs, a muted channel, the per-frame hook, and the C++ module API on the reference test's five recordings."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tgcc_twin as tt
from mcarray_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR_TIE = 1e-9


def _module(fs, d, gate, max_arrays=1):
    return api.TemporalGCCBinauralLocalisation(fs, [0.0, d], use_power_floor=gate, max_arrays=max_arrays)


def _compare(res, a, pcm, fs, d, gate, label):
    """library outputs of array a vs the twin on every frame; returns the number of voiced frames and allowed pick differences."""
    free = tt.run_stream(pcm, fs, d, gate)
    k_gpu = res["delay_idx"][a].astype(int)
    assert np.array_equal(res["voiced"][a].astype(bool), free["voiced"]), label
    diff = np.nonzero(k_gpu != free["k"])[0]
    for f in diff:
        assert free["voiced"][f] and free["gap"][f] < NEAR_TIE, (label, f, k_gpu[f], free["k"][f], free["gap"][f])
    nv = int(free["voiced"].sum())
    assert len(diff) <= 0.01 * nv, (label, len(diff), nv)
    forced = np.where(k_gpu != free["k"], k_gpu, -1)
    tw = tt.run_stream(pcm, fs, d, gate, forced=forced) if len(diff) else free
    e_ix = np.abs(res["index"][a] - tw["index"]).max()
    e_doa = np.abs(res["doa"][a].astype(np.float64) - tw["doa"]).max()
    e_prob = np.abs(res["prob"][a].astype(np.float64) - tw["prob"]).max()
    e_pow = (np.abs(res["power"][a].astype(np.float64) - tw["power"]) / np.maximum(np.abs(tw["power"]), 1.0)).max()
    print("%s: %d frames, %d voiced, %d pick differences; |index| %.3g, |doa| %.3g deg, |prob| %.3g, power rel %.3g"
          % (label, len(k_gpu), nv, len(diff), e_ix, e_doa, e_prob, e_pow))
    assert e_ix <= 1e-10, label
    assert e_doa <= 1e-5, label
    assert e_prob <= 1e-6, label
    assert e_pow <= 1e-6, label
    return nv, len(diff)


@pytest.mark.parametrize("gate", [True, False])
@pytest.mark.parametrize("fs, d", tt.PARITY_CONFIGS)
def test_stream_parity(fs, d, gate):
    pcm = tt.parity_streams(fs, d, gate)
    m = _module(fs, d, gate, max_arrays=len(pcm))
    W, hop, nd = tt.geometry(fs, d)
    assert (m.W, m.hop, m.nd) == (W, hop, nd)
    F = (pcm.shape[2] - W) // hop + 1
    res = m.process(pcm[:, :, :(F - 1) * hop + W].astype(np.float32), want_index=True)
    for a in range(len(pcm)):
        _compare(res, a, pcm[a, :, :(F - 1) * hop + W], fs, d, gate, "fs %d d %g gate %d stream %d" % (fs, d, gate, a))


def _concat(parts):
    return {k: (np.concatenate([p[k] for p in parts], axis=1) if parts[0][k] is not None else None) for k in parts[0]}


def _bits_equal(x, y, keys=("doa", "prob", "voiced", "power", "delay_idx", "index")):
    for k in keys:
        assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape, k
        assert x[k].tobytes() == y[k].tobytes(), k


def _call_cuts(pcm, m, cuts, want_index=True):
    """runs frames [0, F) of pcm [A][2][T] through module m in calls of len(cut) frames each."""
    parts, f0 = [], 0
    for n in cuts:
        seg = pcm[:, :, f0 * m.hop:(f0 + n - 1) * m.hop + m.W]
        parts.append(m.process(seg, want_index=want_index))
        f0 += n
    return _concat(parts)


def test_bits_across_call_splits_batches_and_state_blobs():
    fs, d = 44100, 0.086
    W, hop, nd = tt.geometry(fs, d)
    x0, others = tt.bits_streams(fs, d)
    x = x0.astype(np.float32)[None]
    F = (x.shape[2] - W) // hop + 1
    whole = _call_cuts(x, _module(fs, d, True), [F])
    cuts = [1, 7, 12, 19, 20]
    cuts.append(F - sum(cuts))
    assert cuts[-1] > 0 and sum(cuts[:3]) == 20       # one split right after the last floor-estimation frame
    _bits_equal(whole, _call_cuts(x, _module(fs, d, True), cuts))

    # the stream inside a batch of 64 others
    batch = others.astype(np.float32)
    pos = 37
    batch[pos] = x[0]
    inb = _call_cuts(batch, _module(fs, d, True, max_arrays=64), [F])
    _bits_equal(whole, {k: (v[pos:pos + 1] if v is not None else None) for k, v in inb.items()})

    # a state blob saved after the first part and loaded into a new module
    m1 = _module(fs, d, True)
    first = _call_cuts(x, m1, [25])
    blob = m1.state_save()
    rest = x[:, :, 25 * hop:]
    m2 = _module(fs, d, True)
    m2.state_load(blob)
    second = _call_cuts(rest, m2, [F - 25])
    _bits_equal(whole, _concat([first, second]))


def test_muted_channel():
    """channel 1 exact zeros: every correlation is 0, stddev(R_i) = 0, the division is skipped, index = tri / 0.1."""
    fs, d = 44100, 0.086
    pcm = tt.muted_stream(fs, d)
    W, hop, nd = tt.geometry(fs, d)
    F = (pcm.shape[1] - W) // hop + 1
    pcm = pcm[:, :(F - 1) * hop + W]
    m = _module(fs, d, False)
    res = m.process(pcm.astype(np.float32)[None], want_index=True)
    _compare(res, 0, pcm, fs, d, False, "muted")
    assert np.array_equal(res["index"][0], np.tile(tt.triangle(nd) / 0.1, (F, 1)))
    assert (res["delay_idx"][0] == nd // 2).all()


def test_frame_hook_matches_the_twin():
    """processParametrisation on double frames: doa, prob and power <= 1e-9 absolute, index <= 1e-10 (the frame-API bar)."""
    fs, d = 44100, 0.086
    pcm = tt.hook_stream(fs, d)
    m = _module(fs, d, True)
    tw = tt.Twin(fs, d, True)
    worst = dict(doa=0.0, prob=0.0, power=0.0, index=0.0)
    nv = 0
    for f, (L, R) in enumerate(tt.frames_of(pcm, m.W, m.hop)):
        g = m.process_frame(L, R)
        k_free, _, _, _, gap = tt.frame_result(L, R, m.nd)
        forced = None
        if g["voiced"] and g["delay_idx"] != k_free:
            assert gap < NEAR_TIE, (f, g["delay_idx"], k_free, gap)
            forced = g["delay_idx"]
        t = tw.frame(L, R, forced)
        assert g["voiced"] == t["voiced"], f
        assert g["delay_idx"] == t["k"], f
        nv += int(t["voiced"])
        for k in ("doa", "prob", "power"):
            worst[k] = max(worst[k], abs(g[k] - t[k]))
        worst["index"] = max(worst["index"], np.abs(g["index"] - t["index"]).max())
    print("frame hook: %d frames, %d voiced, worst %s" % (f + 1, nv, worst))
    assert nv > 10
    assert worst["doa"] <= 1e-9 and worst["prob"] <= 1e-9 and worst["power"] <= 1e-9
    assert worst["index"] <= 1e-10


def test_cxx_reference_property_end_to_end(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "test_temporal_gcc"
    lib_dir = os.path.join(ROOT, "mcarray_amd")
    subprocess.check_call([cxx, "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "test_temporal_gcc.cpp"), "-o", str(exe), "-L" + lib_dir, "-lmcarray_hip",
                           "-Wl,-rpath," + lib_dir], timeout=300)
    for name, pcm, _ in tt.reference_recordings():
        pcm.T.astype(np.int16).tofile(str(tmp_path / (name + ".raw")))      # interleaved
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL PASSED" in r.stdout
