"""GPU: soft nulls at the other look directions of an MVDR sources call (mca_hip_mvdr_set_null_gain; k_mvdr_solve_t<..., NULLS = true, ...>
of mvdr_solve.h) against the float64 twin of the dense definition (tests/mvdr_nulls_twin.py).

The bar is the one tests/test_gpu_mvdr.py sets for this solve: 5e-4 of the peak for spectra and audio, 5e-6 for the covariance.
tests/test_mvdr_nulls_twin.py shows that the nulled spectra differ from plain MVDR's by more than 0.1 of the peak on the scene
used here, so a kernel that ignores the gain cannot pass.  Measured on an MI355X, the worst case of each test over its streams, sources, calls and
parameters (spectra / audio, of the peak): every row-slot count 2.6e-4 / 2.7e-4 at gain 10 and 2.7e-4 / 2.8e-4 at gain 100 (the
worst cases are 13 and 16 microphones with four directions; 2 ... 11 microphones stay under 1.8e-4); N = 1024: 2.0e-4 / 2.1e-4;
N = 2048: 2.3e-4 / 1.6e-4; coincident directions 9.2e-5 / 5.9e-5; 64 streams of 4 microphones 2.3e-5 / 1.6e-5; the covariance
4.1e-7."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from mcarray_amd import api, synth

import mvdr_nulls_twin as nt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC_TOL, AUDIO_TOL, COV_TOL = 5e-4, 5e-4, 5e-6


def _irregular(M):
    return np.sort(np.random.default_rng(M).uniform(0.0, 0.04 * M, M))


def _check_against_twin(r, tw, a, what=""):
    """every source of stream a of the GPU result r against the twin's result tw"""
    worst = [0.0, 0.0]
    for s in range(tw["spec"].shape[0]):
        assert np.all(np.isfinite(r["spec"][a, s])) and np.all(np.isfinite(r["out"][a, s])), (what, a, s)
        es = np.abs(r["spec"][a, s] - tw["spec"][s]).max() / np.abs(tw["spec"][s]).max()
        ea = np.abs(r["out"][a, s] - tw["out"][s]).max() / np.abs(tw["out"][s]).max()
        print("%s stream %d source %d: spectra %.2e audio %.2e of the peak" % (what, a, s, es, ea))
        assert es <= SPEC_TOL, (what, a, s)
        assert ea <= AUDIO_TOL, (what, a, s)
        worst = [max(worst[0], es), max(worst[1], ea)]
    return worst


def _check_covariance(bf, tw, a):
    ec = np.abs(bf.covariance(a) - tw["phi"]).max() / np.abs(tw["phi"]).max()
    print("stream %d: covariance %.2e" % (a, ec))
    assert ec <= COV_TOL, a


def _two_calls_against_twin(xs, fs, N, F, A, S, gain, what):
    """a fresh context, two calls (the second continues the recursion and every source's overlap-add) against the twin"""
    hop = N // 2
    pcm = np.stack([nt.scene(xs, fs, N, 2 * F, a) for a in range(A)])
    doa = nt.drifting_doa(A, 2 * F, S)
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=gain)
    r1 = bf.process_sources(pcm[:, :, :(F + 1) * hop].copy(), doa[:, :F].copy())
    assert r1["out"].shape == (A, S, F * hop) and r1["spec"].shape == (A, S, F, N // 2 + 1)
    tws = []
    for a in range(A):
        tw = nt.mvdr_nulls_stream(fs, N, xs, pcm[a, :, :(F + 1) * hop].astype(np.float64), doa[a, :F], gain)
        _check_against_twin(r1, tw, a, what)
        _check_covariance(bf, tw, a)
        tws.append(tw)
    r2 = bf.process_sources(pcm[:, :, F * hop:].copy(), doa[:, F:].copy())
    for a in range(A):
        tw = nt.mvdr_nulls_stream(fs, N, xs, pcm[a, :, F * hop:].astype(np.float64), doa[a, F:], gain, state=tws[a])
        _check_against_twin(r2, tw, a, what + " second call")
        _check_covariance(bf, tw, a)
    bf.close()


@pytest.mark.parametrize("gain", [10.0, 100.0])
@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("M", [2, 3, 4, 5, 8, 11, 13, 16])
def test_nulls_every_row_slot_count(M, S, gain):
    """every number of row slots per lane with a full and a partly empty last slot, more directions than microphones (M = 2, 3),
    the register-tight instantiations (13 and 16 microphones with three and four directions); bin 0, where all directions
    coincide, is part of every spectrum"""
    _two_calls_against_twin(_irregular(M), 16000, 256, 6, 2, S, gain, "M %d S %d gain %g" % (M, S, gain))


@pytest.mark.parametrize("N,fs,F,S", [(1024, 48000, 6, 3), (2048, 96000, 4, 4)])
def test_nulls_long_frames(N, fs, F, S):
    _two_calls_against_twin(synth.ULA16, fs, N, F, 2, S, 100.0, "N %d" % N)


@pytest.mark.parametrize("gain", [10.0, 100.0])
@pytest.mark.parametrize("case", ["pair", "two_of_three"])
def test_nulls_coincident_directions(case, gain):
    fs, N, F, A = 48000, 256, 8, 2
    xs = synth.ULA8
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    doa = nt.drifting_doa(A, F, 3)
    if case == "pair":
        doa = np.ascontiguousarray(doa[:, :, [0, 0]])
        equal = (0, 1)
    else:
        doa = np.ascontiguousarray(doa[:, :, [0, 1, 0]])
        equal = (0, 2)
    S = doa.shape[2]
    r = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=gain).process_sources(pcm, doa)
    plain = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S).process_sources(pcm, doa)
    for a in range(A):
        tw = nt.mvdr_nulls_stream(fs, N, xs, pcm[a].astype(np.float64), doa[a], gain)
        _check_against_twin(r, tw, a, case)
    if case == "pair":
        # two equal directions and nothing else: each output is the plain MVDR output
        for s in equal:
            es = np.abs(r["spec"][:, s] - plain["spec"][:, s]).max() / np.abs(plain["spec"][:, s]).max()
            ea = np.abs(r["out"][:, s] - plain["out"][:, s]).max() / np.abs(plain["out"][:, s]).max()
            print("%s source %d against plain MVDR: spectra %.2e audio %.2e of the peak" % (case, s, es, ea))
            assert es <= SPEC_TOL and ea <= AUDIO_TOL, s
    # the equal pair gives equal outputs (each nulls the same third direction, and its twin not at all)
    es = np.abs(r["spec"][:, equal[0]] - r["spec"][:, equal[1]]).max() / np.abs(r["spec"][:, equal[0]]).max()
    print("%s: the equal pair differs by %.2e of the peak" % (case, es))
    assert es <= SPEC_TOL


def test_nulls_duplicate_of_the_own_direction_changes_nothing():
    """three directions of which two are equal: the equal pair's outputs are what plain MVDR nulling the third direction alone
    gives, i.e. the two-direction nulling call without the duplicate"""
    fs, N, F, A, gain = 48000, 256, 8, 2, 100.0
    xs = synth.ULA8
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    doa3 = np.ascontiguousarray(nt.drifting_doa(A, F, 2)[:, :, [0, 1, 0]])
    r3 = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=3, null_gain=gain).process_sources(pcm, doa3)
    r2 = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=2, null_gain=gain).process_sources(pcm, doa3[:, :, :2].copy())
    for s in (0, 2):
        es = np.abs(r3["spec"][:, s] - r2["spec"][:, 0]).max() / np.abs(r2["spec"][:, 0]).max()
        print("source %d of three against source 0 of two: %.2e of the peak" % (s, es))
        assert es <= SPEC_TOL


@pytest.mark.parametrize("geo", ["ula16", "m13", "five"])
def test_nulls_byte_identities(geo):
    # (four directions on 16 microphones: the instantiation with two passes through the column loop)
    xs, fs, N, F, S = {"ula16": (synth.ULA16, 48000, 256, 7, 4), "m13": (_irregular(13), 16000, 256, 6, 3),
                       "five": ([0.0, 0.03, 0.07, 0.10, 0.20], 8000, 256, 9, 2)}[geo]
    A = 3
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    pcm[2] = pcm[0] * np.float32(1e-18)       # the covariance trace stays under 1e-30: the w = d/M branch per direction
    doa = nt.drifting_doa(A, F, S)
    never = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S)
    plain = never.process_sources(pcm, doa)
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=100.0)
    assert bf.get_null_gain() == 100.0 and never.get_null_gain() == 0.0
    r = bf.process_sources(pcm, doa)
    assert not np.array_equal(r["spec"][:2], plain["spec"][:2])
    # the covariance a call leaves does not depend on the gain
    for a in range(A):
        assert np.array_equal(bf.covariance(a), never.covariance(a)), a
    # silence: w = d/M per direction, the bytes of the plain sources call
    assert np.abs(r["out"][2]).max() > 0.0
    assert np.array_equal(r["spec"][2].view(np.float32), plain["spec"][2].view(np.float32)) and np.array_equal(r["out"][2], plain["out"][2])
    # gain 0 is the plain sources call
    bf.reset()
    bf.set_null_gain(0.0)
    z = bf.process_sources(pcm, doa)
    assert np.array_equal(z["spec"].view(np.float32), plain["spec"].view(np.float32)) and np.array_equal(z["out"], plain["out"])
    # one direction under a gain is the single-look path, through both entry points
    bf.reset()
    bf.set_null_gain(100.0)
    one = api.MvdrBeamformer(fs, xs, N, max_streams=A).process(pcm, doa[:, :, 1].copy(), want_spec=True)
    q = bf.process_sources(pcm, doa[:, :, 1:2].copy())
    assert np.array_equal(q["spec"][:, 0].view(np.float32), one["spec"].view(np.float32)) and np.array_equal(q["out"][:, 0], one["out"])
    bf.reset()
    q = bf.process(pcm, doa[:, :, 1].copy(), want_spec=True)
    assert np.array_equal(q["spec"].view(np.float32), one["spec"].view(np.float32)) and np.array_equal(q["out"], one["out"])
    # reset, then the same call: the same bytes
    bf.reset()
    again = bf.process_sources(pcm, doa)
    assert np.array_equal(again["spec"].view(np.float32), r["spec"].view(np.float32)) and np.array_equal(again["out"], r["out"])


@pytest.mark.parametrize("S", [3, 4])
def test_nulls_chunked_calls_equal_one_call(S):
    fs, N, F = 48000, 256, 48
    xs = synth.ULA16
    pcm = nt.scene(xs, fs, N, F, 0)[None]
    doa = nt.drifting_doa(1, F, S)
    one = api.MvdrBeamformer(fs, xs, N, max_sources=S, null_gain=100.0).process_sources(pcm, doa)
    bf = api.MvdrBeamformer(fs, xs, N, max_sources=S, null_gain=100.0)
    hop = N // 2
    outs, specs = [], []
    for (t0, t1) in [(0, 1), (1, 18), (18, 19), (19, 48)]:
        r = bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop], doa[:, t0:t1])
        outs.append(r["out"]); specs.append(r["spec"])
    assert np.array_equal(np.concatenate(specs, axis=2), one["spec"])
    assert np.array_equal(np.concatenate(outs, axis=2), one["out"])


def test_nulls_tail_workgroups_cut_along_the_frames():
    """64 streams x 513 bins = 513 solve workgroups: the one behind the last whole round goes in a second launch cut along the
    frames (api_mvdr.hip), over two calls"""
    fs, N, F, A, S, gain = 16000, 1024, 10, 64, 2, 100.0
    xs = synth.REEM_C
    base = np.stack([nt.scene(xs, fs, N, 2 * F, a) for a in range(3)])
    pick = np.arange(A) % 3
    pcm = base[pick]
    doa = nt.drifting_doa(3, 2 * F, S)[pick]
    hop = N // 2
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=gain)
    r1 = bf.process_sources(pcm[:, :, :(F + 1) * hop].copy(), doa[:, :F].copy())
    r2 = bf.process_sources(pcm[:, :, F * hop:].copy(), doa[:, F:].copy())
    r = dict(spec=np.concatenate([r1["spec"], r2["spec"]], axis=2), out=np.concatenate([r1["out"], r2["out"]], axis=2))
    tws = {}
    for a in (0, 31, 63):
        if pick[a] not in tws:
            tws[pick[a]] = nt.mvdr_nulls_stream(fs, N, xs, pcm[a].astype(np.float64), doa[a], gain)
        _check_against_twin(r, tws[pick[a]], a, "64 streams")
        _check_covariance(bf, tws[pick[a]], a)
    # streams with the same input give the same bytes wherever they sit in the batch (stream 63 is the one in the tail launch)
    assert np.array_equal(r["spec"][0], r["spec"][3]) and np.array_equal(r["out"][1], r["out"][61])
    assert np.array_equal(r["spec"][0], r["spec"][63]) and np.array_equal(r["out"][0], r["out"][63])
    assert np.array_equal(bf.covariance(0), bf.covariance(63))


def test_nulls_state_blobs():
    fs, N, F, S = 16000, 256, 30, 4
    hop = N // 2
    xs = synth.REEM_C
    pcm = nt.scene(xs, fs, N, F, 0)[None]
    doa = nt.drifting_doa(1, F, S)
    one = api.MvdrBeamformer(fs, xs, N, max_sources=S, null_gain=100.0).process_sources(pcm, doa)
    b, c = api.MvdrBeamformer(fs, xs, N, max_sources=S, null_gain=100.0), api.MvdrBeamformer(fs, xs, N, max_sources=S, null_gain=100.0)
    plain = api.MvdrBeamformer(fs, xs, N, max_sources=S)
    size = lambda bf: bf._lib.mca_hip_mvdr_state_size(bf.h)
    assert size(b) == size(plain)
    first = b.process_sources(pcm[:, :, :(11 + 1) * hop], doa[:, :11])
    blob = b.state_save()
    assert len(blob) == size(plain) == len(plain.state_save())
    c.state_load(blob)
    rest = c.process_sources(pcm[:, :, 11 * hop:], doa[:, 11:])
    assert np.array_equal(np.concatenate([first["out"], rest["out"]], axis=2), one["out"])
    assert np.array_equal(np.concatenate([first["spec"], rest["spec"]], axis=2), one["spec"])
    # the gain is no part of the blob: it loads into a context with gain 0, which goes on from that covariance as a plain context
    # does (the spectra do not depend on the overlap-add tails, the audio past the first hop neither) ...
    plain.process_sources(pcm[:, :, :(11 + 1) * hop], doa[:, :11])
    other = api.MvdrBeamformer(fs, xs, N, max_sources=S)
    other.state_load(blob)
    assert other.get_null_gain() == 0.0
    assert np.array_equal(other.covariance(0), b.covariance(0))
    p2a, p2b = plain.process_sources(pcm[:, :, 11 * hop:], doa[:, 11:]), other.process_sources(pcm[:, :, 11 * hop:], doa[:, 11:])
    assert np.array_equal(p2a["spec"], p2b["spec"]) and np.array_equal(p2a["out"][:, :, hop:], p2b["out"][:, :, hop:])
    # ... and, given the gain, as the context that saved it
    other.state_load(blob)
    other.set_null_gain(100.0)
    again = other.process_sources(pcm[:, :, 11 * hop:], doa[:, 11:])
    assert np.array_equal(again["out"], rest["out"]) and np.array_equal(again["spec"], rest["spec"])


def test_nulls_reject_bad_gains():
    fs, N = 16000, 256
    xs = synth.REEM_C
    pcm = nt.scene(xs, fs, N, 4, 0)[None]
    doa = nt.drifting_doa(1, 4, 2)
    for bad in (-1.0, float("nan"), float("inf"), 1001.0):
        with pytest.raises(api.MCArrayHipError, match=r"\[0,1000\]"):
            api.MvdrBeamformer(fs, xs, N, max_sources=2, null_gain=bad)
    bf = api.MvdrBeamformer(fs, xs, N, max_sources=2, null_gain=10.0)
    before = bf.process_sources(pcm, doa)
    for bad in (-1.0, float("nan"), float("inf"), 1001.0):
        with pytest.raises(api.MCArrayHipError, match=r"\[0,1000\]"):
            bf.set_null_gain(bad)
    assert bf.get_null_gain() == 10.0 and bf.null_gain == 10.0
    bf.reset()
    after = bf.process_sources(pcm, doa)                                      # the context is still usable, the gain as it was
    assert np.array_equal(after["out"], before["out"])
    bf.set_null_gain(1000.0)
    bf.reset()
    r = bf.process_sources(pcm, doa)
    assert np.all(np.isfinite(r["out"])) and not np.array_equal(r["out"], before["out"])


def test_localise_two_sources_then_nulls_16_microphones():
    """the 16-microphone localiser writes doa_rad [A][F][2] on the device and the nulling call consumes that tensor as it is"""
    import torch
    fs, N, F, A, S, gain = 48000, 1024, 16, 3, 2, 100.0
    xs = synth.ULA16
    hop = N // 2
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    dev = torch.device("cuda:0")
    t_pcm = torch.from_numpy(pcm).to(dev)
    loc = api.Context(fs, xs, N, 0.5, S, max_arrays=A)
    t_bin = torch.empty((A, F, S), dtype=torch.int32, device=dev)
    t_doa = torch.empty((A, F, S), dtype=torch.float32, device=dev)
    t_prob = torch.empty((A, F, S), dtype=torch.float32, device=dev)
    loc.process_frames_dev(t_pcm, F, t_bin, t_doa, t_prob, localise=True, separate=False)
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=gain)
    t_out = torch.empty((A, S, F * hop), dtype=torch.float32, device=dev)
    t_spec = torch.empty((A, S, F, N // 2 + 1, 2), dtype=torch.float32, device=dev)
    bf.process_sources_dev(t_pcm, F, t_doa, out_pcm=t_out, out_spec=t_spec)
    torch.cuda.synchronize()
    doa, spec = t_doa.cpu().numpy(), t_spec.cpu().numpy()
    r = dict(out=t_out.cpu().numpy(), spec=spec[..., 0] + 1j * spec[..., 1])
    for a in range(A):
        tw = nt.mvdr_nulls_stream(fs, N, xs, pcm[a].astype(np.float64), doa[a], gain)
        _check_against_twin(r, tw, a, "localiser chain")


def test_cxx_class_nulls(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "test_mvdr_nulls"
    lib_dir = os.path.join(ROOT, "mcarray_amd")
    subprocess.check_call([cxx, "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "test_mvdr_nulls.cpp"), "-o", str(exe), "-L" + lib_dir,
                           "-lmcarray_hip", "-Wl,-rpath," + lib_dir], timeout=300)
    fs, N, M, S, F, g0, g1 = 16000, 512, 6, 3, 30, 100.0, 10.0
    hop = N // 2
    xs = [0.035 * m for m in range(M)]                         # the array of the C++ program
    pcm = nt.scene(xs, fs, N, F, 0)
    pcm.tofile(str(tmp_path / "pcm.f32"))
    r = subprocess.run([str(exe), str(tmp_path / "pcm.f32"), str(tmp_path / "out.f32"), str(fs), str(N), str(M), str(S), str(g0), str(g1)],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL PASSED" in r.stdout
    k = int([ln for ln in r.stdout.splitlines() if ln.startswith("switch_frame")][0].split()[1])
    assert 0 < k < F
    out = np.fromfile(str(tmp_path / "out.f32"), dtype=np.float32).reshape(S, F * hop)
    doa = np.empty((1, F, S), dtype=np.float32)
    doa[0] = np.array([0.35, -0.6, 1.1, -0.1])[:S]             # as in the C++ program
    bf = api.MvdrBeamformer(fs, xs, N, max_sources=S, null_gain=g0)
    a = bf.process_sources(pcm[None, :, :(k + 1) * hop], doa[:, :k])["out"][0]
    bf.set_null_gain(g1)
    b = bf.process_sources(pcm[None, :, k * hop:], doa[:, k:])["out"][0]
    assert np.array_equal(out, np.concatenate([a, b], axis=1))
    plain = api.MvdrBeamformer(fs, xs, N, max_sources=S).process_sources(pcm[None], doa)["out"][0]
    assert not np.array_equal(out[:, k * hop:], plain[:, k * hop:])
