"""GPU: several look directions per frame through one MVDR analysis, covariance recursion and factorisation
(mca_hip_mvdr_set_max_sources, mca_hip_mvdr_sources_frames_*; k_mvdr_solve_t of mvdr_solve.h).

Nothing new is defined numerically: output s of a call is what the single-look call gives on the same stream state with
doa[:, :, s], and the covariance afterwards is what any of those calls leaves.  So the oracle for output s is
oracle.pyoracle.MVDR(...).stream(pcm, doa[:, s]) at the tolerances of tests/test_gpu_mvdr.py for this solve (5e-4 of the call's
peak for spectra and audio, 5e-6 for the covariance), and against the single-look GPU path the comparison is of bytes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from mcarray_amd import api, synth
from oracle import pyoracle as po
from parity_helpers import assert_bins

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC_TOL, AUDIO_TOL, COV_TOL = 5e-4, 5e-4, 5e-6
OFFSETS = np.array([0.0, -0.5, 0.45, -0.8])           # look direction of source s relative to source 0 (radians)


def _scene(xs, fs, N, F, a):
    n = (F + 1) * N // 2
    return (synth.noise_source_stream(xs, np.deg2rad(20.0 - 30 * a), fs, n, 5 + a)
            + synth.noise_source_stream(xs, np.deg2rad(-50.0 + 40 * a), fs, n, 15 + a, snr_db=60)).astype(np.float32)


def _ospec(o):
    return o["spec"][:, 0::2] + 1j * o["spec"][:, 1::2]


def _drifting_doa(A, F, S):
    """[A][F][S]: drifts per frame, differs per source and per stream"""
    return (np.deg2rad(20.0 - 30 * np.arange(A))[:, None, None] + 0.01 * np.arange(F)[None, :, None]
            + OFFSETS[None, None, :S]).astype(np.float32)


def _check_against_oracle(r, og, pcm_a, doa_a, a, skip_first_hop=False):
    """every source of stream a against an oracle run of its own (all continue from copies of the same oracle state: the
    covariance does not depend on the look direction, so one oracle per source, fed the same stream, holds that state)"""
    S = doa_a.shape[1]
    for s in range(S):
        o = og[s].stream(pcm_a.astype(np.float64), doa_a[:, s].astype(np.float64), want_spec=True)
        sp = _ospec(o)
        es = np.abs(r["spec"][a, s] - sp).max() / np.abs(sp).max()
        h = r["out"].shape[2] // doa_a.shape[0] if skip_first_hop else 0
        ea = np.abs(r["out"][a, s, h:] - o["out"][h:]).max() / np.abs(o["out"]).max()
        print("stream %d source %d: spectra %.2e audio %.2e of the peak" % (a, s, es, ea))
        assert es <= SPEC_TOL, (a, s)
        assert ea <= AUDIO_TOL, (a, s)


GEOMETRIES = [
    (synth.ULA16, 48000, 1024, 24),       # BASELINE configs[3] geometry
    (synth.ULA8, 48000, 1024, 20),
    (synth.REEM_C, 16000, 512, 20),       # the reference's 4-microphone test array
    (synth.BINAURAL, 16000, 1024, 12),
    ([0.0, 0.03, 0.07, 0.10, 0.20], 8000, 256, 30),
    (synth.ULA16, 96000, 2048, 5),
]


@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("xs,fs,N,F", GEOMETRIES)
def test_sources_stream_matches_oracle(xs, fs, N, F, S):
    A = 3
    pcm = np.stack([_scene(xs, fs, N, F, a) for a in range(A)])
    doa = _drifting_doa(A, F, S)
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S)
    r = bf.process_sources(pcm, doa)
    assert r["out"].shape == (A, S, F * (N // 2)) and r["spec"].shape == (A, S, F, N // 2 + 1)
    ogs = []
    for a in range(A):
        og = [po.MVDR(fs, N, xs) for _ in range(S)]
        _check_against_oracle(r, og, pcm[a], doa[a], a)
        ec = np.abs(bf.covariance(a) - og[0].covariance()).max() / np.abs(og[0].covariance()).max()
        print("stream %d: covariance %.2e" % (a, ec))
        assert ec <= COV_TOL, a
        ogs.append(og)
    # a second call continues the recursion and every source's overlap-add (the oracle's stream() restarts its overlap-add
    # tail per call; the GPU carries it: audio is compared past the first hop)
    doa2 = doa[:, ::-1].copy()
    r2 = bf.process_sources(pcm, doa2)
    _check_against_oracle(r2, ogs[1], pcm[1], doa2[1], 1, skip_first_hop=True)
    assert np.abs(bf.covariance(1) - ogs[1][0].covariance()).max() <= COV_TOL * np.abs(ogs[1][0].covariance()).max()


def _irregular(M):
    return np.sort(np.random.default_rng(M).uniform(0.0, 0.04 * M, M))


@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("geo", ["ula16_1024", "m13_1024", "reemc_512", "five_256", "ula8_2048", "m3_256", "m11_512"])
def test_sources_have_the_bytes_of_the_single_look_path(geo, S):
    xs, fs, N, F = {"ula16_1024": (synth.ULA16, 48000, 1024, 7), "m13_1024": (_irregular(13), 48000, 1024, 6),
                    "reemc_512": (synth.REEM_C, 16000, 512, 9), "five_256": ([0.0, 0.03, 0.07, 0.10, 0.20], 8000, 256, 11),
                    "ula8_2048": (synth.ULA8, 96000, 2048, 4),
                    # with five_256 and m13_1024: a partly empty last row slot at every number of row slots per lane (1 ... 4)
                    "m3_256": (_irregular(3), 8000, 256, 11), "m11_512": (_irregular(11), 16000, 512, 7)}[geo]
    A = 3
    pcm = np.stack([_scene(xs, fs, N, F, a) for a in range(A)])
    pcm[2] = pcm[0] * np.float32(1e-18)       # the covariance trace stays under 1e-30: the w = d/M branch, per source, with an output
    rng = np.random.default_rng(S)
    doa = rng.uniform(-1.4, 1.4, (A, F, S)).astype(np.float32)
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S)
    r = bf.process_sources(pcm, doa)
    assert np.abs(r["out"][2]).max() > 0.0
    cov = [bf.covariance(a) for a in range(A)]
    for s in range(S):
        one = api.MvdrBeamformer(fs, xs, N, max_streams=A)
        q = one.process(pcm, doa[:, :, s].copy(), want_spec=True)
        assert np.array_equal(r["spec"][:, s].view(np.float32), q["spec"].view(np.float32)), s
        assert np.array_equal(r["out"][:, s], q["out"]), s
        for a in range(A):
            assert np.array_equal(one.covariance(a), cov[a]), (s, a)
    # output s does not change when the other columns change ...
    other = doa.copy()
    other[:, :, 1:] = rng.uniform(-1.4, 1.4, (A, F, S - 1)).astype(np.float32)
    r2 = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S).process_sources(pcm, other)
    assert np.array_equal(r2["out"][:, 0], r["out"][:, 0]) and np.array_equal(r2["spec"][:, 0], r["spec"][:, 0])
    assert not np.array_equal(r2["out"][:, 1], r["out"][:, 1])
    # ... nor when S changes (a context with a larger maximum, fewer sources in the call; n_sources = 1 through the new entry)
    big = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=4)
    for S2 in (1, 2, 4):
        if S2 == S:
            continue
        d2 = np.ascontiguousarray(np.concatenate([doa, doa], axis=2)[:, :, 1:1 + S2])          # columns 1, 2, ... of doa, cyclically
        big.reset()
        r3 = big.process_sources(pcm, d2)
        assert np.array_equal(r3["out"][:, 0], r["out"][:, 1]) and np.array_equal(r3["spec"][:, 0], r["spec"][:, 1]), S2


@pytest.mark.parametrize("M", [3, 6, 7, 9, 11, 13, 15])
def test_sources_every_row_slot_count(M):
    """As test_mvdr_every_row_slot_count with four look directions: every number of row slots per lane, the partly empty last
    slot, the register-tight instantiations (13 ... 15 microphones: four directions in two passes of two), one frame per call."""
    fs, N, F, A, S = 16000, 256, 9, 2, 4
    rng = np.random.default_rng(M)
    xs = np.sort(rng.uniform(0.0, 0.04 * M, M))
    pcm = np.stack([_scene(xs, fs, N, F, a) for a in range(A)])
    doa = rng.uniform(-1.3, 1.3, (A, F, S)).astype(np.float32)
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S)
    hop = N // 2
    specs = [bf.process_sources(pcm[:, :, t * hop:(t + 2) * hop], doa[:, t:t + 1])["spec"] for t in range(F)]
    spec = np.concatenate(specs, axis=2)
    for a in range(A):
        for s in range(S):
            og = po.MVDR(fs, N, xs)
            sp = _ospec(og.stream(pcm[a].astype(np.float64), doa[a, :, s].astype(np.float64), want_spec=True))
            e = np.abs(spec[a, s] - sp).max() / np.abs(sp).max()
            print("M %d stream %d source %d: spectra %.2e of the peak" % (M, a, s, e))
            assert e <= SPEC_TOL, (M, a, s)
        assert np.abs(bf.covariance(a) - og.covariance()).max() <= COV_TOL * np.abs(og.covariance()).max()


def test_sources_tail_workgroups_cut_along_the_frames():
    """64 streams x 513 bins = 513 solve workgroups: the one behind the last whole round goes in a second launch cut along the
    frames (api_mvdr.hip), here with two look directions, over two calls."""
    fs, N, F, A, S = 16000, 1024, 10, 64, 2
    xs = synth.REEM_C
    base = np.stack([_scene(xs, fs, N, 2 * F, a) for a in range(3)])
    pick = np.arange(A) % 3
    pcm = base[pick]
    doa = _drifting_doa(3, 2 * F, S)[pick]
    hop = N // 2
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S)
    r1 = bf.process_sources(pcm[:, :, :(F + 1) * hop].copy(), doa[:, :F].copy())
    r2 = bf.process_sources(pcm[:, :, F * hop:].copy(), doa[:, F:].copy())
    r = dict(spec=np.concatenate([r1["spec"], r2["spec"]], axis=2), out=np.concatenate([r1["out"], r2["out"]], axis=2))
    for a in (0, 31, 63):
        og = [po.MVDR(fs, N, xs) for _ in range(S)]
        _check_against_oracle(r, og, pcm[a], doa[a], a)
        assert np.abs(bf.covariance(a) - og[0].covariance()).max() <= COV_TOL * np.abs(og[0].covariance()).max(), a
    # streams with the same input give the same bytes wherever they sit in the batch (stream 63 is the one in the tail launch)
    assert np.array_equal(r["spec"][0], r["spec"][3]) and np.array_equal(r["out"][1], r["out"][61])
    assert np.array_equal(r["spec"][0], r["spec"][63]) and np.array_equal(r["out"][0], r["out"][63])
    assert np.array_equal(bf.covariance(0), bf.covariance(63))


@pytest.mark.parametrize("S", [3, 4])
def test_sources_chunked_calls_equal_one_call(S):
    fs, N, F = 48000, 1024, 48
    xs = synth.ULA16
    pcm = _scene(xs, fs, N, F, 0)[None]
    doa = _drifting_doa(1, F, S)
    one = api.MvdrBeamformer(fs, xs, N, max_sources=S).process_sources(pcm, doa)
    bf = api.MvdrBeamformer(fs, xs, N, max_sources=S)
    hop = N // 2
    outs, specs = [], []
    for (t0, t1) in [(0, 1), (1, 18), (18, 19), (19, 48)]:
        r = bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop], doa[:, t0:t1])
        outs.append(r["out"]); specs.append(r["spec"])
    assert np.array_equal(np.concatenate(specs, axis=2), one["spec"])
    assert np.array_equal(np.concatenate(outs, axis=2), one["out"])
    bf.reset()
    again = bf.process_sources(pcm, doa)
    assert np.array_equal(again["out"], one["out"]) and np.array_equal(again["spec"], one["spec"])


def _first_hop_without_carry(spec_frame, hop):
    """the first hop of a call's audio when the overlap-add tail is zero: the first half of frame 0's inverse transform"""
    return np.fft.irfft(spec_frame.astype(np.complex128), 2 * hop)[..., :hop]


def test_sources_left_out_restart_from_silence():
    fs, N, F, A = 16000, 512, 10, 2
    xs = synth.REEM_C
    hop = N // 2
    pcm = np.stack([_scene(xs, fs, N, 4 * F, a) for a in range(A)])
    doa = _drifting_doa(A, 4 * F, 3)
    part = lambda i: pcm[:, :, i * F * hop:((i + 1) * F + 1) * hop].copy()
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=3)
    bf.process_sources(part(0), doa[:, :F])
    bf.process_sources(part(1), doa[:, F:2 * F, :2].copy())                  # source 2 left out
    r = bf.process_sources(part(2), doa[:, 2 * F:3 * F])
    peak = np.abs(r["out"]).max()
    # fp32 transforms of 512 points: the bar of the delay-and-sum audio checks (2e-5 of the peak)
    fresh = _first_hop_without_carry(r["spec"][:, :, 0], hop)
    e2 = np.abs(r["out"][:, 2, :hop] - fresh[:, 2]).max() / peak
    e0 = np.abs(r["out"][:, 0, :hop] - fresh[:, 0]).max() / peak
    print("first hop against the carry-free inverse transform: left-out source %.2e, continued source %.2e of the peak" % (e2, e0))
    assert e2 <= 2e-5
    assert e0 > 1e-2                                                          # a continued source carries its tail
    # a single-look call uses slot 0 and leaves out the others
    bf.process(part(3)[:, :, :3 * hop], doa[:, 3 * F:3 * F + 2, 0].copy())
    r = bf.process_sources(pcm[:, :, (3 * F + 2) * hop:].copy(), doa[:, 3 * F + 2:])
    fresh = _first_hop_without_carry(r["spec"][:, :, 0], hop)
    peak = np.abs(r["out"]).max()
    for s in (1, 2):
        assert np.abs(r["out"][:, s, :hop] - fresh[:, s]).max() <= 2e-5 * peak, s
    assert np.abs(r["out"][:, 0, :hop] - fresh[:, 0]).max() > 1e-2 * peak


def test_sources_state_blobs():
    fs, N, F, S = 16000, 512, 40, 4
    hop = N // 2
    xs = synth.REEM_C
    pcm = _scene(xs, fs, N, F, 0)[None]
    doa = _drifting_doa(1, F, S)
    one = api.MvdrBeamformer(fs, xs, N, max_sources=S).process_sources(pcm, doa)
    b, c = api.MvdrBeamformer(fs, xs, N, max_sources=S), api.MvdrBeamformer(fs, xs, N, max_sources=S)
    first = b.process_sources(pcm[:, :, :(15 + 1) * hop], doa[:, :15])
    blob = b.state_save()
    c.state_load(blob)
    rest = c.process_sources(pcm[:, :, 15 * hop:], doa[:, 15:])
    assert np.array_equal(np.concatenate([first["out"], rest["out"]], axis=2), one["out"])
    assert np.array_equal(np.concatenate([first["spec"], rest["spec"]], axis=2), one["spec"])
    # a context with another maximum refuses the blob, in both directions
    with pytest.raises(api.MCArrayHipError, match="max_sources"):
        api.MvdrBeamformer(fs, xs, N, max_sources=2).state_load(blob)
    plain = api.MvdrBeamformer(fs, xs, N)
    with pytest.raises(api.MCArrayHipError, match="max_sources"):
        plain.state_load(blob)
    p1 = plain.process(pcm[:, :, :(15 + 1) * hop], doa[:, :15, 0].copy())["out"]
    pblob = plain.state_save()
    with pytest.raises(api.MCArrayHipError, match="max_sources"):
        c.state_load(pblob)
    # the blob of a plain context is what it was (header + covariances + traces + one tail per stream) and loads into a plain context;
    # so does that of a context whose maximum was set to 1
    K, tri = N // 2 + 1, len(xs) * (len(xs) + 1) // 2
    assert len(pblob) == 48 + K * tri * 8 + K * 4 + hop * 4
    assert len(blob) == len(pblob) + (S - 1) * hop * 4
    p2 = api.MvdrBeamformer(fs, xs, N, max_sources=1)
    p2.state_load(pblob)
    rest = p2.process(pcm[:, :, 15 * hop:], doa[:, 15:, 0].copy())["out"]
    assert np.array_equal(np.concatenate([p1, rest], axis=1), one["out"][:, 0])
    # raising the maximum keeps slot 0 and starts the new slots at zero
    p3 = api.MvdrBeamformer(fs, xs, N)
    p3.process(pcm[:, :, :(15 + 1) * hop], doa[:, :15, 0].copy())
    p3.set_max_sources(2)
    r = p3.process_sources(pcm[:, :, 15 * hop:], doa[:, 15:, :2].copy())
    assert np.array_equal(r["out"][:, 0], one["out"][:, 0, 15 * hop:])
    fresh = _first_hop_without_carry(r["spec"][:, 1, 0], hop)
    assert np.abs(r["out"][:, 1, :hop] - fresh).max() <= 2e-5 * np.abs(r["out"]).max()


def test_localise_two_sources_then_mvdr_16_microphones():
    """BASELINE configs[3] end to end with two sources: the 16-microphone localiser writes doa_rad [A][F][2] on the device and the
    MVDR call consumes that tensor as it is."""
    import torch
    fs, N, F, A, S = 48000, 1024, 48, 3, 2
    xs = synth.ULA16
    hop = N // 2
    pcm = np.stack([_scene(xs, fs, N, F, a) for a in range(A)])
    dev = torch.device("cuda:0")
    t_pcm = torch.from_numpy(pcm).to(dev)
    loc = api.Context(fs, xs, N, 0.5, S, max_arrays=A)
    t_bin = torch.empty((A, F, S), dtype=torch.int32, device=dev)
    t_doa = torch.empty((A, F, S), dtype=torch.float32, device=dev)
    t_prob = torch.empty((A, F, S), dtype=torch.float32, device=dev)
    loc.process_frames_dev(t_pcm, F, t_bin, t_doa, t_prob, localise=True, separate=False)
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S)
    t_out = torch.empty((A, S, F * hop), dtype=torch.float32, device=dev)
    t_spec = torch.empty((A, S, F, N // 2 + 1, 2), dtype=torch.float32, device=dev)
    bf.process_sources_dev(t_pcm, F, t_doa, out_pcm=t_out, out_spec=t_spec)
    torch.cuda.synchronize()
    bins, doa, out = t_bin.cpu().numpy(), t_doa.cpu().numpy(), t_out.cpu().numpy()
    spec = t_spec.cpu().numpy()
    spec = spec[..., 0] + 1j * spec[..., 1]
    for a in range(A):
        o = po.ssl_stream(fs, N, xs, pcm[a].astype(np.float64), S, 0.5, want_map=True, want_audio=False)
        ties = assert_bins(bins[a], o["bin"], o["energy"], loc.P, max_ties=3)      # the bar of the two-source localiser tests
        print("stream %d: %d fragile-frame differences" % (a, ties))
        for s in range(S):
            om = po.MVDR(fs, N, xs).stream(pcm[a].astype(np.float64), doa[a, :, s].astype(np.float64), want_spec=True)
            assert np.abs(spec[a, s] - _ospec(om)).max() <= SPEC_TOL * np.abs(_ospec(om)).max(), (a, s)
            assert np.abs(out[a, s] - om["out"]).max() <= AUDIO_TOL * np.abs(om["out"]).max(), (a, s)


def test_cxx_class_sources(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "test_mvdr_sources"
    lib_dir = os.path.join(ROOT, "mcarray_amd")
    subprocess.check_call([cxx, "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "test_mvdr_sources.cpp"), "-o", str(exe), "-L" + lib_dir,
                           "-lmcarray_hip", "-Wl,-rpath," + lib_dir], timeout=300)
    fs, N, M, S, F = 16000, 512, 6, 3, 30
    hop = N // 2
    xs = [0.035 * m for m in range(M)]                         # the array of the C++ program
    pcm = _scene(xs, fs, N, F, 0)
    pcm.tofile(str(tmp_path / "pcm.f32"))
    r = subprocess.run([str(exe), str(tmp_path / "pcm.f32"), str(tmp_path / "out.f32"), str(fs), str(N), str(M), str(S)],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL PASSED" in r.stdout
    k = int([ln for ln in r.stdout.splitlines() if ln.startswith("switch_frame")][0].split()[1])
    assert 0 < k < F
    out = np.fromfile(str(tmp_path / "out.f32"), dtype=np.float32).reshape(S, F * hop)
    first, second = np.array([0.35, -0.6, 1.1, -0.1]), np.array([0.30, -0.7, 0.9, 0.2])      # as in the C++ program
    doa = np.empty((1, F, S), dtype=np.float32)
    doa[0, :k] = first[:S]
    doa[0, k:] = second[:S]
    ref = api.MvdrBeamformer(fs, xs, N, max_sources=S).process_sources(pcm[None], doa)["out"][0]
    assert np.array_equal(out, ref)


def test_sources_reject_bad_arguments():
    fs, N = 16000, 512
    xs = synth.REEM_C
    pcm = _scene(xs, fs, N, 4, 0)[None]
    for bad in (0, 5):
        with pytest.raises(api.MCArrayHipError, match="max_sources"):
            api.MvdrBeamformer(fs, xs, N, max_sources=bad)
    bf = api.MvdrBeamformer(fs, xs, N, max_sources=2)
    with pytest.raises(api.MCArrayHipError, match="n_sources"):
        bf.process_sources(pcm, np.zeros((1, 4, 3), dtype=np.float32))
    with pytest.raises(api.MCArrayHipError, match="n_sources"):
        api.MvdrBeamformer(fs, xs, N).process_sources(pcm, np.zeros((1, 4, 2), dtype=np.float32))
    with pytest.raises(api.MCArrayHipError, match="both NULL"):
        bf.process_sources(pcm, np.zeros((1, 4, 2), dtype=np.float32), want_audio=False, want_spec=False)
    with pytest.raises(api.MCArrayHipError):
        bf.set_max_sources(7)
    r = bf.process_sources(pcm, np.zeros((1, 4, 2), dtype=np.float32))         # the context is still usable
    assert np.all(np.isfinite(r["out"]))
