"""GPU: the Capon spatial spectrum of the covariance an MVDR context holds and its peaks (mca_hip_mvdr_spectrum_*; k_mvdr_spectrum and
k_mvdr_spectrum_pick in kernels_mvdr_spectrum.hip) against the float64 twin of the dense definition (tests/mvdr_spectrum_twin.py).

The bar is the one tests/test_gpu_mvdr.py sets for this module's solve: a row differs from the twin's by at most 5e-4 of the row's
maximum, peak values by the same, and the peak indices of the compared slots are exactly the twin's
(tests/test_mvdr_spectrum_twin.py shows that every compared peak stands clear of its neighbours and of the next-ranked peak by ten
times that).  The worst cases have not been measured on an MI355X yet; a numpy emulation of the kernel's operations in complex64 on
the float64-recursed covariance gave 2e-6 ... 1.7e-5 of the row's maximum, every test prints its figures."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from mcarray_amd import api, synth

import mvdr_nulls_twin as nt
import mvdr_spectrum_twin as st

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 5e-4
INVALID = -1                                   # MCA_HIP_ERR_INVALID_ARGUMENT
WEIGHTINGS = {"power": st.POWER, "normalised": st.NORMALISED}


def _irregular(M):
    return np.sort(np.random.default_rng(M).uniform(0.0, 0.04 * M, M))        # the arrays of tests/test_gpu_mvdr_nulls.py


_cache = {}


def _feed(key, xs, fs, N, pcm):
    """a context that has processed pcm [A][M][(F+1) hop] towards 0 rad, and the twin's covariance of every stream (computed once per key)"""
    A = pcm.shape[0]
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A)
    bf.process(pcm, 0.0)
    if key not in _cache:
        F = pcm.shape[2] // (N // 2) - 1
        _cache[key] = [nt.mvdr_nulls_stream(fs, N, xs, pcm[a].astype(np.float64), np.zeros((F, 1)), 0.0)["phi"] for a in range(A)]
    return bf, _cache[key]


def _row_error(row, ref, what):
    assert np.all(np.isfinite(row)), what
    e = np.abs(row - ref).max() / ref.max()
    print("%s: %.2e of the row's maximum" % (what, e))
    assert e <= TOL, what
    return e


def _check_rows(bf, phis, xs, fs, N, D, band, weighting, what, n_peaks=1):
    bf.configure_spectrum(D, band[0], band[1], weighting, n_peaks)
    r = bf.spectrum(len(phis))
    assert r["spectrum"].shape == (len(phis), D) and r["peak_doa"].shape == (len(phis), n_peaks) == r["peak_val"].shape
    for a, phi in enumerate(phis):
        ref = st.spectrum(phi, fs, N, xs, D, band[0], band[1], WEIGHTINGS[weighting])
        _row_error(r["spectrum"][a], ref, "%s stream %d" % (what, a))
    return r


@pytest.mark.parametrize("weighting", ["power", "normalised"])
@pytest.mark.parametrize("M", [2, 3, 4, 5, 8, 11, 13, 16])
def test_spectrum_every_row_slot_count(M, weighting):
    xs, fs, N, F, A = _irregular(M), 16000, 256, 6, 2
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    bf, phis = _feed(("slots", M), xs, fs, N, pcm)
    _check_rows(bf, phis, xs, fs, N, 61, (1, 127), weighting, "M %d %s" % (M, weighting))
    bf.close()


@pytest.mark.parametrize("D", [2, 63, 64, 65, 129, 361])
def test_spectrum_angle_counts_at_the_lane_edges(D):
    xs, fs, N, F, A = synth.ULA8, 48000, 256, 6, 2
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    bf, phis = _feed("ula8", xs, fs, N, pcm)
    _check_rows(bf, phis, xs, fs, N, D, (1, 127), "normalised", "D %d" % D)
    g = bf.spectrum_grid()
    assert g.shape == (D,) and np.array_equal(g, st.grid(D).astype(np.float32))
    bf.close()


@pytest.mark.parametrize("band", [(0, 128), (17, 17), (63, 64), (10, 63), (64, 128), (128, 128)])
def test_spectrum_bands(band):
    """the full band (bin 0 adds a constant), one bin, two bins across the boundary of the kernel's chunks of 64 bins, a band that
    ends on the boundary, one that starts on it, and the chunk that holds bin N/2 alone"""
    xs, fs, N, F, A = synth.ULA8, 48000, 256, 6, 2
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    bf, phis = _feed("ula8", xs, fs, N, pcm)
    for weighting in ("power", "normalised"):
        _check_rows(bf, phis, xs, fs, N, 65, band, weighting, "band %s %s" % (band, weighting))
    bf.close()


@pytest.mark.parametrize("N,fs", [(1024, 48000), (2048, 96000)])
def test_spectrum_long_frames(N, fs):
    xs, F, A = synth.ULA16, 4, 2
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    bf, phis = _feed(("long", N), xs, fs, N, pcm)
    _check_rows(bf, phis, xs, fs, N, 181, (8, 71), "normalised", "N %d" % N)
    _check_rows(bf, phis, xs, fs, N, 181, (8, 71), "power", "N %d power" % N)
    bf.close()


@pytest.mark.parametrize("name", sorted(st.NAMED))
def test_spectrum_peaks_of_the_named_scenes(name):
    sc = st.named_scene(name)
    bf, phis = _feed(("named", name), sc["xs"], sc["fs"], sc["N"], sc["pcm"][None])
    weighting = "normalised" if sc["weighting"] == st.NORMALISED else "power"
    P = st.spectrum(phis[0], sc["fs"], sc["N"], sc["xs"], sc["D"], sc["band"][0], sc["band"][1], sc["weighting"])
    idx, doa, val = st.peaks(P, sc["slots"])
    r = _check_rows(bf, phis, sc["xs"], sc["fs"], sc["N"], sc["D"], sc["band"], weighting, name, n_peaks=sc["slots"])
    g = bf.spectrum_grid()
    for s in range(sc["slots"]):
        print("%s slot %d: twin index %d value %.6g, GPU doa %.6f value %.6g" % (name, s, idx[s], val[s], r["peak_doa"][0, s], r["peak_val"][0, s]))
        assert r["peak_doa"][0, s] == doa[s], (name, s)                    # exactly the twin's grid point (or slot 0's for an empty slot)
        assert abs(r["peak_val"][0, s] - val[s]) <= TOL * P.max(), (name, s)
        if idx[s] >= 0:
            assert r["peak_doa"][0, s] == g[idx[s]] and r["peak_val"][0, s] == r["spectrum"][0, idx[s]]
        else:
            assert r["peak_val"][0, s] == 0.0 and r["peak_doa"][0, s] == r["peak_doa"][0, 0]
    if name == "five_m30_25":
        assert idx.tolist()[2] == -1                                       # the empty-slot rule is exercised
    bf.close()


def test_spectrum_many_streams():
    """64 streams of 4 microphones, each with its own scene, one of them all zero; the workgroups of a stream and the rows of the
    outputs are indexed by the stream"""
    xs, fs, N, F, A, D = synth.REEM_C, 16000, 256, 6, 64, 61
    pcm = np.stack([st.two_sources(xs, fs, N, F, -60.0 + 2 * a, 50.0 - a, seed=a) for a in range(A)])
    pcm[17] = 0.0
    fresh = api.MvdrBeamformer(fs, xs, N, max_streams=A)
    fresh.configure_spectrum(D, n_peaks=3)
    z = fresh.spectrum()
    assert z["spectrum"].shape == (A, D) and np.all(z["spectrum"] == 0.0) and np.all(z["peak_val"] == 0.0) and np.all(z["peak_doa"] == 0.0)
    fresh.close()
    bf, phis = _feed("many", xs, fs, N, pcm)
    r = _check_rows(bf, [p for a, p in enumerate(phis) if a < 17], xs, fs, N, D, (1, 127), "normalised", "64 streams", n_peaks=3)
    r = bf.spectrum()
    for a in range(A):
        ref = st.spectrum(phis[a], fs, N, xs, D, 1, 127, st.NORMALISED)
        if a == 17:
            assert np.all(ref == 0.0) and np.all(r["spectrum"][a] == 0.0) and np.all(r["peak_val"][a] == 0.0) and np.all(r["peak_doa"][a] == 0.0)
        else:
            _row_error(r["spectrum"][a], ref, "64 streams, stream %d" % a)
            i0 = int(np.argmax(r["spectrum"][a]))
            assert r["peak_val"][a, 0] == r["spectrum"][a, i0] and r["peak_doa"][a, 0] == bf.spectrum_grid()[i0]
    # fewer streams than the context holds: the rows of the first ones, the same bytes
    part = bf.spectrum(5)
    assert np.array_equal(part["spectrum"], r["spectrum"][:5]) and np.array_equal(part["peak_doa"], r["peak_doa"][:5])
    bf.close()


def test_spectrum_state_and_reproducibility():
    xs, fs, N, F, A, D = synth.ULA16, 48000, 256, 8, 2, 181
    hop = N // 2
    pcm = np.stack([nt.scene(xs, fs, N, 2 * F, a) for a in range(A)])
    first, second = pcm[:, :, :(F + 1) * hop].copy(), pcm[:, :, F * hop:].copy()
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A)
    quiet = api.MvdrBeamformer(fs, xs, N, max_streams=A)                      # makes no spectrum call
    bf.process(first, 0.3)
    quiet.process(first, 0.3)
    bf.configure_spectrum(D, 1, 127, "normalised", 2)
    r1 = bf.spectrum()
    r2 = bf.spectrum()
    for k in r1:
        assert np.array_equal(r1[k].view(np.uint32), r2[k].view(np.uint32)), k
    assert r1["spectrum"].max() > 0
    # the call writes no state: the covariance, and every byte of the next call's audio and spectra
    for a in range(A):
        assert np.array_equal(bf.covariance(a), quiet.covariance(a)), a
    blob = bf.state_save()
    assert blob == quiet.state_save()
    o1, o2 = bf.process(second, 0.3, want_spec=True), quiet.process(second, 0.3, want_spec=True)
    assert np.array_equal(o1["out"], o2["out"]) and np.array_equal(o1["spec"].view(np.float32), o2["spec"].view(np.float32))
    assert not np.array_equal(bf.spectrum()["spectrum"], r1["spectrum"])      # the covariance has moved on
    # a second context that loads the state gives the spectrum's bytes
    other = api.MvdrBeamformer(fs, xs, N, max_streams=A)
    other.state_load(blob)
    other.configure_spectrum(D, 1, 127, "normalised", 2)
    r3 = other.spectrum()
    for k in r1:
        assert np.array_equal(r1[k].view(np.uint32), r3[k].view(np.uint32)), k
    # reconfiguring between calls takes effect: weighting, band, angle count and peak count, each against the twin
    phis = [nt.mvdr_nulls_stream(fs, N, xs, first[a].astype(np.float64), np.full((F, 1), np.float32(0.3)), 0.0)["phi"] for a in range(A)]
    for (D2, band, weighting, n_peaks) in [(D, (1, 127), "power", 2), (D, (20, 90), "power", 2), (91, (20, 90), "normalised", 4), (D, (1, 127), "normalised", 2)]:
        r = _check_rows(other, phis, xs, fs, N, D2, band, weighting, "reconfigured %d %s %s" % (D2, band, weighting), n_peaks=n_peaks)
        assert other.spectrum_config == dict(n_angles=D2, bin_lo=band[0], bin_hi=band[1], weighting=WEIGHTINGS[weighting], n_peaks=n_peaks)
    assert np.array_equal(r["spectrum"], r1["spectrum"]) and np.array_equal(r["peak_doa"], r1["peak_doa"])   # back at the first configuration


def test_spectrum_refused_arguments():
    import ctypes as C
    from mcarray_amd import _lib
    xs, fs, N, F, A = synth.REEM_C, 16000, 256, 6, 3
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    bf = api.MvdrBeamformer(fs, xs, N, max_streams=A)
    bf.process(pcm, 0.0)
    lib, fp = bf._lib, _lib.c_fp
    buf = np.zeros((A, 361), dtype=np.float32)
    # before configure
    assert lib.mca_hip_mvdr_spectrum_host(bf.h, A, buf.ctypes.data_as(fp), None, None) == INVALID
    assert lib.mca_hip_mvdr_spectrum_dev(bf.h, A, None, None, None, None) == INVALID
    with pytest.raises(api.MCArrayHipError, match="configure"):
        bf.spectrum()
    with pytest.raises(api.MCArrayHipError):
        bf.spectrum_grid()
    bf.configure_spectrum(61, 5, 100, "power", 2)
    before = bf.spectrum()

    def cfg(n_angles=61, bin_lo=5, bin_hi=100, weighting=0, n_peaks=2, size=None):
        c = _lib.MvdrSpectrumConfig()
        c.struct_size = C.sizeof(_lib.MvdrSpectrumConfig) if size is None else size
        c.n_angles, c.bin_lo, c.bin_hi, c.weighting, c.n_peaks = n_angles, bin_lo, bin_hi, weighting, n_peaks
        return c
    bad = [cfg(n_angles=1), cfg(n_angles=0), cfg(n_angles=362), cfg(bin_lo=-1), cfg(bin_lo=101), cfg(bin_hi=N // 2 + 1), cfg(bin_lo=129, bin_hi=129),
           cfg(weighting=2), cfg(weighting=-1), cfg(n_peaks=0), cfg(n_peaks=5), cfg(size=8)]
    for c in bad:
        assert lib.mca_hip_mvdr_spectrum_configure(bf.h, C.byref(c)) == INVALID, [getattr(c, f) for f, _ in c._fields_]
        assert b"" != lib.mca_hip_mvdr_last_error(bf.h)
    assert lib.mca_hip_mvdr_spectrum_configure(bf.h, None) == INVALID
    with pytest.raises(api.MCArrayHipError, match="n_angles"):
        bf.configure_spectrum(1000)
    assert bf.spectrum_config["n_angles"] == 61
    # the spectrum call's own arguments
    for n in (0, -1, A + 1):
        assert lib.mca_hip_mvdr_spectrum_host(bf.h, n, buf.ctypes.data_as(fp), None, None) == INVALID, n
        assert lib.mca_hip_mvdr_spectrum_dev(bf.h, n, None, None, None, None) == INVALID, n
    assert lib.mca_hip_mvdr_spectrum_host(bf.h, A, None, None, None) == INVALID
    assert lib.mca_hip_mvdr_spectrum_dev(bf.h, A, None, None, None, None) == INVALID
    # the configuration is as it was, the context usable
    after = bf.spectrum()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    g = np.zeros(61, dtype=np.float32)
    assert lib.mca_hip_mvdr_spectrum_get_grid(bf.h, g.ctypes.data_as(fp)) == 0 and np.array_equal(g, st.grid(61).astype(np.float32))
    # any one output alone is a valid call
    only = np.zeros((A, 2), dtype=np.float32)
    assert lib.mca_hip_mvdr_spectrum_host(bf.h, A, None, only.ctypes.data_as(fp), None) == 0 and np.array_equal(only, before["peak_doa"])
    assert lib.mca_hip_mvdr_spectrum_host(bf.h, A, None, None, only.ctypes.data_as(fp)) == 0 and np.array_equal(only, before["peak_val"])
    # timing: kernel_id 3 counts the spectrum calls
    bf.set_timing(True)
    bf.spectrum()
    n, ms = bf.get_timing(api.MvdrBeamformer.K_SPECTRUM)
    assert n == 1 and ms > 0.0
    assert lib.mca_hip_mvdr_get_timing(bf.h, 4, None, None) == INVALID


def test_spectrum_device_pointers():
    import torch
    xs, fs, N, F, A, D = synth.ULA8, 48000, 256, 6, 2, 65
    pcm = np.stack([nt.scene(xs, fs, N, F, a) for a in range(A)])
    bf, _ = _feed("ula8", xs, fs, N, pcm)
    bf.configure_spectrum(D, n_peaks=2)
    host = bf.spectrum()
    dev = torch.device("cuda:0")
    s = torch.zeros((A, D), dtype=torch.float32, device=dev)
    d = torch.zeros((A, 2), dtype=torch.float32, device=dev)
    v = torch.zeros((A, 2), dtype=torch.float32, device=dev)
    bf.spectrum_dev(A, spectrum=s, peak_doa=d, peak_val=v)
    torch.cuda.synchronize()
    assert np.array_equal(s.cpu().numpy(), host["spectrum"]) and np.array_equal(d.cpu().numpy(), host["peak_doa"]) and np.array_equal(v.cpu().numpy(), host["peak_val"])
    bf.close()


def test_spectrum_loop_chunk_peaks_look_directions():
    """three chunks of 8 frames: after each, the two peaks of the spectrum are the look directions of the next process_sources chunk;
    the twin does the same in float64"""
    c = st.LOOP
    pcm, ref = st.loop_twin()
    hop, F = c["N"] // 2, c["F"]
    bf = api.MvdrBeamformer(c["fs"], c["xs"], c["N"], max_sources=c["n_peaks"])
    bf.configure_spectrum(c["D"], c["band"][0], c["band"][1], "normalised", c["n_peaks"])
    look = np.array(c["first"], dtype=np.float32)
    for j in range(c["chunks"]):
        r = bf.process_sources(pcm[None, :, j * F * hop:((j + 1) * F + 1) * hop], np.broadcast_to(look, (1, F, c["n_peaks"])))
        for s in range(c["n_peaks"]):
            es = np.abs(r["spec"][0, s] - ref[j]["spec"][s]).max() / np.abs(ref[j]["spec"][s]).max()
            ea = np.abs(r["out"][0, s] - ref[j]["out"][s]).max() / np.abs(ref[j]["out"][s]).max()
            print("chunk %d source %d: spectra %.2e audio %.2e of the peak" % (j, s, es, ea))
            assert es <= TOL and ea <= TOL, (j, s)
        sp = bf.spectrum()
        _row_error(sp["spectrum"][0], ref[j]["P"], "chunk %d spectrum" % j)
        assert np.array_equal(sp["peak_doa"][0], ref[j]["doa"]), (j, sp["peak_doa"][0], ref[j]["doa"])
        look = sp["peak_doa"][0].copy()
    assert sorted(np.rint(np.rad2deg(look)).tolist()) == sorted(c["deg"])
    bf.close()


def test_cxx_class_spectrum(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "test_mvdr_spectrum"
    lib_dir = os.path.join(ROOT, "mcarray_amd")
    subprocess.check_call([cxx, "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "test_mvdr_spectrum.cpp"), "-o", str(exe), "-L" + lib_dir,
                           "-lmcarray_hip", "-Wl,-rpath," + lib_dir], timeout=300)
    sc = st.named_scene("ula16_20_32")
    sc["pcm"].tofile(str(tmp_path / "pcm.f32"))
    D, lo, hi, P = sc["D"], sc["band"][0], sc["band"][1], 3
    r = subprocess.run([str(exe), str(tmp_path / "pcm.f32"), str(tmp_path / "out.f32"), str(sc["fs"]), str(sc["N"]), str(D), str(lo), str(hi), str(P)],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL PASSED" in r.stdout
    out = np.fromfile(str(tmp_path / "out.f32"), dtype=np.float32)          # grid [D], spectrum [D], peak doa [P], peak value [P]
    assert out.size == 2 * D + 2 * P
    bf, phis = _feed(("named", "ula16_20_32"), sc["xs"], sc["fs"], sc["N"], sc["pcm"][None])
    bf.configure_spectrum(D, lo, hi, "normalised", P)
    py = bf.spectrum()
    assert np.array_equal(out[:D], bf.spectrum_grid()) and np.array_equal(out[D:2 * D], py["spectrum"][0])
    assert np.array_equal(out[2 * D:2 * D + P], py["peak_doa"][0]) and np.array_equal(out[2 * D + P:], py["peak_val"][0])
    assert sorted(np.rint(np.rad2deg(out[2 * D:2 * D + 2])).tolist()) == [20.0, 32.0]
    bf.close()
