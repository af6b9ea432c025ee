"""CPU: the numpy restatement of TemporalGCCBinauralLocalisation (tests/tgcc_twin.py) against the reference's own lines and
asserted property, the inputs of the GPU tests against near-ties, and the library's exports of the mca_hip_tgcc_* ABI."""
import ctypes as C
import os

import numpy as np
import pytest

import tgcc_twin as tt
from mcarray_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TGCC_SYMBOLS = ["mca_hip_tgcc_create", "mca_hip_tgcc_destroy", "mca_hip_tgcc_last_error", "mca_hip_tgcc_reset",
                "mca_hip_tgcc_get_geometry", "mca_hip_tgcc_frames_dev", "mca_hip_tgcc_frames_host", "mca_hip_tgcc_process_frame",
                "mca_hip_tgcc_state_size", "mca_hip_tgcc_state_save", "mca_hip_tgcc_state_load"]


@pytest.mark.parametrize("nd", [2, 3, 10, 12, 23])
@pytest.mark.parametrize("W", [6615, 2400])
def test_closed_form_matches_literal_transcription(nd, W):
    rng = np.random.default_rng(nd * 1000 + W)
    for trial in range(2):
        L = rng.standard_normal(W) * 300 + (50.0 if trial else 0.0)
        R = rng.standard_normal(W) * 300 + np.roll(L, 3) * 0.5
        lit = tt.frame_index_literal(L, R, nd)
        closed = tt.frame_index(L, R, nd)
        rel = np.abs(closed - lit) / np.abs(lit)
        print("nd", nd, "W", W, "max relative difference", rel.max())
        assert rel.max() <= 1e-12


def test_triangle_values():
    assert np.allclose(tt.triangle(10), [0, .02, .04, .06, .08, .1, .08, .06, .04, .02], rtol=0, atol=1e-15)
    assert tt.triangle(10)[0] == 0.0 and tt.triangle(10)[5] == 0.1


def test_samples2degrees_matches_the_reference_tables():
    # BinauralLocalisation.cpp:265-268
    t8 = [90.0000, 45.5847, 25.3769, 8.2132, -8.2132, -25.3769, -45.5847, -90.0000]
    t10 = [90.0000, 51.0576, 33.7490, 19.4712, 6.3794, -6.3794, -19.4712, -33.7490, -51.0576, -90.0000]
    for nd, table in ((8, t8), (10, t10)):
        got = np.array([tt.samples2degrees(k, nd) - 90 for k in range(nd)])
        print(nd, got)
        assert np.abs(got - np.array(table)).max() <= 1e-4


def test_geometry_of_the_reference_constructor():
    assert [tt.geometry(fs, 0.086)[0] for fs in (16000, 44100, 48000, 96000)] == [2400, 6615, 7200, 14400]
    assert [tt.geometry(fs, 0.086)[2] for fs in (16000, 44100, 48000, 96000)] == [3, 10, 11, 23]
    assert tt.geometry(44100, 0.086)[1] == 3307


def test_reference_property_on_five_recordings():
    """testBinauralLocalisation (test_mcarray.cpp:305-339): gate on, every callback's DOA in the file's accepted range and at
    least 40 callbacks per file.  (With the recordings' seed 2016 instead of 1, left90's first voiced frame -- the frame that
    holds the end of the quiet lead-in, a third of it signal -- picks pair 2, and its halved DOA of 16.9 deg is outside [30, 90].)"""
    for name, pcm, (lo, hi) in tt.reference_recordings():
        r = tt.run_stream(pcm, 44100, 0.086, True)
        d = r["doa"][r["voiced"]]
        print(name, "callbacks", len(d), "DOA range", d.min(), d.max())
        assert len(d) >= 40, name
        assert np.all((d >= lo) & (d <= hi)), (name, d[(d < lo) | (d > hi)])


def _min_gap(pcm, fs, d, gate):
    r = tt.run_stream(pcm, fs, d, gate)
    return r["gap"][r["voiced"]].min()


def test_gpu_inputs_have_no_near_ties():
    """every voiced frame of every input the GPU tests use has a relative gap >= 1e-8 between its two largest normalised index
    values, so a pick can only differ between the library and the twin through a real error."""
    gaps = {}
    for fs, d in tt.PARITY_CONFIGS:
        for gate in (True, False):
            for j, s in enumerate(tt.parity_streams(fs, d, gate)):
                gaps[(fs, d, gate, j)] = _min_gap(s, fs, d, gate)
    for name, pcm, _ in tt.reference_recordings():
        gaps[name] = _min_gap(pcm, 44100, 0.086, True)
    gaps["muted"] = _min_gap(tt.muted_stream(), 44100, 0.086, False)
    gaps["hook"] = _min_gap(tt.hook_stream(), 44100, 0.086, True)
    x, batch = tt.bits_streams()
    gaps["bits"] = _min_gap(x, 44100, 0.086, True)
    gaps["bits batch"] = min(_min_gap(b, 44100, 0.086, True) for b in batch)
    for k, v in gaps.items():
        print(k, v)
    assert min(gaps.values()) >= 1e-8


def test_library_exports_every_tgcc_entry_point():
    bound = {name for name, _, _ in _lib.SYMBOLS}
    assert set(TGCC_SYMBOLS) <= bound
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in TGCC_SYMBOLS:
        assert hasattr(lib, name), name
    assert _lib.TgccConfig.mic_xyz.size == 6 * 8


@pytest.mark.parametrize("fs, d, text", [(8000, 0.086, "Sample frequency has to be a least 8048.84"),
                                         (96000, 0.2, "at most 32"), (192000, 0.01, "sample_rate")])
def test_create_refuses_unsupported_geometry(fs, d, text):
    """nd < 2 with the reference's own message (BinauralLocalisation.cpp:76-80), nd > 32 and fs > 96 kHz: refused before any
    device is touched."""
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    cfg = _lib.TgccConfig()
    cfg.struct_size = C.sizeof(_lib.TgccConfig)
    cfg.sample_rate = fs
    cfg.mic_xyz[3] = d
    cfg.use_power_floor = 1
    cfg.max_arrays = 1
    h = C.c_void_p()
    rc = lib.mca_hip_tgcc_create(C.byref(cfg), C.byref(h))
    assert rc != 0 and not h.value
    assert text in lib.mca_hip_tgcc_last_error(None).decode()
