"""The mirror fold of the merged steering table (csrc/fold_table.h) on the CPU: tests/cxx/fold_table_cli.cpp is compiled with the host
compiler and run on the delays of the reference's float chain (oracle/np_twin.py), for the flagship geometry (8 microphones, 0.04 m,
48 kHz, 0.5 degrees: D = 361) and the 4-microphone one.

Rounding: the product rounds a double to float and the float to fp16 ((_Float16)(float)cos), and the fold keeps that chain so that column
c stays what the unfolded table holds, bit for bit; the expected values here are the numpy float64 evaluation rounded the same way.  A
direct float64 -> fp16 rounding differs from it only at double-rounding ties (at most one fp16 unit), which is asserted too."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import np_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, STEP_DEG, N, K, DP = 48000, 0.5, 1024, 513, 384
GEOMETRIES = {"ula8": [0.04 * m for m in range(8)], "ula4": [0.04 * m for m in range(4)]}


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("fold") / "fold_table_cli"
    subprocess.check_call([cxx, "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "mcarray_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "fold_table_cli.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def unit_delays():
    """the D float delays of the unit spacing (pair (0, 1)): the same for both geometries"""
    d = np_twin.delay_table(FS, GEOMETRIES["ula8"][:2], STEP_DEG)[0]
    assert np.array_equal(d, d.astype(np.float32).astype(np.float64))
    return d.astype(np.float32)


def run_cli(cli, tmp_path, delays, D, G):
    src, out = tmp_path / "delays.f32", tmp_path / "tables.bin"
    np.asarray(delays, dtype=np.float32).tofile(src)
    line = subprocess.check_output([cli, str(src), str(D), str(DP), str(G), str(K), str(out)], text=True).split()
    info = {k: int(v) for k, v in (w.split("=") for w in line)}
    if not info["fold"]:
        assert not out.exists()
        return info, None
    half, ns = info["Kp"] // 2, info["Kp"] // 64
    raw = np.fromfile(out, dtype=np.uint16)
    n_half = ns * 192 * 32
    assert raw.size == 2 * n_half + DP * info["Kp"]
    tabs = {"even": raw[:n_half].reshape(ns, 192, 32), "odd": raw[n_half:2 * n_half].reshape(ns, 192, 32), "full": raw[2 * n_half:].reshape(DP, 2 * half)}
    return info, tabs


def f16_chain(x):
    return x.astype(np.float32).astype(np.float16)


def ulp_distance(a_bits, b_bits):
    def key(b):
        b = b.astype(np.int32)
        return np.where(b & 0x8000, -(b & 0x7fff), b & 0x7fff)
    return np.abs(key(a_bits) - key(b_bits))


@pytest.mark.parametrize("name", ["ula8", "ula4"])
def test_fold_tables_of_the_bench_geometries(cli, unit_delays, tmp_path, name):
    G = len(GEOMETRIES[name]) - 1
    D = unit_delays.size
    assert D == 361
    info, t = run_cli(cli, tmp_path, unit_delays, D, G)
    assert info["fold"] == 1
    c = info["c"]
    assert c == 180
    ms = np.unique(np.outer(np.arange(K), np.arange(1, G + 1)))
    n, half = ms.size, info["Kp"] // 2
    assert info["n_merged"] == n and half == (n + 63) // 64 * 64 and half == {"ula8": 1984, "ula4": 1088}[name]

    d64 = unit_delays.astype(np.float64)
    j = np.arange(c + 1)
    tj = np.where(j == 0, d64[c], 0.5 * (d64[c + j] - d64[c - j]))
    ph = 2.0 * np.pi * ms[None, :].astype(np.float64) * tj[:, None] / N           # [j][r]
    want_even, want_odd = np.zeros((192, half), np.float16), np.zeros((192, half), np.float16)
    want_even[:c + 1, :n], want_odd[:c + 1, :n] = f16_chain(np.cos(ph)), f16_chain(-np.sin(ph))
    got_even = t["even"].transpose(1, 0, 2).reshape(192, half)                   # [stage][col][32] -> [col][depth]
    got_odd = t["odd"].transpose(1, 0, 2).reshape(192, half)
    assert np.array_equal(got_even, want_even.view(np.uint16))
    assert np.array_equal(got_odd, want_odd.view(np.uint16))
    # (a direct rounding of the float64 values: the same but for double-rounding ties)
    direct = max(int(ulp_distance(got_even[:c + 1, :n], np.cos(ph).astype(np.float16).view(np.uint16)).max()),
                 int(ulp_distance(got_odd[:c + 1, :n], (-np.sin(ph)).astype(np.float16).view(np.uint16)).max()))
    assert direct <= 1

    # the full-width table: planar K order, the mirror column with the same cos and the negated -sin, zero behind D and behind n
    full = t["full"]
    assert not full[D:].any() and not full[:, n:half].any() and not full[:, half + n:].any()
    assert np.array_equal(full[c:D, :half], got_even[:c + 1]) and np.array_equal(full[c:D, half:], got_odd[:c + 1])
    assert np.array_equal(full[c - 1::-1, :half], got_even[1:c + 1])
    neg = np.where(got_odd[1:c + 1] & 0x7fff, got_odd[1:c + 1] ^ 0x8000, got_odd[1:c + 1])
    assert np.array_equal(full[c - 1::-1, half:], neg)

    # against today's table (the unfolded one: every column from its own delay): bit for bit at column c, elsewhere at most one fp16
    # unit apart in under 2 % of the entries
    ph_t = 2.0 * np.pi * ms[None, :].astype(np.float64) * d64[:, None] / N        # [d][r]
    today_c, today_s = f16_chain(np.cos(ph_t)).view(np.uint16), f16_chain(-np.sin(ph_t)).view(np.uint16)
    assert np.array_equal(full[c, :n], today_c[c]) and np.array_equal(full[c, half:half + n], today_s[c])
    # "One fp16 unit": the two entries are roundings of cos / sin at phases |dphi| = 2 pi m |t_fold - delay[d]| / N apart (at most 2.1e-5 rad),
    # so they differ by at most |dphi| plus half a unit of either rounding -- one unit (the spacing of fp16 at the larger entry) wherever
    # that spacing exceeds the phase shift, i.e. everywhere but next to the zero crossings, where an entry's own spacing is far below
    # 2e-5 and the distance counted in those units is large (85 at an entry of 2^-12) while the difference itself stays 2e-5.
    t_fold = np.concatenate([-tj[:0:-1], tj])                                   # the delay column d steers with after the fold
    dphi = 2.0 * np.pi * ms[None, :].astype(np.float64) * np.abs(t_fold - d64)[:, None] / N
    assert dphi.max() < 2.5e-5
    diffs, bounds, changed = [], [], 0
    for got, today in ((full[:D, :n], today_c), (full[:D, half:half + n], today_s)):
        a, b = got.view(np.float16).astype(np.float64), today.view(np.float16).astype(np.float64)
        unit = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float16)).astype(np.float64)
        diffs.append(np.abs(a - b)); bounds.append(dphi + unit)
        changed += int((got != today).sum())
    diffs, bounds = np.stack(diffs), np.stack(bounds)
    share = changed / diffs.size
    print("%s: %.3f %% of the entries differ from the unfolded table, largest difference %.3g (%.3f of its bound), largest phase shift %.3g rad"
          % (name, 100 * share, diffs.max(), (diffs / bounds).max(), dphi.max()))
    assert (diffs <= bounds).all()
    assert diffs.max() <= 2.0 ** -11                                            # one unit at the table's scale, entries in [0.5, 1]
    assert share < 0.02


def test_a_delay_moved_by_1e_5_samples_does_not_fold(cli, unit_delays, tmp_path):
    d = unit_delays.copy()
    d[100] += np.float32(1e-5)
    assert run_cli(cli, tmp_path, d, d.size, 7)[0]["fold"] == 0


def test_an_even_grid_does_not_fold(cli, unit_delays, tmp_path):
    assert run_cli(cli, tmp_path, unit_delays[:360], 360, 7)[0]["fold"] == 0
