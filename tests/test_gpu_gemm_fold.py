"""GPU, kernel level: k_srp_gemm_f16_fold (csrc/kernels_gemm.hip) through the test-only launcher of tests/cxx/gemm_harness.hip.

Random planar fp16 rows against random even / odd half-width tables (zero from j > c, as fold_table.h builds them); the map planes and
the scan partials go in filled with NaN.  Shapes: one tile, a ragged tile and two tiles of rows; D = 361, 321 and 383 (every padding case
of Dp = 384: 23, 63 and 1 columns); the depth of the 8-microphone rows (2 x 1 984), of the 4-microphone rows as build_merged_tables lays
them out (2 x 1 088) and 2 x 800 (an odd number of stages).

Bar: the fp32 accumulation bound of two products of K / 2 terms each, K / 2 * 2^-24 * sum |a| |b| per element, plus one rounding of the
sum of the two planes; the scan partials (32 weighted rows) to the bar of the same form, 32 * 2^-24 * sum |w| |c| plus one rounding.

Every call checks the hipError_t the harness returns; after the first non-zero one every later test of the module skips (nothing more
goes to a GPU that has just reported a fault)."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP, U = 384, 2.0 ** -24
_FAULT = {"err": None}

CASES = [(rows, D, 1984) for rows in (256, 300, 512) for D in (361, 321, 383)] + [(300, D, half) for half in (1088, 800) for D in (361, 321, 383)]


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "tests", "cxx", "libgemm_harness.so")
    if not os.path.exists(path):
        pytest.fail("%s is missing: build() makes it (tests/cxx/gemm_harness.mk)" % path)
    h = ctypes.CDLL(path)
    h.gh_fold.restype = ctypes.c_int
    h.gh_fold.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                          ctypes.c_void_p, ctypes.c_void_p]
    return h


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _FAULT["err"]:
        pytest.skip("an earlier call failed (%s): nothing more goes to this GPU" % _FAULT["err"])


def scan_weights():
    w = np.empty(32, np.float32)
    w[31] = np.float32(1) - np.float32(0.8)
    for t in range(30, -1, -1):
        w[t] = w[t + 1] * np.float32(0.8)
    return w


@pytest.mark.parametrize("rows,D,half", CASES)
def test_fold_kernel(lib, rows, D, half):
    rng = np.random.default_rng(1000 * rows + 10 * D + half)
    Kp, c, ns = 2 * half, (D - 1) // 2, half // 32
    rows_pad, rows_alloc = (rows + 255) // 256 * 256, rows + 8
    n_chunks = (rows_alloc + 31) // 32
    A = rng.standard_normal((rows_pad, Kp)).astype(np.float16)
    tab = np.zeros((2, 192, half), np.float16)                                   # [even / odd][column pair][depth]
    tab[:, :c + 1] = rng.uniform(-1, 1, (2, c + 1, half)).astype(np.float16)
    Bf = np.ascontiguousarray(tab.reshape(2, 192, ns, 32).transpose(0, 2, 1, 3))  # [y][stage][192][32]
    C = np.full((2, rows_alloc, DP), np.nan, np.float32)
    part = np.full((2, n_chunks, D), np.nan, np.float32)
    nv = np.full(n_chunks, -7, np.int32)
    w = scan_weights()
    err = lib.gh_fold(A.ctypes.data, Bf.ctypes.data, rows, rows_alloc, Kp, D, w.ctypes.data, C.ctypes.data, part.ctypes.data, nv.ctypes.data)
    if err:
        _FAULT["err"] = "hipError_t %d" % err
    assert err == 0

    # rows behind `rows` untouched, no NaN in front of them, padding columns exactly zero
    assert np.isnan(C[:, rows:]).all()
    assert not np.isnan(C[:, :rows]).any()
    assert not C[:, :rows, D:].any() and not np.signbit(C[:, :rows, D:]).any()
    # the mirror, bit for bit
    p0, p1 = C[0, :rows, :D], C[1, :rows, :D]
    j = np.arange(1, c + 1)
    assert np.array_equal(p0[:, c + j].view(np.uint32), p0[:, c - j].view(np.uint32))
    assert np.array_equal(p1[:, c + j].view(np.uint32), (-p1[:, c - j]).view(np.uint32))

    # plane 0 + plane 1 against the float64 product with the full-width table
    full = np.zeros((D, Kp), np.float64)
    full[c:, :half], full[c:, half:] = tab[0, :c + 1], tab[1, :c + 1]
    full[c - j, :half], full[c - j, half:] = tab[0, j], -tab[1, j].astype(np.float64)
    A64 = A[:rows].astype(np.float64)
    ref = A64 @ full.T
    got = (p0 + p1).astype(np.float64)
    bar = half * U * (np.abs(A64) @ np.abs(full).T) + U * np.abs(ref)
    ratio = float((np.abs(got - ref) / bar).max())
    print("rows %d D %d depth 2 x %d: largest error / bar %.4f (largest error %.3g of largest |C| %.3g)" % (rows, D, half, ratio, np.abs(got - ref).max(), np.abs(ref).max()))
    assert ratio <= 1.0
    # (each plane alone: its half of the product)
    for y, (lo, hi) in enumerate(((0, half), (half, Kp))):
        ref_y = A64[:, lo:hi] @ full[:, lo:hi].T
        bar_y = half * U * (np.abs(A64[:, lo:hi]) @ np.abs(full[:, lo:hi]).T)
        assert (np.abs(C[y, :rows, :D] - ref_y) <= bar_y).all()

    # the chunk-local scan results: the weighted sum of each plane's own rows, written for every chunk that starts in front of `rows`
    last = (rows - 1) >> 5
    assert (nv[:last + 1] == 32).all() and (nv[last + 1:] == -7).all()
    assert np.isnan(part[:, last + 1:]).all()
    whole = rows // 32
    blocks = C[:, :whole * 32, :D].astype(np.float64).reshape(2, whole, 32, D)
    ref_p = np.einsum("t,yctd->ycd", w.astype(np.float64), blocks)
    bar_p = 32 * U * np.einsum("t,yctd->ycd", np.abs(w).astype(np.float64), np.abs(blocks)) + U * np.abs(ref_p)
    ratio_p = float((np.abs(part[:, :whole] - ref_p) / np.maximum(bar_p, 1e-300)).max())
    print("scan partials: largest error / bar %.4f" % ratio_p)
    assert not np.isnan(part[:, :whole]).any() and ratio_p <= 1.0
    assert np.array_equal(part[0, :whole][:, c + j].view(np.uint32), part[0, :whole][:, c - j].view(np.uint32))
    assert np.array_equal(part[1, :whole][:, c + j].view(np.uint32), (-part[1, :whole][:, c - j]).view(np.uint32))
