"""CPU: the twin of the transform harness (tests/xform_twin.py) checked on its own -- its references against a direct O(N^2) DFT and
the conventions of the headers, its bars against the figures they are quoted with, the single-precision reference and the rounded
float64 results inside every bar, the integer restatement of pair_balance against the rule, and the build product's symbols."""
import ctypes as C
import os

import numpy as np
import pytest

import xform_twin as T


def _close(a, b, tol=1e-12):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= tol * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("n", [8, 16, 64])
def test_references_against_the_direct_dft(n):
    rng = np.random.default_rng(n)
    z = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
    x = rng.standard_normal((3, n))
    assert _close(T.ref_cfft(z), T.dft_direct(z))
    assert _close(T.ref_cfft(z, True), T.dft_direct(z, True))                       # unnormalised inverse
    full = T.dft_direct(x)
    assert _close(T.ref_rfft(x), full[:, :n // 2 + 1])                              # CCS order k = 0..N/2
    spec = full[:, :n // 2 + 1].copy()
    assert _close(T.ref_irfft(spec), x)                                             # 1/N inverse
    spec[:, 0] += 1e3j
    spec[:, -1] -= 1e3j
    assert _close(T.ref_irfft(spec), x)                                             # imaginary parts of DC and Nyquist ignored
    # the half-window input of rfft1024: the caller passes (x[2m], x[2m+1]) / 2 and the split step gives X unscaled
    assert _close(T.rfft_from_half_packed(T.half_packed(x)), full[:, :n // 2 + 1])
    # the sub-sequence order of the 2048 / 4096 chains: x[r n + q], q = 0..r-1
    for r in (4, 8):
        if n >= 2 * r:
            assert _close(T.rfft_by_subsequences(x, r), full[:, :n // 2 + 1])


def test_index_maps():
    assert [T.br3(i) for i in range(8)] == [0, 4, 2, 6, 1, 5, 3, 7]
    assert [T.dr16(p) for p in range(16)] == [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]
    assert all(T.dr16(T.dr16(p)) == p for p in range(16)) and all(T.br3(T.br3(i)) == i for i in range(8))
    assert sorted(T.lam_of(l) for l in range(64)) == list(range(64))
    for bits in (2, 3, 5, 11):
        perm = T.bitrev_perm(bits)
        assert sorted(perm.tolist()) == list(range(1 << bits)) and (perm[perm] == np.arange(1 << bits)).all()
    assert T.bitrev(1, 5) == 16 and T.bitrev(6, 3) == 3
    # a decimation-in-frequency transform without its final reordering leaves y[k] at bitrev(k): undo_bitrev puts it back
    n, bits = 16, 4
    y = np.arange(n) + 0j
    raw = np.zeros(n, dtype=complex)
    raw[T.bitrev_perm(bits)] = y
    assert (T.undo_bitrev(raw, bits) == y).all()


def test_in_register_dft_orders_restated():
    """radix-2 decimation in frequency leaves output br3(i) in register i (fft8's comment); 4 x 4 leaves dr16(p) in register p"""
    z = np.random.default_rng(1).standard_normal(8) + 1j * np.random.default_rng(2).standard_normal(8)
    v = z.copy()
    for span in (4, 2, 1):
        for base in range(0, 8, 2 * span):
            for r in range(span):
                a, b = v[base + r], v[base + r + span]
                v[base + r], v[base + r + span] = a + b, (a - b) * np.exp(-2j * np.pi * r / (2 * span))
    want = T.dft_direct(z)
    assert _close([v[i] for i in range(8)], [want[T.br3(i)] for i in range(8)])
    z = np.random.default_rng(3).standard_normal(16) + 1j * np.random.default_rng(4).standard_normal(16)
    first = np.stack([T.dft_direct(z[j::4]) for j in range(4)], axis=1)           # [q][j]: X4 of x[j + 4 i] at q
    first = first * np.exp(-2j * np.pi * np.outer(np.arange(4), np.arange(4)) / 16)
    regs = np.stack([T.dft_direct(first[q]) for q in range(4)])                   # register 4 q + r = output q + 4 r
    want = T.dft_direct(z)
    assert _close(regs.reshape(-1), [want[T.dr16(p)] for p in range(16)])
    assert (T.bfly4_f32(np.eye(4, dtype=np.complex64)) == np.round(T.dft_direct(np.eye(4))).astype(np.complex64)).all()
    assert (T.bfly4_f32(np.eye(4, dtype=np.complex64), True) == np.round(T.dft_direct(np.eye(4), True)).astype(np.complex64)).all()


def test_bars_evaluate_to_the_quoted_figures():
    assert abs(T.hard_bar(1024) / 5.76e-6 - 1) < 2e-3
    assert abs(T.hard_bar(512) / 5.18e-6 - 1) < 2e-3
    assert abs(T.hard_bar(4096) / 6.9e-6 - 1) < 2e-3
    assert T.hard_bar(2048, T.MU_PRODUCT) > T.hard_bar(2048) > T.hard_bar(1024)
    assert T.U == 2.0 ** -24 and T.TIGHT_FACTOR == 16.0


def test_single_precision_reference_is_inside_the_hard_bar():
    """numpy's own single-precision transform of every random input of case 4 is far under the hard bar (2.7e-8 against 5.76e-6
    at 1024 points), and a kernel at TIGHT_FACTOR times its error still is."""
    worst = 0.0
    for si, scale in enumerate(T.SCALES):
        z = T.random_complex(T.N_RANDOM, 1024, scale, 1000 + si)
        x = T.random_real(T.N_RANDOM, 1024, scale, 1000 + si)
        spec = T.random_complex(T.N_RANDOM, 513, scale, 1000 + si)
        for got, ref, n in ((T.np32_cfft(z), T.ref_cfft(z), 1024), (T.np32_cfft(z, True), T.ref_cfft(z, True), 1024),
                            (T.np32_rfft(x), T.ref_rfft(x), 1024), (T.np32_irfft(spec), T.ref_irfft(spec), 1024),
                            (T.np32_cfft(z[:, :512]), T.ref_cfft(z[:, :512]), 512), (T.np32_cfft(z[:, :4]), T.ref_cfft(z[:, :4]), 4)):
            e = T.norm_err(got, ref).max()
            assert 0 < T.TIGHT_FACTOR * e <= T.hard_bar(n), (scale, n, e)
        worst = max(worst, T.norm_err(T.np32_cfft(z), T.ref_cfft(z)).max())
    assert worst < 4e-8                                                             # the 2.7e-8 the tight bar was sized on


def test_rounded_float64_results_of_the_bases_are_inside_the_elementwise_bar():
    for n in (4, 8, 16, 512, 1024):
        ref = T.ref_cfft(T.complex_basis(n))
        assert np.abs(ref.astype(np.complex64).astype(np.complex128) - ref).max() <= T.hard_bar(n) * np.abs(ref).max(axis=-1).min()
        ref = T.ref_cfft(T.complex_basis(n), True)
        assert np.abs(ref.astype(np.complex64).astype(np.complex128) - ref).max() <= T.hard_bar(n) * np.abs(ref).max(axis=-1).min()
    for n in (8, 1024, 4096):
        ref = T.ref_rfft(T.real_basis(n, 0, min(n, 1024)))
        assert _close(np.abs(ref), 1.0)                                             # an impulse in: every output has modulus 1
        assert np.abs(ref.astype(np.complex64).astype(np.complex128) - ref).max() <= T.hard_bar(n)
    for n in (512, 1024, 2048):
        rows, tags = T.ccs_basis(n)
        assert len(rows) == n and tags[0] == (0, "re") and tags[n // 2] == (n // 2, "re") and tags[-1] == (n // 2 - 1, "im")
        ref = T.ref_irfft(rows)
        amp = np.abs(ref).max(axis=-1)
        assert _close(amp[1:n // 2] * n, 2.0, 1e-5) and _close(amp[[0, n // 2]] * n, 1.0)
        assert (np.abs(ref.astype(np.float32).astype(np.float64) - ref).max(axis=-1) <= T.hard_bar(n) * amp).all()


def test_arithmetic_references_are_the_documented_formulas():
    acc, a, b = T.carith_operands()
    a64, b64, c64 = a.astype(np.complex128), b.astype(np.complex128), acc.astype(np.complex128)
    for op, want in (("cmul", a64 * b64), ("cmulc", a64 * np.conj(b64)), ("cmac", c64 + a64 * b64), ("cmacc", c64 + a64 * np.conj(b64)),
                     ("cnmac", c64 - a64 * b64), ("cnmacc", c64 - a64 * np.conj(b64))):
        re, im, bar_re, bar_im = T.carith_ref(op, acc, a, b)
        assert np.abs(re - want.real).max() <= 1e-15 * np.abs(want).max() or (np.abs(re - want.real) <= 1e-15 * (bar_re / T.U + 1e-300)).all(), op
        assert (np.abs(im - want.imag) <= 1e-15 * (bar_im / T.U + 1e-300)).all(), op
        # the float32-rounded float64 value is inside the bar (half of it: one rounding against two)
        assert (np.abs(re.astype(np.float32).astype(np.float64) - re) <= bar_re / 2).all() and (np.abs(im.astype(np.float32) - im) <= bar_im / 2).all(), op
    assert (T.carith_exact32("csub_jb", a, b) == (a64 - 1j * b64).astype(np.complex64)).all()
    assert (T.carith_exact32("cadd_jb", a, b) == (a64 + 1j * b64).astype(np.complex64)).all()
    assert (T.carith_exact32("cmul_mj", a, b) == -1j * a).all() and (T.carith_exact32("cmul_pj", a, b) == 1j * a).all()
    assert (T.carith_exact32("cscale", a, b) == (a64 * b64.real).astype(np.complex64)).all()
    # four distinct magnitudes, all 16 sign patterns of (3, -5) (7, 11), zero operands, magnitudes over 2^+-30
    first = set((x.real, x.imag, y.real, y.imag) for x, y in zip(a[:64].tolist(), b[:64].tolist()))
    assert first == set((sa * 3.0, sb * 5.0, sc * 7.0, sd * 11.0) for sa in (1, -1) for sb in (1, -1) for sc in (1, -1) for sd in (1, -1))
    assert (a[64:80] == 0).sum() == 4 and (a[64:80].real == 0).sum() == 8 and (b[64:80].imag == 0).sum() == 8
    mags = np.abs(np.concatenate([a[80:].real, a[80:].imag]))
    assert mags.min() < 2.0 ** -28 and mags.max() > 2.0 ** 28 and len(a) == 80 + 4096


def test_integer_restatement_of_pair_balance_agrees_with_the_rule():
    cases = T.pair_balance_cases()
    seen = set()
    for name, ma, mb in cases:
        got = T.pair_balance_int(ma, mb)
        assert got == T.pair_balance_f64(ma, mb), name
        seen.add(got[:2])
    # 3 exponents apart stays untouched although the maxima are more than a factor 8 apart; 4 apart is scaled although less than 16
    by_name = {name: (ma, mb) for name, ma, mb in cases}
    ma, mb = by_name["a 3 exponents above b, mantissas 1.875 / 1.125, maxima in lanes 0 / 0"]
    assert ma.max() / mb.max() > 8 and T.pair_balance_int(ma, mb)[:2] == (0, 0)
    ma, mb = by_name["a 4 exponents above b, mantissas 1.125 / 1.875, maxima in lanes 31 / 32"]
    assert ma.max() / mb.max() < 16 and T.pair_balance_int(ma, mb)[:2] == (0, 4)
    assert {(0, 0), (0, 4), (4, 0), (0, 5), (0, 59), (0, 60), (60, 0)} <= seen and (0, 61) not in seen and (0, 100) not in seen
    assert T.pair_balance_int(*by_name["both channels exact zeros"][0:2]) == (0, 0, 0, 0)
    # the inputs of the balanced-pair test have the levels they are named by
    for d in (0, 3, 4, 20, 40, 60, 80):
        for swap in (False, True):
            a, b = T.level_pair(d, swap, 7000)
            na, nb, alive_a, alive_b = T.pair_balance_int(T.lane_maxima_512(a), T.lane_maxima_512(b))
            n = min(d, T.PB_MAX_SHIFT) if d >= T.PB_MIN_SHIFT else 0
            assert (na, nb, alive_a, alive_b) == ((n, 0, 1, 1) if swap else (0, n, 1, 1)), (d, swap)


def test_table_references():
    v, names = T.fft_table_ref()
    assert names[T.TW_T2 + 3 * 8 + 5] == "t2[s=3][l0=5]" and abs(v[T.TW_T2 + 3 * 8 + 5] - np.exp(-2j * np.pi * 15 / 64)) < 1e-15
    assert abs(v[T.TW_TS + 2 * 64 + 1] - np.exp(-2j * np.pi * 129 / 1024)) < 1e-15 and abs(v[7 * 64 + 63] - np.exp(-2j * np.pi * 441 / 512)) < 1e-15
    assert _close(np.abs(v), 1.0)
    v, defined, names = T.f1k_table_ref()
    assert defined.sum() == 1024 and abs(v[63 * 18 + 15] - np.exp(-2j * np.pi * 945 / 1024)) < 1e-15
    v, names = T.f1k_wb_ref()
    assert len(v) == 192 and abs(v[3 * 17 + 2] - np.exp(-2j * np.pi * 3 / 64)) < 1e-15 and names[3 * 17 + 2] == "wb[3] of lane 17"


def test_harness_library_exports_every_entry_point():
    if not os.path.exists(T.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(T.LIB_PATH)
    for name in T.ENTRY_POINTS:
        assert hasattr(lib, name), name
    # every entry point the GPU test calls goes through Harness._call by one of these names
    src = open(os.path.join(T.ROOT, "tests", "xform_twin.py")).read()
    import re
    assert set(re.findall(r'_(?:call|xf)\("(xh_[a-z0-9_]+)"', src)) <= set(T.ENTRY_POINTS)
