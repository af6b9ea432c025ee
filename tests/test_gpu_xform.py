"""GPU: the wave-level transforms and packed complex products of csrc/fft512.h, fft1024c.h, fft_block.h and pair_balance.h, one
primitive at a time, against float64 references (tests/xform_twin.py) through the test-only kernels of tests/cxx/xform_harness.hip.

Every call checks the hipError_t the harness returns; after the first non-zero one every later test of the module skips with that
error in its message (nothing more goes to a GPU that has just reported a fault).

Bars (xform_twin's docstring): arithmetic 2u (|p| + |q| [+ |acc|]) or bit for bit; hard bar B(N, mu) of Higham Thm 24.2, normwise on
random input and per element on the flat-magnitude bases; tight bar TIGHT_FACTOR (16) x the error of numpy's single-precision
transform of the same input.

MEASURED (MI355X; the table per primitive is in DESIGN.md section 4.14): the largest tight-bar ratio of any primitive is 6.3
(load_frames -> block_fft_dit -> split_forward at logH = 4: 1.2e-7 against numpy's 3.7e-8); the wave-level transforms are at 4.4 .. 5.2,
the real-output inverses at 1.1 (numpy's single-precision irfft is itself at 1.15e-7).  Largest normwise error on the random inputs
1.4e-7 (hard bars 5.18e-6 .. 1.55e-5), largest elementwise error on the bases 3.6e-7 of the largest output (combine4096_m, bar
1.55e-5), round trips 1.8e-7, table entries within 0.69 u of float64.  No primitive is exempt from the tight bar."""
import numpy as np
import pytest

import xform_twin as T

pytestmark = pytest.mark.gpu

# the largest kernel / numpy-single error ratio measured on an MI355X (random inputs of case 4)
TIGHT_MEASURED_MAX = 6.3
# primitives whose measured ratio is above TIGHT_FACTOR yet under their hard bar keep the hard bar only: {name: measured ratio}
TIGHT_EXEMPT = {}

_FAULT = {"err": None}


class _Guarded(T.Harness):
    def _call(self, name, *args):
        if _FAULT["err"]:
            pytest.skip("an earlier call failed (%s): nothing more goes to this GPU" % _FAULT["err"])
        try:
            super()._call(name, *args)
        except T.HipError as e:
            _FAULT["err"] = str(e)
            raise


@pytest.fixture(scope="module")
def hx():
    try:
        return _Guarded()
    except FileNotFoundError as e:
        pytest.fail(str(e))


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _FAULT["err"]:
        pytest.skip("an earlier call failed (%s): nothing more goes to this GPU" % _FAULT["err"])


# ---- the transforms, one entry per primitive ------------------------------------------------------------------------------------------
class X:
    """kind: cf / ci complex forward / inverse, rf real -> one-sided, ri one-sided -> real.  run(h, x[n, in_len]) -> y[n, out_len]"""

    def __init__(self, name, kind, n, run, in_len=None, mu=T.MU_TABLE, ref=None, ref32=None, basis=None, where_in=None, where_out=None):
        self.name, self.kind, self.n, self.run, self.mu = name, kind, n, run, mu
        self.in_len = in_len if in_len is not None else {"cf": n, "ci": n, "rf": n, "ri": n // 2 + 1}[kind]
        self.ref = ref or {"cf": T.ref_cfft, "ci": lambda z: T.ref_cfft(z, True), "rf": T.ref_rfft, "ri": T.ref_irfft}[kind]
        self.ref32 = ref32 or {"cf": T.np32_cfft, "ci": lambda z: T.np32_cfft(z, True), "rf": T.np32_rfft, "ri": T.np32_irfft}[kind]
        self.basis = basis
        self.where_in = where_in or (lambda i: "position %d" % i)
        self.where_out = where_out or (lambda k: "position %d" % k)
        self.bar = T.hard_bar(n, mu)

    def random(self, count, scale, seed):
        if self.kind in ("rf",):
            return T.random_real(count, self.in_len, scale, seed)
        x = T.random_complex(count, self.in_len, scale, seed)
        return x

    def __repr__(self):
        return self.name


def _pair_fwd(balance):
    return lambda h, x: h.rfft512_pair(balance, x.reshape(-1, 2, 512)).reshape(-1, 514)


def _pair_ref(f):
    return lambda x: np.concatenate([f(x[..., :x.shape[-1] // 2]), f(x[..., x.shape[-1] // 2:])], axis=-1)


def _pair_ccs_basis():
    rows, tags = T.ccs_basis(512)
    z = np.zeros_like(rows)
    return (np.concatenate([np.concatenate([rows, z], axis=1), np.concatenate([z, rows], axis=1)]),
            [("a",) + t for t in tags] + [("b",) + t for t in tags])


def _grouped(call, nch, out_len):
    """rows three by three into frames of nch channels (zero rows pad the last frame)"""
    def run(h, x):
        n = x.shape[0]
        pad = (-n) % nch
        if pad:
            x = np.concatenate([x, np.zeros((pad, x.shape[1]), dtype=x.dtype)])
        return call(h, x.reshape(-1, nch, x.shape[1])).reshape(-1, out_len)[:n]
    return run


def _w8(i):
    return T.where_wave(i)


def _sample_1024(s):
    return "sample %d = component %d of %s" % (s, s & 1, T.where_wave(s >> 1))


XFORMS = [
    X("cfft512_regs<false>", "cf", 512, lambda h, z: h.cfft512(0, z), where_in=_w8, where_out=lambda k: T.where_wave(k, T.br3)),
    X("cfft512_regs<false, AHEAD>", "cf", 512, lambda h, z: h.cfft512(1, z), where_in=_w8, where_out=lambda k: T.where_wave(k, T.br3)),
    X("cfft512_regs<true>", "ci", 512, lambda h, z: h.cfft512(2, z), where_in=_w8, where_out=lambda k: T.where_wave(k, T.br3)),
    X("rfft1024<false>", "rf", 1024, lambda h, x: h.rfft1024(0, x), where_in=_sample_1024, where_out=lambda k: "lane %d" % (k & 63)),
    X("rfft1024<true>", "rf", 1024, lambda h, x: h.rfft1024(1, x), where_in=_sample_1024, where_out=lambda k: "lane %d" % (k & 63)),
    X("irfft1024", "ri", 1024, lambda h, s: h.irfft1024(s), where_in=lambda k: "lane %d" % (k & 63), where_out=_sample_1024),
    X("rfft512_pair", "rf", 512, _pair_fwd(0), in_len=1024, ref=_pair_ref(T.ref_rfft), ref32=_pair_ref(T.np32_rfft),
      where_in=lambda s: "channel %s %s" % ("ab"[s >> 9], T.where_wave(s & 511)), where_out=lambda k: "channel %s bin %d (lane %d)" % ("ab"[k // 257], k % 257, (k % 257) & 63)),
    X("irfft512_pair", "ri", 512, lambda h, s: h.irfft512_pair(s.reshape(-1, 2, 257)).reshape(-1, 1024), in_len=514,
      ref=_pair_ref(T.ref_irfft), ref32=_pair_ref(T.np32_irfft), basis=_pair_ccs_basis,
      where_out=lambda s: "channel %s %s" % ("ab"[s >> 9], T.where_wave(s & 511, T.br3))),
    X("rfft512_pair -> combine2048_m", "rf", 2048, lambda h, x: h.rfft_sub(2048, x), mu=T.MU_PRODUCT,
      where_in=lambda s: "sub-sequence %d %s" % (s & 3, T.where_wave(s >> 2)), where_out=lambda k: "m = %d, q = %d" % (k & 511, k >> 9)),
    X("rfft512_pair -> combine4096_m", "rf", 4096, lambda h, x: h.rfft_sub(4096, x), mu=T.MU_PRODUCT,
      where_in=lambda s: "sub-sequence %d %s" % (s & 7, T.where_wave(s >> 3)), where_out=lambda k: "m = %d, q = %d" % (k & 511, k >> 9)),
    X("split2048_inv -> irfft512_pair", "ri", 2048, lambda h, s: h.irfft2048(s), mu=T.MU_PRODUCT,
      where_in=lambda k: "m = %d" % min(k % 512, 512 - k % 512), where_out=lambda s: "sub-sequence %d %s" % (s & 3, T.where_wave(s >> 2, T.br3))),
]
for _inv in (False, True):
    for _opt, _perm in ((3, 0), (7, 0), (3, 1)):
        XFORMS.append(X("fft1024c<%s, %d>%s" % ("true" if _inv else "false", _opt, " row = lam" if _perm else ""), "ci" if _inv else "cf", 1024,
                        (lambda i, o, p: lambda h, z: h.fft1024c(i, o, p, z))(_inv, _opt, _perm), where_in=_w8,
                        where_out=(lambda p: lambda k: ("residue %d = lane %d register %d" % (k & 63, [l for l in range(64) if T.lam_of(l) == (k & 63)][0], T.dr16(k >> 6)))
                                   if p else T.where_wave(k, T.dr16))(_perm)))
for _logh in range(2, 12):
    for _nch in (1, 3):
        _h = 1 << _logh
        XFORMS.append(X("load_frames -> block_fft_dit -> split_forward logH = %d nch = %d" % (_logh, _nch), "rf", 2 * _h,
                        _grouped((lambda lh: lambda h, x: h.block_rfft(lh, x))(_logh), _nch, _h + 1)))
        XFORMS.append(X("block_ifft_dif logH = %d nch = %d" % (_logh, _nch), "ci", _h,
                        _grouped((lambda lh: lambda h, z: T.undo_bitrev(h.block_ifft(lh, z), lh))(_logh), _nch, _h),
                        where_out=(lambda lh: lambda k: "position %d (stored at %d)" % (k, T.bitrev(k, lh)))(_logh)))
BY_NAME = {x.name: x for x in XFORMS}
IDS = [x.name.replace(" ", "_") for x in XFORMS]


def _describe_basis_row(x, i, tag):
    if tag is not None:
        return "unit %s bin %s" % (tag[-1], " ".join(str(t) for t in tag[:-1]))
    if x.kind in ("cf", "ci"):
        n = x.in_len
        return "%s at %s %d (%s)" % ("1" if i < n else "j", "input" if x.kind == "cf" else "bin", i % n, x.where_in(i % n))
    return "impulse at %s" % x.where_in(i)


def _assert_elementwise(x, first, rows, tags, got, ref):
    ref_max = np.abs(ref).max(axis=-1, keepdims=True)
    err = np.abs(got.astype(ref.dtype) - ref)
    over = err - x.bar * ref_max
    if (over > 0).any():
        i, k = np.unravel_index(np.argmax(over), over.shape)
        raise AssertionError("%s: %s -> output %d (%s): |error| %.3g of the largest output, bar B(%d, %gu) = %.3g; %d outputs of %d inputs over the bar"
                             % (x.name, _describe_basis_row(x, first + i, tags[first + i] if tags else None), k, x.where_out(k), err[i, k] / ref_max[i, 0],
                                x.n, x.mu / T.U, x.bar, int((over > 0).sum()), int((over > 0).any(axis=1).sum())))
    return float((err / ref_max).max())


# ---- cases 1 and 2: the whole basis ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x", XFORMS, ids=IDS)
def test_whole_basis_elementwise(hx, x):
    """An impulse 1 and an impulse j at every input index of the complex forward transforms, an impulse at every sample of the real
    ones, a unit real and a unit imaginary bin at every k of the inverses (DC and Nyquist of the CCS inverses: real only): every
    output within B(N, mu) of the largest, which covers every lane, register, exchange address and twiddle entry."""
    tags = None
    if x.basis:
        rows, tags = x.basis()
    elif x.kind in ("cf", "ci"):
        rows = T.complex_basis(x.in_len)
    elif x.kind == "ri":
        rows, tags = T.ccs_basis(x.n)
    else:
        rows = None
    worst = 0.0
    if rows is None:                                            # real impulses, 1024 at a time
        for first in range(0, x.in_len, 1024):
            chunk = T.real_basis(x.in_len, first, min(1024, x.in_len - first))
            worst = max(worst, _assert_elementwise(x, first, chunk, None, x.run(hx, chunk), x.ref(chunk)))
    else:
        worst = _assert_elementwise(x, 0, rows, tags, x.run(hx, rows), x.ref(rows))
    print("FIGURE basis %s: largest elementwise error %.3g (bar %.3g)" % (x.name, worst, x.bar))


# ---- case 3: the imaginary parts of DC and Nyquist are ignored --------------------------------------------------------------------------
@pytest.mark.parametrize("name,positions", [("irfft1024", (0, 512)), ("irfft512_pair", (0, 256, 257, 513)), ("split2048_inv -> irfft512_pair", (0, 1024))])
def test_dc_and_nyquist_imaginary_parts_are_ignored(hx, name, positions):
    x = BY_NAME[name]
    spec = x.random(8, 1.0, 31)
    for p in positions:
        spec[:, p] = spec[:, p].real
    clean = x.run(hx, spec)
    dirty_in = spec.copy()
    for p in positions:
        dirty_in[:, p] += 1e3j
    dirty = x.run(hx, dirty_in)
    assert np.array_equal(clean.view(np.uint32), dirty.view(np.uint32)), "%s: 1e3 in the imaginary parts of DC / Nyquist moves %d output samples" % (
        name, int((clean.view(np.uint32) != dirty.view(np.uint32)).sum()))


# ---- case 4: random inputs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x", XFORMS, ids=IDS)
def test_random_inputs_hard_and_tight_bar(hx, x):
    worst_ratio = 0.0
    for si, scale in enumerate(T.SCALES):
        inp = x.random(T.N_RANDOM, scale, 1000 + si)
        ref = x.ref(inp)
        e = T.norm_err(x.run(hx, inp), ref)
        e32 = T.norm_err(x.ref32(inp), ref)
        ratio = np.where(e32 > 0, e / np.where(e32 > 0, e32, 1.0), np.where(e > 0, np.inf, 0.0))   # (a 4-point transform can be exact)
        worst_ratio = max(worst_ratio, float(ratio.max()))
        print("FIGURE random %s scale %g: largest normwise error %.3g (hard bar %.3g), numpy single %.3g, largest ratio %.3g"
              % (x.name, scale, e.max(), x.bar, e32.max(), ratio.max()))
        assert e.max() <= x.bar, "%s, scale %g, transform %d: normwise error %.3g over the hard bar B(%d, %gu) = %.3g" % (
            x.name, scale, int(np.argmax(e)), e.max(), x.n, x.mu / T.U, x.bar)
        if x.name not in TIGHT_EXEMPT:
            assert (e <= T.TIGHT_FACTOR * e32).all(), "%s, scale %g, transform %d: normwise error %.3g is %.1f x numpy's single-precision transform of the same input (%.3g), allowed %g x" % (
                x.name, scale, int(np.argmax(ratio)), e[np.argmax(ratio)], ratio.max(), e32[np.argmax(ratio)], T.TIGHT_FACTOR)


@pytest.mark.parametrize("name", ["rfft1024", "rfft512_pair", "fft1024c", "2048"])
def test_round_trips(hx, name):
    """inverse(forward(x)) against x: the bars of the two transforms added"""
    for si, scale in enumerate(T.SCALES):
        if name == "rfft1024":
            x = T.random_real(T.N_RANDOM, 1024, scale, 2000 + si)
            y, bar = hx.irfft1024(hx.rfft1024(0, x)), 2 * T.hard_bar(1024)
        elif name == "rfft512_pair":
            x = T.random_real(T.N_RANDOM, 1024, scale, 2010 + si)
            y, bar = hx.irfft512_pair(hx.rfft512_pair(0, x.reshape(-1, 2, 512))).reshape(-1, 1024), 2 * T.hard_bar(512)
        elif name == "fft1024c":
            x = T.random_complex(T.N_RANDOM, 1024, scale, 2020 + si)
            y, bar = hx.fft1024c(1, 3, 0, hx.fft1024c(0, 3, 0, x)) / np.float32(1024), 2 * T.hard_bar(1024)
        else:
            x = T.random_real(T.N_RANDOM, 2048, scale, 2030 + si)
            y, bar = hx.irfft2048(hx.rfft_sub(2048, x)), 2 * T.hard_bar(2048, T.MU_PRODUCT)
        e = T.norm_err(y, x.astype(np.complex128 if np.iscomplexobj(x) else np.float64))
        print("FIGURE round trip %s scale %g: largest normwise error %.3g (bar %.3g)" % (name, scale, e.max(), bar))
        assert e.max() <= bar, "%s round trip, scale %g, transform %d: %.3g over %.3g" % (name, scale, int(np.argmax(e)), e.max(), bar)


# ---- cases 5 and 6: exact scaling, the variants and the waves agree ------------------------------------------------------------------------
@pytest.mark.parametrize("x", XFORMS, ids=IDS)
def test_power_of_two_scaling_is_exact_and_waves_agree(hx, x):
    """No threshold or absolute constant hides in a transform: the input times 2^+-20 gives the output bits times 2^+-20 (nothing
    leaves the normal range).  The four waves of a workgroup (two workgroups) give the bits of wave 0 on the same input."""
    inp = x.random(6, 1.0, 3000)
    inp = np.concatenate([inp, np.repeat(inp[:1], 8, axis=0)])
    y0 = x.run(hx, inp)
    same = y0[6:].view(np.uint32)
    assert (same == same[:1]).all(), "%s: transform %d of 8 on one input differs from the first in %d words (wave %d of its workgroup)" % (
        x.name, int(np.argmax((same != same[:1]).any(axis=1))), int((same != same[:1]).sum()), (6 + int(np.argmax((same != same[:1]).any(axis=1)))) % 4)
    for e in (20, -20):
        s = np.float32(2.0 ** e)
        y = x.run(hx, inp * s)
        diff = y != y0 * s
        assert not diff.any(), "%s: input x 2^%d moves the bits of %d outputs; first: transform %d output %d (%s): %r against %r" % (
            x.name, e, int(diff.sum()), *np.argwhere(diff)[0], x.where_out(int(np.argwhere(diff)[0][1])), y[tuple(np.argwhere(diff)[0])], (y0 * s)[tuple(np.argwhere(diff)[0])])


@pytest.mark.parametrize("a,b", [("rfft1024<true>", "rfft1024<false>"), ("cfft512_regs<false, AHEAD>", "cfft512_regs<false>"),
                                 ("fft1024c<false, 7>", "fft1024c<false, 3>"), ("fft1024c<true, 7>", "fft1024c<true, 3>"),
                                 ("fft1024c<false, 3> row = lam", "fft1024c<false, 3>"), ("fft1024c<true, 3> row = lam", "fft1024c<true, 3>")])
def test_variants_agree_bit_for_bit(hx, a, b):
    xa, xb = BY_NAME[a], BY_NAME[b]
    for scale in T.SCALES:
        inp = xa.random(16, scale, 4000)
        ya, yb = xa.run(hx, inp).view(np.uint32), xb.run(hx, inp).view(np.uint32)
        assert np.array_equal(ya, yb), "%s against %s, scale %g: %d words differ, first at transform %d output %d" % (
            a, b, scale, int((ya != yb).sum()), int(np.argwhere(ya != yb)[0][0]), int(np.argwhere(ya != yb)[0][1]) // 2)


# ---- case 7: complex arithmetic ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", T.CARITH_OPS)
def test_complex_arithmetic(hx, op):
    acc, a, b = T.carith_operands()
    got = hx.carith(op, acc, a, b)
    if op in T.CARITH_TWO_ROUNDINGS:
        re, im, bar_re, bar_im = T.carith_ref(op, acc, a, b)
        for part, g, r, bar in (("real", got.real.astype(np.float64), re, bar_re), ("imaginary", got.imag.astype(np.float64), im, bar_im)):
            bad = np.abs(g - r) > bar
            assert not bad.any(), "%s, %s part, operand %d: acc %r a %r b %r gives %r, float64 %r, bar 2u (|p| + |q| + |acc|) = %.3g; %d of %d over" % (
                op, part, int(np.argmax(bad)), acc[np.argmax(bad)], a[np.argmax(bad)], b[np.argmax(bad)], g[np.argmax(bad)], r[np.argmax(bad)], bar[np.argmax(bad)],
                int(bad.sum()), len(bad))
    else:
        want = T.carith_exact32(op, a, b)
        bad = (got.real != want.real) | (got.imag != want.imag)
        assert not bad.any(), "%s (a single rounding: bit for bit), operand %d: a %r b %r gives %r, wanted %r; %d of %d differ" % (
            op, int(np.argmax(bad)), a[np.argmax(bad)], b[np.argmax(bad)], got[np.argmax(bad)], want[np.argmax(bad)], int(bad.sum()), len(bad))


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("points", [4, 8, 16])
def test_in_register_dfts(hx, points, inverse):
    """bfly4 / fft8 / fft16 in natural order (through br3 / dr16) against the float64 DFT of their inputs, per element, on the basis
    and on random input; the additions of bfly4 are single roundings: bit for bit against float32"""
    name = "%s<%s>" % ({4: "bfly4", 8: "fft8", 16: "fft16"}[points], "true" if inverse else "false")
    inp = np.concatenate([T.complex_basis(points)] + [T.random_complex(256, points, s, 5000 + points) for s in T.SCALES])
    got = hx.small_dft(points, inverse, inp)
    ref = T.ref_cfft(inp, inverse)
    bar = T.hard_bar(points)
    ref_max = np.abs(ref).max(axis=-1, keepdims=True)
    over = np.abs(got.astype(np.complex128) - ref) - bar * ref_max
    if (over > 0).any():
        i, k = np.unravel_index(np.argmax(over), over.shape)
        what = ("impulse %s at input %d" % ("1" if i < points else "j", i % points)) if i < 2 * points else "random input %d" % (i - 2 * points)
        raise AssertionError("%s: %s -> output %d (register %d): error %.3g of the largest output, bar B(%d, 4u) = %.3g" % (
            name, what, k, (T.br3(k) if points == 8 else T.dr16(k) if points == 16 else k), (over[i, k] + bar * ref_max[i, 0]) / ref_max[i, 0], points, bar))
    if points == 4:
        want = T.bfly4_f32(inp, inverse)
        bad = (got.real != want.real) | (got.imag != want.imag)
        assert not bad.any(), "%s: output %d of input %d differs from the float32 additions: %r against %r" % (
            name, int(np.argwhere(bad)[0][1]), int(np.argwhere(bad)[0][0]), got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------------
def _assert_table(table, got, ref, names, mask=None):
    err = np.abs(got.astype(np.complex128) - ref)
    if mask is not None:
        err = np.where(mask, err, 0.0)
    bad = err > T.MU_TABLE
    assert not bad.any(), "%s: entry %d, %s, is %r, float64 %r: off by %.3g = %.1f u, allowed mu = 4u (the assumption behind every hard bar); %d entries over" % (
        table, int(np.argmax(err)), names[int(np.argmax(err))], got[np.argmax(err)], ref[np.argmax(err)], err.max(), err.max() / T.U, int(bad.sum()))
    print("FIGURE table %s: largest |entry - float64| %.2f u" % (table, err.max() / T.U))


def test_fft_table_entries(hx):
    ref, names = T.fft_table_ref()
    _assert_table("fft_table_init without a window", hx.tables(0), ref, names)
    window = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(1024) / 1024)).astype(np.float32) + np.float32(0.125)
    got = hx.tables(1, window)
    _assert_table("fft_table_init with a window", got[:T.TW_WIN], ref, names)
    want = (np.float32(0.5) * window).view(np.complex64)
    bad = got[T.TW_WIN:].view(np.uint32).reshape(-1, 2) != want.view(np.uint32).reshape(-1, 2)
    assert not bad.any(), "fft_table_init: win[r = %d][lane = %d] is %r, half the window there is %r" % (
        int(np.argwhere(bad)[0][0]) >> 6, int(np.argwhere(bad)[0][0]) & 63, got[T.TW_WIN + np.argwhere(bad)[0][0]], want[np.argwhere(bad)[0][0]])


def test_f1k_table_entries(hx):
    ref, defined, names = T.f1k_table_ref()
    got = hx.tables(2)
    _assert_table("f1k_table_init", got, ref, names, defined)
    assert not got[~defined].any(), "f1k_table_init writes the padding words of a row"
    ref, names = T.f1k_wb_ref()
    _assert_table("F1kLane::init", hx.tables(3), ref, names)


# ---- case 8 and the other wave reductions ------------------------------------------------------------------------------------------------------
def test_max3abs_max2abs(hx):
    rng = np.random.default_rng(6000)
    x = (rng.standard_normal((4096, 3)) * 2.0 ** rng.integers(-30, 31, (4096, 3))).astype(np.float32)
    x[:64] = np.array([[a, b, c] for a in (-3.0, 0.0, 2.0, -0.0) for b in (5.0, -7.0, 0.0, 1.0) for c in (-11.0, 0.5, 0.0, 13.0)], dtype=np.float32)
    for three, name, want in ((1, "max3abs", np.abs(x).max(axis=1)), (0, "max2abs", np.abs(x[:, :2]).max(axis=1))):
        got = hx.maxabs(three, x)
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), "%s%r is %r, wanted %r; %d of %d differ" % (name, tuple(x[np.argmax(bad)][:3 if three else 2]), got[np.argmax(bad)], want[np.argmax(bad)], int(bad.sum()), len(bad))


@pytest.mark.parametrize("background", [0.5, 0.0])
def test_wave_max64_2_every_pair_of_lanes(hx, background):
    """a = 1 in lane p only, b = 1 in lane q only, for all 64 x 64 (p, q): both maxima are exactly 1 in every lane.  Pins the
    row_bcast masks at lanes 15 / 16, 31 / 32 and 47 / 48."""
    p, q = np.divmod(np.arange(4096), 64)
    ab = np.full((4096, 2, 64), background, dtype=np.float32)
    ab[np.arange(4096), 0, p] = 1.0
    ab[np.arange(4096), 1, q] = 1.0
    got = hx.wave_max64_2(ab)
    bad = got != 1.0
    if bad.any():
        w, ch, lane = np.argwhere(bad)[0]
        raise AssertionError("wave_max64_2, background %g: with a = 1 in lane %d and b = 1 in lane %d, lane %d reads max %s = %r; wrong for %d (p, q) pairs, the lanes p of a wrong result: %s" % (
            background, p[w], q[w], lane, "ab"[ch], got[w, ch, lane], int(bad.any(axis=(1, 2)).sum()), sorted(set(p[bad[:, 0].any(axis=1)].tolist()))[:16]))


# ---- case 9: the decisions of pair_balance ------------------------------------------------------------------------------------------------------
def test_pair_balance_decisions(hx):
    cases = T.pair_balance_cases()
    got = hx.pair_balance(np.stack([np.stack([ma, mb]) for _, ma, mb in cases]))
    for (name, ma, mb), g in zip(cases, got):
        want = T.pair_balance_int(ma, mb)
        assert tuple(int(v) for v in g) == want, "pair_balance, %s: (na, nb, alive_a, alive_b) = %r, the integer restatement gives %r" % (name, tuple(int(v) for v in g), want)


# ---- case 10: the balanced pair transform keeps each channel's own rounding ---------------------------------------------------------------------
@pytest.mark.parametrize("swap", [False, True], ids=["b_weaker", "a_weaker"])
@pytest.mark.parametrize("d", [0, 3, 4, 20, 40, 60, 80])
def test_balanced_pair_keeps_each_channels_rounding(hx, d, swap):
    """pair_balance_512 -> rfft512_pair -> pair_restore_512 with one channel at 2^-d of the other: each spectrum against the float64
    transform of THAT channel alone, relative to its OWN norm, B(512, 4u) (d = 80: times 2^(d - 60) for the weaker channel,
    PB_MAX_SHIFT caps the shift).  d < 4: the bits of the unbalanced transform."""
    pairs = np.stack([np.stack(T.level_pair(d, swap, 7000 + i)) for i in range(16)])
    got = hx.rfft512_pair(1, pairs)
    bar = T.hard_bar(512)
    weak = 0 if swap else 1
    for ch in (0, 1):
        e = T.norm_err(got[:, ch], T.ref_rfft(pairs[:, ch]))
        b = bar * (2.0 ** max(0, d - T.PB_MAX_SHIFT) if ch == weak else 1.0)
        print("FIGURE balanced pair d = %d %s channel %s: largest error relative to its own norm %.3g (bar %.3g)" % (d, "weaker" if ch == weak else "stronger", "ab"[ch], e.max(), b))
        assert e.max() <= b, "pair_balance_512 -> rfft512_pair -> pair_restore_512, channel %s (%s, 2^-%d): pair %d is off by %.3g of its own norm, bar %.3g" % (
            "ab"[ch], "weaker" if ch == weak else "stronger", d, int(np.argmax(e)), e.max(), b)
    if d < T.PB_MIN_SHIFT:
        plain = hx.rfft512_pair(0, pairs)
        assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)), "channels %d exponents apart: the balanced chain moves %d words of the unbalanced rfft512_pair" % (
            d, int((got.view(np.uint32) != plain.view(np.uint32)).sum()))


def test_balanced_pair_zero_channel_and_unbalanced_bar(hx):
    """A channel of exact zeros comes out as exact zeros (not its partner's rounding noise); rfft512_pair WITHOUT the balance is held
    to B relative to the pair's combined norm -- the header's stated reason for the balance."""
    a = T.random_real(8, 512, 1.0, 7100)
    z = np.zeros_like(a)
    for name, pairs, dead in (("b", np.stack([a, z], axis=1), 1), ("a", np.stack([z, a], axis=1), 0)):
        got = hx.rfft512_pair(1, pairs)
        assert not got[:, dead].view(np.uint32).any() or not np.abs(got[:, dead]).any(), "channel %s of exact zeros comes out with %d non-zero bins, largest %.3g" % (
            name, int((np.abs(got[:, dead]) > 0).sum()), np.abs(got[:, dead]).max())
        assert T.norm_err(got[:, 1 - dead], T.ref_rfft(pairs[:, 1 - dead])).max() <= T.hard_bar(512)
    for d in (20, 40):
        pairs = np.stack([np.stack(T.level_pair(d, False, 7200 + i)) for i in range(16)])
        got = hx.rfft512_pair(0, pairs).reshape(16, -1)
        ref = np.concatenate([T.ref_rfft(pairs[:, 0]), T.ref_rfft(pairs[:, 1])], axis=-1)
        e = T.norm_err(got, ref)
        assert e.max() <= T.hard_bar(512), "rfft512_pair without the balance, channels 2^-%d apart: %.3g of the pair's combined norm, bar %.3g" % (d, e.max(), T.hard_bar(512))
