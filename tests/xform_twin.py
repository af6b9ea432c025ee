"""The twin of tests/cxx/xform_harness.hip: float64 references, inputs and error bars for the wave-level transforms and packed
complex products of csrc/fft512.h, fft1024c.h, fft_block.h and pair_balance.h, and the ctypes binding of the harness library.
Importable without a GPU (tests/test_xform_twin.py checks the twin itself; tests/test_gpu_xform.py checks the kernels against it).

Conventions (the header comments): unnormalised forward; 1/N inverse for irfft1024 / the 2048 chain, 1/512 for irfft512_pair,
unnormalised for cfft512_regs<true>, fft1024c<true> and block_ifft_dif; one-sided (CCS) bin order k = 0..N/2; the imaginary parts of
DC and Nyquist are ignored by the real-output inverses.

Bars
  arithmetic   the float64 value of the documented formula; a two-instruction product may be off by 2u (|p| + |q|) per component
               (u = 2^-24; p, q the two exact products of the component: one rounding of the first product, one of the fma), the
               accumulating forms by 2u (|p| + |q| + |acc|).  Single roundings are compared bit for bit.
  hard         Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2: an FFT whose twiddles are off by at most mu obeys
               ||y^ - y|| <= B ||y||,  B = L eta / (1 - L eta),  L = log2 N,  eta = mu + gamma4 (sqrt 2 + mu),  gamma4 = 4u / (1 - 4u).
               mu = 4u where a twiddle comes straight from a table, 16u where it is a product of up to three entries (2048 / 4096).
  elementwise  for inputs whose outputs all have one modulus (an impulse; a unit bin into an inverse): |y^[k] - y[k]| <= B max|y|.
  tight        random inputs only: at most TIGHT_FACTOR x the normwise error numpy's own single-precision transform makes on the same
               input (4 x for twiddles that carry up to an ulp each through three products per point, 4 x for the spread between
               inputs; a lower precision class sits more than 2^8 above)."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "cxx", "libxform_harness.so")

U = 2.0 ** -24
MU_TABLE = 4 * U
MU_PRODUCT = 16 * U
TIGHT_FACTOR = 16.0
SCALES = (1.0, 32768.0, 1e-6)          # unit, 16-bit PCM as float, small
N_RANDOM = 64


def hard_bar(n, mu=MU_TABLE):
    g4 = 4 * U / (1 - 4 * U)
    eta = mu + g4 * (np.sqrt(2.0) + mu)
    le = np.log2(n) * eta
    return le / (1 - le)


# ---- index maps of the headers ------------------------------------------------------------------------------------------------------
def br3(i):
    return ((i & 1) << 2) | (i & 2) | ((i >> 2) & 1)


def dr16(p):
    return (p >> 2) + 4 * (p & 3)


def bitrev(i, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (i & 1)
        i >>= 1
    return r


def bitrev_perm(bits):
    return np.array([bitrev(i, bits) for i in range(1 << bits)], dtype=np.int64)


def undo_bitrev(raw, logh):
    """block_ifft_dif leaves y[k] at position bitrev(k)."""
    return np.ascontiguousarray(np.asarray(raw)[..., bitrev_perm(logh)])


def lam_of(lane):
    return lane if lane <= 32 else 96 - lane


def where_wave(index, regmap=None):
    """lane / register of element `index` under the distribution index = lane + 64 * position (regmap: position -> register)."""
    lane, pos = int(index) & 63, int(index) >> 6
    return "lane %d register %d" % (lane, regmap(pos) if regmap else pos)


# ---- references (float64) -----------------------------------------------------------------------------------------------------------
def dft_direct(x, inverse=False):
    """O(N^2) float64 DFT along the last axis, unnormalised in both directions."""
    x = np.asarray(x, dtype=np.complex128)
    n = x.shape[-1]
    k = np.arange(n)
    w = np.exp((2j if inverse else -2j) * np.pi * np.outer(k, k) / n)
    return x @ w


def _c(x):
    return np.asarray(x, dtype=np.complex128)


def _r(x):
    return np.asarray(x, dtype=np.float64)


def _ccs_real_ends(spec):
    spec = _c(spec).copy()
    spec[..., 0] = spec[..., 0].real
    spec[..., -1] = spec[..., -1].real
    return spec


def ref_cfft(z, inverse=False):
    """cfft512_regs / fft1024c / fft8 / fft16 / bfly4 / block_ifft_dif: unnormalised both ways."""
    z = _c(z)
    return np.fft.ifft(z, axis=-1) * z.shape[-1] if inverse else np.fft.fft(z, axis=-1)


def ref_rfft(x):
    """rfft1024 (of x: the kernel's caller hands over (x[2m], x[2m+1]) / 2), rfft512_pair per channel, the 2048 / 4096 chains,
    load_frames -> block_fft_dit -> split_forward (of x * window)."""
    return np.fft.rfft(_r(x), axis=-1)


def ref_irfft(spec):
    """irfft1024, irfft512_pair per channel, split2048_inv -> irfft512_pair: 1/N, imaginary parts of DC and Nyquist ignored."""
    spec = _ccs_real_ends(spec)
    return np.fft.irfft(spec, n=2 * (spec.shape[-1] - 1), axis=-1)


def half_packed(x):
    """what rfft1024's caller passes: z[m] = (x[2m] + j x[2m+1]) / 2"""
    x = _r(x)
    return 0.5 * (x[..., 0::2] + 1j * x[..., 1::2])


def rfft_from_half_packed(z):
    """The split step of rfft1024 restated: X[k] from the H-point transform of the half-packed sequence."""
    z = _c(z)
    h = z.shape[-1]
    zf = np.fft.fft(z, axis=-1)
    zk = np.concatenate([zf, zf[..., :1]], axis=-1)
    zp = np.conj(zk[..., ::-1])
    k = np.arange(h + 1)
    return (zk + zp) + np.exp(-2j * np.pi * k / (2 * h)) * (-1j) * (zk - zp)


def rfft_by_subsequences(x, r):
    """The 2048 / 4096 chain restated: X[k] = sum_q W_N^(q k) S_q[k mod (N / r)], S_q the transform of x[r n + q]."""
    x = _r(x)
    n = x.shape[-1]
    m = n // r
    k = np.arange(n // 2 + 1)
    out = np.zeros(x.shape[:-1] + (n // 2 + 1,), dtype=np.complex128)
    for q in range(r):
        s = np.fft.fft(x[..., q::r], axis=-1)
        out += np.exp(-2j * np.pi * q * k / n) * s[..., k % m]
    return out


# the single-precision reference of the tight bar: numpy (>= 2.0) transforms complex64 / float32 in single precision
def np32_cfft(z, inverse=False):
    z = np.asarray(z, dtype=np.complex64)
    y = np.fft.ifft(z, axis=-1, norm="forward") if inverse else np.fft.fft(z, axis=-1)
    assert y.dtype == np.complex64
    return y


def np32_rfft(x):
    y = np.fft.rfft(np.asarray(x, dtype=np.float32), axis=-1)
    assert y.dtype == np.complex64
    return y


def np32_irfft(spec):
    spec = _ccs_real_ends(spec).astype(np.complex64)
    y = np.fft.irfft(spec, n=2 * (spec.shape[-1] - 1), axis=-1)
    assert y.dtype == np.float32
    return y


def norm_err(got, ref):
    """normwise relative error per transform (last axis)"""
    got, ref = np.asarray(got), np.asarray(ref)
    d = np.linalg.norm((got.astype(ref.dtype) - ref).reshape(ref.shape[0], -1), axis=1)
    return d / np.linalg.norm(ref.reshape(ref.shape[0], -1), axis=1)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def random_real(n_transforms, length, scale, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_transforms, length)) * scale).astype(np.float32)


def random_complex(n_transforms, length, scale, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((n_transforms, length)) + 1j * rng.standard_normal((n_transforms, length))) * scale).astype(np.complex64)


def complex_basis(n):
    """impulse 1 and impulse j at every index: [2 n][n]; row i < n has 1 at i, row n + i has j at i"""
    e = np.eye(n, dtype=np.complex64)
    return np.concatenate([e, 1j * e], axis=0)


def real_basis(n, first=0, count=None):
    count = n - first if count is None else count
    e = np.zeros((count, n), dtype=np.float32)
    e[np.arange(count), first + np.arange(count)] = 1.0
    return e


def ccs_basis(n):
    """a unit real bin at every k = 0..n/2 and a unit imaginary bin at every k = 1..n/2-1: ([n][n/2+1], list of (k, part))"""
    kk = n // 2 + 1
    rows, tags = [], []
    for k in range(kk):
        v = np.zeros(kk, dtype=np.complex64); v[k] = 1.0
        rows.append(v); tags.append((k, "re"))
    for k in range(1, kk - 1):
        v = np.zeros(kk, dtype=np.complex64); v[k] = 1j
        rows.append(v); tags.append((k, "im"))
    return np.stack(rows), tags


# ---- complex arithmetic -----------------------------------------------------------------------------------------------------------------
CARITH_OPS = ("cmul", "cmulc", "cmac", "cmacc", "cnmac", "cnmacc", "csub_jb", "cadd_jb", "cscale", "cmul_mj", "cmul_pj")
CARITH_TWO_ROUNDINGS = CARITH_OPS[:6]


def carith_ref(op, acc, a, b):
    """-> (re, im, bar_re, bar_im) in float64 for the two-instruction products; operands are complex arrays of float32 values
    (their products are exact in float64)."""
    acc, a, b = _c(acc), _c(a), _c(b)
    ax, ay, bx, by, cx, cy = a.real, a.imag, b.real, b.imag, acc.real, acc.imag
    if op == "cmul":        # (a.x b.x - a.y b.y, a.x b.y + a.y b.x)
        t = (ax * bx, -ay * by, ax * by, ay * bx, 0 * cx, 0 * cy)
    elif op == "cmulc":     # a conj(b) = (a.x b.x + a.y b.y, a.y b.x - a.x b.y)
        t = (ax * bx, ay * by, ay * bx, -ax * by, 0 * cx, 0 * cy)
    elif op == "cmac":
        t = (ax * bx, -ay * by, ax * by, ay * bx, cx, cy)
    elif op == "cmacc":
        t = (ax * bx, ay * by, ay * bx, -ax * by, cx, cy)
    elif op == "cnmac":
        t = (-ax * bx, ay * by, -ax * by, -ay * bx, cx, cy)
    elif op == "cnmacc":
        t = (-ax * bx, -ay * by, -ay * bx, ax * by, cx, cy)
    else:
        raise ValueError(op)
    p_re, q_re, p_im, q_im, c_re, c_im = t
    return (p_re + q_re + c_re, p_im + q_im + c_im,
            2 * U * (np.abs(p_re) + np.abs(q_re) + np.abs(c_re)), 2 * U * (np.abs(p_im) + np.abs(q_im) + np.abs(c_im)))


def carith_exact32(op, a, b):
    """the single-rounding forms, in float32 like the instruction: -> complex64"""
    a, b = np.asarray(a, dtype=np.complex64), np.asarray(b, dtype=np.complex64)
    ax, ay, bx, by = a.real, a.imag, b.real, b.imag
    if op == "csub_jb":     # a - j b
        re, im = ax + by, ay - bx
    elif op == "cadd_jb":   # a + j b
        re, im = ax - by, ay + bx
    elif op == "cscale":    # a * b.x
        re, im = ax * bx, ay * bx
    elif op == "cmul_mj":   # -j a
        re, im = ay, -ax
    elif op == "cmul_pj":   # +j a
        re, im = -ay, ax
    else:
        raise ValueError(op)
    return (re.astype(np.float32) + 1j * im.astype(np.float32)).astype(np.complex64)


def bfly4_f32(x, inverse=False):
    """bfly4 in float32, addition by addition: [..., 4] complex64 -> [..., 4]"""
    x = np.asarray(x, dtype=np.complex64)
    a0, a1, a2, a3 = (x[..., i] for i in range(4))
    t0, t1, t2, t3 = a0 + a2, a0 - a2, a1 + a3, a1 - a3
    mj, pj = carith_exact32("csub_jb", t1, t3), carith_exact32("cadd_jb", t1, t3)
    return np.stack([t0 + t2, pj if inverse else mj, t0 - t2, mj if inverse else pj], axis=-1).astype(np.complex64)


def carith_operands():
    """(acc, a, b): (3, -5) (7, 11) under its 16 sign patterns with an accumulator of two more magnitudes under its 4, operands with
    zero components, and 4096 random triples with magnitudes over 2^+-30 -- a swapped half or a wrong sign cannot cancel"""
    acc, a, b = [], [], []
    for s in range(16):
        for t in range(4):
            a.append(complex(3 * (-1) ** (s & 1), -5 * (-1) ** ((s >> 1) & 1)))
            b.append(complex(7 * (-1) ** ((s >> 2) & 1), 11 * (-1) ** ((s >> 3) & 1)))
            acc.append(complex(13 * (-1) ** (t & 1), 17 * (-1) ** ((t >> 1) & 1)))
    for z in range(16):     # zero components: bit i of z clears a.x, a.y, b.x, b.y
        a.append(complex(0 if z & 1 else 3, 0 if z & 2 else -5))
        b.append(complex(0 if z & 4 else 7, 0 if z & 8 else 11))
        acc.append(complex(13, -17) if z & 1 else 0j)
    rng = np.random.default_rng(20240607)

    def mag(n):
        return (rng.choice([-1.0, 1.0], n) * rng.uniform(1, 2, n) * 2.0 ** rng.integers(-30, 31, n)).astype(np.float32)
    n = 4096
    ra, rb, rc = mag(n) + 1j * mag(n), mag(n) + 1j * mag(n), mag(n) + 1j * mag(n)
    f = lambda lst, r: np.concatenate([np.array(lst, dtype=np.complex64), r.astype(np.complex64)])
    return f(acc, rc), f(a, ra), f(b, rb)


# ---- pair_balance -------------------------------------------------------------------------------------------------------------------
PB_MIN_SHIFT, PB_SCREEN, PB_MAX_SHIFT = 4, 8.0, 60


def pair_balance_int(ma, mb):
    """pair_balance restated on the bits: the per-lane screen in float32, the exponent fields of the two wave maxima.
    -> (na, nb, alive_a, alive_b)"""
    ma, mb = np.asarray(ma, dtype=np.float32), np.asarray(mb, dtype=np.float32)
    na = nb = 0
    alive_a, alive_b = int(np.any(ma > 0)), int(np.any(mb > 0))
    s = np.float32(PB_SCREEN)
    if np.any(ma > s * mb) or np.any(mb > s * ma):
        ba, bb = int(ma.max().view(np.uint32)), int(mb.max().view(np.uint32))
        if ba != 0 and bb != 0:
            d = (ba >> 23) - (bb >> 23)
            n = min(abs(d), PB_MAX_SHIFT)
            if n >= PB_MIN_SHIFT:
                na, nb = (n if d < 0 else 0), (n if d > 0 else 0)
    return na, nb, alive_a, alive_b


def pair_balance_f64(ma, mb):
    """the rule as the header states it: a channel whose largest sample lies PB_MIN_SHIFT or more binary exponents below its
    partner's goes through the transform multiplied by 2^(exponents apart), at most 2^PB_MAX_SHIFT; zeros stay zeros"""
    ma, mb = _r(ma), _r(mb)
    xa, xb = ma.max(), mb.max()
    na = nb = 0
    if xa > 0 and xb > 0:
        d = int(np.frexp(xa)[1]) - int(np.frexp(xb)[1])
        n = min(abs(d), PB_MAX_SHIFT)
        if n >= PB_MIN_SHIFT:
            na, nb = (n if d < 0 else 0), (n if d > 0 else 0)
    return na, nb, int(xa > 0), int(xb > 0)


def pair_balance_cases():
    """[(name, ma[64], mb[64])]: maxima 0, 3, 4, 5, 59, 60, 61 and 100 exponents apart in both directions, mantissas on either side
    (so that "a factor 8 apart" and "4 exponents apart" disagree), the maxima in lanes 0, 31, 32, 63; a channel of zeros, both zero,
    a single non-zero sample"""
    cases = []
    lanes = (0, 31, 32, 63)
    for d in (0, 3, 4, 5, 59, 60, 61, 100):
        for m_hi, m_lo in ((1.0, 1.0), (1.125, 1.875), (1.875, 1.125)):
            for pa in lanes:
                for pb in lanes:
                    hi, lo = np.float32(m_hi * 2.0 ** (d - d // 2)), np.float32(m_lo * 2.0 ** (-(d // 2)))
                    s = np.full(64, hi * np.float32(0.25), dtype=np.float32); s[pa] = hi
                    w = np.full(64, lo * np.float32(0.25), dtype=np.float32); w[pb] = lo
                    cases.append(("a %d exponents above b, mantissas %g / %g, maxima in lanes %d / %d" % (d, m_hi, m_lo, pa, pb), s, w))
                    s2 = np.full(64, hi * np.float32(0.25), dtype=np.float32); s2[pb] = hi
                    w2 = np.full(64, lo * np.float32(0.25), dtype=np.float32); w2[pa] = lo
                    cases.append(("b %d exponents above a, mantissas %g / %g, maxima in lanes %d / %d" % (d, m_hi, m_lo, pa, pb), w2, s2))
    z = np.zeros(64, dtype=np.float32)
    for p in lanes:
        live = np.full(64, 0.25, dtype=np.float32); live[p] = 1.5
        one = z.copy(); one[p] = 3e-5
        cases.append(("b exact zeros, maximum of a in lane %d" % p, live, z))
        cases.append(("a exact zeros, maximum of b in lane %d" % p, z, live))
        cases.append(("a single non-zero sample of a in lane %d" % p, one, z))
        cases.append(("a single non-zero sample of b in lane %d" % p, z, one))
        cases.append(("a single non-zero sample of a in lane %d beside a live b" % p, one, live))
    cases.append(("both channels exact zeros", z, z))
    return cases


def level_pair(d, swap, seed):
    """two 512-sample channels, the largest sample of the weaker exactly d binary exponents below the stronger's (same mantissa)"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(512)
    g = rng.standard_normal(512)
    b = g * (np.abs(a).max() / np.abs(g).max()) * 2.0 ** -d
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    b32[np.argmax(np.abs(g))] = np.float32(np.sign(g[np.argmax(np.abs(g))])) * np.abs(a32).max() * np.float32(2.0 ** -d)
    return (b32, a32) if swap else (a32, b32)


def lane_maxima_512(x):
    """per lane, the largest |x[lane + 64 r]| / 2 of a 512-sample channel (what pair_balance_512 hands to pair_balance)"""
    return np.abs(np.asarray(x, dtype=np.float32).reshape(8, 64) * np.float32(0.5)).max(axis=0)


# ---- the device tables ----------------------------------------------------------------------------------------------------------------
TW_T1, TW_T2, TW_TS, TW_WIN, TW_WORDS = 0, 512, 576, 832, 1344
F1K_ROW = 18


def _w(num, den):
    return np.exp(-2j * np.pi * np.asarray(num, dtype=np.float64) / den)


def fft_table_ref():
    """-> (values[TW_WIN], names[TW_WIN]) of fft_table_init"""
    v, names = np.zeros(TW_WIN, dtype=np.complex128), [None] * TW_WIN
    for q in range(8):
        for lane in range(64):
            v[TW_T1 + q * 64 + lane] = _w(lane * q, 512); names[TW_T1 + q * 64 + lane] = "t1[q=%d][lane=%d]" % (q, lane)
    for s in range(8):
        for l0 in range(8):
            v[TW_T2 + s * 8 + l0] = _w(l0 * s, 64); names[TW_T2 + s * 8 + l0] = "t2[s=%d][l0=%d]" % (s, l0)
    for i in range(4):
        for lane in range(64):
            v[TW_TS + i * 64 + lane] = _w(lane + 64 * i, 1024); names[TW_TS + i * 64 + lane] = "ts[i=%d][lane=%d]" % (i, lane)
    return v, names


def f1k_table_ref():
    """-> (values[64 * 18], defined[64 * 18], names) of f1k_table_init (words 16, 17 of a row are padding)"""
    v = np.zeros(64 * F1K_ROW, dtype=np.complex128)
    defined = np.zeros(64 * F1K_ROW, dtype=bool)
    names = ["pad"] * (64 * F1K_ROW)
    for lane in range(64):
        for q in range(16):
            v[lane * F1K_ROW + q] = _w(lane * q, 1024); defined[lane * F1K_ROW + q] = True
            names[lane * F1K_ROW + q] = "tab[lane=%d][q=%d]" % (lane, q)
    return v, defined, names


def f1k_wb_ref():
    v = np.array([[_w((lane & 15) * q, 64) for q in (1, 2, 3)] for lane in range(64)]).reshape(-1)
    return v, ["wb[%d] of lane %d" % (q, lane) for lane in range(64) for q in (1, 2, 3)]


# ---- the harness library -----------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = ("xh_carith", "xh_small_dft", "xh_maxabs", "xh_wave_max64_2", "xh_pair_balance", "xh_table_words", "xh_tables",
                "xh_cfft512", "xh_rfft1024", "xh_irfft1024", "xh_rfft512_pair", "xh_irfft512_pair", "xh_rfft_sub", "xh_irfft2048",
                "xh_fft1024c", "xh_block_rfft", "xh_block_ifft")


class HipError(RuntimeError):
    def __init__(self, entry, code):
        super().__init__("%s returned hipError_t %d" % (entry, code))
        self.entry, self.code = entry, code


def _c2f(z):
    """complex64 [n] -> float32 [n, 2]"""
    return np.ascontiguousarray(z, dtype=np.complex64).view(np.float32).reshape(-1, 2)


class Harness:
    """libxform_harness.so through ctypes: numpy in, numpy out; a non-zero hipError_t raises HipError"""

    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise FileNotFoundError("%s is missing: run build() of __graft_entry__.py (make -C tests/cxx)" % path)
        self.lib = C.CDLL(path)

    def _call(self, name, *args):
        fn = getattr(self.lib, name)
        fn.restype = C.c_int
        conv = []
        for a in args:
            if isinstance(a, np.ndarray):
                assert a.flags["C_CONTIGUOUS"]
                conv.append(a.ctypes.data_as(C.c_void_p))
            elif a is None:
                conv.append(C.c_void_p(None))
            else:
                conv.append(C.c_int(int(a)))
        rc = fn(*conv)
        if rc != 0:
            raise HipError(name, rc)

    def carith(self, op, acc, a, b):
        n = len(a)
        inp = np.ascontiguousarray(np.stack([_c2f(acc), _c2f(a), _c2f(b)], axis=1))
        out = np.zeros(n, dtype=np.complex64)
        self._call("xh_carith", CARITH_OPS.index(op), inp, out, n)
        return out

    def small_dft(self, points, inverse, x):
        x = np.ascontiguousarray(x, dtype=np.complex64)
        assert x.shape[-1] == points
        out = np.zeros_like(x)
        self._call("xh_small_dft", points, int(inverse), x, out, x.size // points)
        return out

    def maxabs(self, three, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.shape[-1] == 3
        out = np.zeros(x.shape[0], dtype=np.float32)
        self._call("xh_maxabs", int(three), x, out, x.shape[0])
        return out

    def wave_max64_2(self, ab):
        ab = np.ascontiguousarray(ab, dtype=np.float32)
        assert ab.shape[1:] == (2, 64)
        out = np.zeros_like(ab)
        self._call("xh_wave_max64_2", ab, out, ab.shape[0])
        return out

    def pair_balance(self, mab):
        mab = np.ascontiguousarray(mab, dtype=np.float32)
        assert mab.shape[1:] == (2, 64)
        out = np.zeros((mab.shape[0], 4), dtype=np.int32)
        self._call("xh_pair_balance", mab, out, mab.shape[0])
        return out

    def tables(self, which, window=None):
        words = {0: TW_WIN, 1: TW_WORDS, 2: 64 * F1K_ROW, 3: 192}[which]
        out = np.zeros(words, dtype=np.complex64)
        w = None if window is None else np.ascontiguousarray(window, dtype=np.float32)
        self._call("xh_tables", which, w, out)
        return out

    def _xf(self, name, head, x, in_dtype, in_len, out_dtype, out_len):
        x = np.ascontiguousarray(x, dtype=in_dtype)
        assert x.shape[-1] == in_len, (name, x.shape, in_len)
        lead = x.shape[:-1]
        out = np.zeros(lead + (out_len,), dtype=out_dtype)
        self._call(name, *head, x, out, int(np.prod(lead, dtype=np.int64)))
        return out

    def cfft512(self, variant, z):                      # 0 forward, 1 forward AHEAD, 2 inverse
        return self._xf("xh_cfft512", (variant,), z, np.complex64, 512, np.complex64, 512)

    def rfft1024(self, ahead, x):
        return self._xf("xh_rfft1024", (int(ahead),), x, np.float32, 1024, np.complex64, 513)

    def irfft1024(self, spec):
        return self._xf("xh_irfft1024", (), spec, np.complex64, 513, np.float32, 1024)

    def rfft512_pair(self, balance, ab):                # [..., 2, 512] -> [..., 2, 257]
        ab = np.ascontiguousarray(ab, dtype=np.float32)
        assert ab.shape[-2:] == (2, 512)
        out = self._xf("xh_rfft512_pair", (int(balance),), ab.reshape(ab.shape[:-2] + (1024,)), np.float32, 1024, np.complex64, 514)
        return out.reshape(ab.shape[:-2] + (2, 257))

    def irfft512_pair(self, spec):                      # [..., 2, 257] -> [..., 2, 512]
        spec = np.ascontiguousarray(spec, dtype=np.complex64)
        assert spec.shape[-2:] == (2, 257)
        out = self._xf("xh_irfft512_pair", (), spec.reshape(spec.shape[:-2] + (514,)), np.complex64, 514, np.float32, 1024)
        return out.reshape(spec.shape[:-2] + (2, 512))

    def rfft_sub(self, n, x):                           # n = 2048, 4096
        return self._xf("xh_rfft_sub", (n,), x, np.float32, n, np.complex64, n // 2 + 1)

    def irfft2048(self, spec):
        return self._xf("xh_irfft2048", (), spec, np.complex64, 1025, np.float32, 2048)

    def fft1024c(self, inverse, opt, perm, z):
        return self._xf("xh_fft1024c", (int(inverse), opt, int(perm)), z, np.complex64, 1024, np.complex64, 1024)

    def block_rfft(self, logh, x, window=None):         # [n, nch, 2 H] -> [n, nch, H + 1]
        x = np.ascontiguousarray(x, dtype=np.float32)
        h = 1 << logh
        n, nch = x.shape[0], x.shape[1]
        assert x.shape == (n, nch, 2 * h)
        w = np.ones(2 * h, dtype=np.float32) if window is None else np.ascontiguousarray(window, dtype=np.float32)
        out = np.zeros((n, nch, h + 1), dtype=np.complex64)
        self._call("xh_block_rfft", logh, nch, x, w, out, n)
        return out

    def block_ifft(self, logh, z):                      # [n, nch, H] natural -> [n, nch, H] as the kernel leaves it (bit-reversed)
        z = np.ascontiguousarray(z, dtype=np.complex64)
        n, nch = z.shape[0], z.shape[1]
        assert z.shape == (n, nch, 1 << logh)
        out = np.zeros_like(z)
        self._call("xh_block_ifft", logh, nch, z, out, n)
        return out
