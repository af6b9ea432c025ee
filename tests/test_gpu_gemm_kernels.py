"""GPU, kernel level: every contraction kernel of csrc/kernels_gemm.hip but the fold one (tests/test_gpu_gemm_fold.py) and the two in-order
plane sums of csrc/kernels_stream.hip, through the test-only launchers of tests/cxx/gemm_harness.hip / gemm_harness_stream.hip, against
the float64 twin tests/gemm_twin.py (pinned by tests/test_gemm_twin.py).

Three families of operands per kernel:
  basis   A is a permutation matrix (row f has one 1.0 at k = pi(f); for the two-plane kernels once in the hi and once in the lo plane),
          B random in every column: the map summed over its planes is the table column of pi(f), the plane of the K segment that owns
          pi(f) holds it and every other plane an exact +0 -- bit for bit.  Pins every K index, stage, ring slot, swizzle, fragment lane,
          output row and column and the owning segment.
  ints    uniform integers in [-3, 3] in every plane at the product's depths: every partial sum is an integer below 2^24, so the result
          is the int64 product whatever the order -- bit for bit.
  gauss   A standard normal, B uniform in [-1, 1], rounded to the operand type (two planes: hi = fp16(x), lo = fp16(x - hi)); reference:
          the float64 value of the kernel's formula on the rounded operands; bar per element and plane n u sum |a| |b| (u = 2^-24, n =
          terms of the segment; three products: 3 n and the three magnitudes), for the planes summed the sum of those plus u |ref|; two
          planes also against the float64 product of the unsplit values, + 2^-22 sum |a| |b| for the dropped lo x lo term.
          Normwise, ||c^ - c|| / ||c||: at most twice that of one sequential float32 accumulation of the same products (k ascending).
Every case: rows behind `rows` and frames outside [frame0, frame0 + chunk_frames) keep their NaN, no NaN where a result belongs, the plane
of an empty K segment is exact zeros.  The row padding the 256-row kernels load is NaN: no row reads another.

Every call checks the hipError_t the harness returns; after the first non-zero one every later test of the module skips (nothing more
goes to a GPU that has just reported a fault)."""
import ctypes
import os

import numpy as np
import pytest

import gemm_twin as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = T.U
_FAULT = {"err": None}
P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "tests", "cxx", "libgemm_harness.so")
    if not os.path.exists(path):
        pytest.fail("%s is missing: build() makes it (tests/cxx/gemm_harness.mk)" % path)
    h = ctypes.CDLL(path)
    for name, args in (("gh_f32", [P, P, I, I, I, I, I, I, I, P]), ("gh_f16", [I, I, P, P, I, I, I, I, I, I, I, P]),
                       ("gh_repair", [I, P, P, I, I, I, I, I, I, I, I, P]), ("gh_v2", [P, P, I, I, I, I, I, I, P]),
                       ("gh_v3", [P, P, I, I, I, I, I, I, P, P, P, I, I, P]), ("gh_sum_planes", [P, LL, I, LL]),
                       ("gh_repair_patch", [P, I, I, I, P, I, I, I, I, P, I, P, I, LL, I, I, I, P, I, I])):
        getattr(h, name).restype = I
        getattr(h, name).argtypes = args
    h.gh_constants.restype = None
    h.gh_constants.argtypes = [P]
    return h


@pytest.fixture(scope="module")
def consts(lib):
    out = np.zeros(5, np.int32)
    lib.gh_constants(out.ctypes.data)
    return dict(zip(("REPAIR_GROUP", "HIST_FRAMES", "HIST_UNITS", "REPAIR_KSPLIT_MAX", "FOLD_NS"), (int(v) for v in out)))


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _FAULT["err"]:
        pytest.skip("an earlier call failed (%s): nothing more goes to this GPU" % _FAULT["err"])


def call(fn, *args):
    err = fn(*args)
    if err:
        _FAULT["err"] = "hipError_t %d" % err
    assert err == 0


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_bits(got, want):
    return np.array_equal(bits(got), bits(want))


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
# name: (launcher kind, operand planes, K step, row tile, column tile)
KERNELS = {"f32": ("f32", 1, 16, 128, 192), "f16_192": ("f16", 1, 32, 128, 192), "f16x3_192": ("f16", 2, 32, 128, 192), "f16_64": ("f16", 1, 32, 128, 64),
           "f16x3_64": ("f16", 2, 32, 128, 64), "v3": ("v", 1, 32, 256, 384), "v2": ("v", 2, 32, 256, 384)}


def launch(lib, kern, a_planes, b_planes, rows, chunk, total, frame0, ksplit, part_args=None):
    """a_planes: list of [rows][Kp], b_planes: list of [Kp][Dp], in the operand type -> C [ksplit][arrays * total][Dp] float32 (NaN where nothing was written)"""
    kind, planes, _, bm, bn = KERNELS[kern]
    Kp, Dp = b_planes[0].shape
    assert len(a_planes) == len(b_planes) == planes and a_planes[0].shape == (rows, Kp)
    na = T.n_arrays(rows, chunk)
    C = np.full((ksplit, na * total, Dp), np.nan, np.float32)
    if kind == "f32":
        A, B = np.ascontiguousarray(a_planes[0], np.float32), np.ascontiguousarray(b_planes[0], np.float32)
        call(lib.gh_f32, A.ctypes.data, B.ctypes.data, rows, chunk, total, frame0, Kp, Dp, ksplit, C.ctypes.data)
        return C
    A = np.concatenate([np.asarray(a, np.float16) for a in a_planes], axis=1)                 # [rows][planes * Kp], lo behind hi
    B = np.ascontiguousarray(np.stack([np.asarray(b, np.float16).T for b in b_planes]))       # [planes][Dp][Kp]
    if kind == "f16":
        A = np.ascontiguousarray(A)
        call(lib.gh_f16, planes, bn, A.ctypes.data, B.ctypes.data, rows, chunk, total, frame0, Kp, Dp, ksplit, C.ctypes.data)
        return C
    Apad = np.full(((rows + 255) // 256 * 256, planes * Kp), np.nan, np.float16)               # the kernel loads whole 256-row tiles
    Apad[:rows] = A
    Bt = T.tile_bt(B)
    if planes == 2:
        call(lib.gh_v2, Apad.ctypes.data, Bt.ctypes.data, rows, chunk, total, frame0, Kp, ksplit, C.ctypes.data)
    elif part_args is None:
        call(lib.gh_v3, Apad.ctypes.data, Bt.ctypes.data, rows, chunk, total, frame0, Kp, ksplit, C.ctypes.data, None, None, 0, 0, None)
    else:
        part, nv, D, n_chunks, w = part_args
        call(lib.gh_v3, Apad.ctypes.data, Bt.ctypes.data, rows, chunk, total, frame0, Kp, ksplit, C.ctypes.data, part.ctypes.data, nv.ctypes.data, D, n_chunks, w.ctypes.data)
    return C


def written_rows(C, rows, chunk, total, frame0):
    """asserts that exactly the mapped rows were written, whole; -> got [ksplit][rows][Dp]"""
    _, _, flat = T.row_map(rows, chunk, total, frame0)
    mask = np.zeros(C.shape[1], bool)
    mask[flat] = True
    assert np.isnan(C[:, ~mask]).all(), "a row behind `rows` or a frame outside the chunk was written"
    assert not np.isnan(C[:, mask]).any(), "NaN (or nothing) where a result belongs"
    return C[:, flat]


def operand_type(kern):
    return np.float32 if kern == "f32" else np.float16


# ---- basis ---------------------------------------------------------------------------------------------------------------------------
BASIS = ([("f32", 2080, 192, 1), ("f32", 2080, 384, 16), ("f32", 2080, 576, 14)] +
         [(k, 2080, Dp, ks) for k in ("f16_192", "f16x3_192") for Dp, ks in ((192, 1), (384, 8), (576, 16))] +
         [(k, 2080, 64, ks) for k in ("f16_64", "f16x3_64") for ks in (1, 2, 16)] +
         [(k, Kp, 384, ks) for k in ("v3", "v2") for Kp in (32, 64, 96, 128, 160, 2080) for ks in (1, 2, 4)])


@pytest.mark.parametrize("kern,Kp,Dp,ksplit", BASIS)
def test_basis(lib, kern, Kp, Dp, ksplit):
    _, planes, bk, _, _ = KERNELS[kern]
    rng = np.random.default_rng([Kp, Dp, ksplit, planes])
    rows = Kp
    pi = rng.permutation(Kp)
    assert (pi != np.arange(Kp)).any()
    unit = np.zeros((rows, Kp), operand_type(kern))
    unit[np.arange(rows), pi] = 1
    zero = np.zeros_like(unit)
    if kern == "f32":
        b_planes = [rng.uniform(-1, 1, (Kp, Dp)).astype(np.float32)]
    elif planes == 1:
        b_planes = [rng.uniform(-1, 1, (Kp, Dp)).astype(np.float16)]
    else:
        b_planes = list(T.split_f16(rng.uniform(-0.5, 0.5, (Kp, Dp)).astype(np.float32)))      # (hi + lo is a float32: tests/test_gemm_twin.py)
    owner = np.empty(Kp, np.int64)
    for z, (lo, hi) in enumerate(T.k_ranges(Kp, bk, ksplit)):
        owner[lo:hi] = z
    runs = [([unit], b_planes[0].astype(np.float64))] if planes == 1 else [
        ([unit, zero], b_planes[0].astype(np.float64) + b_planes[1].astype(np.float64)),      # 1 x Bhi + 1 x Blo (+ 0 x Bhi)
        ([zero, unit], b_planes[0].astype(np.float64))]                                       # Alo x Bhi alone: there is no Alo x Blo
    for a_planes, table in runs:
        C = launch(lib, kern, a_planes, b_planes, rows, rows, rows, 0, ksplit)
        got = written_rows(C, rows, rows, rows, 0)
        col = (0.0 + table[pi]).astype(np.float32)         # (the accumulators start at +0: a table entry of -0 leaves +0)
        assert np.array_equal(col.astype(np.float64), table[pi])
        want = np.zeros_like(got)
        want[owner[pi], np.arange(rows)] = col
        bad = bits(got) != bits(want)
        if bad.any():
            z, f, d = np.argwhere(bad)[0]
            pytest.fail("%d elements differ (unit in A plane %d), first at plane %d row %d column %d: got %r (0x%08x), want %r (0x%08x); k = %d of segment %d, table planes there %s"
                        % (bad.sum(), [float(a.sum()) for a in a_planes].index(float(rows)), z, f, d, got[z, f, d], bits(got)[z, f, d], want[z, f, d], bits(want)[z, f, d], pi[f],
                           owner[pi[f]], [float(b[pi[f], d]).hex() for b in b_planes]))


# ---- ints and gauss ------------------------------------------------------------------------------------------------------------------
def ONE(rows):
    return (rows, rows, rows + 5, 2)                  # one array of `rows` frames at frame 2 of rows + 5


THREE = (300, 100, 140, 32)                           # 3 arrays x 100 frames into 140 at 32: the 128-row tiles 0 and 1 straddle two arrays each
TWO = (320, 160, 224, 32)                             # 2 arrays x 160 frames into 224 at 32 (the 256-row tile 0 straddles them)
SHAPES = ([("f32",) + s for s in ((ONE(1), 3104, 192, 16), (ONE(128), 2080, 384, 14), (ONE(130), 2080, 576, 16), (THREE, 7200, 384, 8), (ONE(300), 3968, 192, 2),
                                   (ONE(130), 7200, 192, 1))] +
          [(k,) + s for k in ("f16_192", "f16x3_192") for s in ((ONE(1), 2592, 192, 10), (ONE(128), 7200, 384, 16), (ONE(130), 3968, 576, 2), (THREE, 7200, 384, 8),
                                                                 (ONE(300), 2592, 192, 10), (ONE(130), 7200, 192, 1))] +
          [(k,) + s for k in ("f16_64", "f16x3_64") for s in ((ONE(1), 2592, 64, 10), (ONE(130), 7200, 64, 16), (THREE, 3968, 64, 2), (ONE(300), 7200, 64, 1), (ONE(128), 2592, 64, 8))] +
          [(k,) + s for k in ("v3", "v2") for s in ((ONE(256), 7200, 384, 1), (ONE(300), 3968, 384, 2), (ONE(512), 7200, 384, 4), (TWO, 3968, 384, 4), (TWO, 7200, 384, 2),
                                                     (ONE(300), 7200, 384, 1))])
TIGHT_ROWS = 32          # rows the sequential float32 yardstick is run on


def make_operands(kern, family, rng, rows, Kp, Dp):
    """-> a_planes, b_planes (operand type), and for gauss on two planes the unsplit float32 pair (else None)"""
    _, planes, _, _, _ = KERNELS[kern]
    ot = operand_type(kern)
    if family == "ints":
        return [rng.integers(-3, 4, (rows, Kp)).astype(ot) for _ in range(planes)], [rng.integers(-3, 4, (Kp, Dp)).astype(ot) for _ in range(planes)], None
    a32, b32 = rng.standard_normal((rows, Kp)).astype(np.float32), rng.uniform(-1, 1, (Kp, Dp)).astype(np.float32)
    if planes == 2:
        return list(T.split_f16(a32)), list(T.split_f16(b32)), (a32, b32)
    return [a32.astype(ot)], [b32.astype(ot)], None


def check_values(kern, family, got, a_planes, b_planes, unsplit, ksplit, what):
    """got [ksplit][rows][Dp] against the twin: ints bit for bit, gauss to the derived bars and the normwise one"""
    _, planes, bk, _, _ = KERNELS[kern]
    ref, mag, n = T.ref_planes(a_planes, b_planes, bk, ksplit)
    for z in range(ksplit):
        if n[z] == 0:
            assert not bits(got[z]).any(), "the plane of the empty K segment %d is not exact zeros" % z
    if family == "ints":
        assert np.abs(ref).max() < 2 ** 24 and np.array_equal(got.astype(np.float64), ref), "not the integer product"
        return
    nprod = 3 if planes == 2 else 1
    bar = nprod * n[:, None, None] * U * mag
    err = np.abs(got - ref)
    live = bar > 0
    r_plane = float((err[live] / bar[live]).max()) if live.any() else 0.0
    assert (err[~live] == 0).all()
    tot, ref_t = got.astype(np.float64).sum(0), ref.sum(0)
    bar_t = bar.sum(0) + U * np.abs(ref_t)
    r_sum = float((np.abs(tot - ref_t) / bar_t).max())
    print("%s %s: largest error / bar %.4f per plane, %.4f summed (largest error %.3g of largest |C| %.3g)" % (kern, what, r_plane, r_sum, np.abs(tot - ref_t).max(), np.abs(ref_t).max()))
    assert r_plane <= 1.0 and r_sum <= 1.0
    if unsplit is not None:                          # "~fp32 accuracy": against the product of the unsplit float32 values
        a64, b64 = unsplit[0].astype(np.float64), unsplit[1].astype(np.float64)
        ref_u = a64 @ b64
        bar_u = bar_t + 2.0 ** -22 * (np.abs(a64) @ np.abs(b64))
        r_u = float((np.abs(tot - ref_u) / bar_u).max())
        print("%s %s: against the unsplit product %.4f of its bar" % (kern, what, r_u))
        assert r_u <= 1.0
    # normwise, on the first rows: the planes summed in float32, plane 0 first (as k_sum_planes and the scans do)
    t = min(TIGHT_ROWS, got.shape[1])
    acc = got[0, :t].copy()
    for z in range(1, ksplit):
        acc += got[z, :t]
    seq = T.seq_f32([a[:t] for a in a_planes], b_planes)
    nrm = np.linalg.norm(ref_t[:t])
    e_k, e_s = np.linalg.norm(acc - ref_t[:t]) / nrm, np.linalg.norm(seq - ref_t[:t]) / nrm
    print("%s %s: normwise error %.3g, sequential float32 %.3g, ratio %.3f" % (kern, what, e_k, e_s, e_k / e_s))
    assert e_k <= 2.0 * e_s


@pytest.mark.parametrize("family", ["ints", "gauss"])
@pytest.mark.parametrize("kern,rowmap,Kp,Dp,ksplit", SHAPES)
def test_values(lib, kern, rowmap, Kp, Dp, ksplit, family):
    rows, chunk, total, frame0 = rowmap
    rng = np.random.default_rng([rows, chunk, Kp, Dp, ksplit, int(family == "ints"), KERNELS[kern][1]])
    a_planes, b_planes, unsplit = make_operands(kern, family, rng, rows, Kp, Dp)
    C = launch(lib, kern, a_planes, b_planes, rows, chunk, total, frame0, ksplit)
    got = written_rows(C, rows, chunk, total, frame0)
    check_values(kern, family, got, a_planes, b_planes, unsplit, ksplit, "rows %d (%d per array) Kp %d Dp %d ksplit %d" % (rows, chunk, Kp, Dp, ksplit))


# ---- the scan partials of k_srp_gemm_f16_v3 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["ints", "gauss"])
@pytest.mark.parametrize("D", [361, 321, 383])
@pytest.mark.parametrize("ksplit", [1, 2])
def test_v3_scan_partials(lib, D, ksplit, family):
    rows, chunk, total, frame0 = TWO
    Kp, Dp, n_chunks, na = 3968, 384, 7, 2
    rng = np.random.default_rng([D, ksplit, int(family == "ints")])
    a_planes, b_planes, _ = make_operands("v3", family, rng, rows, Kp, Dp)
    part = np.full((ksplit, na, n_chunks, D), np.nan, np.float32)
    nv = np.full((na, n_chunks), -7, np.int32)
    w = T.scan_weights()
    C = launch(lib, "v3", a_planes, b_planes, rows, chunk, total, frame0, ksplit, (part, nv, D, n_chunks, w))
    got = written_rows(C, rows, chunk, total, frame0)
    check_values("v3", family, got, a_planes, b_planes, None, ksplit, "with partials, D %d ksplit %d" % (D, ksplit))
    # chunks 1..5 of both arrays are written (frames 32..191), for d < D; chunk 0, chunk 6 and nothing else
    c0, c1 = frame0 // 32, (frame0 + chunk) // 32
    assert np.isnan(part[:, :, :c0]).all() and np.isnan(part[:, :, c1:]).all()
    assert not np.isnan(part[:, :, c0:c1]).any()
    assert (nv[:, c0:c1] == 32).all() and (nv[:, :c0] == -7).all() and (nv[:, c1:] == -7).all()
    # every plane's partials (plane y at part_plane_stride = arrays x n_chunks x D) are the weighted sums of that plane's own map rows
    blocks = C.reshape(ksplit, na, total // 32, 32, Dp)[:, :, c0:c1, :, :D]
    b64 = blocks.astype(np.float64)
    ref_p = np.einsum("t,yactd->yacd", w.astype(np.float64), b64)
    bar_p = 32 * U * np.einsum("t,yactd->yacd", np.abs(w).astype(np.float64), np.abs(b64)) + U * np.abs(ref_p)
    ratio = float((np.abs(part[:, :, c0:c1] - ref_p) / np.maximum(bar_p, 1e-300)).max())
    print("scan partials D %d ksplit %d %s: largest error / bar %.4f" % (D, ksplit, family, ratio))
    assert ratio <= 1.0
    if family == "ints":                             # the map rows are integers: the epilogue's fma chains and lane sums, bit for bit
        for y in range(ksplit):
            for a in range(na):
                for c in range(c1 - c0):
                    assert same_bits(part[y, a, c0 + c], T.part_lane_order(blocks[y, a, c], w)), (y, a, c)


# ---- k_srp_gemm_repair -----------------------------------------------------------------------------------------------------------------
# (BN, Dp, pass_rows, listed units, list0, repair_ksplit, repair_items, segments expected): 33 units = 132 rows = 2 row tiles
REPAIR = [(192, 384, 160, 0, 5, 32, 0, None), (192, 384, 160, 1, 5, 32, 0, 32), (192, 384, 160, 33, 5, 32, 40, 8), (192, 384, 160, 33, 5, 32, 100, 16),
          (192, 384, 160, 33, 5, 32, 128, 32), (192, 384, 160, 50, 5, 32, 0, 32), (192, 192, 160, 33, 1, 16, 0, 16), (64, 64, 160, 33, 7, 32, 40, 16),
          (64, 64, 160, 50, 7, 16, 0, 16), (64, 64, 160, 0, 7, 32, 0, None)]


@pytest.mark.parametrize("BN,Dp,pass_rows,n_units,list0,ksplit,items,k_eff", REPAIR)
def test_repair_contraction(lib, consts, BN, Dp, pass_rows, n_units, list0, ksplit, items, k_eff):
    Kp, grid_x = 2080, 3
    rng = np.random.default_rng([BN, Dp, n_units, ksplit, items])
    kern = "f16x3_%d" % BN
    a_planes, b_planes, _ = make_operands(kern, "gauss", rng, pass_rows, Kp, Dp)
    A = np.ascontiguousarray(np.concatenate(a_planes, axis=1))
    B = np.ascontiguousarray(np.stack([b.T for b in b_planes]))
    Cx = np.full(ksplit * ((pass_rows + 127) // 128 * 128) * Dp, np.nan, np.float32)
    call(lib.gh_repair, BN, A.ctypes.data, B.ctypes.data, pass_rows, list0 + n_units, list0, Kp, Dp, ksplit, items, grid_x, Cx.ctypes.data)
    n_rows = min(pass_rows, n_units * consts["REPAIR_GROUP"])
    if n_rows == 0:
        assert np.isnan(Cx).all()
        return
    assert T.repair_ksplit_eff(ksplit, n_rows, Dp, items) == k_eff
    n_work = (n_rows + 127) // 128 * (Dp // BN) * k_eff
    assert n_work > 10 * grid_x or n_units == 1          # the grid walks its work items
    # the same rows through k_srp_gemm_f16<true, BN> with k_eff segments: same tile routine, same segments -> same bits
    ref = launch(lib, kern, [a[:n_rows] for a in a_planes], b_planes, n_rows, n_rows, n_rows, 0, k_eff)
    stride = T.repair_plane_stride(n_rows, Dp)
    want = np.full(Cx.shape, np.nan, np.float32)
    for z in range(k_eff):
        want[z * stride:z * stride + n_rows * Dp] = ref[z].ravel()
    assert np.array_equal(np.isnan(Cx), np.isnan(want)), "written outside [k_eff][repair_plane_stride] x n_rows, or not everywhere inside"
    ok = ~np.isnan(want)
    assert same_bits(Cx[ok], want[ok])


# ---- the in-order plane sums ---------------------------------------------------------------------------------------------------------
def spread(rng, shape):
    """values whose float32 sum depends on the order: magnitudes over 2^30, both signs"""
    return (rng.standard_normal(shape) * 2.0 ** rng.uniform(0, 30, shape)).astype(np.float32)


def sum_in_order(planes):
    acc = planes[0].copy()
    for p in planes[1:]:
        acc = acc + p                                # float32 + float32, rounded once
    return acc


@pytest.mark.parametrize("planes", [1, 2, 3, 4, 5, 8, 9, 16])
def test_sum_planes(lib, planes):
    rng = np.random.default_rng(planes)
    n4 = 300                                         # two workgroups, the second ragged
    stride = 4 * n4 + 8
    C = spread(rng, (planes - 1) * stride + 4 * n4)
    C0 = C.copy()
    views = [C0[p * stride:p * stride + 4 * n4] for p in range(planes)]
    assert planes < 3 or not same_bits(sum_in_order(views), sum_in_order(views[::-1])), "the order would not show"
    call(lib.gh_sum_planes, C.ctypes.data, n4, planes, stride)
    assert same_bits(C[:4 * n4], sum_in_order(views))
    assert same_bits(C[4 * n4:], C0[4 * n4:])        # the other planes and the gaps between them are read only


# (repair_ksplit, repair_items, Dp, units listed behind list0): 10 units fit pass_rows = 40
PATCH = [(1, 0, 384, 7), (2, 0, 384, 7), (3, 0, 384, 7), (4, 0, 384, 7), (5, 0, 384, 7), (8, 0, 384, 12), (9, 0, 64, 7), (16, 0, 192, 7), (32, 0, 384, 7), (32, 20, 384, 12)]


@pytest.mark.parametrize("ksplit,items,Dp,n_units", PATCH)
def test_repair_patch(lib, consts, ksplit, items, Dp, n_units):
    G, HF, HU = consts["REPAIR_GROUP"], consts["HIST_FRAMES"], consts["HIST_UNITS"]
    arrays, n_frames, c_planes, pass_rows, list0, grid_x = 2, 10, 3, 40, 2, 5
    gpa = (n_frames + G - 1) // G                    # the last unit of an array runs past n_frames: those frames are skipped
    assert gpa * G > n_frames
    hist_base = arrays * gpa
    need_len = hist_base + arrays * HU
    rng = np.random.default_rng([ksplit, items, Dp, n_units])
    # units of both arrays, their ragged last units and history units of both, in no order; two junk entries in front of list0
    order = [1, 2 * gpa - 1, hist_base, gpa, hist_base + 2 * HU - 1, gpa - 1, 0, hist_base + HU, gpa + 1, hist_base + 1, hist_base + HU - 1, hist_base + 2]
    assert len(set(order)) == len(order) and max(order) < need_len
    lst = np.array([0, 0] + order, np.int32)
    n_here = min(n_units, pass_rows // G)
    n_rows = n_here * G
    planes_x = T.repair_ksplit_eff(ksplit, n_rows, Dp, items)
    if items:
        assert planes_x < ksplit
    xstride = T.repair_plane_stride(n_rows, Dp)
    Cx = spread(rng, ksplit * ((pass_rows + 127) // 128 * 128) * Dp)
    c_stride = arrays * n_frames * Dp + 64
    C = spread(rng, (c_planes - 1) * c_stride + arrays * n_frames * Dp)
    hist = spread(rng, (arrays, HF, Dp))
    need = np.ones(need_len, np.int32)
    wantC, wantH, want_need = C.copy(), hist.copy(), need.copy()
    for g in range(n_here):
        e = int(lst[list0 + g])
        want_need[e] = 0
        for j in range(G):
            r = g * G + j
            row = sum_in_order([Cx[z * xstride + r * Dp:z * xstride + (r + 1) * Dp] for z in range(planes_x)])
            if e >= hist_base:
                a, f = divmod(e - hist_base, HU)
                wantH[a, f * G + j] = row
            else:
                a, u = divmod(e, gpa)
                f = u * G + j
                if f >= n_frames:
                    continue
                o = (a * n_frames + f) * Dp
                wantC[o:o + Dp] = row
                for pl in range(1, c_planes):
                    wantC[pl * c_stride + o:pl * c_stride + o + Dp] = 0.0
    call(lib.gh_repair_patch, Cx.ctypes.data, pass_rows, ksplit, items, lst.ctypes.data, len(lst), list0 + n_units, list0, gpa, need.ctypes.data, need_len, C.ctypes.data, c_planes,
         c_stride, arrays, n_frames, Dp, hist.ctypes.data, hist_base, grid_x)
    assert np.array_equal(need, want_need)
    assert same_bits(C, wantC)
    assert same_bits(hist, wantH)
