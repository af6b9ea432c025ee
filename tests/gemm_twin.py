"""The contraction kernels of csrc/kernels_gemm.hip restated in plain numpy, float64: what tests/test_gpu_gemm_kernels.py compares the
kernels with, pinned on its own by tests/test_gemm_twin.py.

  * the table layouts: [planes][Dp][Kp] (k contiguous, the 128-row fp16 kernels), its tiling by 32-deep K stages [planes][Kp / 32][Dp][32]
    (the 256 x 384 kernels) and [Kp][Dp] (the fp32 kernel);
  * the K-segment rule of every split-K kernel: nk = Kp / bk steps, per = ceil(nk / ksplit), segment z = steps [z per, min((z + 1) per, nk)),
    empty where z per >= nk;
  * the row map: row r of a launch is frame frame0 + r % chunk_frames of array r // chunk_frames in a map of total_frames frames per array;
  * repair_ksplit_eff / repair_plane_stride as the comments of mca_internal.h state them;
  * the reference products per K segment, their magnitudes (for the error bars) and a sequential float32 accumulation (the yardstick of
    the normwise bar)."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32


# ---- layouts -------------------------------------------------------------------------------------------------------------------------
def tile_bt(B):
    """[planes][Dp][Kp] -> [planes][Kp / 32][Dp][32]: a 32-deep K stage of all columns is contiguous."""
    P, Dp, Kp = B.shape
    assert Kp % 32 == 0
    return np.ascontiguousarray(B.reshape(P, Dp, Kp // 32, 32).transpose(0, 2, 1, 3))


def untile_bt(Bt):
    P, ns, Dp, w = Bt.shape
    assert w == 32
    return np.ascontiguousarray(Bt.transpose(0, 2, 1, 3).reshape(P, Dp, ns * 32))


def split_f16(x):
    """x (float32) -> hi = fp16(x), lo = fp16(x - hi): the operand planes of the three-product kernels."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


# ---- K segments ----------------------------------------------------------------------------------------------------------------------
def segments(nk, ksplit):
    """(first step, end step) of every segment z < ksplit; an empty segment has end <= first."""
    per = -(-nk // ksplit)
    return [(z * per, min((z + 1) * per, nk)) for z in range(ksplit)]


def k_ranges(Kp, bk, ksplit):
    """the segments as element ranges [lo, hi) of the K axis, hi == lo for an empty one"""
    assert Kp % bk == 0
    out = []
    for s0, s1 in segments(Kp // bk, ksplit):
        lo = min(s0, Kp // bk) * bk
        out.append((lo, max(s1 * bk, lo)))
    return out


# ---- rows ----------------------------------------------------------------------------------------------------------------------------
def row_map(rows, chunk_frames, total_frames, frame0):
    """row r -> (array, frame in the map, flat row arr * total_frames + frame)"""
    r = np.arange(rows)
    arr = r // chunk_frames
    frame = frame0 + r - arr * chunk_frames
    return arr, frame, arr * total_frames + frame


def n_arrays(rows, chunk_frames):
    return -(-rows // chunk_frames)


# ---- the repair pass -----------------------------------------------------------------------------------------------------------------
def repair_plane_stride(n_rows, Dp):
    """elements between the partial maps of the repair contraction: the rows rounded up to whole 128-row tiles"""
    return -(-n_rows // 128) * 128 * Dp


def repair_ksplit_eff(ksplit, n_rows, Dp, items_max):
    """K segments really used: halved while more than 4 and while (row tiles x column tiles x segments) exceeds items_max; 0: never"""
    if items_max <= 0:
        return ksplit
    tiles = -(-n_rows // 128) * (1 if Dp == 64 else Dp // 192)
    k = ksplit
    while k > 4 and tiles * k > items_max:
        k >>= 1
    return k


# ---- reference products --------------------------------------------------------------------------------------------------------------
def products(a_planes, b_planes):
    """The (A, B) pairs a kernel multiplies, float64, B as [Kp][D], in the order it accumulates them per K step:
    one plane: Ahi Bhi; two: Alo Bhi, Ahi Blo, Ahi Bhi (the small terms first; Alo Blo is dropped)."""
    a = [np.asarray(x, np.float64) for x in a_planes]
    b = [np.asarray(x, np.float64) for x in b_planes]
    if len(a) == 1:
        return [(a[0], b[0])]
    return [(a[1], b[0]), (a[0], b[1]), (a[0], b[0])]


def ref_planes(a_planes, b_planes, bk, ksplit):
    """-> ref [ksplit][rows][D] float64, mag [ksplit][rows][D] = sum over the products of sum_k |a| |b|, n [ksplit] = terms per product.
    a_planes: list of [rows][Kp]; b_planes: list of [Kp][D]."""
    prods = products(a_planes, b_planes)
    rows, Kp = prods[0][0].shape
    D = prods[0][1].shape[1]
    ref = np.zeros((ksplit, rows, D))
    mag = np.zeros((ksplit, rows, D))
    n = np.zeros(ksplit, np.int64)
    for z, (lo, hi) in enumerate(k_ranges(Kp, bk, ksplit)):
        n[z] = hi - lo
        for a, b in prods:
            ref[z] += a[:, lo:hi] @ b[lo:hi]
            mag[z] += np.abs(a[:, lo:hi]) @ np.abs(b[lo:hi])
    return ref, mag, n


def seq_f32(a_planes, b_planes):
    """One float32 accumulator per element, k ascending, the products of a K step in the kernel's order: acc = fl(acc + fl(a b))."""
    prods = [(a.astype(np.float32), b.astype(np.float32)) for a, b in products(a_planes, b_planes)]
    rows, Kp = prods[0][0].shape
    acc = np.zeros((rows, prods[0][1].shape[1]), np.float32)
    for k in range(Kp):
        for a, b in prods:
            acc += a[:, k, None] * b[None, k, :]
    return acc


def scan_weights():
    """the 32 weights of a scan chunk as api.hip builds them, float32: w[31] = 1 - 0.8f, w[t] = w[t + 1] * 0.8f"""
    w = np.empty(32, np.float32)
    w[31] = np.float32(1) - np.float32(0.8)
    for t in range(30, -1, -1):
        w[t] = w[t + 1] * np.float32(0.8)
    return w


def part_lane_order(block, w):
    """The chunk result of k_srp_gemm_f16_v3's epilogue, float32, in its order.  block: [32][D] float32 map rows of one chunk.
    Lane group g (of four) holds the rows 16 b + 4 g + r (b = 0, 1; r = 0..3) and runs one fma chain over them from zero, b outer;
    the groups are then added as (s0 + s1) + (s2 + s3).  The fused multiply-add is formed in extended precision (a product of two
    float32 is exact there) and rounded once."""
    ld = np.longdouble
    s = []
    for g in range(4):
        acc = np.zeros(block.shape[1], np.float32)
        for b in range(2):
            for r in range(4):
                t = 16 * b + 4 * g + r
                acc = (ld(w[t]) * block[t].astype(ld) + acc.astype(ld)).astype(np.float32)
        s.append(acc)
    return (s[0] + s[1]) + (s[2] + s[3])
