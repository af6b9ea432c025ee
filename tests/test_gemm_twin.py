"""CPU: tests/gemm_twin.py on its own -- the rules tests/test_gpu_gemm_kernels.py holds the contraction kernels to are checked here
against brute-force restatements, so that a wrong twin cannot pass a wrong kernel."""
import numpy as np
import pytest

import gemm_twin as T

# every (Kp, K step, ksplit) the GPU module sends: fp32 steps of 16, fp16 steps of 32 (the 256 x 384 kernels: stages of 32)
KP_F32 = (2080, 3104, 3968, 7200)
KP_F16 = (32, 64, 96, 128, 160, 2080, 2592, 3968, 7200)
KSPLITS = (1, 2, 4, 8, 10, 14, 16, 32)
SEG_CASES = [(kp, 16, ks) for kp in KP_F32 for ks in KSPLITS] + [(kp, 32, ks) for kp in KP_F16 for ks in KSPLITS]


@pytest.mark.parametrize("Kp,bk,ksplit", SEG_CASES)
def test_segments_partition_the_k_range(Kp, bk, ksplit):
    nk = Kp // bk
    owner = np.full(nk, -1)
    for z, (s0, s1) in enumerate(T.segments(nk, ksplit)):
        for s in range(s0, s1):              # (an empty range where s1 <= s0)
            assert 0 <= s < nk and owner[s] == -1
            owner[s] = z
    assert (owner >= 0).all() and (np.diff(owner) >= 0).all()
    # the same rule on the element axis: contiguous, in order, [0, Kp) covered once, every range inside it
    edge = 0
    for lo, hi in T.k_ranges(Kp, bk, ksplit):
        assert 0 <= lo <= hi <= Kp
        if hi > lo:
            assert lo == edge
            edge = hi
    assert edge == Kp


def test_the_empty_segments_the_gpu_module_relies_on():
    # fp32 (steps of 16): 3 104 / 16 = 194 steps in 16 segments of 13: segment 15 starts at step 195; 2 080 / 16 = 130 steps in 14 segments
    # of 10 and in 16 of 9; fp16 (steps of 32): 2 592 / 32 = 81 steps in 10 segments of 9: segment 9 starts exactly at step 81
    assert T.segments(194, 16)[15] == (195, 194)
    assert T.segments(130, 14)[13] == (130, 130)
    assert T.segments(130, 16)[15] == (135, 130) and T.segments(130, 16)[14] == (126, 130)
    assert T.segments(81, 10)[9] == (81, 81) and T.segments(81, 10)[8] == (72, 81)
    assert T.k_ranges(3104, 16, 16)[15] == (3104, 3104)
    # more segments than steps (the 256 x 384 kernels at one stage)
    assert T.segments(1, 4) == [(0, 1), (1, 1), (2, 1), (3, 1)]


def test_tiling_round_trip():
    rng = np.random.default_rng(1)
    B = rng.integers(0, 1 << 16, (2, 384, 160)).astype(np.uint16)
    Bt = T.tile_bt(B)
    assert Bt.shape == (2, 5, 384, 32)
    for p, s, d, j in ((0, 0, 0, 0), (1, 4, 383, 31), (1, 2, 17, 5), (0, 3, 200, 30)):
        assert Bt[p, s, d, j] == B[p, d, 32 * s + j]
    # element by element on a small one
    b = rng.integers(0, 1 << 16, (1, 3, 64)).astype(np.uint16)
    bt = T.tile_bt(b)
    for d in range(3):
        for k in range(64):
            assert bt[0, k // 32, d, k % 32] == b[0, d, k]
    assert np.array_equal(T.untile_bt(Bt), B)


@pytest.mark.parametrize("rows,chunk,total,frame0", [(1, 1, 1, 0), (130, 130, 140, 3), (300, 100, 140, 32), (250, 100, 140, 32), (320, 160, 224, 32), (512, 512, 512, 0)])
def test_row_map_against_a_loop(rows, chunk, total, frame0):
    arr, frame, flat = T.row_map(rows, chunk, total, frame0)
    r = 0
    for a in range(T.n_arrays(rows, chunk)):
        for f in range(chunk):
            if r == rows:
                break
            assert (arr[r], frame[r], flat[r]) == (a, frame0 + f, a * total + frame0 + f)
            r += 1
    assert r == rows
    assert len(set(flat.tolist())) == rows and flat.max() < T.n_arrays(rows, chunk) * total


def test_repair_rules():
    assert T.repair_plane_stride(1, 384) == 128 * 384 and T.repair_plane_stride(128, 64) == 128 * 64 and T.repair_plane_stride(129, 192) == 256 * 192
    # 132 rows x 384 columns = 2 x 2 tiles: 32 segments are 128 items, 16 are 64, 8 are 32
    assert T.repair_ksplit_eff(32, 132, 384, 0) == 32
    assert T.repair_ksplit_eff(32, 132, 384, 128) == 32
    assert T.repair_ksplit_eff(32, 132, 384, 100) == 16
    assert T.repair_ksplit_eff(32, 132, 384, 40) == 8
    assert T.repair_ksplit_eff(32, 132, 384, 1) == 4          # never below 4
    assert T.repair_ksplit_eff(2, 132, 384, 1) == 2
    assert T.repair_ksplit_eff(32, 132, 64, 40) == 16         # 64 columns: one column tile


def test_reference_products_on_a_case_done_by_hand():
    a = np.array([[1.0, 2.0] + [0.0] * 62])
    b = np.zeros((64, 1))
    b[0, 0], b[1, 0], b[40, 0] = 3.0, -5.0, 7.0
    a[0, 40] = 2.0
    ref, mag, n = T.ref_planes([a], [b], 32, 2)
    assert ref[:, 0, 0].tolist() == [-7.0, 14.0] and mag[:, 0, 0].tolist() == [13.0, 14.0] and n.tolist() == [32, 32]
    # two planes: Ahi Bhi + Alo Bhi + Ahi Blo, the lo x lo term dropped
    ref2, mag2, _ = T.ref_planes([a, 0.5 * a], [b, 0.25 * b], 32, 1)
    assert ref2[0, 0, 0] == 7.0 * (1 + 0.5 + 0.25) and mag2[0, 0, 0] == 27.0 * 1.75
    assert np.array_equal(T.seq_f32([a], [b]), np.array([[7.0]], np.float32))


def test_split_planes_and_lane_order():
    x = np.random.default_rng(2).uniform(-0.5, 0.5, 4096).astype(np.float32)
    hi, lo = T.split_f16(x)
    s = hi.astype(np.float64) + lo.astype(np.float64)
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)          # hi + lo is a float32 (what the basis cases rely on)
    assert np.abs(s - x).max() <= 2.0 ** -23
    # the epilogue's order against exact rational arithmetic on small integers
    from fractions import Fraction
    w = T.scan_weights()
    blk = np.random.default_rng(3).integers(-50000, 50000, (32, 2)).astype(np.float32)
    got = T.part_lane_order(blk, w)

    def rnd(q):                      # a Fraction to the nearest float32, ties to even: exact via float64 only when q is one; so round by hand
        f = np.float32(float(q))
        cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        return min(cands, key=lambda c: (abs(Fraction(float(c)) - q), int(np.float32(c).view(np.uint32)) & 1))
    for d in range(2):
        s = []
        for g in range(4):
            acc = Fraction(0)
            for b in range(2):
                for r in range(4):
                    t = 16 * b + 4 * g + r
                    acc = Fraction(float(rnd(Fraction(float(w[t])) * Fraction(float(blk[t, d])) + acc)))
            s.append(np.float32(float(acc)))
        assert got[d] == (s[0] + s[1]) + (s[2] + s[3])
