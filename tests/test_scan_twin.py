"""CPU pins of tests/scan_twin.py, the numpy twin tests/test_gpu_scan_kernels.py compares the scan / peak-pick / repair-plan kernels with:
its fused multiply-add against libm's fmaf, its peak pick against a plain float64 selectDOA, the soundness and the precision of its
sensitivity rule (with the four one-clause-short mutants shown unsound), the soundness of its candidate columns, and its repair plans
against their brute-force definition."""
import ctypes
import ctypes.util
from fractions import Fraction

import numpy as np
import pytest

import scan_twin as T

F = np.float32
TAU = F(2.0 ** -10)


# ---- arithmetic -------------------------------------------------------------------------------------------------------------------------
def test_fma32_is_fmaf():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(1)
    n = 100000
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(np.float32)
    b = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(np.float32)
    c = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(np.float32)
    # heavy cancellation: c = -RN(a b) (the residual of a product), and c one float32 spacing off it; and halfway cases: a b + c with c tiny
    k = n // 4
    c[:k] = -(a[:k] * b[:k])
    c[k:2 * k] = np.nextafter(-(a[k:2 * k] * b[k:2 * k]), F(0))
    c[2 * k:3 * k] = (a[2 * k:3 * k] * b[2 * k:3 * k]) * F(2.0 ** -24) * rng.choice([-1, 1], k).astype(np.float32)
    got = T.fma32(a, b, c)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.count_nonzero(got[:2 * k]) > k          # the residuals are there, not flushed


def test_exact_reciprocal_and_quotient():
    for P in (1, 3, 6, 28, 120, 1000):
        d = 30 * P
        r = T.exact_reciprocal(F(d))
        for nb in (np.nextafter(r, F(0)), np.nextafter(r, F(1))):
            assert abs(Fraction(float(r)) - Fraction(1, d)) <= abs(Fraction(float(nb)) - Fraction(1, d))
        # the three-instruction quotient is the correctly rounded one on energies in range
        rng = np.random.default_rng(P)
        E = (rng.uniform(-15 * P, 15 * P, 4000)).astype(np.float32)
        x = (E - F(-15.0) * F(P)).astype(np.float32)
        want = (x.astype(np.float64) / d).astype(np.float32)          # (RN of the RN-to-double quotient of 24-bit operands: no double rounding, 53 >= 2 * 24 + 2)
        assert np.array_equal(T.normalised_energy(E, P).view(np.uint32), want.view(np.uint32))


def test_recursion_pieces_agree():
    """the chunked scan (partial + carry) is the serial recursion whenever the composition is exact: mu = omu = 1 on integers"""
    rng = np.random.default_rng(2)
    C = rng.integers(-3, 4, (3, 70, 9)).astype(np.float32)
    voiced = (rng.random(70) < 0.6).astype(np.uint8)
    Cs = T.plane_sum(C)
    assert np.array_equal(Cs, C.sum(0))
    part, nv = T.chunk_scan(Cs, voiced, 1.0, 1.0)
    assert nv.sum() == voiced.sum()
    state = rng.integers(-5, 6, 9).astype(np.float32)
    for fused in (True, False):
        e_start, out = T.carry(part, nv, state, 1.0, fused)
        energy = T.run_chunks(Cs, voiced, e_start, 1.0, 1.0)
        want = state + np.cumsum(Cs * voiced[:, None], axis=0)
        assert np.array_equal(energy, want) and np.array_equal(out, want[-1])
    lb = T.lookback(part, state, 1.0, True)
    assert np.array_equal(lb[0], state) and np.array_equal(lb[2], state + part[0] + part[1])
    part6 = np.ones((6, 2), np.float32)
    lb = T.lookback(part6, np.full(2, 100.0, np.float32), 1.0, False)
    assert lb[4, 0] == 104.0 and lb[5, 0] == 4.0                      # the cut after four chunks drops the state and chunk 0


def test_plane_order_is_visible():
    """a + b = b + a exactly, so 'plane 1 before plane 0' cannot change a sum; any other reordering of three planes can"""
    C = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], np.float32)
    assert T.plane_sum(C)[0] == T.plane_sum(C, order=[1, 0, 2])[0]
    assert T.plane_sum(C)[0] != T.plane_sum(C, order=[1, 2, 0])[0]


# ---- the peak pick -----------------------------------------------------------------------------------------------------------------------
def test_pick_is_selectdoa():
    rng = np.random.default_rng(3)
    for D in range(3, 41):
        rows = [rng.uniform(0, 1, D), rng.uniform(-1, 1, D), rng.integers(0, 3, D) / 4.0, rng.integers(-1, 2, D) / 2.0, np.zeros(D), np.full(D, 0.5),
                np.arange(D) / 64.0, -np.arange(D) / 64.0]
        for En in rows:
            En = En.astype(np.float32)
            for S in range(1, 5):
                bins, vals = T.pick(En, S)
                wb, wv = T.select_doa_f64(En, S)
                assert list(bins) == wb and [float(v) for v in vals] == wv, (D, S, En)


# ---- rows and perturbations --------------------------------------------------------------------------------------------------------------
def families(rng, n, D):
    lat = np.array([0.4, 0.9, 1.5, 3.0]) * float(TAU)
    out = []
    for i in range(n):
        k = i % 6
        if k == 4:                                                  # exact multiples of tau: differences of exactly tau, where <= and < part
            En = 0.5 + float(TAU) * rng.integers(-3, 4, D)
        elif k == 5:
            En = float(TAU) * rng.integers(-2, 3, D)
        elif k == 0:
            En = rng.uniform(0, 1, D)
        elif k == 1:
            En = 0.5 + rng.choice(lat, D) * rng.choice([-1, 1], D)
        elif k == 2:
            En = rng.choice(lat, D) * rng.choice([-1, 1], D)
        else:
            En = 0.5 + 0.3 * np.sin(np.arange(D) * rng.uniform(0.2, 1.5) + rng.uniform(0, 6)) + rng.choice(lat, D) * rng.choice([-1, 1], D)
        out.append(En.astype(np.float32))
    return out


def perturbations(rng, D, n):
    h = float(TAU) / 2
    out = [np.full(D, h), np.full(D, -h)]
    for i in range(n):
        out.append(rng.uniform(-h, h, D) if i % 2 else rng.choice([-1.0, 0.0, 1.0], D) * 0.999 * h)
    return out


def single_element(D):
    h = 0.999 * float(TAU) / 2
    out = []
    for i in range(D):
        for s in (-h, h):
            d = np.zeros(D)
            d[i] = s
            out.append(d)
    return out


def perturbed(En, d):
    return (En.astype(np.float64) + d).astype(np.float32)


def tent(D, k, top, step):
    return (top - step * np.abs(np.arange(D) - k)).astype(np.float32)


def crafted_sensitive():
    """(row, S, perturbations) that only ONE clause catches"""
    t = float(TAU)
    rows = []
    # zero: no positive peak, the pick is the first zero entry; the only candidate is a peak of slightly negative energy, every first
    # difference far from zero
    rows.append((tent(12, 5, -0.3 * t, 3 * t), 1, single_element(12)))
    rows.append((tent(9, 6, -0.45 * t, 5 * t), 1, single_element(9)))
    # runner: two clean peaks 0.6 tau apart, one source
    En = np.concatenate([tent(9, 4, 0.5, 4 * t), tent(9, 4, 0.5 - 0.6 * t, 4 * t)]).astype(np.float32)
    rows.append((En, 1, single_element(18)))
    # order: the same two peaks, two sources (and a third far below)
    En = np.concatenate([tent(9, 4, 0.5, 4 * t), tent(9, 4, 0.5 - 0.6 * t, 4 * t), tent(9, 4, 0.3, 4 * t)]).astype(np.float32)
    rows.append((En, 2, single_element(27)))
    # uncertain: a flat top two wide
    En = tent(14, 6, 0.5, 4 * t)
    En[7] = En[6] - F(0.4 * t)
    rows.append((En, 1, single_element(14)))
    return rows


def test_sens_is_sound_and_every_clause_is_needed():
    rng = np.random.default_rng(4)
    cases = []
    for D in (5, 9, 16, 23):
        for En in families(rng, 120, D):
            cases.append((En, 1 + len(cases) % 4, perturbations(rng, D, 12)))
    cases += crafted_sensitive()
    clauses = ("order", "runner", "uncertain", "zero")
    escaped = dict.fromkeys(clauses, 0)
    changed = 0
    for En, S, deltas in cases:
        base = T.pick(En, S)
        moved = False
        for d in deltas:
            got = T.pick(perturbed(En, d), S)
            if not np.array_equal(got[0], base[0]):
                moved = True
                break
        if not moved:
            continue
        changed += 1
        assert T.sens(En, S, TAU), (En, S)
        for c in clauses:
            escaped[c] += not T.sens(En, S, TAU, drop=c)
    assert changed > 100
    assert all(escaped[c] > 0 for c in clauses), escaped           # each mutant lets a row through whose picks changed


def test_crafted_rows_reach_the_zero_clause():
    for En, S, deltas in crafted_sensitive()[:2]:
        assert T.sens(En, S, TAU) and not T.sens(En, S, TAU, drop="zero")
        base = T.pick(En, S)[0]
        assert any(not np.array_equal(T.pick(perturbed(En, d), S)[0], base) for d in deltas)


def test_sens_does_not_flag_clean_rows():
    t = float(TAU)
    clean = [(tent(20, 9, 0.5, 5 * t), 1), (tent(7, 1, 0.9, 9 * t), 1), (tent(40, 37, 0.7, 4.5 * t), 1),
             (np.concatenate([tent(11, 5, 0.6, 5 * t), tent(11, 5, 0.4, 5 * t)]), 2),
             (np.concatenate([tent(11, 5, 0.3, 5 * t), tent(11, 5, 0.8, 5 * t), tent(11, 5, 0.55, 5 * t)]), 3),
             (np.concatenate([tent(9, 4, 0.3, 6 * t), tent(9, 4, 0.4, 6 * t), tent(9, 4, 0.5, 6 * t), tent(9, 4, 0.6, 6 * t)]), 4)]
    for En, S in clean:
        En = En.astype(np.float32)
        assert np.abs(np.diff(En)).min() > 4 * t
        assert not T.sens(En, S, TAU), (En, S)


# ---- candidate columns -------------------------------------------------------------------------------------------------------------------
def test_candidates_are_sound():
    rng = np.random.default_rng(5)
    partial = 0
    for D in (6, 11, 24, 40):
        for En in families(rng, 90, D):
            mask, full = T.candidates(En, TAU)
            assert mask.all() or not full
            partial += not mask.all()
            for d in perturbations(rng, D, 10):
                exact = perturbed(En, d)
                hybrid = np.where(mask, exact, En)
                a, b = T.pick(hybrid, 1), T.pick(exact, 1)
                assert a[0][0] == b[0][0] and a[1][0] == b[1][0], (En, d)
    assert partial > 20


def test_candidates_crafted():
    t = float(TAU)
    mask, full = T.candidates(np.full(17, 0.5, np.float32), TAU)
    assert full and mask.all()
    # One sharp peak at column k: the only guaranteed window is (k - 1 rising, k falling), its bound En[k]; only position k - 1 (whose
    # second derivative is weighted with En[k]) reaches En[k] - tau, and a position reads En[dd - 1 .. dd + 3]: columns k - 2 .. k + 2
    for D, k in ((30, 12), (30, 2), (30, 27), (9, 1)):
        mask, full = T.candidates(tent(D, k, 0.5, 6 * t), TAU)
        want = np.zeros(D, bool)
        want[max(k - 2, 0):min(k + 2, D - 1) + 1] = True
        assert not full and np.array_equal(mask, want), (D, k)
    # forced / unsure frames take every column
    mask, full = T.candidates(tent(30, 12, 0.5, 6 * t), TAU, full=True)
    assert full and mask.all()


# ---- the repair plan ---------------------------------------------------------------------------------------------------------------------
def brute_rows(t, voiced, history):
    """{t} and the REPAIR_WARM advancing rows before it; history rows -HIST_FRAMES .. -1 all advance"""
    before = [u for u in range(-T.HIST_FRAMES if history else 0, t) if u < 0 or voiced is None or voiced[u]]
    return [t] + before[-T.REPAIR_WARM:]


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("hist_valid", [False, True])
def test_plan_rows_is_the_definition(gated, hist_valid):
    rng = np.random.default_rng(6 + gated + 2 * hist_valid)
    for n in (1, 17, 33, 70, 161):
        for density in (0.05, 0.5, 1.0):
            voiced = (rng.random(n) < density).astype(np.uint8) if gated else None
            flags = ((rng.random(n) < 0.08) & (voiced != 0 if gated else True)).astype(np.uint8)
            gpa, a = (n + 3) // 4, 1
            hb = 3 * gpa
            units, cfrom = T.plan_rows(flags, voiced, a, gpa, hb, hist_valid)
            history = hist_valid and not gated
            want_units, want_from = set(), {}
            for t in np.flatnonzero(flags):
                rows = brute_rows(int(t), voiced, history)
                for r in rows:
                    want_units.add(a * gpa + r // 4 if r >= 0 else hb + a * T.HIST_UNITS + (r + T.HIST_FRAMES) // 4)
                first = min(rows)
                want_from[t // 32] = min(want_from.get(t // 32, T.NO_FLAG), -1 if first < 0 else first // 32)
            assert units == want_units and cfrom == want_from


def test_plan_cand_is_the_definition():
    rng = np.random.default_rng(9)
    D = 12
    for hist_valid in (False, True):
        for n in (20, 70):
            flags = (rng.random(n) < 0.1).astype(np.uint8)
            dead = (rng.random(n) < 0.7).astype(np.uint8)
            masks = {int(t): rng.random(D) < 0.3 for t in np.flatnonzero(flags)}
            gpa, a = (n + 3) // 4, 0
            hb = 2 * gpa
            got, cfrom = T.plan_cand(flags, masks, dead, a, gpa, hb, hist_valid)
            want, want_from = set(), {}
            for t in np.flatnonzero(flags):
                rows = brute_rows(int(t), None, hist_valid)
                for r in rows:
                    if r < 0 or not dead[r]:
                        want.add(T.unit_of(r, a, gpa, hb))
                first = min(rows)
                want_from[t // 32] = min(want_from.get(t // 32, T.NO_FLAG), -1 if first < 0 else first // 32)
            assert set(got) == want and cfrom == want_from
            for e, m in got.items():                  # a unit's columns: at least those of every flagged frame with a live row in it
                for t in np.flatnonzero(flags):
                    if any((r < 0 or not dead[r]) and T.unit_of(r, a, gpa, hb) == e for r in brute_rows(int(t), None, hist_valid)):
                        assert (m | ~masks[int(t)]).all()
