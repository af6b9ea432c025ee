"""GPU, kernel level: the kernels of csrc/kernels_stream.hip that turn the correlation map into DOA bins -- k_scan_partial, k_scan_carry,
k_scan_pick<PL, MODE>, k_scan_repick<PL, false>, k_gate, k_doa_fill, k_hist_list, k_hist_settle -- one kernel per call through the
test-only launchers of tests/cxx/scan_harness.hip, against the numpy twin tests/scan_twin.py (pinned by tests/test_scan_twin.py).
Everything here is deterministic float32 or integer logic: the comparisons are bit for bit, not tolerances (k_gate's log10f excepted:
its frames are kept 1e-3 dB from the floor).

Every buffer a kernel may not touch carries NaN or a sentinel integer -- the pad columns D .. Dp - 1 of the map included -- and is checked.
Every call checks the hipError_t the harness returns; after the first non-zero one every later test of the module skips (nothing more
goes to a GPU that has just reported a fault).

Not covered: k_scan_repick<PL, true> (tests/test_gpu_steer_tail.py has its transform-and-patch half) and the bits of the device log10f."""
import ctypes
import os

import numpy as np
import pytest

import scan_twin as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FAULT = {"err": None}
CONTRACTION = "fused"                                   # the reading of g * E + b the carry and the look-back compile to
P, I, FL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
F = np.float32
TAU = F(2.0 ** -10)
NO_FLAG = 0x7F7F7F7F
MU_REAL, OMU_REAL = F(0.8), F(1) - F(0.8)


class Dims(ctypes.Structure):
    _fields_ = [(k, I) for k in ("arrays", "n_frames", "D", "Dp", "S", "P", "c_planes", "chunk")] + [("mu", FL), ("omu", FL), ("inv_norm", FL)]


class Pick(ctypes.Structure):
    _fields_ = [("PL", I), ("mode", I), ("lookback", I), ("C", P), ("voiced", P), ("part", P), ("part_planes", I), ("state_in", P), ("e_start", P), ("state_out", P),
                ("grid", P), ("doa_bin", P), ("doa_rad", P), ("prob", P), ("energy", P), ("tau", FL), ("flags", P), ("gpa", I), ("need", P), ("list", P), ("list_len", I),
                ("n_list", P), ("chunk_from", P), ("clist", P), ("clist_len", I), ("n_clist", P), ("last_vchunk", P), ("stats", P), ("dead", P), ("unsure", P),
                ("lazy", I), ("hist_valid", I), ("hist_base", I), ("hist_C_out", P), ("e_hist_out", P), ("umask", P), ("umask_words", I), ("n_miss", P), ("pred", P)]


class Repick(ctypes.Structure):
    _fields_ = [("PL", I), ("grid_x", I), ("C", P), ("voiced", P), ("e_start", P), ("flags", P), ("clist", P), ("clist_len", I), ("n_clist", P), ("chunk_from", P),
                ("last_vchunk", P), ("n_list", P), ("state_out", P), ("grid", P), ("doa_bin", P), ("doa_rad", P), ("prob", P), ("energy", P), ("hist_C_in", P),
                ("e_hist_in", P)]


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "tests", "cxx", "libscan_harness.so")
    if not os.path.exists(path):
        pytest.fail("%s is missing: build() makes it (tests/cxx/gemm_harness.mk)" % path)
    h = ctypes.CDLL(path)
    D = ctypes.c_double
    for name, args in (("sh_partial", [P] * 5), ("sh_carry", [P, I, P, I] + [P] * 7), ("sh_pick", [P, P]), ("sh_repick", [P, P]),
                       ("sh_gate", [P, I, I, I, I, FL, D, P, P, P, P]), ("sh_doa_fill", [P, I, I, I] + [P] * 6), ("sh_hist_list", [P, P, I, P, I]),
                       ("sh_hist_settle", [P, P, P, P, I, I, I, FL, FL]), ("sh_product_pl", [I])):
        getattr(h, name).restype = I
        getattr(h, name).argtypes = args
    h.sh_constants.restype = None
    h.sh_constants.argtypes = [P]
    out = np.zeros(8, np.int32)
    h.sh_constants(out.ctypes.data)
    assert list(out) == [T.SCAN_CHUNK, 32, T.REPAIR_WARM, T.REPAIR_GROUP, T.HIST_FRAMES, T.HIST_UNITS, 20, 4]      # the twin's constants are the product's
    return h


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _FAULT["err"]:
        pytest.skip("an earlier call failed (%s): nothing more goes to this GPU" % _FAULT["err"])


def call(fn, *args):
    err = fn(*args)
    if err:
        _FAULT["err"] = "hipError_t %d" % err
    assert err == 0


def ptr(x):
    return None if x is None else x.ctypes.data


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_bits(got, want):
    return np.array_equal(bits(got), bits(want))


def dp_of(D):
    """the product's padded map width (api.hip: 64 for the small fp16 grids, else a multiple of 192), restated"""
    return 64 if D <= 64 else (D + 191) // 192 * 192


class Sh:
    def __init__(self, arrays, n, D, S=1, P=1, planes=1, mu=MU_REAL, omu=OMU_REAL):
        self.arrays, self.n, self.D, self.S, self.P, self.planes, self.mu, self.omu = arrays, n, D, S, P, planes, F(mu), F(omu)
        self.Dp, self.nc, self.gpa = dp_of(D), (n + 31) // 32, (n + 3) // 4

    def dims(self):
        return Dims(self.arrays, self.n, self.D, self.Dp, self.S, self.P, self.planes, 32, float(self.mu), float(self.omu), float(T.exact_reciprocal(F(30.0) * F(self.P))))

    def pad(self, vals):
        """[planes][arrays][n][D] -> the map with NaN in the pad columns"""
        C = np.full((self.planes, self.arrays, self.n, self.Dp), np.nan, np.float32)
        C[..., :self.D] = vals
        return C

    def grid(self):
        return (np.arange(self.D, dtype=np.float32) * F(0.01) - F(1.5)).astype(np.float32)


class R:
    pass


def run_partial(lib, sh, C, voiced):
    part = np.full((sh.arrays, sh.nc, sh.D), np.nan, np.float32)
    nv = np.full((sh.arrays, sh.nc), -77, np.int32)
    d = sh.dims()
    call(lib.sh_partial, ctypes.addressof(d), ptr(C), ptr(voiced), ptr(part), ptr(nv))
    return part, nv


def run_carry(lib, sh, mode, part, nv, state_in):
    r = R()
    planes = part.shape[0] if part.ndim == 4 else 1
    r.e_start = np.full((sh.arrays, sh.nc, sh.D), np.nan, np.float32)
    r.state_out = np.full((sh.arrays, sh.D), np.nan, np.float32)
    r.n_list, r.n_clist, r.last_vchunk = np.array([5], np.int32), np.array([7, 0], np.int32), np.full(sh.arrays, -9, np.int32)
    d = sh.dims()
    m1 = mode == 1
    call(lib.sh_carry, ctypes.addressof(d), mode, ptr(part), planes, ptr(nv), ptr(state_in), ptr(r.e_start), ptr(r.state_out), ptr(r.n_list) if m1 else None,
         ptr(r.n_clist) if m1 else None, ptr(r.last_vchunk) if m1 else None)
    return r


def run_pick(lib, sh, C, PL=None, mode=0, lookback=0, voiced=None, part=None, state_in=None, e_start=None, tau=TAU, unsure=None, dead=None, lazy=0, hist_valid=0,
             cand=False, need=None, last_vchunk=None, pred=None, energy=True):
    r = R()
    rows = sh.arrays * sh.n
    r.PL = PL or lib.sh_product_pl(sh.D)
    r.grid = sh.grid()
    r.e_start = np.full((sh.arrays, sh.nc, sh.D), np.nan, np.float32) if lookback else np.ascontiguousarray(e_start, np.float32).copy()
    r.state_out = np.full((sh.arrays, sh.D), np.nan, np.float32)
    r.doa_bin = np.full((sh.arrays, sh.n, sh.S), -99, np.int32)
    r.doa_rad = np.full((sh.arrays, sh.n, sh.S), np.nan, np.float32)
    r.prob = np.full((sh.arrays, sh.n, sh.S), np.nan, np.float32)
    r.energy = np.full((sh.arrays, sh.n, sh.D), np.nan, np.float32) if energy else None
    q = Pick()
    q.PL, q.mode, q.lookback = r.PL, mode, lookback
    q.C, q.voiced, q.part, q.state_in = ptr(C), ptr(voiced), ptr(part), ptr(state_in)
    q.part_planes = 0 if part is None else (part.shape[0] if part.ndim == 4 else 1)
    q.e_start, q.state_out, q.grid, q.doa_bin, q.doa_rad, q.prob, q.energy = ptr(r.e_start), ptr(r.state_out), ptr(r.grid), ptr(r.doa_bin), ptr(r.doa_rad), ptr(r.prob), ptr(r.energy)
    keep = [C, voiced, part, state_in, unsure, dead, pred]
    if mode == 1:
        r.list_len = sh.arrays * sh.gpa + sh.arrays * T.HIST_UNITS
        r.hist_base = sh.arrays * sh.gpa
        r.flags = np.full((sh.arrays, sh.n), 7, np.uint8)
        r.need = np.zeros(r.list_len, np.int32) if need is None else need.astype(np.int32).copy()
        r.list = np.full(r.list_len, -5, np.int32)
        r.n_list = np.zeros(1, np.int32)
        r.chunk_from = np.full((sh.arrays, sh.nc), NO_FLAG, np.int32)
        r.clist = np.full(sh.arrays * sh.nc, -5, np.int32)
        r.n_clist = np.zeros(2, np.int32)
        r.last_vchunk = np.full(sh.arrays, -9, np.int32) if lookback else np.asarray(last_vchunk, np.int32).copy()
        r.stats = np.zeros(4, np.uint64)
        r.hist_C_out = np.full((sh.arrays, T.HIST_FRAMES, sh.Dp), np.nan, np.float32) if lazy else None
        r.e_hist_out = np.full((sh.arrays, sh.D), np.nan, np.float32) if lazy else None
        r.umask = np.zeros((r.list_len, sh.Dp // 32), np.uint32) if cand else None
        r.n_miss = np.zeros(1 + rows, np.int32) if pred is not None else None
        if r.n_miss is not None:
            r.n_miss[1:] = -5
        q.tau, q.flags, q.gpa, q.need, q.list, q.list_len, q.n_list = float(tau), ptr(r.flags), sh.gpa, ptr(r.need), ptr(r.list), r.list_len, ptr(r.n_list)
        q.chunk_from, q.clist, q.clist_len, q.n_clist, q.last_vchunk, q.stats = ptr(r.chunk_from), ptr(r.clist), r.clist.size, ptr(r.n_clist), ptr(r.last_vchunk), ptr(r.stats)
        q.dead, q.unsure, q.lazy, q.hist_valid, q.hist_base = ptr(dead), ptr(unsure), lazy, hist_valid, r.hist_base
        q.hist_C_out, q.e_hist_out, q.umask, q.umask_words, q.n_miss, q.pred = ptr(r.hist_C_out), ptr(r.e_hist_out), ptr(r.umask), sh.Dp // 32 if cand else 0, ptr(r.n_miss), ptr(pred)
    d = sh.dims()
    call(lib.sh_pick, ctypes.addressof(d), ctypes.addressof(q))
    del keep
    if not lookback:
        assert np.isnan(r.state_out).all() and same_bits(r.e_start, e_start)          # the serial-carry form leaves both alone
    return r


def sums(sh, C):
    return [T.plane_sum(C[:, a, :, :sh.D]) for a in range(sh.arrays)]


def expected(sh, Cs, voiced, e_start):
    """the twin's energies, normalised energies, bins (-1: gated out) and values from the given start values"""
    x = R()
    x.energy = np.stack([T.run_chunks(Cs[a], None if voiced is None else voiced[a], e_start[a], sh.mu, sh.omu) for a in range(sh.arrays)])
    x.En = T.normalised_energy(x.energy, sh.P)
    x.bins = np.full((sh.arrays, sh.n, sh.S), -1, np.int32)
    x.prob = np.full((sh.arrays, sh.n, sh.S), np.nan, np.float32)
    for a in range(sh.arrays):
        for t in range(sh.n):
            if voiced is None or voiced[a, t]:
                x.bins[a, t], x.prob[a, t] = T.pick(x.En[a, t], sh.S)
    return x


def check_outputs(sh, r, x):
    assert np.array_equal(r.doa_bin, x.bins)
    assert r.doa_bin.max() <= sh.D - 2
    on = x.bins >= 0
    assert same_bits(r.prob[on], x.prob[on]) and np.isnan(r.prob[~on]).all()            # gated-out frames: prob / doa_rad untouched
    assert same_bits(r.doa_rad[on], r.grid[x.bins[on]]) and np.isnan(r.doa_rad[~on]).all()
    if r.energy is not None:
        assert same_bits(r.energy, x.energy)


# ---- the recursion ---------------------------------------------------------------------------------------------------------------------
# (D, frames, arrays, planes, S): both edges of every pick width (512: the widest grid a context accepts; 514: the widest the pick covers, nine
# waves and a ninth slice of the carry with two live lanes), one to six chunks, the LDS opt-in (Dp = 576)
SHAPES = [(3, 1, 1, 1, 1), (4, 31, 3, 2, 2), (37, 32, 1, 3, 3), (61, 33, 3, 1, 4), (130, 70, 1, 5, 2), (131, 161, 1, 2, 1), (361, 70, 3, 1, 2), (386, 33, 1, 2, 4),
          (387, 161, 1, 1, 3), (512, 70, 1, 3, 1), (514, 161, 3, 2, 2)]


def operands(family, sh, rng):
    n, D = sh.n, sh.D
    if family == "ints":
        vals = rng.integers(-3, 4, (sh.planes, sh.arrays, n, D)).astype(np.float32)
        state = rng.integers(-9, 10, (sh.arrays, D)).astype(np.float32)
    elif family == "impulses":
        # one power of two per (array, column), anywhere in the call: its exponent at a later frame counts the advancing frames exactly
        vals = np.zeros((sh.planes, sh.arrays, n, D), np.float32)
        for a in range(sh.arrays):
            t = rng.integers(0, n, D)
            vals[rng.integers(0, sh.planes, D), a, t, np.arange(D)] = np.exp2(rng.integers(70, 91, D)).astype(np.float32)
        state = np.exp2(rng.integers(70, 91, (sh.arrays, D))).astype(np.float32)
    else:
        vals = rng.standard_normal((sh.planes, sh.arrays, n, D)).astype(np.float32)
        state = rng.standard_normal((sh.arrays, D)).astype(np.float32)
    return sh.pad(vals), state


def gate_mask(sh, rng):
    v = (rng.random((sh.arrays, sh.n)) < 0.5).astype(np.uint8)
    v[:, :32] = 1                                                         # chunks of 32, 0 and 1 advancing frames
    v[:, 32:64] = 0
    if sh.n > 64:
        v[:, 64:96] = 0
        v[:, min(70, sh.n - 1)] = 1
    return np.ascontiguousarray(v[:, :sh.n])


def match_variant(got, fused, unfused, exact):
    """the kernel's composition is the CONTRACTION reading; on exact operands the two readings agree"""
    assert same_bits(got, fused if CONTRACTION == "fused" else unfused)
    if exact:
        assert same_bits(fused, unfused)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%d_f%d_a%d_p%d_S%d" % s)
@pytest.mark.parametrize("family", ["ints", "impulses", "real"])
def test_recursion(lib, family, shape):
    D, n, arrays, planes, S = shape
    mu, omu = {"ints": (1.0, 1.0), "impulses": (0.5, 0.5), "real": (MU_REAL, OMU_REAL)}[family]
    sh = Sh(arrays, n, D, S=S, P=6 if family == "real" else 1, planes=planes, mu=mu, omu=omu)
    rng = np.random.default_rng(D * 1000 + n)
    C, state = operands(family, sh, rng)
    Cs = sums(sh, C)
    exact = family != "real"
    for voiced in (None, gate_mask(sh, rng)):
        va = (lambda a: None) if voiced is None else (lambda a: voiced[a])
        part, nv = run_partial(lib, sh, C, voiced)
        tw = [T.chunk_scan(Cs[a], va(a), sh.mu, sh.omu) for a in range(arrays)]
        assert same_bits(part, np.stack([p for p, _ in tw])) and np.array_equal(nv, np.stack([c for _, c in tw]))
        # the serial carry, then the pick from the kernel's own start values
        cr = run_carry(lib, sh, 1 if voiced is not None else 0, part, nv, state)
        both = [[T.carry(part[a], nv[a], state[a], sh.mu, fused) for a in range(arrays)] for fused in (True, False)]
        match_variant(np.concatenate([cr.e_start.reshape(arrays, -1), cr.state_out], axis=1),
                      *[np.concatenate([np.stack([e for e, _ in b]).reshape(arrays, -1), np.stack([s for _, s in b])], axis=1) for b in both], exact)
        if voiced is not None:
            lv = [max([c for c in range(sh.nc) if nv[a, c] > 0], default=-1) for a in range(arrays)]
            assert list(cr.last_vchunk) == lv and cr.n_list[0] == 0 and list(cr.n_clist) == [0, 0]
        else:
            assert cr.n_list[0] == 5 and cr.last_vchunk[0] == -9            # mode 0 resets nothing
        r = run_pick(lib, sh, C, voiced=voiced, e_start=cr.e_start)
        check_outputs(sh, r, expected(sh, Cs, voiced, cr.e_start))
        if voiced is None:
            # the four-chunk look-back inside the pick
            r = run_pick(lib, sh, C, lookback=4, part=part, state_in=state)
            lb = [np.stack([T.lookback(part[a], state[a], sh.mu, fused) for a in range(arrays)]) for fused in (True, False)]
            if exact and sh.nc <= 5:
                assert same_bits(lb[0], cr.e_start)                         # nothing cut yet: the carry's values
            if family == "ints" and sh.nc > 5:
                assert not np.array_equal(lb[0][:, 5], cr.e_start[:, 5])    # the cut after four chunks is visible
            match_variant(r.e_start, lb[0], lb[1], exact)
            x = expected(sh, Cs, None, r.e_start)
            check_outputs(sh, r, x)
            assert same_bits(r.state_out, x.energy[:, -1])


# ---- the pick on crafted rows ----------------------------------------------------------------------------------------------------------
def tent(D, k, top, step):
    return top - step * np.abs(np.arange(D) - k)


def crafted_rows(D, rng):
    """energies E (the map rows themselves: mu = 0, omu = 1, P = 1; En = (E + 15) / 30)"""
    rows = [np.zeros(D), np.arange(D) * 0.01, -np.arange(D) * 0.01, tent(D, 1, 5.0, 0.01), tent(D, D - 2, 5.0, 0.01), tent(D, D // 2, 5.0, 0.01),
            -20.0 - tent(D, D // 2, 5.0, 0.01), rng.uniform(-14, 14, D), rng.uniform(-40, -16, D), rng.integers(-2, 3, D).astype(float),
            rng.integers(0, 2, D).astype(float), -20.0 + rng.integers(-1, 2, D).astype(float)]
    for k in (1, 2):                                                        # a larger value behind the last position: never picked
        e = tent(D, max(D // 3, 1), 2.0, 0.01)
        e[D - k:] = 9.0 + np.arange(k)
        rows.append(e)
        e = rng.uniform(0, 1, D)
        e[D - k:] = 9.0
        rows.append(e)
    for q in (2, 3, 4, 5, 7):                                               # combs: equal peaks (first index wins), rising and falling ones, on every
        for off in range(q):                                                # residue, so on both sides of every lane boundary of every width
            comb = ((np.arange(D) % q) == off).astype(float)
            rows += [comb, comb * (1.0 + np.arange(D) / 1024.0), comb * (2.0 - np.arange(D) / 1024.0), -20.0 - comb]
    return np.array(rows, np.float32)


@pytest.mark.parametrize("D", [3, 4, 37, 61, 130, 131, 361, 386, 387, 512, 514])
def test_pick_crafted(lib, D):
    rng = np.random.default_rng(D)
    E = crafted_rows(D, rng)
    n = E.shape[0]
    widths = [pl for pl in (2, 6, 8) if pl * 64 >= D - 2]
    assert lib.sh_product_pl(D) == widths[0]
    for S in (1, 2, 3, 4):
        sh = Sh(1, n, D, S=S, mu=0.0, omu=1.0)
        C = sh.pad(E[None, None])
        zero = np.zeros((1, sh.nc, D), np.float32)
        x = expected(sh, [E], None, zero)
        assert same_bits(x.energy[0], E)
        for pl in widths:                                                   # a wider pick than the product's gives the same answers
            r = run_pick(lib, sh, C, PL=pl, e_start=zero)
            check_outputs(sh, r, x)
    if D > 4:
        assert x.bins[0, 0].tolist() == [1, 1, 1, 1]                        # a flat row: the first zero entry, and the just-zeroed one again
        assert x.bins[0, 3, 0] == 1 and x.bins[0, 4, 0] == D - 2            # a peak at position 0 and at D - 3


# ---- flags -----------------------------------------------------------------------------------------------------------------------------
def en_to_e(En):
    return (30.0 * (np.asarray(En, np.float64) - 0.5)).astype(np.float32)


def flag_rows(D, rng, n):
    """normalised-energy rows: the twin test's crafted rows of every clause, clean rows, the random families"""
    t = float(TAU)
    lat = np.array([0.4, 0.9, 1.5, 3.0]) * t
    rows = [tent(D, D // 2, -0.3 * t, 3 * t), tent(D, 2, -0.45 * t, 5 * t), tent(D, D // 2, 0.5, 5 * t), tent(D, 1, 0.5, 5 * t)]
    e = tent(D, D // 2, 0.5, 4 * t)
    e[D // 2 + 1] = e[D // 2] - 0.4 * t
    rows.append(e)
    if D >= 18:
        h = D // 2
        rows.append(np.concatenate([tent(h, h // 2, 0.5, 4 * t), tent(D - h, h // 2, 0.5 - 0.6 * t, 4 * t)]))
    # the bounds themselves, on exact multiples of tau (clean slopes of 3 tau): a candidate of energy exactly -tau under a zero pick; two
    # peaks exactly tau apart (one source: the runner-up; two sources, a third peak far below: the order of the picks)
    rows.append(t * (-1.0 - 3.0 * np.abs(np.arange(D) - D // 2)))
    for tops in ((0, -1), (0, -1, -40)):
        w = D // len(tops)
        if w >= 9:
            k = np.arange(D)
            seg = np.minimum(k // w, len(tops) - 1)
            rows.append(0.5 + t * (np.array(tops)[seg] - 3.0 * np.abs(k - (seg * w + w // 2))))
    while len(rows) < n:
        k = len(rows) % 6
        if k == 4:                                                          # exact multiples of tau (en_to_e and the quotient keep them exact): first
            rows.append(0.5 + t * rng.integers(-3, 4, D))                   # differences and gaps of exactly tau, where <= and < part
        elif k == 5:
            rows.append(t * rng.integers(-2, 3, D))
        elif k == 0:
            rows.append(rng.uniform(0, 1, D))
        elif k == 1:
            rows.append(0.5 + rng.choice(lat, D) * rng.choice([-1, 1], D))
        elif k == 2:
            rows.append(rng.choice(lat, D) * rng.choice([-1, 1], D))
        else:
            rows.append(0.5 + 0.3 * np.sin(np.arange(D) * rng.uniform(0.05, 1.5)) + rng.choice(lat, D) * rng.choice([-1, 1], D))
    return np.array(rows[:n])


def expected_flags(sh, x, voiced, unsure, lazy, tau=TAU):
    return np.stack([T.flags_of(x.En[a], None if voiced is None else voiced[a], None if unsure is None else unsure[a], sh.S, tau, lazy)[0] for a in range(sh.arrays)])


@pytest.mark.parametrize("D,S", [(9, 1), (37, 2), (130, 4), (131, 1), (386, 3), (387, 2), (512, 1), (514, 2)])
def test_flags(lib, D, S):
    rng = np.random.default_rng(100 + D)
    n = 70
    sh = Sh(2, n, D, S=S, mu=0.0, omu=1.0)
    E = np.stack([en_to_e(flag_rows(D, rng, n)) for _ in range(2)])
    E[1] = E[1][::-1]                                                       # (the clean rows last in one array, first in the other)
    C = sh.pad(E[None])
    zero = np.zeros((2, sh.nc, D), np.float32)
    x = expected(sh, list(E), None, zero)
    for lazy in (0, 1):
        r = run_pick(lib, sh, C, mode=1, lookback=4, part=zero, state_in=np.zeros((2, D), np.float32), lazy=lazy)
        want = expected_flags(sh, x, None, None, bool(lazy))
        assert np.array_equal(r.flags, want)
        assert int(r.stats[0]) == int(want.sum())
        assert 0 < want.sum() < want.size
        check_outputs(sh, r, x)
        assert list(r.last_vchunk) == [sh.nc - 1] * 2
    assert r.flags[0, 2] == 0 and r.flags[0, 3] == 0 and r.flags[0, 0] == 1 and r.flags[0, 4] == 1      # clean tents; the zero clause; the flat top


def clean_call(sh, rng):
    """every row a clean single peak (never sensitive for one source), at a random column"""
    t = float(TAU)
    En = np.stack([[tent(sh.D, int(rng.integers(2, sh.D - 2)), 0.5, 5 * t) for _ in range(sh.n)] for _ in range(sh.arrays)])
    return en_to_e(En)


FLAT = en_to_e(np.full(1, 0.5))[0]


def test_unsure_frames(lib):
    rng = np.random.default_rng(7)
    sh = Sh(3, 70, 40, mu=0.0, omu=1.0)
    E = clean_call(sh, rng)
    unsure = np.zeros((3, 70), np.uint8)
    unsure[0, 30] = unsure[1, 66] = 1
    zero = np.zeros((3, sh.nc, 40), np.float32)
    r = run_pick(lib, sh, sh.pad(E[None]), mode=1, lookback=4, part=zero, state_in=zero[:, 0].copy(), unsure=unsure, lazy=1)
    want = np.zeros((3, 70), np.uint8)
    want[0, 30:37] = 1                                                     # across the batch boundary
    want[1, 66:70] = 1                                                     # to the end of its array; the next array's first frames stay clear
    assert np.array_equal(r.flags, want) and int(r.stats[0]) == 11
    x = expected(sh, list(E), None, zero)
    assert np.array_equal(expected_flags(sh, x, None, unsure, True), want)


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
def check_plan(sh, r, units, cfrom, need0=None, n_flagged=None):
    """units: the set the twin lists; cfrom: {(a, chunk): chunk_from}"""
    need0 = np.zeros(r.list_len, np.int32) if need0 is None else need0
    fresh = {e for e in units if not need0[e]}
    k = int(r.n_list[0])
    assert k == len(fresh) and set(r.list[:k].tolist()) == fresh and (r.list[k:] == -5).all()
    want_need = need0.copy()
    want_need[list(units)] = 1
    assert np.array_equal(r.need, want_need)
    want_from = np.full((sh.arrays, sh.nc), NO_FLAG, np.int32)
    for (a, c), v in cfrom.items():
        want_from[a, c] = v
    assert np.array_equal(r.chunk_from, want_from)
    kc = int(r.n_clist[0])
    assert kc == len(cfrom) and set(r.clist[:kc].tolist()) == {a * sh.nc + c for a, c in cfrom} and (r.clist[kc:] == -5).all() and r.n_clist[1] == 0
    assert int(r.stats[1]) == len(fresh)
    if n_flagged is not None:
        assert int(r.stats[0]) == n_flagged


def plan_of(sh, r, flags, voiced, hist_valid):
    units, cfrom = set(), {}
    for a in range(sh.arrays):
        u, cf = T.plan_rows(flags[a], None if voiced is None else voiced[a], a, sh.gpa, r.hist_base, hist_valid)
        units |= u
        cfrom.update({(a, c): v for c, v in cf.items()})
    return units, cfrom


def test_plan_whole_rows_ungated(lib):
    rng = np.random.default_rng(8)
    sh = Sh(2, 70, 40, mu=0.0, omu=1.0)
    E = clean_call(sh, rng)
    for t in (0, 15, 16, 17, 31, 32):
        E[0, t] = FLAT                                                      # a flat row is sensitive
    E[1, 40] = E[1, 42] = FLAT                                              # two flagged frames that share units: listed once
    E[1, 63] = FLAT                                                         # its earliest row, 47, is the only one of its range in unit 11
    zero = np.zeros((2, sh.nc, 40), np.float32)
    need0 = np.zeros(2 * sh.gpa + 2 * T.HIST_UNITS, np.int32)
    need0[sh.gpa + 9] = 1                                                   # a unit of frame 40's range already on the list: not listed again
    for need in (None, need0):
        r = run_pick(lib, sh, sh.pad(E[None]), mode=1, lookback=4, part=zero, state_in=zero[:, 0].copy(), need=need)
        want = np.zeros((2, 70), np.uint8)
        want[0, [0, 15, 16, 17, 31, 32, 69]] = 1
        want[1, [40, 42, 63, 69]] = 1
        assert np.array_equal(r.flags, want)
        units, cfrom = plan_of(sh, r, want, None, False)
        assert cfrom == {(0, 0): 0, (0, 1): 0, (0, 2): 1, (1, 1): 0, (1, 2): 1}
        assert sh.gpa + 9 in units and len(units) == 9 + 5 + 5 + 7         # array 0: units 0 .. 8 and 13 .. 17; array 1: 6 .. 10 once, and 11 .. 17
        assert sh.gpa + 11 in units
        check_plan(sh, r, units, cfrom, need, n_flagged=11)


def test_plan_whole_rows_gated(lib):
    rng = np.random.default_rng(9)
    sh = Sh(2, 161, 37, mu=0.0, omu=1.0)
    E = clean_call(sh, rng)
    voiced = np.zeros((2, 161), np.uint8)
    voiced[0, [0, 1, 2, 3, 100, 101, 102, 160]] = 1                         # the walk from 160 crosses three chunks and > 64 silent frames, and ends at row 0
    adv = [20, 25, 30] + list(range(33, 47)) + [50]                         # frame 50: exactly 17 advancing predecessors over two chunks:
    voiced[1, adv] = 1                                                      # the sixteen from 25 on are its rows, frame 20 stays out
    voiced[1, 120] = 1
    E[1, 50] = FLAT
    zero = np.zeros((2, sh.nc, 37), np.float32)
    r = run_pick(lib, sh, sh.pad(E[None]), mode=1, voiced=voiced, e_start=zero, last_vchunk=[5, 3])
    want = np.zeros((2, 161), np.uint8)
    want[0, 160] = want[1, 50] = want[1, 120] = 1
    assert np.array_equal(r.flags, want)
    units, cfrom = plan_of(sh, r, want, voiced, False)
    assert cfrom[(0, 5)] == 0 and cfrom[(1, 1)] == 0 and sh.gpa + 6 in units and sh.gpa + 5 not in units
    assert {0, 25, 40} <= units
    check_plan(sh, r, units, cfrom, n_flagged=3)
    x = expected(sh, list(E), voiced, zero)
    check_outputs(sh, r, x)


def test_plan_history_and_lazy(lib):
    rng = np.random.default_rng(10)
    sh = Sh(2, 70, 40, planes=2, mu=MU_REAL, omu=OMU_REAL, P=1)
    vals = rng.standard_normal((2, 2, 70, 40)).astype(np.float32) * F(0.01)
    vals[0] += en_to_e(tent(40, 20, 0.5, 5 * float(TAU)))                   # one stable peak (mu = 0.8: which frames get flagged while it builds up is the twin's call)
    vals[:, 0, :8] = 0.0                                                    # flat rows from a zero state: flagged frames below REPAIR_WARM
    C = sh.pad(vals)
    Cs = sums(sh, C)
    state = np.zeros((2, 40), np.float32)
    part = np.stack([T.chunk_scan(Cs[a], None, sh.mu, sh.omu)[0] for a in range(2)])
    r = run_pick(lib, sh, C, mode=1, lookback=4, part=part, state_in=state, lazy=1, hist_valid=1)
    x = expected(sh, Cs, None, r.e_start)
    check_outputs(sh, r, x)
    want = expected_flags(sh, x, None, None, True)
    assert np.array_equal(r.flags, want)
    if not want[:, :16].any():
        pytest.fail("the case needs a flagged frame below REPAIR_WARM")
    units, cfrom = plan_of(sh, r, want, None, True)
    assert min(cfrom.values()) == -1 and max(units) >= r.hist_base
    check_plan(sh, r, units, cfrom, n_flagged=int(want.sum()))
    # lazy: the last HIST_FRAMES coarse rows (planes summed) and the energies in front of them
    for a in range(2):
        assert same_bits(r.hist_C_out[a, :, :40], Cs[a][-16:]) and np.isnan(r.hist_C_out[a, :, 40:]).all()
        assert same_bits(r.e_hist_out[a], x.energy[a, 70 - 17])


def test_plan_candidate_columns(lib):
    rng = np.random.default_rng(11)
    sh = Sh(2, 70, 131, mu=0.0, omu=1.0)
    E = clean_call(sh, rng)
    t = float(TAU)
    flat_top = tent(131, 60, 0.5, 5 * t)
    flat_top[61] = flat_top[60] - 0.3 * t                                   # sensitive, but a narrow set of columns
    for a, f in ((0, 3), (0, 20), (0, 21), (0, 45), (1, 33), (1, 64)):
        E[a, f] = en_to_e(flat_top if f != 45 else np.roll(flat_top, 40))
    E[1, 50] = FLAT                                                         # every column
    dead = np.zeros((2, 70), np.uint8)
    dead[0, 4:16] = 1                                                       # units 1 .. 3 of frame 20's range hold only dead rows: not listed
    dead[1, 17:33] = 1                                                      # frame 33: only its own row lives
    unsure = np.zeros((2, 70), np.uint8)
    unsure[0, 60] = unsure[1, 38] = 1                                       # clean frames the analysis could not vouch for: they and their six successors take
    #                                                                         every column -- in a chunk that also holds a narrow frame (45; 33), and across a chunk boundary
    zero = np.zeros((2, sh.nc, 131), np.float32)
    r = run_pick(lib, sh, sh.pad(E[None]), mode=1, lookback=4, part=zero, state_in=zero[:, 0].copy(), cand=True, dead=dead, unsure=unsure)
    x = expected(sh, list(E), None, zero)
    want = expected_flags(sh, x, None, unsure, False)
    assert np.array_equal(r.flags, want) and want[0, 3] and want[1, 50] and want.sum() == 9 + 7 + 7
    assert want[0, 60:67].all() and want[1, 38:45].all() and not T.sens(x.En[0, 66], 1, TAU) and not T.sens(x.En[1, 44], 1, TAU)
    units, cfrom, ncol, nall = {}, {}, 0, 0
    for a in range(2):
        masks = {}
        for f in np.flatnonzero(want[a]):
            forced_or_unsure = f == 69 or bool(unsure[a, max(f - 6, 0):f + 1].any())
            masks[int(f)], full = T.candidates(x.En[a, f], TAU, full=forced_or_unsure)
            assert full or not forced_or_unsure
            ncol += int(masks[int(f)].sum())
            nall += full
        u, cf = T.plan_cand(want[a], masks, dead[a], a, sh.gpa, r.hist_base, False)
        units.update(u)
        cfrom.update({(a, c): v for c, v in cf.items()})
    assert 1 not in units and 2 not in units and 3 not in units and 0 in units and 5 in units
    assert not masks[64].all() and 0 < masks[64].sum() < 12
    assert masks[44].all() and not T.candidates(x.En[1, 44], TAU)[1]          # (the last successor: every column only because of the unsure frame)
    check_plan(sh, r, set(units), cfrom, n_flagged=23)
    assert int(r.stats[2]) == ncol and int(r.stats[3]) == nall and nall == 3 + 14
    got = np.unpackbits(r.umask.view(np.uint8), axis=1, bitorder="little")[:, :131].astype(bool)
    for e in range(r.list_len):
        assert np.array_equal(got[e], units.get(e, np.zeros(131, bool))), e
    assert not np.unpackbits(r.umask.view(np.uint8), axis=1, bitorder="little")[:, 131:].any()


def test_miss_list(lib):
    rng = np.random.default_rng(12)
    sh = Sh(2, 70, 131, mu=0.0, omu=1.0)
    E = clean_call(sh, rng)
    E[0, 40] = FLAT                                                         # chunk 1 of array 0 holds a flag; the last chunks hold the forced frames
    zero = np.zeros((2, sh.nc, 131), np.float32)
    x = expected(sh, list(E), None, zero)
    pred = np.array([int(x.bins[0, 3, 0]), -1], np.int32)
    r = run_pick(lib, sh, sh.pad(E[None]), mode=1, lookback=4, part=zero, state_in=zero[:, 0].copy(), pred=pred)
    assert r.PL == 6
    want = {a * 70 + f for a in range(2) for f in range(70) if f // 32 == 0 or (a == 1 and f // 32 == 1) if x.bins[a, f, 0] != pred[a]}
    k = int(r.n_miss[0])
    assert k == len(want) and set(r.n_miss[1:1 + k].tolist()) == want and (r.n_miss[1 + k:] == -5).all()
    assert 3 not in want and 0 < len(want) < 96
    r = run_pick(lib, sh, sh.pad(E[None]), PL=8, mode=1, lookback=4, part=zero, state_in=zero[:, 0].copy(), pred=pred)
    assert r.n_miss[0] == 0 and (r.n_miss[1:] == -5).all()                  # the widest pick appends nothing


# ---- the second pick -------------------------------------------------------------------------------------------------------------------
def run_repick(lib, sh, C, voiced, e_start, flags, clist, chunk_from, last_vchunk, grid_x, hist=None, bins0=None):
    r = R()
    r.grid = sh.grid()
    r.clist = np.full(sh.arrays * sh.nc, -5, np.int32)
    r.clist[:len(clist)] = clist
    r.n_clist = np.array([len(clist), 0], np.int32)
    r.chunk_from = chunk_from.astype(np.int32).copy()
    r.n_list = np.array([3], np.int32)
    r.state_out = np.full((sh.arrays, sh.D), np.nan, np.float32)
    r.doa_bin = np.full((sh.arrays, sh.n, sh.S), -99, np.int32) if bins0 is None else bins0.copy()
    r.doa_rad = np.full((sh.arrays, sh.n, sh.S), np.nan, np.float32)
    r.prob = np.full((sh.arrays, sh.n, sh.S), np.nan, np.float32)
    r.energy = np.full((sh.arrays, sh.n, sh.D), np.nan, np.float32)
    lv = np.asarray(last_vchunk, np.int32)
    q = Repick()
    q.PL, q.grid_x, q.C, q.voiced, q.e_start, q.flags = lib.sh_product_pl(sh.D), grid_x, ptr(C), ptr(voiced), ptr(e_start), ptr(flags)
    q.clist, q.clist_len, q.n_clist, q.chunk_from, q.last_vchunk, q.n_list = ptr(r.clist), r.clist.size, ptr(r.n_clist), ptr(r.chunk_from), ptr(lv), ptr(r.n_list)
    q.state_out, q.grid, q.doa_bin, q.doa_rad, q.prob, q.energy = ptr(r.state_out), ptr(r.grid), ptr(r.doa_bin), ptr(r.doa_rad), ptr(r.prob), ptr(r.energy)
    if hist is not None:
        q.hist_C_in, q.e_hist_in = ptr(hist[1]), ptr(hist[0])
    d = sh.dims()
    call(lib.sh_repick, ctypes.addressof(d), ctypes.addressof(q))
    return r


def check_repick(sh, r, Cs, voiced, flags, e_start, clist, chunk_from, last_vchunk, hist=None, bins0=None):
    want_bin = np.full((sh.arrays, sh.n, sh.S), -99, np.int32) if bins0 is None else bins0.copy()
    touched = np.zeros((sh.arrays, sh.n), bool)
    want_prob = np.full((sh.arrays, sh.n, sh.S), np.nan, np.float32)
    want_energy = np.full((sh.arrays, sh.n, sh.D), np.nan, np.float32)
    want_state = np.full((sh.arrays, sh.D), np.nan, np.float32)
    want_from = chunk_from.copy()
    for ci in clist:
        a, c = divmod(int(ci), sh.nc)
        h = None if hist is None else (hist[0][a], hist[1][a, :, :sh.D])
        picks, rows, E = T.repick(Cs[a], None if voiced is None else voiced[a], flags[a], e_start[a], c, int(chunk_from[a, c]), sh.mu, sh.omu, sh.P, sh.S, hist=h)
        for t, (b, v) in picks.items():
            want_bin[a, t], want_prob[a, t], touched[a, t] = b, v, True
        for t, row in rows.items():
            want_energy[a, t] = row
        if c == last_vchunk[a]:
            want_state[a] = E
        want_from[a, c] = NO_FLAG
    assert np.array_equal(r.doa_bin, want_bin)
    assert same_bits(r.prob[touched], want_prob[touched]) and np.isnan(r.prob[~touched]).all()
    assert same_bits(r.doa_rad[touched], r.grid[want_bin[touched]]) and np.isnan(r.doa_rad[~touched]).all()
    assert same_bits(r.energy, want_energy) and same_bits(r.state_out, want_state)
    assert np.array_equal(r.chunk_from, want_from)                          # every consumed entry reset, no other touched
    assert r.n_list[0] == 0 and list(r.n_clist) == [0, 0]
    return touched


@pytest.mark.parametrize("D,planes", [(37, 1), (131, 2), (387, 1)])
def test_repick_ungated(lib, D, planes):
    rng = np.random.default_rng(13 + D)
    sh = Sh(2, 161, D, S=2, P=6, planes=planes)
    C = sh.pad(rng.standard_normal((planes, 2, 161, D)).astype(np.float32))
    Cs = sums(sh, C)
    e_start = rng.standard_normal((2, sh.nc, D)).astype(np.float32)
    hist = (rng.standard_normal((2, D)).astype(np.float32), np.full((2, 16, sh.Dp), np.nan, np.float32))
    hist[1][:, :, :D] = rng.standard_normal((2, 16, D))
    flags = np.zeros((2, 161), np.uint8)
    flags[0, [3, 40, 41, 70, 160]] = 1
    flags[1, [5, 100]] = 1
    chunk_from = np.full((2, sh.nc), NO_FLAG, np.int32)
    chunk_from[0, [0, 1, 2, 5]] = [0, 1, 1, 4]                              # a start in the chunk itself and in the chunk before
    chunk_from[1, [0, 3]] = [-1, 2]                                         # and from the history
    clist = [1, 0, 5, 2, 6 + 0, 6 + 3]
    for grid_x, listed in ((2, clist[:5]), (8, clist[:1]), (3, []), (4, clist)):
        cf = np.full((2, sh.nc), NO_FLAG, np.int32)
        for ci in listed:
            cf[divmod(ci, sh.nc)] = chunk_from[divmod(ci, sh.nc)]
        r = run_repick(lib, sh, C, None, e_start, flags, listed, cf, [5, 3], grid_x, hist=hist)
        touched = check_repick(sh, r, Cs, None, flags, e_start, listed, cf, [5, 3], hist=hist)
        assert touched.sum() == sum(int(flags[divmod(ci, sh.nc)[0], divmod(ci, sh.nc)[1] * 32:divmod(ci, sh.nc)[1] * 32 + 32].sum()) for ci in listed)


def test_repick_gated(lib):
    rng = np.random.default_rng(14)
    sh = Sh(2, 161, 130, S=1, P=6, planes=3)
    C = sh.pad(rng.standard_normal((3, 2, 161, 130)).astype(np.float32))
    Cs = sums(sh, C)
    e_start = rng.standard_normal((2, sh.nc, 130)).astype(np.float32)
    voiced = (rng.random((2, 161)) < 0.3).astype(np.uint8)
    flags = np.zeros((2, 161), np.uint8)
    flags[0, [70, 150]] = flags[1, [33, 160]] = 1
    voiced[flags != 0] = 1
    chunk_from = np.full((2, sh.nc), NO_FLAG, np.int32)
    chunk_from[0, [2, 4]] = [0, 0]                                          # two and four chunks back
    chunk_from[1, [1, 5]] = [1, 3]
    clist = [2, 4, 6 + 1, 6 + 5]
    r = run_repick(lib, sh, C, voiced, e_start, flags, clist, chunk_from, [4, 5], 3)
    check_repick(sh, r, Cs, voiced, flags, e_start, clist, chunk_from, [4, 5])


@pytest.mark.parametrize("cand", [False, True])
def test_pick_then_repick_chain(lib, cand):
    """the real outputs of a coarse pass go into the second pick, after a host-side 'repair' that copies the exact map's rows of the listed
    units (candidate columns: at the unit's columns only)"""
    rng = np.random.default_rng(15 + cand)
    sh = Sh(2, 100, 131, S=1, P=6)
    exact = rng.standard_normal((1, 2, 100, 131)).astype(np.float32)
    exact[0, :, :, 40] += 8.0                                               # a stable peak, so that most frames are not sensitive
    exact[0, 0, 50:53, 90] += 8.0                                           # and a second one of the same height for a few frames
    coarse = (exact + rng.standard_normal(exact.shape).astype(np.float32) * F(1e-3)).astype(np.float32)
    C = sh.pad(coarse)
    Cs = sums(sh, C)
    state, tau = np.zeros((2, 131), np.float32), F(2.0 ** -14)
    part = np.stack([T.chunk_scan(Cs[a], None, sh.mu, sh.omu)[0] for a in range(2)])
    r = run_pick(lib, sh, C, mode=1, lookback=4, part=part, state_in=state, cand=cand, tau=tau)
    x = expected(sh, Cs, None, r.e_start)
    check_outputs(sh, r, x)
    assert np.array_equal(r.flags, expected_flags(sh, x, None, None, False, tau)) and 2 < r.flags.sum() < 100
    k = int(r.n_list[0])
    for e in r.list[:k]:
        a, u = divmod(int(e), sh.gpa)
        cols = np.unpackbits(r.umask[e].view(np.uint8), bitorder="little")[:131].astype(bool) if cand else np.ones(131, bool)
        rows = slice(4 * u, min(4 * u + 4, 100))
        C[0, a, rows, :131] = np.where(cols, exact[0, a, rows], C[0, a, rows, :131])
    kc = int(r.n_clist[0])
    clist = r.clist[:kc].tolist()
    Cs2 = sums(sh, C)
    r2 = run_repick(lib, sh, C, None, r.e_start, r.flags, clist, r.chunk_from, r.last_vchunk, 4, bins0=r.doa_bin)
    check_repick(sh, r2, Cs2, None, r.flags, r.e_start, clist, r.chunk_from, r.last_vchunk, bins0=r.doa_bin)


# ---- the small kernels -----------------------------------------------------------------------------------------------------------------
def test_hist_list_and_settle(lib):
    lst, need, n_list = np.full(40, -5, np.int32), np.zeros(40, np.int32), np.array([9], np.int32)
    call(lib.sh_hist_list, ptr(lst), ptr(need), 40, ptr(n_list), 12)
    assert list(lst[:12]) == list(range(12)) and (lst[12:] == -5).all() and list(need) == [1] * 12 + [0] * 28 and n_list[0] == 12
    rng = np.random.default_rng(16)
    for D in (3, 131, 512):
        Dp = dp_of(D)
        e_hist = rng.standard_normal((3, D)).astype(np.float32)
        hist_C = np.full((3, 16, Dp), np.nan, np.float32)
        hist_C[:, :, :D] = rng.standard_normal((3, 16, D))
        state, n_list = np.full((3, D), np.nan, np.float32), np.array([9], np.int32)
        call(lib.sh_hist_settle, ptr(e_hist), ptr(hist_C), ptr(state), ptr(n_list), 3, D, Dp, float(MU_REAL), float(OMU_REAL))
        want = e_hist.copy()
        for j in range(16):
            want = T.iir_step(MU_REAL, want, OMU_REAL, hist_C[:, j, :D])
        assert same_bits(state, want) and n_list[0] == 0


@pytest.mark.parametrize("S", [1, 4])
def test_doa_fill(lib, S):
    rng = np.random.default_rng(17 + S)
    for n in (33, 1500):                                                    # 1 500 frames: a thread fills a segment of two
        voiced = (rng.random((3, n)) < 0.3).astype(np.uint8)
        voiced[0] = 0                                                       # no voiced frame at all
        voiced[1, :n // 2] = 0                                              # the first voiced frame late
        voiced[1, n // 2] = 1
        voiced[2, n - 1] = 0
        bins = rng.integers(0, 500, (3, n, S)).astype(np.int32)
        rad, prob = rng.standard_normal((3, n, S)).astype(np.float32), rng.standard_normal((3, n, S)).astype(np.float32)
        last = [rng.integers(0, 500, (3, S)).astype(np.int32), rng.standard_normal((3, S)).astype(np.float32), rng.standard_normal((3, S)).astype(np.float32)]
        want, want_last = [bins.copy(), rad.copy(), prob.copy()], [v.copy() for v in last]
        for a in range(3):
            cur = [v[a].copy() for v in last]
            for t in range(n):
                for w, c in zip(want, cur):
                    if voiced[a, t]:
                        c[:] = w[a, t]
                    else:
                        w[a, t] = c
            for w, c in zip(want_last, cur):
                w[a] = c
        call(lib.sh_doa_fill, ptr(voiced), 3, n, S, ptr(bins), ptr(rad), ptr(prob), ptr(last[0]), ptr(last[1]), ptr(last[2]))
        assert np.array_equal(bins, want[0]) and same_bits(rad, want[1]) and same_bits(prob, want[2])
        assert np.array_equal(last[0], want_last[0]) and same_bits(last[1], want_last[1]) and same_bits(last[2], want_last[2])


def test_gate(lib):
    rng = np.random.default_rng(18)
    n, fft_n, needed, margin, eps = 200, 1024, 48000, F(3.0), 1e-10
    power = (10.0 ** rng.uniform(-6, -2, (3, n))).astype(np.float32)
    state = np.zeros((3, 4))
    state[1] = [3.0e-3, 20 * 1024.0, 0.0, 0.0]                              # an estimation under way
    state[2] = [-41.5, 60 * 1024.0, -41.5, 1.0]                             # a floor from an earlier call
    want_state, floors, first = state.copy(), [], []
    shown = np.full((3, n), np.nan)
    for a in range(3):
        acc, consumed, floor_db, est = state[a]
        t = 0
        while t < n and not est:
            acc += float(power[a, t]) * fft_n + eps
            consumed += fft_n
            shown[a, t] = acc
            if consumed >= needed:
                est = 1.0
                floor_db = 10.0 * np.log10(acc / consumed) + float(margin)
                acc = shown[a, t] = floor_db
            t += 1
        want_state[a] = [acc, consumed, floor_db, est]
        floors.append(floor_db)
        first.append(t)
    # later frames: keep every power at least 1e-3 dB from the floor (a hundred float32 spacings at 100 dB: the device log10f is not bit-pinned)
    for a in range(3):
        db = 10.0 * np.log10(power[a].astype(np.float64))
        near = np.abs(db - floors[a]) < 1e-3
        near[:first[a]] = False
        power[a, near] *= F(1.01)
    st = state.copy()
    voiced = np.full((3, n), 7, np.uint8)
    pout, post0 = np.full((3, n), np.nan, np.float32), np.full(3, -9, np.int32)
    call(lib.sh_gate, ptr(power), 3, n, fft_n, needed, float(margin), eps, ptr(st), ptr(voiced), ptr(pout), ptr(post0))
    assert first[0] == 47 and first[1] == 27 and first[2] == 0
    assert np.allclose(st, want_state, rtol=1e-12, atol=0) and np.array_equal(st[:, 3], want_state[:, 3]) and np.array_equal(st[:, 1], want_state[:, 1])
    assert list(post0) == [46, 26, 0]
    for a in range(3):
        db = 10.0 * np.log10(power[a].astype(np.float64))
        assert (voiced[a, :first[a]] == 0).all() and np.array_equal(voiced[a, first[a]:], (db[first[a]:] > floors[a]).astype(np.uint8))
        assert np.allclose(pout[a, :first[a]], shown[a, :first[a]].astype(np.float32), rtol=1e-6) and np.allclose(pout[a, first[a]:], db[first[a]:], atol=1e-4)
    assert 0 < voiced[0].sum() < n - 47


# ---- the widest grid the pick's lanes cover ---------------------------------------------------------------------------------------------
def test_pick_at_D_514(lib):
    """D = 514 = 8 * 64 + 2 is the last grid whose positions 64 lanes of eight cover (mca_internal.h: "the peak pick handles D <= 514"); the
    block, max(round_up(514, 64), 512), is 576 threads: nine waves, which k_scan_pick<8, MODE> is bound to (with a bound of 512 the runtime
    turned the launch down, hipError_t 719).  Crafted rows in both modes, and the recursion with the look-back on three planes."""
    D = 514
    rng = np.random.default_rng(D)
    E = crafted_rows(D, rng)
    for S in (1, 4):
        sh = Sh(1, E.shape[0], D, S=S, mu=0.0, omu=1.0)
        zero = np.zeros((1, sh.nc, D), np.float32)
        x = expected(sh, [E], None, zero)
        r = run_pick(lib, sh, sh.pad(E[None, None]), e_start=zero)
        assert r.PL == 8
        check_outputs(sh, r, x)
    r = run_pick(lib, sh, sh.pad(E[None, None]), mode=1, lookback=4, part=zero, state_in=zero[:, 0].copy())
    check_outputs(sh, r, x)
    assert np.array_equal(r.flags, expected_flags(sh, x, None, None, False)) and int(r.stats[0]) == int(r.flags.sum())
    sh = Sh(2, 70, D, S=2, P=6, planes=3)
    C, state = operands("real", sh, rng)
    Cs = sums(sh, C)
    part, nv = run_partial(lib, sh, C, None)
    r = run_pick(lib, sh, C, lookback=4, part=part, state_in=state)
    assert same_bits(r.e_start, np.stack([T.lookback(part[a], state[a], sh.mu, CONTRACTION == "fused") for a in range(2)]))
    x = expected(sh, Cs, None, r.e_start)
    check_outputs(sh, r, x)
    assert same_bits(r.state_out, x.energy[:, -1])
