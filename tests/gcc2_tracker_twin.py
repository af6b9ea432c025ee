"""The particle-filter DOA tracker of FreqGCCBinauralLocalisation, restated in numpy float64 and integers (DESIGN.md, section
"The DOA tracker", [BUILD-DEFINES]).  It does not call the library: setProbability (gcc2_prob_at) and the wave order of the row's
min / sum (gcc2_row_min_sum) are restated here, so that the GPU outputs can be compared with it as bits.

Every floating-point step below is one IEEE double operation (numpy never contracts a multiply and an add), random numbers and the
resampling are integer arithmetic, and the two sums whose order matters (the row sum, the weighted mean) run in the order of a
64-lane wave: lane l folds elements l, l + 64, ... in turn, then a xor butterfly 32, 16, ... 1."""
import numpy as np

U64 = np.uint64
G = U64(0x9E3779B97F4A7C15)
HALFPI = 1.57079632679489661923
PI = 3.14159265358979323846


def _u64(v):
    return np.asarray(v).astype(U64)


def mix(z):
    """the splitmix64 finaliser, elementwise on uint64 (mod 2^64)"""
    z = _u64(z)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def draw(key, c):
    """output number c of a splitmix64 stream started at key"""
    with np.errstate(over="ignore"):
        return mix(_u64(key) + G * (_u64(c) + U64(1)))


def make_key(seed, a, track, upd):
    with np.errstate(over="ignore"):
        k = mix(_u64(seed) + G)
        for v in (a, track, upd):
            k = mix((k ^ _u64(v)) + G)
    return k


def gauss(key, i):
    """sum of the twelve 16-bit fields of three draws, centred and scaled: exact, mean 0, variance 1 - 2^-32, support +-6"""
    i = _u64(i)
    s = np.zeros(i.shape, dtype=np.int64)
    for j in range(3):
        d = draw(key, U64(3) * i + U64(j))
        for sh in (0, 16, 32, 48):
            s += ((d >> U64(sh)) & U64(0xFFFF)).astype(np.int64)
    return (2 * s - 12 * 65535).astype(np.float64) / 131072.0


def unif(key, c):
    return (draw(key, c) >> U64(11)).astype(np.float64) * 2.0 ** -53


def wave_sum(v):
    """sum of v[0..n) in the order of gcc2_row_min_sum: 64 lanes, lane l folds l, l + 64, ..., then the xor butterfly"""
    v = np.asarray(v, dtype=np.float64)
    n = len(v)
    acc = np.zeros(64)
    for k in range((n + 63) // 64):
        part = v[k * 64:(k + 1) * 64]
        acc[:len(part)] = acc[:len(part)] + part
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ off]
    return float(acc[0])


def row_min_sum_adj(row):
    """-> min, sum - min * D of a correlation row (BinauralLocalisation.cpp:584-588), the sum in wave order"""
    row = np.asarray(row, dtype=np.float64)
    mn = float(row.min())
    return mn, wave_sum(row) - mn * float(len(row))


def prob_at(row, mn, sum_adj, step, grid, doa):
    """setProbability (BinauralLocalisation.cpp:590-630) at the angles doa (float64 array), the reference's mixed arithmetic:
    angle2DOAidx clamps a FLOAT copy of the angle, the interpolation uses the double one"""
    row = np.asarray(row, dtype=np.float64)
    doa = np.atleast_1d(np.asarray(doa, dtype=np.float64))
    g64 = np.asarray(grid, dtype=np.float32).astype(np.float64)
    D = len(row)
    a = doa.astype(np.float32).astype(np.float64)
    a = np.maximum(a, -HALFPI).astype(np.float32).astype(np.float64)
    a = np.minimum(a, HALFPI).astype(np.float32).astype(np.float64)
    idx = ((a + HALFPI) / float(np.float32(step))).astype(np.int64)
    idx = np.clip(idx, 0, D - 1)
    angle = g64[idx]
    inner = (idx > 0) & (idx < D - 1)
    lo = np.where(angle > doa, idx - 1, idx)
    lo = np.clip(lo, 0, D - 2)
    pc, nc, pd, nd = row[lo], row[lo + 1], g64[lo], g64[lo + 1]
    slope = (nc - pc) / (nd - pd)
    p = np.where(inner, slope * (doa - pd) + pc, row[idx])
    pb = (p - mn) / sum_adj if sum_adj > 0.0 else np.zeros(len(doa))
    return np.where(pb < 0.01, 0.0, pb)


def resample_ancestors(q, u):
    """systematic resampling on integer weights q (uint64 [N], sum Q > 0) with the offset u in [0, 1) -> ancestor of every slot"""
    q = _u64(q)
    N = len(q)
    C = np.cumsum(q, dtype=U64)
    Q = int(C[-1])
    T = np.floor((np.arange(N, dtype=np.float64) + u) * (float(Q) / float(N))).astype(U64)
    return np.minimum(np.searchsorted(C, T, side="right"), N - 1)


class Tracker:
    """One array's tracker.  cfg: n_particles (0 = 500), n_inject (0 = n_particles // 20, -1 = none), seed, sigma_init, sigma_step
    (radians, 0 = the grid step).  a_index: the array's index in the context (0xFFFFFFFF for the frame hook)."""

    def __init__(self, grid, step, a_index=0, n_particles=0, n_inject=0, seed=0, sigma_init=0.0, sigma_step=0.0):
        self.grid = np.asarray(grid, dtype=np.float32)
        self.step = np.float32(step)
        self.a = a_index
        self.N = n_particles or 500
        self.n_inject = 0 if n_inject < 0 else (n_inject or self.N // 20)
        self.seed = seed
        self.sigma_init = float(sigma_init) or float(self.step)
        self.sigma_step = float(sigma_step) or float(self.step)
        D = len(self.grid)
        self.row = np.zeros(D)
        self.x = np.zeros(self.N)
        self.alive, self.track, self.upd = False, 0, 0
        self.doa, self.prob = 0.0, -1.0
        self.silence = 0
        self.last_q = None

    # ---- the filter -----------------------------------------------------------------------------------------------------
    def _seed(self, argmax):
        self.track += 1
        self.upd = 0
        key = make_key(self.seed, self.a, self.track, 0)
        g = gauss(key, np.arange(self.N))
        self.x = np.minimum(np.maximum(float(self.grid[argmax]) + self.sigma_init * g, -PI), PI)
        self.alive = True

    def update(self):
        N = self.N
        self.upd += 1
        key = make_key(self.seed, self.a, self.track, self.upd)
        x = np.minimum(np.maximum(self.x + self.sigma_step * gauss(key, np.arange(N)), -HALFPI), HALFPI)
        mn, sum_adj = row_min_sum_adj(self.row)
        w = prob_at(self.row, mn, sum_adj, self.step, self.grid, x)
        q = np.floor(w * 2.0 ** 40).astype(U64)
        Q = int(q.sum(dtype=U64))
        self.last_q = q
        if Q > 0:
            e = wave_sum(q.astype(np.float64) * x) / float(Q)
            x = x[resample_ancestors(q, float(unif(key, 3 * N)))]
        else:
            e = wave_sum(x) / float(N)
        if self.n_inject > 0:
            j = np.arange(self.n_inject)
            x = x.copy()
            x[N - self.n_inject:] = (unif(key, 3 * N + 1 + j) - 0.5) * PI
        self.x = x
        return e

    # ---- one frame (the control flow of BinauralLocalisation.cpp:429-561) ---------------------------------------------------
    def voiced_frame(self, row, argmax):
        self.row = np.asarray(row, dtype=np.float64)
        mn, sum_adj = row_min_sum_adj(self.row)
        self.prob = float(prob_at(self.row, mn, sum_adj, self.step, self.grid, self.doa)[0])      # :454
        if not self.alive:
            self._seed(int(argmax))                                                                # :457-465
        self.doa = self.update()                                                                   # :473
        self.silence = 0
        return 1

    def silent_frame(self, floor_known, windows_to_decay):
        if not floor_known:
            return 0
        fired = 0
        if self.silence < windows_to_decay:                                                        # :536-548
            if self.alive:
                self.doa = self.update()
                fired = 2
        else:                                                                                      # :551-558
            self.alive = False
        self.silence += 1
        return fired


def run(rows, voiced, argmax, floor_from, windows_to_decay, grid, step, a_index=0, **cfg):
    """rows [F][D] (the row of every voiced frame; other frames are not read), voiced [F], argmax [F], floor_from: the first frame
    at which the power floor is known -> dict(doa, prob float64 [F], fired, track int [F], particles [N], alive, tracker)"""
    F = len(voiced)
    tr = Tracker(grid, step, a_index, **cfg)
    doa, prob = np.zeros(F), np.zeros(F)
    fired, track = np.zeros(F, dtype=np.int64), np.zeros(F, dtype=np.int64)
    for t in range(F):
        if voiced[t]:
            fired[t] = tr.voiced_frame(rows[t], argmax[t])
        else:
            fired[t] = tr.silent_frame(t >= floor_from, windows_to_decay)
        doa[t], prob[t], track[t] = tr.doa, tr.prob, tr.track
    return dict(doa=doa, prob=prob, fired=fired, track=track, particles=tr.x.copy(), alive=tr.alive, tracker=tr)


def reference_grid(step_deg=3.0):
    """-> grid float32 [D], step float32: the float sequence of the reference's constructor (SteeringBeamforming.cpp:39-40,
    doaIdx2angle of microhponeArrayHelpers.cpp:117-120)"""
    step = np.float32(step_deg * np.pi / 180.0)
    D = int(np.round(np.pi / float(step)) + 1)
    pr = np.arange(D, dtype=np.float32) * step
    return (pr.astype(np.float64) - np.pi / 2).astype(np.float32), step
