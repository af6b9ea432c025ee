"""float64 twin of the XYZ geometry of an MVDR context (include/mcarray_hip.h, mca_hip_mvdr_set_geometry).

steering_xyz(): d_m = exp(+j 2 pi k fs (r_m . e) / (N c)), e(theta, eps) = (sin theta cos eps, cos theta cos eps, sin eps), with the x
term spelled as mvdr_nulls_twin.steering spells it and a coordinate that is 0 adding no term, so that an array on the x axis with
eps = 0 is array_equal to it.  grid_xyz(), peaks_circular(), peak_margin_circular(): the periodic grid and the peak rule on the circle.
reduce32(), wrap32(), associate_circular(), window_argmax_circular(), seed_circular(): the float32 half of the tracks, operation by
operation as the header writes it down.

Every other twin of the module (mvdr_nulls_twin, mvdr_mask_twin, mvdr_rtf_twin, mvdr_estmask_twin, mvdr_rtf_nulls_twin,
mvdr_spectrum_twin, mvdr_tracks_twin) reaches its steering vectors through mvdr_nulls_twin.steering and its grid through
mvdr_spectrum_twin.grid / mvdr_tracks_twin.grid64: xyz_mode(elevation) exchanges those (and the peak rule and the association) for
the time of a with block, and the twins then take `xs` as [M][3] positions.  No twin is edited."""
import contextlib

import numpy as np

from mcarray_amd import synth
from oracle import np_twin

import mvdr_nulls_twin as nt
import mvdr_spectrum_twin as sp
import mvdr_tracks_twin as tt

F32 = np.float32
PI_F, TWO_PI_F, INV_TWO_PI_F = F32(3.14159274), F32(6.28318548), F32(0.159154937)


def _xyz(xs):
    r = np.asarray(xs, dtype=np.float64)
    if r.ndim == 1:
        r = np.stack([r, np.zeros_like(r), np.zeros_like(r)], axis=1)
    return r


def steering_xyz(fs, N, xyz, doa, elevation=0.0):
    """doa [S] azimuths -> d [K][S][M]"""
    r = _xyz(xyz)
    k = np.arange(N // 2 + 1, dtype=np.float64)
    th = np.asarray(doa, dtype=np.float64)
    ce, se = np.cos(elevation), np.sin(elevation)
    base = 2 * np.pi * fs / N / np_twin.C_SOUND
    slope = base * r[None, :, 0] * (np.cos(th[:, None] + np.pi / 2) * ce)
    ny, nz = r[:, 1] != 0.0, r[:, 2] != 0.0
    slope[:, ny] += base * r[None, ny, 1] * (-np.cos(th[:, None]) * ce)
    slope[:, nz] -= base * r[None, nz, 2] * se
    return np.exp(-1j * k[:, None, None] * slope[None, :, :])


def grid_xyz(D):
    """theta_i = -pi + i 2 pi / D in double; the device reports (float) theta_i"""
    return -np.pi + np.arange(D, dtype=np.float64) * (2 * np.pi) / D


def local_maxima(P, circular=True):
    D = len(P)
    if circular:
        return [i for i in range(D) if P[i] > 0 and P[i] > P[(i - 1) % D] and P[i] >= P[(i + 1) % D]]
    return [i for i in range(D) if P[i] > 0 and (i == 0 or P[i] > P[i - 1]) and (i == D - 1 or P[i] >= P[i + 1])]


def peaks_circular(P, n_peaks, circular=True):
    """the peak rule on the circle -> (index [n_peaks] (-1: empty slot), peak_doa [n_peaks] float32, peak_val [n_peaks]).  circular=False:
    the rule that does not wrap, on the same periodic grid (what the seam scenes tell apart)"""
    th = grid_xyz(len(P)).astype(F32)
    found = local_maxima(P, circular)
    found.sort(key=lambda i: (-P[i], i))
    idx = np.full(n_peaks, -1, dtype=np.int64)
    doa = np.zeros(n_peaks, dtype=F32)
    val = np.zeros(n_peaks)
    for r in range(n_peaks):
        if r < len(found):
            idx[r], doa[r], val[r] = found[r], th[found[r]], P[found[r]]
        elif found:
            doa[r] = th[found[0]]
    return idx, doa, val


def peak_margin_circular(P, idx):
    """mvdr_spectrum_twin.peak_margin with the neighbours taken round the seam: the least of a compared peak above each of its two
    circular neighbours and above the next-ranked local maximum, of the row's maximum.  idx: the slots of peaks_circular(P, n + 1)."""
    D, top, m = len(P), P.max(), np.inf
    for r, i in enumerate(idx[:-1]):
        if i < 0:
            continue
        m = min(m, P[i] - P[(i - 1) % D], P[i] - P[(i + 1) % D])
        nxt = idx[r + 1]
        m = min(m, P[i] - (P[nxt] if nxt >= 0 else 0.0))
    return m / top


# ---- the tracks on the circle, float32 ----
_ASSOCIATE_LINEAR, _SEED_LINEAR = tt.associate, tt.seed            # as mvdr_tracks_twin has them, whatever xyz_mode() exchanges


def wrap32(d):
    """the shorter way round of a difference of two reduced angles: one rounded addition"""
    d = F32(d)
    if d > PI_F:
        return F32(d - TWO_PI_F)
    if d < -PI_F:
        return F32(d + TWO_PI_F)
    return d


def reduce32(v):
    """a finite float32 angle into [-pi_f, pi_f]: clamp(wrap(fmaf(-two_pi_f, rintf(v * inv_f), v))); anything else stays"""
    v = F32(v)
    if not np.isfinite(v):
        return v
    n = np.rint(F32(v * INV_TWO_PI_F))
    r = F32(np.float64(v) - np.float64(TWO_PI_F) * np.float64(n))          # the fused multiply-add: the product is exact in double
    return min(max(wrap32(r), F32(-PI_F)), PI_F)


def seed_circular(st, doa):
    return _SEED_LINEAR(st, [reduce32(v) for v in np.asarray(doa, dtype=F32)])


def associate_circular(st, own_doa, cand_doa, cand_val, n_tracks, n_own, max_step_rad, min_sep_rad, hold, circular=True):
    """mvdr_tracks_twin.associate on the circle (circular=False: its very arithmetic, for the tests that show what the wrap changes)"""
    if not circular:
        return _ASSOCIATE_LINEAR(st, own_doa, cand_doa, cand_val, n_tracks, n_own, max_step_rad, min_sep_rad, hold)
    theta, alive, miss, gen = st["theta"], st["alive"], st["miss"], st["gen"]
    ms, sep = F32(max_step_rad), F32(min_sep_rad)
    own_doa = np.full(n_own, np.nan, dtype=F32) if own_doa is None else np.asarray(own_doa, dtype=F32)
    cand_doa, cand_val = np.asarray(cand_doa, dtype=F32), np.asarray(cand_val, dtype=F32)
    with np.errstate(invalid="ignore"):
        for s in range(n_own):                                             # 1. own slots
            if not alive[s]:
                continue
            o = reduce32(own_doa[s])
            if np.isfinite(o):
                dl = wrap32(F32(o - theta[s]))
                theta[s] = wrap32(F32(theta[s] + min(max(dl, F32(-ms)), ms)))
                miss[s] = 0
            else:
                miss[s] += 1
        matched, births = set(), []
        for c in range(min(len(cand_doa), tt.MAX_CAND)):                   # 2. candidates in the order given
            psi = reduce32(cand_doa[c])
            if not (cand_val[c] > 0) or not np.isfinite(psi):
                continue
            if any(alive[s] and abs(wrap32(F32(psi - theta[s]))) <= sep for s in range(n_own)):
                continue
            best, bd = -1, F32(0)
            for s in range(n_own, n_tracks):
                if not alive[s] or s in matched:
                    continue
                ds = abs(wrap32(F32(psi - theta[s])))
                if ds <= ms and (best < 0 or ds < bd):
                    best, bd = s, ds
            if best >= 0:
                theta[best], miss[best] = psi, 0
                matched.add(best)
            else:
                births.append(psi)
        for s in range(n_own, n_tracks):                                   # 3. unmatched alive interferer slots
            if alive[s] and s not in matched:
                miss[s] += 1
                if miss[s] > hold:
                    alive[s] = 0
        born = []
        for psi in births:                                                 # 4. births in candidate order
            free = [s for s in range(n_own, n_tracks) if not alive[s]]
            if not free:
                break
            f = free[0]
            theta[f], alive[f], miss[f] = psi, 1, 0
            gen[f] += 1
            born.append(f)
    return born


def window_argmax_circular(T, grid32, theta, max_step_rad):
    """mvdr_tracks_twin.window_argmax with the window taken the shorter way round"""
    T, grid32 = np.asarray(T, dtype=F32), np.asarray(grid32, dtype=F32)
    bv, bi = F32(0), -1
    for i in range(len(grid32)):
        if abs(wrap32(F32(grid32[i] - F32(theta)))) <= F32(max_step_rad) and T[i] > bv:
            bv, bi = T[i], i
    return (grid32[bi] if bi >= 0 else F32(np.nan)), bi




@contextlib.contextmanager
def xyz_mode(elevation=0.0):
    """inside the block the module's twins compute in XYZ geometry at this elevation; `xs` of their calls is [M][3]"""
    saved = (nt.steering, sp.grid, sp.peaks, sp.peak_margin, tt.grid64, tt.associate, tt.window_argmax, tt.seed)
    nt.steering = lambda fs, N, xs, doa: steering_xyz(fs, N, xs, doa, elevation)
    sp.grid, sp.peaks, sp.peak_margin = grid_xyz, peaks_circular, peak_margin_circular
    tt.grid64, tt.associate, tt.window_argmax, tt.seed = grid_xyz, associate_circular, window_argmax_circular, seed_circular
    try:
        yield
    finally:
        nt.steering, sp.grid, sp.peaks, sp.peak_margin, tt.grid64, tt.associate, tt.window_argmax, tt.seed = saved


# ---- scenes ----
SCENE_FS, SCENE_N, SCENE_F, SCENE_D, SCENE_BAND, SCENE_PEAKS = 16000, 256, 12, 72, (1, 127), 3


def scene_xyz():
    return synth.uca(6, 0.045)


def two_sources_xyz(xyz, fs, N, F, az0, az1, seed=0, elevation=0.0):
    """mvdr_spectrum_twin.two_sources for azimuths (radians) round an array at xyz"""
    n = (F + 1) * N // 2
    return (synth.noise_source_stream_xyz(xyz, az0, fs, n, 5 + seed, elevation=elevation)
            + synth.noise_source_stream_xyz(xyz, az1, fs, n, 15 + seed, snr_db=60, elevation=elevation)).astype(np.float32)


# name -> (azimuths of the two talkers, seed).  The seam scenes put the first talker on the grid point next to the seam (index D - 1, and
# again index 0) and the second on index 24; "back" has both talkers off the grid, one of them behind the array.  The seeds are the
# first of 0 ... 5 whose three compared peaks clear the margin tests/test_mvdr_geometry_twin.py asserts (seam_first: 2.3e-3 with seed 0,
# 5.5e-3 with seed 2; back: 5.8e-3 and 6.9e-3 with seeds 0 and 1 -- the larger is taken)
def named_azimuths():
    g = grid_xyz(SCENE_D)
    return {"seam_last": ((g[SCENE_D - 1], g[24]), 0), "seam_first": ((g[0], g[24]), 2), "back": ((2.5, -0.6), 1)}


_scene_cache = {}


def named_scene(name):
    """dict(xyz, pcm float32 [M][(F+1) hop], az, phi complex [K][M][M] (the twin's covariance after the F frames), P float64 [D]);
    computed once"""
    if name not in _scene_cache:
        az, seed = named_azimuths()[name]
        xyz = scene_xyz()
        pcm = two_sources_xyz(xyz, SCENE_FS, SCENE_N, SCENE_F, az[0], az[1], seed)
        with xyz_mode():
            run = nt.mvdr_nulls_stream(SCENE_FS, SCENE_N, xyz, pcm.astype(np.float64), np.zeros((SCENE_F, 1)), 0.0)
            P = sp.spectrum(run["phi"], SCENE_FS, SCENE_N, xyz, SCENE_D, SCENE_BAND[0], SCENE_BAND[1], sp.NORMALISED)
        _scene_cache[name] = dict(xyz=xyz, pcm=pcm, az=az, phi=run["phi"], P=P, run=run)
    return _scene_cache[name]


def drifting_azimuths(A, F, S):
    """[A][F][S] float32 look directions that drift per frame, differ per source and stream, cover the whole circle and leave
    [-pi, pi] on both sides"""
    base = np.array([2.9, -3.4, 0.7, 4.6])[:S]
    return (base[None, None, :] + 0.05 * np.arange(F)[None, :, None] - 1.9 * np.arange(A)[:, None, None]).astype(np.float32)


def array_3d(M=7, seed=2):
    """an array with z != 0: points in a 10 cm cube"""
    return np.random.default_rng(seed).uniform(-0.05, 0.05, (M, 3))
