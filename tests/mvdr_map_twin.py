"""float64 twin of the azimuth x elevation Capon map of an MVDR context (include/mcarray_hip.h, mca_hip_mvdr_map_*).

The DENSE definition on top of mvdr_geometry_twin.steering_xyz and the band rule of mvdr_spectrum_twin: per stream, with Phi[k] the
covariance a frames twin returns and tr[k] its trace,

    theta_i = -pi + i 2 pi / n_az,   eps_j = el_lo + j (el_hi - el_lo)/(n_el - 1),   d = steering_xyz(theta_i, eps_j)
    P[j][i] = sum over k in [bin_lo, bin_hi] with tr[k] > 1e-30 of w[k] / (d^H PhiL[k]^-1 d),   PhiL[k] = Phi[k] + loading tr[k]/M I

through numpy.linalg.solve.  cholesky_route() is the form the kernel uses, in float64; peaks() the peak rule on the grid (8
neighbours, periodic in azimuth); peak_margin() what a compared peak stands above its neighbours and the next-ranked maximum;
scene() the scenes tests/test_gpu_mvdr_map.py compares.  slot_elevations() is the per-slot-elevation variant of the frames twins
(mca_hip_mvdr_set_elevations_*): mvdr_geometry_twin.xyz_mode() with an elevation per look direction."""
import contextlib

import numpy as np

from mcarray_amd import synth

import mvdr_geometry_twin as gt
import mvdr_nulls_twin as nt
import mvdr_spectrum_twin as sp

POWER, NORMALISED = sp.POWER, sp.NORMALISED


def grid_el(n_el, el_lo, el_hi):
    """eps_j in double; the device reports (float) eps_j"""
    step = (el_hi - el_lo) / (n_el - 1) if n_el > 1 else 0.0
    return el_lo + np.arange(n_el, dtype=np.float64) * step


def steering_map(fs, N, xyz, n_az, els):
    """d [K][n_el n_az][M] over the flat list of directions j n_az + i"""
    az = gt.grid_xyz(n_az)
    return np.concatenate([gt.steering_xyz(fs, N, xyz, az, e) for e in els], axis=1)


def capon_map(phi, fs, N, xyz, n_az, els, bin_lo, bin_hi, weighting, loading=1e-3):
    """phi [K][M][M] -> P [n_el][n_az] by the dense definition"""
    ks, tr, M = sp._band(phi, bin_lo, bin_hi)
    P = np.zeros((len(els), n_az))
    if len(ks) == 0:
        return P
    d = steering_map(fs, N, xyz, n_az, els)[ks]                            # [k][D][M]
    PL = phi[ks] + (loading * tr[ks] / M)[:, None, None] * np.eye(M)
    g = np.linalg.solve(PL, np.swapaxes(d, 1, 2))                          # PhiL^-1 d: [k][M][D]
    q = np.real(np.einsum("kdm,kmd->kd", np.conj(d), g))
    w = np.ones(len(ks)) if weighting == POWER else M / tr[ks]
    return (w[:, None] / q).sum(axis=0).reshape(len(els), n_az)


def cholesky_route(phi, fs, N, xyz, n_az, els, bin_lo, bin_hi, weighting, loading=1e-3):
    """the kernel's form in float64: PhiL / (tr/M) = L L^H, q' = ||L^-1 d||^2 = q tr/M, w' = 1 (NORMALISED) or tr/M (POWER)"""
    ks, tr, M = sp._band(phi, bin_lo, bin_hi)
    P = np.zeros((len(els), n_az))
    if len(ks) == 0:
        return P
    d = steering_map(fs, N, xyz, n_az, els)[ks]
    L = np.linalg.cholesky(phi[ks] * (M / tr[ks])[:, None, None] + loading * np.eye(M))
    u = np.linalg.solve(L, np.swapaxes(d, 1, 2))
    q = (np.abs(u) ** 2).sum(axis=1)
    w = tr[ks] / M if weighting == POWER else np.ones(len(ks))
    return (w[:, None] / q).sum(axis=0).reshape(len(els), n_az)


def neighbours(j, i, n_el, n_az):
    """the 8-neighbourhood of (j, i), periodic in azimuth, none beyond the first and last row -> (before, behind): the cells (j, i)
    must be strictly greater than, and those it must be >="""
    im, ip = (i - 1) % n_az, (i + 1) % n_az
    before, behind = [(j, im)], [(j, ip)]
    if j > 0:
        before += [(j - 1, im), (j - 1, i), (j - 1, ip)]
    if j < n_el - 1:
        behind += [(j + 1, im), (j + 1, i), (j + 1, ip)]
    return before, behind


def local_maxima(P):
    n_el, n_az = P.shape
    out = []
    for j in range(n_el):
        for i in range(n_az):
            before, behind = neighbours(j, i, n_el, n_az)
            if P[j, i] > 0 and all(P[j, i] > P[c] for c in before) and all(P[j, i] >= P[c] for c in behind):
                out.append(j * n_az + i)
    return out


def peaks(P, n_peaks, els, ctx_el=0.0):
    """the peak rule -> (flat index [n_peaks] (-1: empty slot), peak_az [n_peaks] float32, peak_el [n_peaks] float32, peak_val [n_peaks])"""
    n_el, n_az = P.shape
    az32, el32 = gt.grid_xyz(n_az).astype(np.float32), np.asarray(els, dtype=np.float64).astype(np.float32)
    flat = P.reshape(-1)
    found = local_maxima(P)
    found.sort(key=lambda c: (-flat[c], c))
    idx = np.full(n_peaks, -1, dtype=np.int64)
    paz = np.zeros(n_peaks, dtype=np.float32)
    pel = np.full(n_peaks, np.float32(ctx_el), dtype=np.float32)
    val = np.zeros(n_peaks)
    for r in range(n_peaks):
        c = found[r] if r < len(found) else (found[0] if found else -1)
        if r < len(found):
            idx[r], val[r] = c, flat[c]
        if c >= 0:
            paz[r], pel[r] = az32[c % n_az], el32[c // n_az]
    return idx, paz, pel, val


def peak_margin(P, idx):
    """the least of: a compared peak above each of its 8 neighbours, and above the next-ranked local maximum -- of the map's maximum.
    idx: the slots of peaks(P, n + 1, ...) for n compared slots, so that the last compared slot has its successor."""
    n_el, n_az = P.shape
    flat, top, m = P.reshape(-1), P.max(), np.inf
    for r, c in enumerate(idx[:-1]):
        if c < 0:
            continue
        before, behind = neighbours(c // n_az, c % n_az, n_el, n_az)
        m = min([m] + [flat[c] - P[n] for n in before + behind])
        nxt = idx[r + 1]
        m = min(m, flat[c] - (flat[nxt] if nxt >= 0 else 0.0))
    return m / top


def steering_slots(fs, N, xyz, doa, els):
    """doa [S] azimuths, els [S] elevations -> d [K][S][M]: look direction s at its own elevation"""
    doa = np.asarray(doa, dtype=np.float64)
    if len(doa) > len(els):
        raise ValueError("more look directions than slot elevations")
    return np.concatenate([gt.steering_xyz(fs, N, xyz, doa[s:s + 1], els[s]) for s in range(len(doa))], axis=1)


@contextlib.contextmanager
def slot_elevations(els, elevation=0.0):
    """mvdr_geometry_twin.xyz_mode(elevation) in which the frames twins (mvdr_nulls_twin, mvdr_mask_twin, mvdr_rtf_twin, ...) steer
    look direction s of a frame at els[s]; a NaN in els is the context's elevation.  Only the frames twins may run inside: the
    spectrum and the tracks keep the context's elevation, outside this block."""
    els = [elevation if np.isnan(e) else float(e) for e in np.asarray(els, dtype=np.float64)]
    with gt.xyz_mode(elevation):
        saved = nt.steering
        nt.steering = lambda fs, N, xs, doa: steering_slots(fs, N, xs, doa, els)
        try:
            yield
        finally:
            nt.steering = saved


# ---- scenes: two noise talkers on grid points of a 36 x 7 grid (elevations -30 ... 60 degrees in steps of 15), one next to the seam ----
FS, N, F, BAND = 16000, 256, 12, (1, 127)
N_AZ, N_EL, EL_LO, EL_HI = 36, 7, np.deg2rad(-30.0), np.deg2rad(60.0)
TALKERS = ((1, 5), (5, 35))                                                # (elevation row, azimuth column)
# name -> the array (mvdr_geometry_twin.array_3d).  A scene is (name, seed): the talkers' noise has seeds 5 + seed and 15 + seed.  The
# margins of the two compared peaks (tests/test_mvdr_map_twin.py asserts 5e-3 of the map's maximum), seeds 0 and 1: array_3d(7, 2) 1.4e-2
# and 5.7e-2 (seeds 2 and 3: 4e-4 and 2.1e-3, not used); array_3d(16, 3) 3.7e-2 and 4.5e-2 (seed 2: 6e-4); array_3d(4, 4) 3.7e-2 and
# 6.6e-2, with further local maxima at no more than 0.17 of the maximum, which no test compares
SCENES = {"cube7": (7, 2), "cube16": (16, 3), "cube4": (4, 4)}
SEEDS = (0, 1)
_cache = {}


def scene(name, seed=0):
    """dict(xyz, els, pcm float32 [M][(F+1) hop], phi (the twin's covariance after the F frames), P float64 [n_el][n_az]); once"""
    if (name, seed) not in _cache:
        M, aseed = SCENES[name]
        xyz = gt.array_3d(M, aseed)
        els, az = grid_el(N_EL, EL_LO, EL_HI), gt.grid_xyz(N_AZ)
        n = (F + 1) * N // 2
        (j0, i0), (j1, i1) = TALKERS
        pcm = (synth.noise_source_stream_xyz(xyz, az[i0], FS, n, 5 + seed, elevation=els[j0])
               + synth.noise_source_stream_xyz(xyz, az[i1], FS, n, 15 + seed, snr_db=60, elevation=els[j1])).astype(np.float32)
        with gt.xyz_mode():
            run = nt.mvdr_nulls_stream(FS, N, xyz, pcm.astype(np.float64), np.zeros((F, 1)), 0.0)
        P = capon_map(run["phi"], FS, N, xyz, N_AZ, els, BAND[0], BAND[1], NORMALISED)
        _cache[(name, seed)] = dict(xyz=xyz, els=els, pcm=pcm, phi=run["phi"], P=P)
    return _cache[(name, seed)]
