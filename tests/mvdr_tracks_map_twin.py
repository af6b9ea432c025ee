"""Twin of the map mode of the tracks of an MVDR context (include/mcarray_hip.h, mca_hip_mvdr_tracks_set_map).

own_map(): the steered map an own track follows, in float64, on top of mvdr_rtf_twin.estimate(), mvdr_geometry_twin.steering_xyz()
and mvdr_map_twin.steering_map():

    d_k, est_k  the estimator on (Psi_s, cpsi_s, Phi, cphi) at g0 = the XYZ geometric vector of (theta_s, eps_s)
    used_k      est_k and tr(Phi_k) > 1e-30 and k in the band
    u_k         d_k / |d_k|
    T[j][i]     sum over the used k of |d(theta_i, eps_j, k)^H u_k|^2 / M

own_map_dense() is the same definition written cell by cell.  window_argmax_map(), associate_map(), seed_map(), fill_map(): the
float32 half, restated operation by operation -- the kernel's lane does these very operations, so the GPU's theta, eps, alive, miss
and gen are compared with array_equal."""
import numpy as np

import mvdr_geometry_twin as gt
import mvdr_map_twin as mp
import mvdr_rtf_twin as rt
import mvdr_tracks_twin as tt

F32 = np.float32
MAX_SLOTS, MAX_CAND = tt.MAX_SLOTS, tt.MAX_CAND
HALF_PI_F = F32(1.57079637)


def clamp_el(v):
    """fminf(fmaxf(v, -pi/2_f), pi/2_f) of a finite float32"""
    return min(max(F32(v), F32(-HALF_PI_F)), HALF_PI_F)


def new_state(n_streams=None):
    st = tt.new_state(n_streams)
    st["eps"] = np.zeros_like(st["theta"])
    return st


def seed_map(st, az, el):
    """az, el [n_tracks]: a pair of finite values sets theta = reduce(az), eps = clamp(el), alive = 1, miss = 0, gen += 1; anything
    else leaves the slot"""
    for s, (v, w) in enumerate(zip(np.asarray(az, dtype=F32), np.asarray(el, dtype=F32))):
        if np.isfinite(v) and np.isfinite(w):
            st["theta"][s], st["eps"][s], st["alive"][s], st["miss"][s] = gt.reduce32(v), clamp_el(w), 1, 0
            st["gen"][s] += 1
    return st


def _step(x, lim):
    return min(max(F32(x), F32(-lim)), F32(lim))


def associate_map(st, own_az, own_el, cand_az, cand_el, cand_val, n_tracks, n_own, max_step_rad, min_sep_rad, hold, max_step_el_rad, min_sep_el_rad):
    """one stream, in place: st of new_state() (1-D arrays), own_az / own_el [n_own] (not finite: none), candidates in the order given.
    Returns the list of the slots born."""
    theta, eps, alive, miss, gen = st["theta"], st["eps"], st["alive"], st["miss"], st["gen"]
    ms, sep, mse, sepe = F32(max_step_rad), F32(min_sep_rad), F32(max_step_el_rad), F32(min_sep_el_rad)
    own_az = np.full(n_own, np.nan, dtype=F32) if own_az is None else np.asarray(own_az, dtype=F32)
    own_el = np.full(n_own, np.nan, dtype=F32) if own_el is None else np.asarray(own_el, dtype=F32)
    cand_az, cand_el, cand_val = (np.asarray(v, dtype=F32) for v in (cand_az, cand_el, cand_val))
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(n_own):                                             # 1. own slots
            if not alive[s]:
                continue
            oa, oe = gt.reduce32(own_az[s]), own_el[s]
            if np.isfinite(oa) and np.isfinite(oe):
                dl = gt.wrap32(F32(oa - theta[s]))
                theta[s] = gt.wrap32(F32(theta[s] + _step(dl, ms)))
                de = F32(clamp_el(oe) - eps[s])
                eps[s] = clamp_el(F32(eps[s] + _step(de, mse)))
                miss[s] = 0
            else:
                miss[s] += 1
        matched, births = set(), []
        for c in range(min(len(cand_az), MAX_CAND)):                       # 2. candidates in the order given
            psi = gt.reduce32(cand_az[c])
            if not (cand_val[c] > 0) or not np.isfinite(psi) or not np.isfinite(cand_el[c]):
                continue
            eta = clamp_el(cand_el[c])
            if any(alive[s] and abs(gt.wrap32(F32(psi - theta[s]))) <= sep and abs(F32(eta - eps[s])) <= sepe for s in range(n_own)):
                continue
            best, bd = -1, F32(0)
            for s in range(n_own, n_tracks):
                if not alive[s] or s in matched:
                    continue
                da, de = abs(gt.wrap32(F32(psi - theta[s]))), abs(F32(eta - eps[s]))
                ds = F32(da + de)
                if da <= ms and de <= mse and (best < 0 or ds < bd):
                    best, bd = s, ds
            if best >= 0:
                theta[best], eps[best], miss[best] = psi, eta, 0
                matched.add(best)
            else:
                births.append((psi, eta))
        for s in range(n_own, n_tracks):                                   # 3. unmatched alive interferer slots
            if alive[s] and s not in matched:
                miss[s] += 1
                if miss[s] > hold:
                    alive[s] = 0
        born = []
        for psi, eta in births:                                            # 4. births in candidate order
            free = [s for s in range(n_own, n_tracks) if not alive[s]]
            if not free:
                break
            f = free[0]
            theta[f], eps[f], alive[f], miss[f] = psi, eta, 1, 0
            gen[f] += 1
            born.append(f)
    return born


def fill_map(st, n_tracks):
    """(doa [n_tracks] float32, el [n_tracks] float32): (theta, eps) of the alive slots; a dead slot reports the lowest alive slot's; a
    stream without an alive slot 0 rad and NaN (unset: the context's elevation).  el is what get_elevations reports: the float of the
    angle clamped to +-pi/2 in double"""
    live = [s for s in range(n_tracks) if st["alive"][s]]
    doa = np.array([st["theta"][s] if st["alive"][s] else (st["theta"][live[0]] if live else F32(0)) for s in range(n_tracks)], dtype=F32)
    el = np.array([st["eps"][s] if st["alive"][s] else (st["eps"][live[0]] if live else F32(np.nan)) for s in range(n_tracks)], dtype=F32)
    return doa, np.clip(el.astype(np.float64), -np.pi / 2, np.pi / 2).astype(F32)


def in_window(az32, el32, theta, eps, max_step_rad, max_step_el_rad):
    """bool [n_el][n_az]: the cells with |wrap(theta_i - theta)| <= max_step and |eps_j - eps| <= max_step_el, compared in float32"""
    wa = np.array([abs(gt.wrap32(F32(g - F32(theta)))) <= F32(max_step_rad) for g in np.asarray(az32, dtype=F32)])
    we = np.abs((np.asarray(el32, dtype=F32) - F32(eps)).astype(F32)) <= F32(max_step_el_rad)
    return we[:, None] & wa[None, :]


def window_argmax_map(T, az32, el32, theta, eps, max_step_rad, max_step_el_rad):
    """float32 T [n_el][n_az] -> (az, el of the cell that maximises T in the window (float32; NaN, NaN if none or not > 0), its flat
    index or -1); the lower flat index wins ties"""
    T = np.asarray(T, dtype=F32)
    win = in_window(az32, el32, theta, eps, max_step_rad, max_step_el_rad)
    bv, bi = F32(0), -1
    for c in np.flatnonzero(win.reshape(-1)):
        if T.reshape(-1)[c] > bv:
            bv, bi = T.reshape(-1)[c], int(c)
    if bi < 0:
        return F32(np.nan), F32(np.nan), -1
    n_az = T.shape[1]
    return F32(az32[bi % n_az]), F32(el32[bi // n_az]), bi


def clear_margin_map(T, az32, el32, theta, eps, max_step_rad, max_step_el_rad):
    """mvdr_tracks_twin.clear_margin on the map: how far the window maximum stands clear of the next cell of the window, as a share of
    the map's maximum (0 for an empty window)"""
    T = np.asarray(T, dtype=np.float64)
    v = np.sort(T[in_window(az32, el32, theta, eps, max_step_rad, max_step_el_rad)])[::-1]
    if len(v) == 0 or not T.max() > 0:
        return 0.0
    return float((v[0] - (v[1] if len(v) > 1 else 0.0)) / T.max())


def _vectors(fs, N, xyz, bin_lo, bin_hi, psi, cpsi, phi, cphi, theta, eps, iterations, ref_mic, min_share, used, est_dtype):
    """u [K][M] (zero where the bin is not used), own, edge, diag: the part of mvdr_tracks_twin.own_spectrum() ahead of the scan, at
    g0 = the XYZ geometric vector of ((float) theta, (float) eps)"""
    K = N // 2 + 1
    g0 = gt.steering_xyz(fs, N, xyz, [float(F32(theta))], float(F32(eps)))[:, 0]
    d, ok, diag = rt.estimate(psi, cpsi, phi, cphi, g0, iterations, ref_mic, min_share, dtype=est_dtype)
    d = d.astype(np.complex128)
    k = np.arange(K)
    band = (k >= bin_lo) & (k <= bin_hi)
    tr = np.real(np.trace(np.asarray(phi), axis1=1, axis2=2))
    own = ok & (tr > 1e-30) & band
    use = own if used is None else np.asarray(used, dtype=bool) & band
    forced = use & ~ok
    if forced.any():
        raw = tt._raw_estimate(np.asarray(psi, dtype=np.complex128), np.asarray(cpsi, dtype=np.float64), np.asarray(phi, dtype=np.complex128),
                               np.asarray(cphi, dtype=np.float64), g0, iterations, ref_mic)
        d[forced] = raw[forced]
    with np.errstate(all="ignore"):
        u = d / np.sqrt(np.sum(np.abs(d) ** 2, axis=1))[:, None]
    u[~use] = 0.0
    return u, own, rt.edge_cells(diag, min_share) & band, diag


def own_map(fs, N, xyz, n_az, els, bin_lo, bin_hi, psi, cpsi, phi, cphi, theta, eps, iterations=2, ref_mic=0, min_share=0.05, used=None,
            est_dtype=np.float64):
    """psi, phi complex [K][M][M], cpsi, cphi [K] of one stream and slot, (theta, eps) its direction, els the map's elevations in
    double -> dict(T float64 [n_el][n_az], used bool [K], edge bool [K], diag).  used: a [K] override of the flags, as
    mvdr_tracks_twin.own_spectrum() takes it."""
    M = np.asarray(phi).shape[1]
    u, own, edge, diag = _vectors(fs, N, xyz, bin_lo, bin_hi, psi, cpsi, phi, cphi, theta, eps, iterations, ref_mic, min_share, used, est_dtype)
    dg = mp.steering_map(fs, N, xyz, n_az, els)                            # [K][D][M]
    T = np.sum(np.abs(np.einsum("kdm,km->kd", np.conj(dg), u)) ** 2, axis=0) / M
    return dict(T=T.reshape(len(els), n_az), used=own, edge=edge, diag=diag)


def own_map_dense(fs, N, xyz, n_az, els, bin_lo, bin_hi, psi, cpsi, phi, cphi, theta, eps, **kw):
    """the definition cell by cell: T[j][i] = sum over the used k of |d(theta_i, eps_j, k)^H u_k|^2 / M"""
    M = np.asarray(phi).shape[1]
    u, own, _, _ = _vectors(fs, N, xyz, bin_lo, bin_hi, psi, cpsi, phi, cphi, theta, eps, kw.get("iterations", 2), kw.get("ref_mic", 0),
                            kw.get("min_share", 0.05), None, np.float64)
    az = gt.grid_xyz(n_az)
    T = np.zeros((len(els), n_az))
    for j, e in enumerate(els):
        for i in range(n_az):
            d = gt.steering_xyz(fs, N, xyz, az[i:i + 1], e)[:, 0]          # [K][M]
            for k in np.flatnonzero(own):
                T[j, i] += abs(np.vdot(d[k], u[k])) ** 2 / M
    return T


# ---- inputs of the tests: a covariance pair with a talker in it, without a frames twin ----
def synthetic_state(fs, N, xyz, az, el, seed=0, snr=4.0):
    """dict(phi, psi complex [K][M][M], cpsi, cphi [K]): Phi = a diffuse-like random Hermitian covariance, Psi = Phi + snr d d^H at the
    direction (az, el); what the estimator reads, in float64"""
    rng = np.random.default_rng(seed)
    M, K = len(xyz), N // 2 + 1
    B = rng.standard_normal((K, M, M)) + 1j * rng.standard_normal((K, M, M))
    phi = np.einsum("kij,klj->kil", B, np.conj(B)) / M + 0.5 * np.eye(M)
    d = gt.steering_xyz(fs, N, xyz, [az], el)[:, 0]
    psi = phi + snr * np.einsum("ki,kj->kij", d, np.conj(d))
    return dict(phi=phi, psi=psi, cpsi=np.ones(K), cphi=np.ones(K))


# ---- the parity inputs of tests/test_gpu_mvdr_tracks_map.py: two streams, two auto calls of 6 frames, two look directions (the first
# protected) at an elevation of their own each; then one update of the tracks seeded 3 degrees and one elevation step behind ----
FS, N = 16000, 256
PARITY_ARRAYS = {"cube4": ("3d", 4, 4), "cube7": ("3d", 7, 2), "cube16": ("3d", 16, 3), "uca8": ("uca", 8, 0.05)}   # Q = 1, 2, 4 and the ring
PARITY_MAPS = ((24, 5), (36, 5), (36, 7))                                  # 120, 180 and 252 directions: one partial tile, a tile and a block, two tiles
PARITY_EL = (0.0, np.deg2rad(60.0))
PARITY_BAND = (4, 124)                                                     # of K = 129: the last chunk is partial
PARITY_S, PARITY_F = 2, 6
PARITY_STEP = 0.3
PARITY_SEED_OFFSET = np.deg2rad(-3.0)
PARITY_TALKERS = ((0.6, np.deg2rad(30.0)), (-1.9, np.deg2rad(15.0)))     # (azimuth, elevation) of the two talkers
# array -> offset of the talkers' noise seeds.  Of the offsets 0, 20, 40 and 60 the one that leaves the fewest bins at a decision edge
# of the estimator on the twin alone (1 ... 3 of a map's 484 cells; with offset 0 the ring has 5, above the 1 % cap)
PARITY_NOISE_SEED = {"cube4": 60, "cube7": 20, "cube16": 40, "uca8": 20}


def parity_xyz(name):
    kind, M, p = PARITY_ARRAYS[name]
    from mcarray_amd import synth
    return gt.array_3d(M, p) if kind == "3d" else np.asarray(synth.uca(M, p))


def parity_inputs(name, A=2):
    """dict(xyz, pcm float32 [A][M][(2F+1) hop], doa float32 [A][2F][S], el float32 [A][S]): two noise talkers at PARITY_TALKERS, the
    streams differ in the noise seeds and in a small offset of the look directions"""
    from mcarray_amd import synth
    xyz = parity_xyz(name)
    n = (2 * PARITY_F + 1) * N // 2
    pcm, doa, el = [], [], []
    for a in range(A):
        (a0, e0), (a1, e1) = PARITY_TALKERS
        pcm.append((synth.noise_source_stream_xyz(xyz, a0, FS, n, 5 + a + PARITY_NOISE_SEED.get(name, 0), elevation=e0)
                    + synth.noise_source_stream_xyz(xyz, a1, FS, n, 15 + a + PARITY_NOISE_SEED.get(name, 0), elevation=e1)).astype(np.float32))
        doa.append(np.tile(np.float32([a0 + 0.02 * a, a1 - 0.03 * a]), (2 * PARITY_F, 1)))
        el.append(np.float32([e0, e1]))
    return dict(xyz=xyz, pcm=np.stack(pcm), doa=np.stack(doa).astype(np.float32), el=np.stack(el).astype(np.float32))


def parity_rtf(name):
    return rt.parity_config(PARITY_ARRAYS[name][1])


def parity_estmask():
    import mvdr_estmask_twin as et
    return et.parity_config(N, PARITY_S, 1)


_STATE = {}


def parity_state(name):
    """[stream] -> the twin's state (phi, psi [S], cpsi [S], cphi) after the two auto calls with look direction s at el[s], float64;
    computed once per array"""
    import mvdr_estmask_twin as et
    if name not in _STATE:
        inp = parity_inputs(name)
        hop, F = N // 2, PARITY_F
        out = []
        for a in range(inp["pcm"].shape[0]):
            st = None
            with mp.slot_elevations(inp["el"][a].astype(np.float64)):
                for t0, t1 in ((0, F), (F, 2 * F)):
                    st = et.auto_stream(FS, N, inp["xyz"], inp["pcm"][a, :, t0 * hop:(t1 + 1) * hop].astype(np.float64), inp["doa"][a, t0:t1],
                                        parity_estmask(), rtf=dict(parity_rtf(name)), state=st)
            out.append(st)
        _STATE[name] = out
    return _STATE[name]


def parity_seeds(inp, el_step):
    """(az [A][S], el [A][S]) float32: 3 degrees and one elevation step behind the look directions"""
    return (inp["doa"][:, -1, :] + F32(PARITY_SEED_OFFSET)).astype(F32), (inp["el"] - F32(el_step)).astype(F32)


# ---- the scene: mvdr_geometry_twin.array_3d(7) with the gain and position errors of mvdr_rtf_twin.rtf_scene(); the protected talker
# walks from (20, 10) to (35, 40) degrees over the chunks, the interferer stays at (-40, 0).  The loop is the auto call with
# n_protected = 1 at the directions and elevations the tracks fill in, the tracks updated per chunk from a 72 x 7 map ----
SCENE_CHUNKS, SCENE_CF = 8, 12
SCENE_TRUTH_AZ = np.deg2rad(np.linspace(20.0, 35.0, SCENE_CHUNKS))
SCENE_TRUTH_EL = np.deg2rad(np.linspace(10.0, 40.0, SCENE_CHUNKS))
SCENE_ITF = (np.deg2rad(-40.0), 0.0)
SCENE_MAP = dict(n_az=72, n_el=7, el_lo=0.0, el_hi=np.deg2rad(60.0))     # steps of 5 and 10 degrees
SCENE_BAND = (4, 124)
# the gates are one grid step in either angle, a hundredth over: a difference of two float32 grid values may round above the step
SCENE_TRACKS = dict(n_tracks=2, n_own=1, max_step_rad=1.01 * np.deg2rad(5.0), min_sep_rad=np.deg2rad(8.0), hold=3,
                    max_step_el_rad=1.01 * np.deg2rad(10.0), min_sep_el_rad=1.01 * np.deg2rad(10.0))


def moving_scene(seed=1):
    """dict(xyz, target, interferer (float64 [M][(F+1) hop], as the perturbed array records them), pcm float32):
    mvdr_tracks_twin.moving_scene() on the 3-D array, the target's direction stepping per chunk in both angles"""
    from mcarray_amd import synth
    from oracle import np_twin
    fs, n_fft, F = rt.SCENE_FS, rt.SCENE_N, SCENE_CHUNKS * SCENE_CF
    xyz = gt.array_3d(7)
    M, hop, K = len(xyz), n_fft // 2, n_fft // 2 + 1
    n = (F + 1) * hop
    rng = np.random.default_rng(seed)
    xp = xyz + 0.008 * rng.standard_normal((M, 3))
    gain = 10.0 ** (rng.uniform(-2.0, 2.0, M) / 20.0)
    itf = gain[:, None] * synth.noise_source_stream_xyz(xp, SCENE_ITF[0], fs, n, 3, elevation=SCENE_ITF[1]).astype(np.float64)
    src = np.zeros((M, n))
    for c in range(SCENE_CHUNKS):
        a, b = c * SCENE_CF * hop, ((c + 1) * SCENE_CF * hop if c < SCENE_CHUNKS - 1 else n)
        src[:, a:b] = gain[:, None] * synth.noise_source_stream_xyz(xp, SCENE_TRUTH_AZ[c], fs, n, 4, sigma=0.1 * 10.0 ** 0.5,
                                                                    elevation=SCENE_TRUTH_EL[c]).astype(np.float64)[:, a:b]
    rng = np.random.default_rng(7)
    pat = np.zeros((F, K))
    for tb in range(0, F, 4):
        for kb in range(0, K, 16):
            if rng.random() < 0.5:
                pat[tb:tb + 4, kb:kb + 16] = 1.0
    T = np_twin.stft_frames(src, n_fft) * pat[:, None, :]
    tgt = np.zeros_like(src)
    for t in range(F):
        tgt[:, t * hop:t * hop + n_fft] += np_twin.irfft_ccs(T[t], n_fft)
    return dict(xyz=xyz, interferer=itf, target=tgt, pcm=(itf + tgt).astype(np.float32))


def scene_grid():
    """(n_az, the map's elevations in double)"""
    m = SCENE_MAP
    return m["n_az"], mp.grid_el(m["n_el"], m["el_lo"], m["el_hi"])


def scene_update(st, trk, xyz, rtf):
    """one update of the tracks on the state st of the auto twin -> the own target found ((NaN, NaN): none)"""
    fs, n_fft = rt.SCENE_FS, rt.SCENE_N
    n_az, els = scene_grid()
    az32, el32 = gt.grid_xyz(n_az).astype(F32), els.astype(F32)
    r = own_map(fs, n_fft, xyz, n_az, els, SCENE_BAND[0], SCENE_BAND[1], st["psi"][0], st["cpsi"][0], st["phi"], st["cphi"], trk["theta"][0], trk["eps"][0], **rtf)
    if trk["alive"][0]:
        paz, pel, _ = window_argmax_map(r["T"], az32, el32, trk["theta"][0], trk["eps"][0], SCENE_TRACKS["max_step_rad"], SCENE_TRACKS["max_step_el_rad"])
    else:
        paz, pel = F32(np.nan), F32(np.nan)
    P = mp.capon_map(st["phi"], fs, n_fft, xyz, n_az, els, SCENE_BAND[0], SCENE_BAND[1], mp.NORMALISED)
    _, pa, pe, pv = mp.peaks(P, 2, els)
    associate_map(trk, [paz], [pel], pa, pe, pv, **SCENE_TRACKS)
    return paz, pel


def scene_loop(sc, tracked):
    """the loop over the chunks -> dict(theta, eps [chunks]: the own track after every chunk (the held seed when not tracked), err_az_deg,
    err_el_deg [chunks] against the truth, share: the target kept over the last chunk, run: the last chunk's run)"""
    import mvdr_estmask_twin as et
    fs, n_fft, hop = rt.SCENE_FS, rt.SCENE_N, rt.SCENE_N // 2
    seeds = ([SCENE_TRUTH_AZ[0], SCENE_ITF[0]], [SCENE_TRUTH_EL[0], SCENE_ITF[1]])
    trk = seed_map(new_state(), *seeds)
    held = fill_map(trk, 2)
    pcm = sc["pcm"].astype(np.float64)
    st, thetas, epss = None, [], []
    for c in range(SCENE_CHUNKS):
        doa, el = fill_map(trk, 2) if tracked else held
        f0, f1 = c * SCENE_CF, (c + 1) * SCENE_CF
        with mp.slot_elevations(el.astype(np.float64)):
            st = et.auto_stream(fs, n_fft, sc["xyz"], pcm[:, f0 * hop:(f1 + 1) * hop], np.tile(doa.astype(np.float64), (SCENE_CF, 1)), et.SCENE_CFG,
                                rtf=et.SCENE_RTF, state=st, want_weights=True)
        last_rows = (doa, el)
        if tracked:
            scene_update(st, trk, sc["xyz"], et.SCENE_RTF)
        thetas.append(float(trk["theta"][0]) if tracked else float(held[0][0]))
        epss.append(float(trk["eps"][0]) if tracked else float(held[1][0]))
    thetas, epss = np.array(thetas), np.array(epss)
    share = tt.target_share(st["w"][:, 0], sc, (SCENE_CHUNKS - 1) * SCENE_CF, SCENE_CHUNKS * SCENE_CF)
    return dict(theta=thetas, eps=epss, err_az_deg=np.rad2deg(np.abs(thetas - SCENE_TRUTH_AZ)), err_el_deg=np.rad2deg(np.abs(epss - SCENE_TRUTH_EL)),
                share=share, run=st, tracks=trk, last_rows=last_rows)


def scene_edge_cells(sc, loop):
    """bool [S][F][K]: the cells of the last chunk at a decision edge of the RTF estimator or of the mask estimator (the module's
    rule: where float32 and float64 may decide differently), on the twin alone; loop: what scene_loop() returned"""
    import mvdr_estmask_twin as et
    fs, n_fft, hop = rt.SCENE_FS, rt.SCENE_N, rt.SCENE_N // 2
    f0, f1 = (SCENE_CHUNKS - 1) * SCENE_CF, SCENE_CHUNKS * SCENE_CF
    doa, el = loop["last_rows"]
    with mp.slot_elevations(el.astype(np.float64)):
        m32 = et.masks(fs, n_fft, sc["xyz"], sc["pcm"][:, f0 * hop:(f1 + 1) * hop], np.tile(doa.astype(np.float64), (SCENE_CF, 1)), dtype=np.float32, **et.SCENE_CFG)
    return np.swapaxes(rt.edges_of(loop["run"]), 0, 1) | et.edge_cells(loop["run"]["masks"], m32)[1][None]


_scene_cache = {}


def scene_runs():
    """dict(sc, tracked, held): moving_scene() and both loops of scene_loop(); computed once"""
    if not _scene_cache:
        sc = moving_scene()
        _scene_cache.update(sc=sc, tracked=scene_loop(sc, True), held=scene_loop(sc, False))
    return _scene_cache


# the twin's figures on the scene (tests/test_mvdr_tracks_map_twin.py recomputes them): the own track's worst azimuth and elevation
# errors against the truth over the chunks (degrees) and the target kept over the last chunk, tracked and held at the seed.  The
# track lags the talker as in DESIGN.md 4.11 (Psi's memory of 20 frames against chunks of 12), and in elevation a 10 cm cube resolves
# little: the track sits a row above the talker at first and climbs a row every few chunks.  The scene's seed is the first of 1 ... 6
# with which at most 1 % of the last chunk's cells sit at a decision edge of either estimator on the twin alone (0.78 %; with seed 3,
# that of mvdr_tracks_twin.moving_scene(), 1.10 %), which is what tests/test_gpu_mvdr_tracks_map.py compares outside of.
SCENE_TWIN = dict(tracked=(5.0, 10.0, 0.742), held=(15.0, 30.0, 0.438))
