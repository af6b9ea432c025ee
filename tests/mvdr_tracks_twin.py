"""Twin of the tracks of the look directions of an MVDR context (include/mcarray_hip.h, mca_hip_mvdr_tracks_*).

own_spectrum(): the steered spectrum an own track follows, in float64, on top of mvdr_rtf_twin.estimate():

    d_k, est_k  the estimator on (Psi_s, cpsi_s, Phi, cphi) at g0 = the geometric vector of theta_s
    used_k      est_k and tr(Phi_k) > 1e-30 and k in the band
    u_k         d_k / |d_k|
    T[i]        sum over the used k of |d(theta_i, k)^H u_k|^2 / M

window_argmax() and associate(): the float32 half, restated operation by operation -- the kernel's lane does these very operations,
so the GPU's theta, alive, miss and gen are compared with array_equal.  fill(): the doa_rad row of the next chunk."""
import numpy as np

import mvdr_nulls_twin as nt
import mvdr_rtf_twin as rt

F32 = np.float32
MAX_SLOTS = 4
MAX_CAND = 8


def grid64(D):
    """theta_i = -pi/2 + i pi/(D-1) in double; the device reports (float) theta_i"""
    return -np.pi / 2 + np.arange(D, dtype=np.float64) * np.pi / (D - 1)


def new_state(n_streams=None):
    shape = (MAX_SLOTS,) if n_streams is None else (n_streams, MAX_SLOTS)
    return dict(theta=np.zeros(shape, dtype=F32), alive=np.zeros(shape, dtype=np.int32), miss=np.zeros(shape, dtype=np.int32),
                gen=np.zeros(shape, dtype=np.int32))


def seed(st, doa):
    """doa [n_tracks]: a finite value sets theta, alive = 1, miss = 0, gen += 1; anything else leaves the slot"""
    for s, v in enumerate(np.asarray(doa, dtype=F32)):
        if np.isfinite(v):
            st["theta"][s], st["alive"][s], st["miss"][s] = v, 1, 0
            st["gen"][s] += 1
    return st


def associate(st, own_doa, cand_doa, cand_val, n_tracks, n_own, max_step_rad, min_sep_rad, hold):
    """one stream, in place: st of new_state() (1-D arrays), own_doa [n_own] (NaN: none), candidates in the order given.  Returns the
    list of the slots born."""
    theta, alive, miss, gen = st["theta"], st["alive"], st["miss"], st["gen"]
    ms, sep = F32(max_step_rad), F32(min_sep_rad)
    own_doa = np.full(n_own, np.nan, dtype=F32) if own_doa is None else np.asarray(own_doa, dtype=F32)
    cand_doa, cand_val = np.asarray(cand_doa, dtype=F32), np.asarray(cand_val, dtype=F32)
    with np.errstate(invalid="ignore"):
        for s in range(n_own):                                             # 1. own slots
            if not alive[s]:
                continue
            o = own_doa[s]
            if np.isfinite(o):
                dl = F32(o - theta[s])
                theta[s] = F32(theta[s] + min(max(dl, F32(-ms)), ms))
                miss[s] = 0
            else:
                miss[s] += 1
        matched, births = set(), []
        for c in range(min(len(cand_doa), MAX_CAND)):                      # 2. candidates in the order given
            psi = cand_doa[c]
            if not (cand_val[c] > 0) or not np.isfinite(psi):
                continue
            if any(alive[s] and abs(F32(psi - theta[s])) <= sep for s in range(n_own)):
                continue
            best, bd = -1, F32(0)
            for s in range(n_own, n_tracks):
                if not alive[s] or s in matched:
                    continue
                ds = abs(F32(psi - theta[s]))
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


def fill(st, n_tracks):
    """[n_tracks] float32: theta of the alive slots; a dead slot reports the lowest alive slot's, or 0 rad"""
    live = [s for s in range(n_tracks) if st["alive"][s]]
    first = st["theta"][live[0]] if live else F32(0)
    return np.array([st["theta"][s] if st["alive"][s] else first for s in range(n_tracks)], dtype=F32)


def window_argmax(T, grid32, theta, max_step_rad):
    """float32 T [D], grid [D] and theta -> (the grid angle (float32) that maximises T within max_step of theta -- the lower index wins
    ties -- or NaN; its index or -1)"""
    T, grid32 = np.asarray(T, dtype=F32), np.asarray(grid32, dtype=F32)
    win = np.abs((grid32 - F32(theta)).astype(F32)) <= F32(max_step_rad)
    bv, bi = F32(0), -1
    for i in np.flatnonzero(win):
        if T[i] > bv:
            bv, bi = T[i], int(i)
    return (grid32[bi] if bi >= 0 else F32(np.nan)), bi


def clear_margin(T, grid32, theta, max_step_rad):
    """how far the window maximum of T stands clear of the next angle in the window, as a share of the row's maximum (0 for an empty
    window): the argmax is compared only where this is >= 5e-3, the rule of tests/test_gpu_mvdr_spectrum.py"""
    T = np.asarray(T, dtype=np.float64)
    win = np.abs((np.asarray(grid32, dtype=F32) - F32(theta)).astype(F32)) <= F32(max_step_rad)
    v = np.sort(T[win])[::-1]
    if len(v) == 0 or not T.max() > 0:
        return 0.0
    return float((v[0] - (v[1] if len(v) > 1 else 0.0)) / T.max())


def _raw_estimate(psi, cpsi, phi, cphi, g0, iterations, ref_mic):
    """the estimator's d without its fallback (for the bins a `used` override switches on), float64"""
    with np.errstate(all="ignore"):
        tau = np.real(np.trace(psi, axis1=1, axis2=2)) / cpsi
        sp = 1.0 / (cpsi * tau)
        sn = np.where(cphi > 0, 1.0 / (cphi * tau), 0.0)
        delta = psi * sp[:, None, None] - phi * sn[:, None, None]
        v = g0 / np.sqrt(g0.shape[1])
        for _ in range(iterations):
            g = np.einsum("kij,kj->ki", delta, v)
            v = g / np.sqrt(np.sum(np.abs(g) ** 2, axis=1))[:, None]
        d = g / g[:, ref_mic][:, None]
    return d


def own_spectrum(fs, N, xs, D, bin_lo, bin_hi, psi, cpsi, phi, cphi, theta, iterations=2, ref_mic=0, min_share=0.05, used=None,
                 est_dtype=np.float64):
    """psi, phi complex [K][M][M], cpsi, cphi [K] of one stream and slot, theta its direction -> dict(T float64 [D], used bool [K],
    edge bool [K]: the bins whose decision sits at an edge (mvdr_rtf_twin.edge_cells), diag).  used: a [K] bool override of the
    flags (the GPU's at the edge bins); a bin it switches on where the estimator fell back takes the estimate without the fallback."""
    K, M = N // 2 + 1, np.asarray(phi).shape[1]
    g0 = nt.steering(fs, N, xs, [float(theta)])[:, 0]
    d, ok, diag = rt.estimate(psi, cpsi, phi, cphi, g0, iterations, ref_mic, min_share, dtype=est_dtype)
    d = d.astype(np.complex128)
    k = np.arange(K)
    band = (k >= bin_lo) & (k <= bin_hi)
    tr = np.real(np.trace(np.asarray(phi), axis1=1, axis2=2))
    own = ok & (tr > 1e-30) & band
    use = own if used is None else np.asarray(used, dtype=bool) & band
    forced = use & ~ok
    if forced.any():
        raw = _raw_estimate(np.asarray(psi, dtype=np.complex128), np.asarray(cpsi, dtype=np.float64), np.asarray(phi, dtype=np.complex128),
                            np.asarray(cphi, dtype=np.float64), g0, iterations, ref_mic)
        d[forced] = raw[forced]
    with np.errstate(all="ignore"):
        u = d / np.sqrt(np.sum(np.abs(d) ** 2, axis=1))[:, None]
    u[~use] = 0.0
    dg = nt.steering(fs, N, xs, grid64(D))                                 # [K][D][M]
    T = np.sum(np.abs(np.einsum("kdm,km->kd", np.conj(dg), u)) ** 2, axis=0) / M
    return dict(T=T, used=own, edge=rt.edge_cells(diag, min_share) & band, diag=diag)


# ---- the parity inputs of tests/test_gpu_mvdr_tracks.py: the auto call's (two streams, two calls of 6 frames, two look directions,
# the first protected), then one update of the tracks seeded at the last frame's look directions ----
FS, N = 16000, 256
PARITY_M = (3, 8, 13, 16)                # Q = 1 ... 4 row slots, and M < 4 Q
PARITY_D = (61, 181)                     # one scan pass and two
PARITY_BAND = (5, 100)                   # chunks cut at both ends
PARITY_S = 2
PARITY_STEP = 0.3
# the tracks are seeded 3 degrees behind the last frame's look directions, as a track a step behind its talker is.  Of the offsets
# -3 ... 3 degrees this one leaves the fewest bins at a decision edge of the estimator (at most 1 of a case's 384 cells; seeded on the
# look direction itself the 16 microphones have 5, above the 1 % cap)
PARITY_SEED_OFFSET = np.deg2rad(-3.0)


def parity_seed(doa):
    """doa float32 [A][F][S] -> the seeds float32 [A][S]"""
    return (doa[:, -1, :] + np.float32(PARITY_SEED_OFFSET)).astype(np.float32)


def parity_setup(M):
    """dict(xs, pcm float32 [2][M][13 hop], doa float32 [2][12][2], rtf, estmask: the configurations of the two)"""
    import mvdr_estmask_twin as et
    xs = et.parity_xs(M)
    pcm, doa = et.parity_inputs(xs, FS, N, PARITY_S)
    rtf = rt.parity_config(len(xs))
    return dict(xs=xs, pcm=pcm, doa=doa, rtf=rtf, estmask=et.parity_config(N, PARITY_S, 1))


_STATE = {}


def parity_state(M):
    """[stream] -> the twin's state (phi, psi [S], cpsi [S], cphi) after the two auto calls, float64; computed once per M"""
    import mvdr_estmask_twin as et
    if M not in _STATE:
        p = parity_setup(M)
        hop, F = N // 2, et.PARITY_F
        rtf = dict(p["rtf"])
        out = []
        for a in range(p["pcm"].shape[0]):
            st = None
            for t0, t1 in ((0, F), (F, 2 * F)):
                st = et.auto_stream(FS, N, p["xs"], p["pcm"][a, :, t0 * hop:(t1 + 1) * hop].astype(np.float64), p["doa"][a, t0:t1], p["estmask"],
                                    rtf=rtf, state=st)
            out.append(st)
        _STATE[M] = out
    return _STATE[M]


# ---- the scene: mvdr_rtf_twin.rtf_scene()'s array with its errors; the protected talker walks from +20 to +35 degrees over the chunks,
# the interferer stays at -40 degrees.  The loop is the auto call with n_protected = 1, the tracks updated per chunk ----
SCENE_CHUNKS, SCENE_CF = 8, 12
SCENE_TRUTH = np.deg2rad(np.linspace(20.0, 35.0, SCENE_CHUNKS))           # the talker's direction in every chunk
SCENE_ITF = np.deg2rad(-40.0)
SCENE_D, SCENE_BAND = 181, (4, 124)
SCENE_TRACKS = dict(n_tracks=2, n_own=1, max_step_rad=np.deg2rad(5.0), min_sep_rad=np.deg2rad(8.0), hold=3)


def moving_scene(seed=3):
    """dict(xs, target, interferer (float64 [M][(F+1) hop], as the perturbed array records them), pcm float32): rtf_scene() with the
    target's direction stepping per chunk -- the same source signal, delayed for the chunk's direction"""
    from mcarray_amd import synth
    from oracle import np_twin
    fs, n_fft, F = rt.SCENE_FS, rt.SCENE_N, SCENE_CHUNKS * SCENE_CF
    xs = np.asarray(synth.ULA8)
    M, hop, K = len(xs), n_fft // 2, n_fft // 2 + 1
    n = (F + 1) * hop
    rng = np.random.default_rng(seed)
    xp = xs + 0.008 * rng.standard_normal(M)
    gain = 10.0 ** (rng.uniform(-2.0, 2.0, M) / 20.0)
    itf = gain[:, None] * synth.noise_source_stream(xp, SCENE_ITF, fs, n, 3).astype(np.float64)
    src = np.zeros((M, n))
    for c, th in enumerate(SCENE_TRUTH):
        a, b = c * SCENE_CF * hop, ((c + 1) * SCENE_CF * hop if c < SCENE_CHUNKS - 1 else n)
        src[:, a:b] = gain[:, None] * synth.noise_source_stream(xp, th, fs, n, 4, sigma=0.1 * 10.0 ** 0.5).astype(np.float64)[:, a:b]
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
    return dict(xs=list(xs), interferer=itf, target=tgt, pcm=(itf + tgt).astype(np.float32))


def target_share(w, sc, f0, f1):
    """w [F][K][M] of the frames f0 ... f1 - 1: the target's power at the output as a share of its power at the reference microphone"""
    from oracle import np_twin
    X = np_twin.stft_frames(sc["target"], rt.SCENE_N)[f0:f1]              # [F][M][K]
    return float(np.sum(np.abs(np.einsum("fkm,fmk->fk", np.conj(w), X)) ** 2) / np.sum(np.abs(X[:, rt.SCENE_REF]) ** 2))


def scene_update(st, trk, xs, rtf):
    """one update of the tracks on the state st of the auto twin -> the own direction found (NaN: none)"""
    import mvdr_spectrum_twin as sp
    fs, n_fft = rt.SCENE_FS, rt.SCENE_N
    g32 = grid64(SCENE_D).astype(F32)
    r = own_spectrum(fs, n_fft, xs, SCENE_D, SCENE_BAND[0], SCENE_BAND[1], st["psi"][0], st["cpsi"][0], st["phi"], st["cphi"], trk["theta"][0], **rtf)
    phi = window_argmax(r["T"], g32, trk["theta"][0], SCENE_TRACKS["max_step_rad"])[0] if trk["alive"][0] else F32(np.nan)
    P = sp.spectrum(st["phi"], fs, n_fft, xs, SCENE_D, SCENE_BAND[0], SCENE_BAND[1], sp.NORMALISED)
    _, pd, pv = sp.peaks(P, 2)
    associate(trk, [phi], pd, pv, **SCENE_TRACKS)
    return phi


def scene_loop(sc, tracked):
    """the loop over the chunks -> dict(theta [chunks]: the own track after every chunk (the held +20 degrees when not tracked),
    err_deg [chunks] against the truth, share: the target kept over the last chunk, run: the last chunk's run)"""
    import mvdr_estmask_twin as et
    fs, n_fft, hop = rt.SCENE_FS, rt.SCENE_N, rt.SCENE_N // 2
    trk = seed(new_state(), [SCENE_TRUTH[0], SCENE_ITF])
    pcm = sc["pcm"].astype(np.float64)
    st, thetas = None, []
    for c in range(SCENE_CHUNKS):
        row = fill(trk, 2) if tracked else np.float32([SCENE_TRUTH[0], SCENE_ITF])
        f0, f1 = c * SCENE_CF, (c + 1) * SCENE_CF
        st = et.auto_stream(fs, n_fft, sc["xs"], pcm[:, f0 * hop:(f1 + 1) * hop], np.tile(row.astype(np.float64), (SCENE_CF, 1)), et.SCENE_CFG,
                            rtf=et.SCENE_RTF, state=st, want_weights=True)
        if tracked:
            scene_update(st, trk, sc["xs"], et.SCENE_RTF)
        thetas.append(float(trk["theta"][0]) if tracked else float(np.float32(SCENE_TRUTH[0])))
    thetas = np.array(thetas)
    share = target_share(st["w"][:, 0], sc, (SCENE_CHUNKS - 1) * SCENE_CF, SCENE_CHUNKS * SCENE_CF)
    return dict(theta=thetas, err_deg=np.rad2deg(np.abs(thetas - SCENE_TRUTH)), share=share, run=st, tracks=trk)


# the twin's figures on the scene (tests/test_mvdr_tracks_twin.py recomputes them): the own track's worst error against the truth over
# the chunks (degrees) and the target kept over the last chunk, tracked and held at +20 degrees.  The track lags the talker: Psi has
# a memory of 1 / (1 - target_alpha) = 20 frames against chunks of 12, and the track moves to where Psi's dominant direction points.
SCENE_TWIN = dict(tracked=(7.0, 0.497), held=(15.0, 0.208))
_scene_cache = {}


def scene_runs():
    """dict(sc, tracked, held): moving_scene() and both loops of scene_loop(); computed once"""
    if not _scene_cache:
        sc = moving_scene()
        _scene_cache.update(sc=sc, tracked=scene_loop(sc, True), held=scene_loop(sc, False))
    return _scene_cache
