"""float64 twin of the MVDR call that steers with a relative transfer function estimated from a target covariance
(include/mcarray_hip.h, mca_hip_mvdr_set_rtf, mca_hip_mvdr_sources_frames_rtf_*).

Per stream, slot s, bin k and frame t, with x the frame's spectra, u the clamped update mask, m the clamped target mask of the slot
(a NaN counts as 0), a_tk = 1 - (1 - alpha) u and b = 1 - (1 - target_alpha) m:

    Phi_t  = a_tk Phi + (1 - a_tk) x x^H,   cphi_t = a_tk cphi + (1 - a_tk)        (both untouched where u == 0)
    Psi_t  = b Psi + (1 - b) x x^H,         cpsi_t = b cpsi + (1 - b)               (both untouched where m == 0)
    tau    = tr(Psi_t) / cpsi_t                                                      needs cpsi_t > 0 and tau > 1e-30
    Delta  = Psi_t / (cpsi_t tau) - [cphi_t > 0] Phi_t / (cphi_t tau)
    v = g0 / sqrt(M);  `iterations` times:  g = Delta v,  n = |g|^2 (needs n > 1e-20),  v_prev = v,  v = g / sqrt(n)
    rho    = Re(v_prev^H g)                                                          needs rho > min_share
                                                                                     needs |g[ref_mic]|^2 > 1e-6 n
    d      = g / g[ref_mic]                                                          (any need not met, or a non-finite value: d = g0)
    w      = PhiL_t^-1 d / (d^H PhiL_t^-1 d),  Y = w^H x

with g0 the geometric steering vector of doa[t][s] and PhiL the loaded covariance of the other twins.  A bin whose noise trace is
<= 1e-30 keeps w = g0 / M.  estimate() is the estimator alone, on any held state and in either precision: its float32 run is what
sets the bars of tests/test_gpu_mvdr_rtf.py.  rtf_scene() is the scene in which the geometric vector distorts the target: gains and
positions the beamformer does not know, and a look direction 4 degrees off."""
import numpy as np

from mcarray_amd import synth
from oracle import np_twin

import mvdr_gate_twin as gt
import mvdr_mask_twin as mt
import mvdr_nulls_twin as nt
from mvdr_postfilter_twin import _slots

DEFAULTS = dict(iterations=2, ref_mic=0, min_share=0.05)


def estimate(psi, cpsi, phi, cphi, g0, iterations=2, ref_mic=0, min_share=0.05, dtype=np.float64):
    """psi, phi [K][M][M], cpsi, cphi [K], g0 [K][M] -> (d [K][M], estimated [K] bool, dict(rho [K], n [iterations][K], tau [K],
    share [K] = |g_ref|^2 / n): what the decisions were taken on).  dtype float32 evaluates every step in single precision."""
    rt = np.dtype(dtype)
    ct = np.complex64 if rt == np.float32 else np.complex128
    psi, phi, g0 = np.asarray(psi).astype(ct), np.asarray(phi).astype(ct), np.asarray(g0).astype(ct)
    cpsi, cphi = np.asarray(cpsi).astype(rt), np.asarray(cphi).astype(rt)
    K, M = g0.shape
    with np.errstate(all="ignore"):
        tau = np.real(np.trace(psi, axis1=1, axis2=2)).astype(rt) / cpsi
        ok = (cpsi > 0) & (tau > 1e-30)
        sp = (rt.type(1) / (cpsi * tau)).astype(rt)
        sn = np.where(cphi > 0, rt.type(1) / (cphi * tau), rt.type(0)).astype(rt)
        delta = (psi * sp[:, None, None] - phi * sn[:, None, None]).astype(ct)
        v = (g0 / rt.type(np.sqrt(M))).astype(ct)
        ns = np.zeros((iterations, K), dtype=rt)
        for it in range(iterations):
            g = np.einsum("kij,kj->ki", delta, v).astype(ct)
            n = np.sum(np.abs(g) ** 2, axis=1).astype(rt)
            ns[it] = n
            ok &= n > 1e-20
            v_prev, v = v, (g / np.sqrt(n)[:, None]).astype(ct)
        rho = np.real(np.sum(np.conj(v_prev) * g, axis=1)).astype(rt)
        ok &= rho > min_share
        share = (np.abs(g[:, ref_mic]) ** 2 / n).astype(rt)
        ok &= np.abs(g[:, ref_mic]) ** 2 > rt.type(1e-6) * n
        d = (g / g[:, ref_mic][:, None]).astype(ct)
        ok &= np.all(np.isfinite(d), axis=1)
        d[:, ref_mic] = 1.0                                                # exactly, whatever the division rounds to
    d = np.where(ok[:, None], d, g0)
    return d, ok, dict(rho=rho, n=ns, tau=tau, share=share)


def edge_cells(diag, min_share=0.05):
    """[K] bool: the cells whose decision sits at an edge (rho within 1e-3 of min_share, |g_ref|^2 / n within a factor 2 of 1e-6, n or
    tau within a factor 10 of its threshold), where float32 and float64 may decide differently"""
    with np.errstate(all="ignore"):
        e = np.abs(diag["rho"] - min_share) <= 1e-3
        e |= (diag["share"] >= 0.5e-6) & (diag["share"] <= 2e-6)
        e |= np.any((diag["n"] >= 1e-21) & (diag["n"] <= 1e-19), axis=0)
        e |= (diag["tau"] >= 1e-31) & (diag["tau"] <= 1e-29)
    return e


def fresh_state(K, M, S, hop):
    return dict(phi=np.zeros((K, M, M), dtype=np.complex128), tail=np.zeros((S, hop)), psi=np.zeros((S, K, M, M), dtype=np.complex128),
                cpsi=np.zeros((S, K)), cphi=np.zeros(K))


def mvdr_rtf_stream(fs, N, xs, pcm, doa_rad, update, target_mask, alpha=0.95, loading=1e-3, target_alpha=None, iterations=2,
                    ref_mic=0, min_share=0.05, pf=None, state=None, want_weights=False, est_dtype=np.float64):
    """pcm [M][(F+1)*hop]; doa_rad [F][S] (or [F]); update [F][K] (None: all 1); target_mask [S][F][K] (None: all 0).  state: the
    dict a former call returned or None (fresh: everything zero).  pf: None or dict(smoothing, gain_floor, noise_scale).
    Returns dict(out [S][F*hop], spec [S][F][K] complex, phi, tail, psi [S][K][M][M], cpsi [S][K], cphi [K], d [F][S][K][M] the
    steering vectors of every frame, est [F][S][K] bool, diag [F][S] the decisions' inputs; w [F][S][K][M] on request) and the
    post-filter's keys with pf.  est_dtype float32: the estimator alone in single precision, on the same float64 state."""
    X = np_twin.stft_frames(pcm, N)                                        # complex [F][M][K]
    F, M, K = X.shape
    hop = N // 2
    doa = np.asarray(doa_rad, dtype=np.float64)
    if doa.ndim == 1:
        doa = doa[:, None]
    S = doa.shape[1]
    ta = alpha if target_alpha is None else target_alpha
    u = np.ones((F, K)) if update is None else gt.clamp(np.broadcast_to(np.asarray(update, dtype=np.float64), (F, K)))
    m = np.zeros((S, F, K)) if target_mask is None else gt.clamp(np.broadcast_to(np.asarray(target_mask, dtype=np.float64), (S, F, K)))
    st = fresh_state(K, M, S, hop) if state is None else state
    Phi, Psi, cpsi, cphi = st["phi"].copy(), _slots(st["psi"], S), _slots(st["cpsi"], S), st["cphi"].copy()
    tail = _slots(st["tail"], S)
    spec = np.zeros((S, F, K), dtype=np.complex128)
    out = np.zeros((S, F * hop))
    D = np.zeros((F, S, K, M), dtype=np.complex128)
    EST = np.zeros((F, S, K), dtype=bool)
    DIAG = [[None] * S for _ in range(F)]
    W = np.zeros((F, S, K, M), dtype=np.complex128) if want_weights else None
    if pf is not None:
        rtail = np.zeros((S, hop)) if state is None else _slots(st["raw_tail"], S)
        A = np.zeros((S, K)) if state is None else _slots(st["A"], S)
        raw, gain, pn, rout = np.zeros_like(spec), np.zeros((S, F, K)), np.zeros((S, F, K)), np.zeros_like(out)
    eye = np.eye(M)
    for t in range(F):
        Xc = X[t].T                                                        # [K][M]
        g0 = nt.steering(fs, N, xs, doa[t])                                # [K][S][M]
        o = u[t] != 0.0
        a = (1.0 - (1.0 - alpha) * u[t][o])[:, None, None]
        Phi[o] = a * Phi[o] + (1.0 - a) * Xc[o][:, :, None] * np.conj(Xc[o][:, None, :])     # the mask twin's operations
        cphi[o] = a[:, 0, 0] * cphi[o] + (1.0 - a[:, 0, 0])
        tr = np.real(np.trace(Phi, axis1=1, axis2=2))
        live = tr > 1e-30
        PL = np.where(live[:, None, None], Phi + (loading * tr / M)[:, None, None] * eye, eye)
        d = np.empty((K, S, M), dtype=np.complex128)
        for s in range(S):
            o = m[s, t] != 0.0
            b = (1.0 - (1.0 - ta) * m[s, t][o])[:, None, None]
            Psi[s][o] = b * Psi[s][o] + (1.0 - b) * Xc[o][:, :, None] * np.conj(Xc[o][:, None, :])
            cpsi[s][o] = b[:, 0, 0] * cpsi[s][o] + (1.0 - b[:, 0, 0])
            d[:, s], EST[t, s], DIAG[t][s] = estimate(Psi[s], cpsi[s], Phi, cphi, g0[:, s], iterations, ref_mic, min_share, est_dtype)
        D[t] = np.swapaxes(d, 0, 1)
        w = nt.null_weights(PL, d, 0.0)
        w[~live] = g0[~live] / M
        Y = np.einsum("ksm,km->sk", np.conj(w), Xc)                        # [S][K]
        if want_weights:
            W[t] = np.swapaxes(w, 0, 1)
        if pf is not None:
            h = np.linalg.solve(PL, np.swapaxes(d, 1, 2))                  # PhiL^-1 d_s  [K][M][S]
            p = pf["noise_scale"] / np.real(np.einsum("ksm,kms->ks", np.conj(d), h)).T      # [S][K]
            p[:, ~live] = 0.0
            Nn = pf["smoothing"] * A + (1.0 - pf["smoothing"]) * np.maximum(np.abs(Y) ** 2 - p, 0.0)
            G = np.where(p == 0.0, 1.0, np.maximum(pf["gain_floor"], Nn / np.where(p == 0.0, 1.0, Nn + p)))
            Z = G * Y
            A = np.abs(Z) ** 2
            raw[:, t], gain[:, t], pn[:, t] = Y, G, p
            y = np_twin.irfft_ccs(Y, N)
            rout[:, t * hop:(t + 1) * hop] = rtail + y[:, :hop]
            rtail = y[:, hop:]
            Y = Z
        spec[:, t] = Y
        y = np_twin.irfft_ccs(Y, N)
        out[:, t * hop:(t + 1) * hop] = tail + y[:, :hop]
        tail = y[:, hop:]
    r = dict(out=out, spec=spec, phi=Phi, tail=tail, psi=Psi, cpsi=cpsi, cphi=cphi, d=D, est=EST, diag=DIAG)
    if pf is not None:
        r.update(raw=raw, raw_out=rout, gain=gain, p=pn, raw_tail=rtail, A=A)
    if want_weights:
        r["w"] = W
    return r


def target_parity_mask(S, A=2, F=12, K=129, seed=23):
    """[A][S][F][K]: the target masks of the GPU tests, a parity mask (mvdr_mask_twin.parity_mask) of its own seed per slot"""
    def one(sd):
        base = mt.parity_mask(A, F, seed=sd)
        return np.tile(base, (1, 1, K // base.shape[2] + 1))[:, :, :K]
    return np.ascontiguousarray(np.stack([one(seed + 7 * s) for s in range(S)], axis=1))


# ---- the parity cases of tests/test_gpu_mvdr_rtf.py: two streams, two calls of 6 frames, nt.scene inputs, mt.parity_mask() as update mask ----
PARITY_F = 6


def parity_config(M):
    """the estimator's parameters of a parity case: every iteration count and a reference microphone in every row slot occur"""
    return dict(target_alpha=0.9, iterations=1 + M % 4, ref_mic=(3 * M) // 4, min_share=0.05)


def parity_inputs(xs, fs, N, S, A=2, F=PARITY_F):
    """(pcm float32 [A][M][(2F+1) hop], doa float32 [A][2F][S], update float32 [A][2F][K], tmask float32 [A][S][2F][K])"""
    K = N // 2 + 1
    pcm = np.stack([nt.scene(xs, fs, N, 2 * F, a) for a in range(A)])
    m = mt.mask_for(K, A, 12)
    upd = np.ascontiguousarray(np.concatenate([m[:, :F], m[:, 6:6 + F]], axis=1))
    tm = target_parity_mask(S, A, 12, K)
    tmask = np.ascontiguousarray(np.concatenate([tm[:, :, :F], tm[:, :, 6:6 + F]], axis=2))
    return pcm, nt.drifting_doa(A, 2 * F, S), upd, tmask


def parity_twin(xs, fs, N, S, pf=None, est_dtype=np.float64, F=PARITY_F):
    """the twin on the inputs above: [stream][call] -> the dict of mvdr_rtf_stream, the second call continuing the first"""
    pcm, doa, upd, tmask = parity_inputs(xs, fs, N, S, F=F)
    hop, cfg = N // 2, parity_config(len(xs))
    res = []
    for a in range(pcm.shape[0]):
        st, calls = None, []
        for t0, t1 in ((0, F), (F, 2 * F)):
            st = mvdr_rtf_stream(fs, N, xs, pcm[a, :, t0 * hop:(t1 + 1) * hop].astype(np.float64), doa[a, t0:t1], upd[a, t0:t1],
                                 tmask[a, :, t0:t1], pf=pf, state=st, est_dtype=est_dtype, **cfg)
            calls.append(st)
        res.append(calls)
    return res


def edges_of(run, min_share=0.05):
    """[F][S][K] bool of a run of mvdr_rtf_stream: the cells at a decision edge"""
    return np.array([[edge_cells(dg, min_share) for dg in row] for row in run["diag"]])


# ---- the scene: sparse_target_scene() of the mask twin on an array the beamformer knows only nominally ----
SCENE_FS, SCENE_N, SCENE_F = 16000, 256, 48
SCENE_LOOK = np.deg2rad(24.0)            # 4 degrees off the target
SCENE_LAST = 24                          # the frames the figures are taken over
SCENE_REF = 0


def rtf_scene(seed=3):
    """dict(xs nominal positions, interferer, target (float64 [M][(F+1)*hop], as the perturbed array records them), pcm (their sum,
    float32), update float32 [F][K] (1 where the target is absent), tmask float32 [1][F][K] (1 where it is present)).
    Microphone gains of +-2 dB and position errors of about 8 mm (fixed seed); the interferer at -40 degrees; the target at +20
    degrees, sparse in time and frequency and 10 dB above the interferer in its cells.  The seed of the perturbation is one of those
    for which the geometric vector loses the target (seeds whose reference microphone has a low gain make it gain level instead: the
    figures are shares of the level at that microphone)."""
    fs, N, F = SCENE_FS, SCENE_N, SCENE_F
    xs = np.asarray(synth.ULA8)
    M = len(xs)
    hop, K = N // 2, N // 2 + 1
    n = (F + 1) * hop
    rng = np.random.default_rng(seed)
    xp = xs + 0.008 * rng.standard_normal(M)
    gain = 10.0 ** (rng.uniform(-2.0, 2.0, M) / 20.0)
    itf = gain[:, None] * synth.noise_source_stream(xp, np.deg2rad(-40.0), fs, n, 3).astype(np.float64)
    src = gain[:, None] * synth.noise_source_stream(xp, np.deg2rad(20.0), fs, n, 4, sigma=0.1 * 10.0 ** 0.5).astype(np.float64)
    rng = np.random.default_rng(7)
    pat = np.zeros((F, K))
    for tb in range(0, F, 4):
        for kb in range(0, K, 16):
            if rng.random() < 0.5:
                pat[tb:tb + 4, kb:kb + 16] = 1.0
    T = np_twin.stft_frames(src, N) * pat[:, None, :]
    tgt = np.zeros_like(src)
    for t in range(F):
        tgt[:, t * hop:t * hop + N] += np_twin.irfft_ccs(T[t], N)
    pt = np.abs(np_twin.stft_frames(tgt, N)[:, SCENE_REF]) ** 2            # [F][K] at the reference microphone
    pi = np.mean(np.abs(np_twin.stft_frames(itf, N)[:, SCENE_REF]) ** 2, axis=0)
    present = pt >= 1e-2 * pi[None, :]
    return dict(xs=list(xs), interferer=itf, target=tgt, pcm=(itf + tgt).astype(np.float32), update=(~present).astype(np.float32),
                tmask=present.astype(np.float32)[None])


def scene_figures(w, sc):
    """w [F][K][M]: the weights a run on the mixture was beamformed with.  (the target's power at the output as a share of its power
    at the reference microphone, the interferer's level under its level at the reference microphone in dB), over the last
    SCENE_LAST frames"""
    res = []
    for x in (sc["target"], sc["interferer"]):
        X = np_twin.stft_frames(x, SCENE_N)[-SCENE_LAST:]                  # [F][M][K]
        pw = np.sum(np.abs(np.einsum("fkm,fmk->fk", np.conj(w[-SCENE_LAST:]), X)) ** 2)
        pr = np.sum(np.abs(X[:, SCENE_REF]) ** 2)
        res.append((pw, pr))
    return res[0][0] / res[0][1], 10.0 * np.log10(res[1][1] / res[1][0])


SCENE_BARS = dict(share_lo=0.85, share_hi=1.15, geometric_below=0.8, suppression_margin_db=3.0)
