"""float64 twin of the RTF-steered MVDR call with soft nulls at the ESTIMATED steering vectors of the other look directions
(include/mcarray_hip.h, mca_hip_mvdr_set_rtf_nulls).

The frame loop of mvdr_rtf_twin.mvdr_rtf_stream with the dense nulls of mvdr_nulls_twin.null_weights on the vectors the frame uses:
per stream, bin and frame, with d_s the vector of slot s (the RTF, or the geometric vector where the estimator fell back), PhiL the
loaded covariance and g = null_gain,

    p_r = 1 / (d_r^H PhiL^-1 d_r),   Phi_s = PhiL + g sum_{r != s} p_r d_r d_r^H,   w_s = Phi_s^-1 d_s / (d_s^H Phi_s^-1 d_s),   Y_s = w_s^H x

p_r d_r d_r^H does not depend on the scale of d_r: the normalisation to the reference microphone does not enter the nulls.  A bin whose
noise trace is <= 1e-30 keeps w = g0 / M.  The post-filter's p stays the plain noise_scale / (d_s^H PhiL^-1 d_s); no recursion sees
the gain.

two_talker_scene() is the scene the nulls are for: two sparse talkers whose cells the update mask protects, so that the noise
covariance holds neither of them, on an array the beamformer knows only nominally.  Measured here in float64 (seed 3; own talker's
share out 0 / out 1, other talker under its level at microphone 0, background likewise; the last 24 frames):

    estimated vectors, g = 0       share 0.950 / 0.973    other  2.4 /  4.4 dB    background 16.4 / 15.5 dB
    geometric vectors, g = 100     share 0.481 / 0.573    other  7.3 /  8.6 dB    background 14.2 / 16.2 dB
    estimated vectors, g = 100     share 0.957 / 0.968    other 13.7 / 14.1 dB    background 13.1 / 14.2 dB

GAIN_CAP_FIGURES are the figures that set the bars of tests/test_gpu_mvdr_rtf_nulls.py at g = 1000: how far the twin with a float32
estimator is from the float64 one on the parity inputs, as a fraction of the peak, over the cells that are at no decision edge.
tests/test_mvdr_rtf_nulls_twin.py measures them again and holds them to the values written here."""
import numpy as np

from mcarray_amd import synth
from oracle import np_twin

import mvdr_gate_twin as gt
import mvdr_nulls_twin as nt
import mvdr_rtf_twin as rt
from mvdr_postfilter_twin import _slots


def mvdr_rtf_nulls_stream(fs, N, xs, pcm, doa_rad, update, target_mask, null_gain, alpha=0.95, loading=1e-3, target_alpha=None,
                          iterations=2, ref_mic=0, min_share=0.05, pf=None, state=None, want_weights=False, est_dtype=np.float64):
    """the arguments and the result of rt.mvdr_rtf_stream, with null_gain behind the masks"""
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
    st = rt.fresh_state(K, M, S, hop) if state is None else state
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
        Phi[o] = a * Phi[o] + (1.0 - a) * Xc[o][:, :, None] * np.conj(Xc[o][:, None, :])
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
            d[:, s], EST[t, s], DIAG[t][s] = rt.estimate(Psi[s], cpsi[s], Phi, cphi, g0[:, s], iterations, ref_mic, min_share, est_dtype)
        D[t] = np.swapaxes(d, 0, 1)
        w = nt.null_weights(PL, d, null_gain)                              # the nulls sit at the vectors the frame uses
        w[~live] = g0[~live] / M
        Y = np.einsum("ksm,km->sk", np.conj(w), Xc)                        # [S][K]
        if want_weights:
            W[t] = np.swapaxes(w, 0, 1)
        if pf is not None:
            h = np.linalg.solve(PL, np.swapaxes(d, 1, 2))                  # PhiL^-1 d_s  [K][M][S]: the plain estimate, also under nulls
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


# ---- the parity cases of tests/test_gpu_mvdr_rtf_nulls.py, on rt.parity_inputs / rt.parity_config ----
PARITY_CASES = [(2, 2), (2, 3), (4, 2), (7, 3), (8, 2), (13, 4), (16, 4)]       # (M, S): every Q, M = 4Q, the two-pass row, S > M
PARITY_GAIN, PARITY_GAIN_CAP = 10.0, 1000.0
EDGE_CAP = 0.03                       # share of a case's cells that may be left out


def parity_twin(xs, fs, N, S, null_gain, pf=None, est_dtype=np.float64, F=rt.PARITY_F):
    """the twin on rt.parity_inputs: [stream][call] -> the dict of mvdr_rtf_nulls_stream, the second call continuing the first"""
    pcm, doa, upd, tmask = rt.parity_inputs(xs, fs, N, S, F=F)
    hop, cfg = N // 2, rt.parity_config(len(xs))
    res = []
    for a in range(pcm.shape[0]):
        st, calls = None, []
        for t0, t1 in ((0, F), (F, 2 * F)):
            st = mvdr_rtf_nulls_stream(fs, N, xs, pcm[a, :, t0 * hop:(t1 + 1) * hop].astype(np.float64), doa[a, t0:t1], upd[a, t0:t1],
                                       tmask[a, :, t0:t1], null_gain, pf=pf, state=st, est_dtype=est_dtype, **cfg)
            calls.append(st)
        res.append(calls)
    return res


def left_out(run64, run32, min_share=0.05):
    """[F][K] bool: the cells of a call that the parity test leaves out.  A null uses every slot's vector, so a cell goes if
    rt.edge_cells flags any slot of it, or if the float32 and the float64 estimator decide differently for any slot."""
    return np.any(rt.edges_of(run64, min_share) | (run64["est"] != run32["est"]), axis=1)


def f32_distance(a, b, pf=False):
    """a, b: the float64 and the float32-estimator run of one call -> (the largest |spec32 - spec64| of an output over the kept cells
    as a fraction of that output's peak |spec64| in the call, cells left out, cells): the way the GPU test measures its distance"""
    lo = left_out(a, b)                                                    # [F][K]
    key = "raw" if pf else "spec"
    worst = max(float(np.max(np.abs(b["spec"][s] - a["spec"][s]) * ~lo) / np.max(np.abs(a[key][s]))) for s in range(a["spec"].shape[0]))
    return worst, int(lo.sum()), lo.size


def estimator_error(xs, fs, N, S, null_gain, pf=None):
    """(the worst f32_distance, the share of cells left out) over both streams and both calls of the parity inputs: what the float32
    estimator alone costs under this gain"""
    r64 = parity_twin(xs, fs, N, S, null_gain, pf=pf)
    r32 = parity_twin(xs, fs, N, S, null_gain, pf=pf, est_dtype=np.float32)
    ds = [f32_distance(a, b, pf is not None) for c64, c32 in zip(r64, r32) for a, b in zip(c64, c32)]
    return max(d[0] for d in ds), sum(d[1] for d in ds) / sum(d[2] for d in ds)


# (M or "ula16", fs, N, S, post-filter) of the parity cases of tests/test_gpu_mvdr_rtf_nulls.py
def parity_xs(M):
    import mvdr_postfilter_twin as pt
    return np.asarray(synth.ULA16) if M == "ula16" else pt.irregular(M)


PARITY_RUNS = [(M, 16000, 256, S, False) for M, S in PARITY_CASES] + [(11, 16000, 256, 3, True), ("ula16", 48000, 1024, 3, False)]

# estimator_error() of every parity run at g = 1000, rounded up to two digits: the float32 estimator's own error, which the gain
# amplifies (at g = 10 it stays under 2.4e-4 in every run).  The GPU test's bar for a run is four times its figure and never below
# the module's 5e-4 of the peak.  tests/test_mvdr_rtf_nulls_twin.py measures them again and holds them to these values.  The twin
# leaves out at most 1.52 % of a run's cells (M = 16, S = 4).
GAIN_CAP_FIGURES = {
    (2, 16000, 256, 2, False): 1.5e-4,
    (2, 16000, 256, 3, False): 1.8e-4,
    (4, 16000, 256, 2, False): 1.6e-3,
    (7, 16000, 256, 3, False): 9.3e-3,
    (8, 16000, 256, 2, False): 1.4e-3,
    (13, 16000, 256, 4, False): 1.1e-2,
    (16, 16000, 256, 4, False): 4.3e-3,
    (11, 16000, 256, 3, True): 1.3e-2,
    ("ula16", 48000, 1024, 3, False): 5.1e-4,
}
SPEC_TOL = 5e-4                       # the module's bar, of the peak: spectra and audio at g = 10


def gain_cap_bar(run):
    return max(SPEC_TOL, 4.0 * GAIN_CAP_FIGURES[run])


# ---- the scene: two sparse talkers on an array the beamformer knows only nominally ----
SCENE_FS, SCENE_N, SCENE_F, SCENE_LAST, SCENE_REF = rt.SCENE_FS, rt.SCENE_N, rt.SCENE_F, rt.SCENE_LAST, rt.SCENE_REF
SCENE_LOOKS = np.deg2rad([24.0, -37.0])          # 4 and 3 degrees off the talkers
SCENE_GAIN = 100.0


def _sparse(x, N, F, seed, keep=0.35):
    """x [M][(F+1) hop] with 4-frame x 16-bin blocks of its spectrogram kept with probability `keep`"""
    hop, K = N // 2, N // 2 + 1
    rng = np.random.default_rng(seed)
    pat = np.zeros((F, K))
    for tb in range(0, F, 4):
        for kb in range(0, K, 16):
            if rng.random() < keep:
                pat[tb:tb + 4, kb:kb + 16] = 1.0
    T = np_twin.stft_frames(x, N) * pat[:, None, :]
    y = np.zeros_like(x)
    for t in range(F):
        y[:, t * hop:t * hop + N] += np_twin.irfft_ccs(T[t], N)
    return y


def two_talker_scene(seed=3):
    """dict(xs nominal positions, talkers [2] and background (float64 [M][(F+1)*hop], as the perturbed array records them), pcm (their
    sum, float32), update float32 [F][K] (1 where neither talker is present), tmask float32 [2][F][K] (1 where the talker is present
    and 10 dB above the other), doa float32 [F][2]).  Gains of +-2 dB and position errors of about 8 mm as in rt.rtf_scene(); a weak
    background at 65 degrees, talker A at +20 and talker B at -40 degrees, both sparse in 4 x 16 blocks."""
    fs, N, F = SCENE_FS, SCENE_N, SCENE_F
    xs = np.asarray(synth.ULA8)
    M = len(xs)
    hop = N // 2
    n = (F + 1) * hop
    rng = np.random.default_rng(seed)
    xp = xs + 0.008 * rng.standard_normal(M)
    gain = 10.0 ** (rng.uniform(-2.0, 2.0, M) / 20.0)
    bg = gain[:, None] * synth.noise_source_stream(xp, np.deg2rad(65.0), fs, n, 3, sigma=0.03).astype(np.float64)
    ta = _sparse(gain[:, None] * synth.noise_source_stream(xp, np.deg2rad(20.0), fs, n, 4, sigma=0.3).astype(np.float64), N, F, 7)
    tb = _sparse(gain[:, None] * synth.noise_source_stream(xp, np.deg2rad(-40.0), fs, n, 5, sigma=0.3).astype(np.float64), N, F, 11)
    pb = np.mean(np.abs(np_twin.stft_frames(bg, N)[:, SCENE_REF]) ** 2, axis=0)           # [K]
    pw = [np.abs(np_twin.stft_frames(x, N)[:, SCENE_REF]) ** 2 for x in (ta, tb)]         # [F][K] at microphone 0
    present = [p >= 0.1 * pb[None, :] for p in pw]
    tmask = np.stack([present[0] & (pw[0] >= 10.0 * pw[1]), present[1] & (pw[1] >= 10.0 * pw[0])]).astype(np.float32)
    update = (~(present[0] | present[1])).astype(np.float32)
    doa = np.tile(SCENE_LOOKS.astype(np.float32)[None, :], (F, 1))
    return dict(xs=list(xs), talkers=[ta, tb], background=bg, pcm=(bg + ta + tb).astype(np.float32), update=update, tmask=tmask, doa=doa)


def scene_figures(w, sc):
    """w [F][S = 2][K][M]: the weights of every frame of a run on the mixture.  Per output s, over the last SCENE_LAST frames: (the
    own talker's power at the output as a share of its power at microphone 0, the other talker's level under its level at microphone
    0 in dB, the background's likewise) -> [2][3]"""
    def through(ws, x):
        X = np_twin.stft_frames(x, SCENE_N)[-SCENE_LAST:]                  # [F][M][K]
        pw = np.sum(np.abs(np.einsum("fkm,fmk->fk", np.conj(ws[-SCENE_LAST:]), X)) ** 2)
        return pw, np.sum(np.abs(X[:, SCENE_REF]) ** 2)
    res = []
    for s in range(2):
        own, other, bg = (through(w[:, s], x) for x in (sc["talkers"][s], sc["talkers"][1 - s], sc["background"]))
        res.append((own[0] / own[1], 10.0 * np.log10(other[1] / other[0]), 10.0 * np.log10(bg[1] / bg[0])))
    return res


def scene_runs(sc=None, gain=SCENE_GAIN):
    """the three runs of the scene table: dict(rtf0, geo, rtf) -> scene_figures of the estimated vectors at g = 0, the geometric
    vectors at `gain` (the masked call: no target mask, so every d is g0) and the estimated vectors at `gain`"""
    sc = two_talker_scene() if sc is None else sc
    pcm = sc["pcm"].astype(np.float64)
    def run(tmask, g):
        r = mvdr_rtf_nulls_stream(SCENE_FS, SCENE_N, sc["xs"], pcm, sc["doa"], sc["update"], tmask, g, want_weights=True)
        return scene_figures(r["w"], sc)
    return dict(rtf0=run(sc["tmask"], 0.0), geo=run(None, gain), rtf=run(sc["tmask"], gain))


def scene_twin(sc, est_dtype=np.float64, gain=SCENE_GAIN):
    """the run of the scene's mixture under the nulls at the estimated vectors, with the weights of every frame"""
    return mvdr_rtf_nulls_stream(SCENE_FS, SCENE_N, sc["xs"], sc["pcm"].astype(np.float64), sc["doa"], sc["update"], sc["tmask"], gain,
                                 want_weights=True, est_dtype=est_dtype)


# f32_distance of the scene's run at g = 100, rounded up to two digits; the GPU test's bar for the scene is four times this and never
# below the module's 5e-4.  tests/test_mvdr_rtf_nulls_twin.py measures it again.
SCENE_F32_FIGURE = 8.7e-7


def scene_bar():
    return max(SPEC_TOL, 4.0 * SCENE_F32_FIGURE)


# relative to the twin's own run, in the style of rt.SCENE_BARS
SCENE_BARS = dict(share_lo=0.85, share_hi=1.15, over_plain_db=6.0, over_geometric_db=3.0, geometric_below=0.8, gpu_margin_db=3.0)
