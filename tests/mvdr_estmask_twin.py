"""float64 twin of the mask estimator of the MVDR context (include/mcarray_hip.h, mca_hip_mvdr_set_mask_estimator,
mca_hip_mvdr_sources_frames_auto_*; k_mvdr_estmask).

Per frame t and bin k, with x the frame's M spectra of the bin and g_s the geometric steering vector of doa[t][s], s = 0 ... S-1:

    e    = sum_m |x_m|^2
    c_s  = |g_s^H x|^2 / (M e)                 in [0, 1]; 0 for every s where e <= 1e-30
    w    = the s with the largest c_s, searched upwards with a strict '>' (ties and NaNs stay with the lower index)
    v    = clamp((c_w - coherence_lo) / (coherence_hi - coherence_lo))       to [0, 1], a NaN counts as 0
    target[s][t][k] = v if s == w, else 0
    update[t][k]    = 1 - max over s < P of target[s][t][k]                 P = n_protected, or S where that is 0 or above S

and target 0, update 1 outside the band [bin_lo, bin_hi].  auto_stream() is the whole call: the masks, then mvdr_rtf_twin's or
mvdr_mask_twin's stream under them.  estimate(..., dtype=float32) is the float32 variant: complex64 spectra from a float32
transform of the float32 windowed frames (what the GPU's analysis holds: its error is relative to the frame's peak, not to the
cell, which is why cells of low energy are edge cells), complex64 steering vectors, float32 arithmetic.  Its distance from the
float64 twin outside edge_cells() sets the mask bar of tests/test_gpu_mvdr_estmask.py."""
import numpy as np

from oracle import np_twin

import mvdr_mask_twin as mt
import mvdr_nulls_twin as nt
import mvdr_postfilter_twin as pt
import mvdr_rtf_twin as rt

DEFAULTS = dict(bin_lo=0, bin_hi=None, coherence_lo=0.0, coherence_hi=0.05, n_protected=0)


def stft_frames32(pcm, N):
    """[M][(F+1)*hop] -> complex64 [F][M][K]: np_twin.stft_frames in single precision throughout"""
    pcm = np.asarray(pcm, dtype=np.float32)
    hop = N // 2
    F = pcm.shape[1] // hop - 1
    w = np_twin.hann(N).astype(np.float32)
    idx = np.arange(N)[None, :] + hop * np.arange(F)[:, None]
    X = np.fft.rfft(pcm[:, idx] * w, axis=-1).transpose(1, 0, 2)
    assert X.dtype == np.complex64                                          # (a numpy that transforms float32 in double would say nothing here)
    return X


def steering_frames(fs, N, xs, doa):
    """doa [F][S] -> g [F][K][S][M]"""
    return np.stack([nt.steering(fs, N, xs, d) for d in np.asarray(doa, dtype=np.float64)])


def estimate(X, g, bin_lo=0, bin_hi=None, coherence_lo=0.0, coherence_hi=0.05, n_protected=0, dtype=np.float64):
    """X [F][M][K] spectra, g [F][K][S][M] steering vectors -> dict(update [F][K], target [S][F][K], c [F][K][S], e [F][K],
    w [F][K] int, band [K] bool).  dtype float32: every step in single precision."""
    ft = np.dtype(dtype)
    ct = np.complex64 if ft == np.float32 else np.complex128
    Xc = np.ascontiguousarray(np.swapaxes(np.asarray(X), 1, 2)).astype(ct)  # [F][K][M]
    g = np.asarray(g).astype(ct)
    F, K, S, M = g.shape
    bin_hi = K - 1 if bin_hi is None else bin_hi
    with np.errstate(all="ignore"):
        e = np.sum((Xc.real ** 2 + Xc.imag ** 2).astype(ft), axis=2, dtype=ft)
        p = np.einsum("fksm,fkm->fks", np.conj(g), Xc).astype(ct)
        num = (p.real ** 2 + p.imag ** 2).astype(ft)
        live = e > 1e-30
        c = np.where(live[..., None], num / np.where(live, ft.type(M) * e, ft.type(1))[..., None], ft.type(0)).astype(ft)
        w = np.zeros((F, K), dtype=np.int64)
        best = c[..., 0].copy()
        for s in range(1, S):
            better = c[..., s] > best
            w[better] = s
            best = np.where(better, c[..., s], best)
        v = ((best - ft.type(coherence_lo)) / ft.type(coherence_hi - coherence_lo)).astype(ft)
        v = np.where(np.isnan(v), ft.type(0), np.minimum(np.maximum(v, ft.type(0)), ft.type(1))).astype(ft)
    band = (np.arange(K) >= bin_lo) & (np.arange(K) <= bin_hi)
    P = S if n_protected == 0 or n_protected > S else n_protected
    target = np.stack([np.where((w == s) & band[None, :], v, ft.type(0)) for s in range(S)]).astype(ft)
    update = np.where((w < P) & band[None, :], ft.type(1) - v, ft.type(1)).astype(ft)
    return dict(update=update, target=target, c=c, e=e, w=np.where(band[None, :], w, 0), band=band)


def masks(fs, N, xs, pcm, doa_rad, dtype=np.float64, **cfg):
    """pcm [M][(F+1)*hop], doa_rad [F][S] (or [F]) -> estimate() on the call's spectra.  float32: pcm as float32, stft_frames32."""
    doa = np.asarray(doa_rad, dtype=np.float64)
    if doa.ndim == 1:
        doa = doa[:, None]
    X = stft_frames32(pcm, N) if np.dtype(dtype) == np.float32 else np_twin.stft_frames(pcm, N)
    return estimate(X, steering_frames(fs, N, xs, doa), dtype=dtype, **cfg)


def edge_cells(d64, d32):
    """[F][K] bool, from the float64 and the float32 run of estimate() on one input.  (low: the cells whose e is under 1e-6 of the
    largest cell energy of their frame; edge: those, the cells whose two largest c differ by less than 1e-4, and the cells whose
    winner differs between the two runs) -- inside the band; outside it nothing is decided"""
    c = np.sort(d64["c"], axis=2)
    low = d64["e"] < 1e-6 * d64["e"].max(axis=1, keepdims=True)
    edge = low | (d64["w"] != d32["w"])
    if c.shape[2] > 1:
        edge |= (c[..., -1] - c[..., -2]) < 1e-4
    return low & d64["band"][None, :], edge & d64["band"][None, :]


def auto_stream(fs, N, xs, pcm, doa_rad, cfg=None, rtf=None, pf=None, alpha=0.95, loading=1e-3, state=None, want_weights=False):
    """the auto call: pcm [M][(F+1)*hop]; doa_rad [F][S]; cfg the estimator's configuration; rtf None (the masked call under the
    update mask) or the dict of mvdr_rtf_stream's parameters (the RTF call under both masks).  Returns that stream's dict with
    update_mask [F][K], target_mask [S][F][K] and masks (the dict of estimate()) beside it."""
    m = masks(fs, N, xs, pcm, doa_rad, **(cfg or {}))
    if rtf is not None:
        r = rt.mvdr_rtf_stream(fs, N, xs, pcm, doa_rad, m["update"], m["target"], alpha=alpha, loading=loading, pf=pf, state=state,
                               want_weights=want_weights, **rtf)
    elif pf is not None:
        r = mt.mvdr_mask_postfilter_stream(fs, N, xs, pcm, doa_rad, 0.0, m["update"], alpha=alpha, loading=loading, state=state, **pf)
    else:
        r = mt.mvdr_mask_stream(fs, N, xs, pcm, doa_rad, 0.0, m["update"], alpha=alpha, loading=loading, state=state, want_weights=want_weights)
    r.update(update_mask=m["update"], target_mask=m["target"], masks=m)
    return r


# ---- the parity cases of tests/test_gpu_mvdr_estmask.py: two streams, two calls of 6 frames, nt.scene inputs, nt.drifting_doa ----
PARITY_F = 6
PARITY_M, PARITY_S = (2, 3, 4, 5, 8, 11, 13, 16), (1, 2, 4)
# (xs, fs, N, S, n_protected): every row-slot count with a full and a partly empty slot x one, two and four look directions, all
# protected (the update mask is then continuous across a winner tie); a competitor; the long frames of k_mvdr_analyse_1024
PARITY_CASES = [("M%d_S%d" % (M, S), M, 16000, 256, S, 0) for M in PARITY_M for S in PARITY_S]
PARITY_CASES += [("M8_S2_P1", 8, 16000, 256, 2, 1), ("ula16_N1024_S2", "ula16", 48000, 1024, 2, 0)]


def parity_xs(M):
    """the arrays of the RTF parity cases, but for two microphones: pt.irregular(2) puts them 3 mm apart, where the steering vectors
    of all look directions nearly coincide in every bin and 3 ... 8 % of the cells are ties of the winner -- 8 cm instead"""
    from mcarray_amd import synth
    return np.asarray(synth.ULA16) if M == "ula16" else np.array([0.0, 0.08]) if M == 2 else pt.irregular(M)


def parity_config(N, S, n_protected=0):
    """the estimator's parameters of a parity case: a band that leaves out bins at both ends; thresholds between which a good share
    of the cells lands, so that the masks take values inside (0, 1) and both saturations (one look direction: the absolute 0.2 / 0.4)"""
    lo, hi = (0.2, 0.4) if S == 1 else (0.3, 0.8)
    return dict(bin_lo=2, bin_hi=N // 2 - 3, coherence_lo=lo, coherence_hi=hi, n_protected=n_protected)


def parity_inputs(xs, fs, N, S, A=2, F=PARITY_F):
    """(pcm float32 [A][M][(2F+1) hop], doa float32 [A][2F][S])"""
    pcm = np.stack([nt.scene(xs, fs, N, 2 * F, a) for a in range(A)])
    return pcm, nt.drifting_doa(A, 2 * F, S)


_PARITY = {}


def parity(case):
    """dict(xs, cfg, pcm, doa, d64 [A], d32 [A] (estimate() over the 2F frames of a stream: the estimator is stateless, so the two
    calls of the GPU test are its halves), low [A], edge [A]); computed once per case"""
    name, M, fs, N, S, P = case
    if name not in _PARITY:
        xs = parity_xs(M)
        cfg = parity_config(N, S, P)
        pcm, doa = parity_inputs(xs, fs, N, S)
        d64 = [masks(fs, N, xs, pcm[a].astype(np.float64), doa[a], **cfg) for a in range(pcm.shape[0])]
        d32 = [masks(fs, N, xs, pcm[a], doa[a], dtype=np.float32, **cfg) for a in range(pcm.shape[0])]
        le = [edge_cells(p, q) for p, q in zip(d64, d32)]
        _PARITY[name] = dict(xs=xs, cfg=cfg, pcm=pcm, doa=doa, d64=d64, d32=d32, low=[x[0] for x in le], edge=[x[1] for x in le])
    return _PARITY[name]


def parity_distance(case):
    """(share of edge cells, largest |float32 - float64| of the target masks outside edge cells, of the update mask outside
    low-energy cells where every direction is protected, else outside edge cells)"""
    p = parity(case)
    n_edge = n_all = 0
    wt = wu = 0.0
    for a in range(len(p["d64"])):
        r, q, low, edge = p["d64"][a], p["d32"][a], p["low"][a], p["edge"][a]
        n_edge, n_all = n_edge + int(edge.sum()), n_all + edge.size
        wt = max(wt, float((np.abs(r["target"] - q["target"]) * ~edge[None]).max()))
        wu = max(wu, float((np.abs(r["update"] - q["update"]) * ~(low if case[5] == 0 else edge)).max()))
    return n_edge / n_all, wt, wu


# the largest distance parity_distance() measures over PARITY_CASES (tests/test_mvdr_estmask_twin.py holds every case under it), and
# the GPU's bar: four times that, the rule of tests/test_gpu_mvdr_rtf.py
MASK_F32_MEASURED = 1.031e-6
MASK_BAR = 4.0 * MASK_F32_MEASURED


# ---- the scene: mvdr_rtf_twin.rtf_scene() with the masks estimated instead of given ----
SCENE_DOAS = np.deg2rad([24.0, -40.0])   # the look direction of the RTF scene (4 degrees off the target) and the interferer as competitor
SCENE_CFG = dict(bin_lo=0, bin_hi=None, coherence_lo=0.0, coherence_hi=0.05, n_protected=1)
SCENE_RTF = dict(iterations=2, ref_mic=0, min_share=0.05)
# the twin's figures on the scene (tests/test_mvdr_estmask_twin.py recomputes them): target share and interferer suppression in dB of
# output 0, without masks and with the estimated ones
SCENE_TWIN = dict(none=(0.009, 17.21), estimated=(0.982, 12.54))


def scene_runs(sc=None):
    """rtf_scene() without masks (update all 1, no target mask: the geometric vector, learning everything) and with the estimated
    ones -> dict(none=(share, dB), estimated=(share, dB), run=the estimated run), figures of output 0 over the last frames"""
    sc = rt.rtf_scene() if sc is None else sc
    pcm = sc["pcm"].astype(np.float64)
    doa = np.tile(SCENE_DOAS, (rt.SCENE_F, 1))
    none = rt.mvdr_rtf_stream(rt.SCENE_FS, rt.SCENE_N, sc["xs"], pcm, doa, None, None, want_weights=True, **SCENE_RTF)
    est = auto_stream(rt.SCENE_FS, rt.SCENE_N, sc["xs"], pcm, doa, SCENE_CFG, rtf=SCENE_RTF, want_weights=True)
    return dict(none=rt.scene_figures(none["w"][:, 0], sc), estimated=rt.scene_figures(est["w"][:, 0], sc), run=est)
