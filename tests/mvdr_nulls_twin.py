"""float64 twin of the MVDR call with soft nulls at the other look directions (include/mcarray_hip.h, mca_hip_mvdr_set_null_gain).

A restatement of the DENSE definition, independent of the kernel's algebra: per stream, bin and frame, with PhiL the loaded
covariance of oracle.np_twin.mvdr_stream, d_s the steering vectors of the frame's S look directions and g = null_gain,

    p_r   = 1 / (d_r^H PhiL^-1 d_r)
    Phi_s = PhiL + g * sum_{r != s} p_r d_r d_r^H
    w_s   = Phi_s^-1 d_s / (d_s^H Phi_s^-1 d_s),    Y_s = w_s^H x

through numpy.linalg.solve on the M x M matrices Phi_s, batched over the bins.  A bin in digital silence (trace <= 1e-30) keeps
w = d / M.  gram_route() is the form the kernel uses (Cholesky factor, Gram matrix of the whitened steering vectors, one small
solve per direction), in float64, for the test that the two agree.  scene() and drifting_doa() are the inputs of
tests/test_gpu_mvdr_sources.py."""
import numpy as np

from mcarray_amd import synth
from oracle import np_twin

OFFSETS = np.array([0.0, -0.5, 0.45, -0.8])           # look direction of source s relative to source 0 (radians)


def scene(xs, fs, N, F, a):
    n = (F + 1) * N // 2
    return (synth.noise_source_stream(xs, np.deg2rad(20.0 - 30 * a), fs, n, 5 + a)
            + synth.noise_source_stream(xs, np.deg2rad(-50.0 + 40 * a), fs, n, 15 + a, snr_db=60)).astype(np.float32)


def drifting_doa(A, F, S):
    """[A][F][S]: drifts per frame, differs per source and per stream"""
    return (np.deg2rad(20.0 - 30 * np.arange(A))[:, None, None] + 0.01 * np.arange(F)[None, :, None]
            + OFFSETS[None, None, :S]).astype(np.float32)


def steering(fs, N, xs, doa):
    """doa [S] -> d [K][S][M], the convention of np_twin.mvdr_stream (Beamformer.cpp:59)"""
    x = np.asarray(xs, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, 0]
    k = np.arange(N // 2 + 1, dtype=np.float64)
    slope = 2 * np.pi * fs / N / np_twin.C_SOUND * x[None, :] * np.cos(np.asarray(doa, dtype=np.float64)[:, None] + np.pi / 2)
    return np.exp(-1j * k[:, None, None] * slope[None, :, :])


def null_weights(PL, d, null_gain):
    """PL [K][M][M] loaded covariances, d [K][S][M] -> w [K][S][M] by the dense definition"""
    K, S, M = d.shape
    dT = np.swapaxes(d, 1, 2)                                              # [K][M][S]
    g0 = np.linalg.solve(PL, dT)                                           # PhiL^-1 d_r
    p = 1.0 / np.real(np.einsum("krm,kmr->kr", np.conj(d), g0))           # [K][S]
    w = np.empty((K, S, M), dtype=np.complex128)
    for s in range(S):
        Phi_s = PL.copy()
        for r in range(S):
            if r != s:
                Phi_s = Phi_s + (null_gain * p[:, r])[:, None, None] * d[:, r, :, None] * np.conj(d[:, r, None, :])
        h = np.linalg.solve(Phi_s, d[:, s, :, None])[:, :, 0]
        w[:, s] = h / np.einsum("km,km->k", np.conj(d[:, s]), h)[:, None]
    return w


def gram_route(PL, d, x, null_gain):
    """the kernel's form in float64: PL [K][M][M], d [K][S][M], x [K][M] -> Y [K][S].  U = L^-1 [d_0 ...], v = L^-1 x, G = U^H U,
    b = U^H v; per direction s with R the others: (g G_RR + diag G_RR) q = g G_Rs, Y_s = (b_s - q^H b_R) / (G_ss - q^H G_Rs)"""
    K, S, M = d.shape
    L = np.linalg.cholesky(PL)
    U = np.linalg.solve(L, np.swapaxes(d, 1, 2))                           # [K][M][S]
    v = np.linalg.solve(L, x[:, :, None])[:, :, 0]
    G = np.einsum("kms,kmr->ksr", np.conj(U), U)
    b = np.einsum("kms,km->ks", np.conj(U), v)
    Y = np.empty((K, S), dtype=np.complex128)
    for s in range(S):
        R = [r for r in range(S) if r != s]
        if not R:
            Y[:, s] = b[:, s] / np.real(G[:, s, s])
            continue
        GRR = G[:, R][:, :, R]
        A = null_gain * GRR + np.real(np.einsum("krr->kr", GRR))[:, :, None] * np.eye(len(R))
        q = np.linalg.solve(A, null_gain * G[:, R, s][:, :, None])[:, :, 0]
        Y[:, s] = (b[:, s] - np.einsum("kr,kr->k", np.conj(q), b[:, R])) / (G[:, s, s] - np.einsum("kr,kr->k", np.conj(q), G[:, R, s]))
    return Y


def mvdr_nulls_stream(fs, N, xs, pcm, doa_rad, null_gain, alpha=0.95, loading=1e-3, state=None, want_weights=False):
    """pcm [M][(F+1)*hop]; doa_rad [F][S].  state: the dict a former call returned (its covariance and overlap-add tails are
    continued) or None for a fresh stream.  Returns dict(out [S][F*hop], spec [S][F][K] complex, phi [K][M][M], tail [S][hop],
    and w [F][S][K][M] on request)."""
    X = np_twin.stft_frames(pcm, N)                                        # complex [F][M][K]
    F, M, K = X.shape
    hop = N // 2
    doa = np.asarray(doa_rad, dtype=np.float64)
    S = doa.shape[1]
    Phi = np.zeros((K, M, M), dtype=np.complex128) if state is None else state["phi"].copy()
    tail = np.zeros((S, hop)) if state is None else state["tail"].copy()
    spec = np.zeros((S, F, K), dtype=np.complex128)
    out = np.zeros((S, F * hop))
    W = np.zeros((F, S, K, M), dtype=np.complex128) if want_weights else None
    eye = np.eye(M)
    for t in range(F):
        Xc = X[t].T                                                        # [K][M]
        d = steering(fs, N, xs, doa[t])
        Phi = alpha * Phi + (1 - alpha) * Xc[:, :, None] * np.conj(Xc[:, None, :])
        tr = np.real(np.trace(Phi, axis1=1, axis2=2))
        live = tr > 1e-30
        PL = np.where(live[:, None, None], Phi + (loading * tr / M)[:, None, None] * eye, eye)
        w = null_weights(PL, d, null_gain)
        w[~live] = d[~live] / M
        spec[:, t] = np.einsum("ksm,km->sk", np.conj(w), Xc)
        if want_weights:
            W[t] = np.swapaxes(w, 0, 1)
        y = np_twin.irfft_ccs(spec[:, t], N)
        out[:, t * hop:(t + 1) * hop] = tail + y[:, :hop]
        tail = y[:, hop:]
    r = dict(out=out, spec=spec, phi=Phi, tail=tail)
    if want_weights:
        r["w"] = W
    return r
