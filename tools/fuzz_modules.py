"""Randomised parity sweep of the 2-channel masking module, the MVDR beamformer and its sources call with soft nulls against the CPU oracle, and of the MVDR auto
call (estimated masks) against the call fed its masks, and of the RTF call under a null gain (nulls at the estimated vectors) against its exact
points, and of the sources call of an XYZ context (full microphone geometry) against its twin (a one-off check like
tools/fuzz_parity.py): random frame lengths, methods / algorithms, channel counts, geometries, memories, loadings, chunked calls.
usage (GPU box): python tools/fuzz_modules.py [cases] [seed]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcarray_amd import api, synth  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import mvdr_nulls_twin as nt  # noqa: E402
import mvdr_geometry_twin as gmt  # noqa: E402


def mask_case(rng):
    fs, N = [(8000, 512), (16000, 1024), (48000, 2048), (44100, 2048), (16000, 1024), (96000, 4096)][int(rng.integers(0, 6))]
    method = int(rng.choice([api.FACTOR, api.RELATIVE, api.FULL, api.NOISY]))
    alg = int(rng.integers(0, 3))
    hop, F = N // 2, int(rng.integers(2, 90))
    d = float(rng.uniform(0.05, 0.2))
    n = (F + 1) * hop
    src = rng.standard_normal(n) * 0.1
    nl = float(rng.choice([0.003, 0.03]))
    left = src + rng.standard_normal(n) * nl
    right = np.roll(src, int(rng.integers(0, 3))) * float(rng.uniform(0.5, 1.0)) + rng.standard_normal(n) * nl
    env = np.repeat(rng.choice([1.0, 0.2, 0.05, 0.6], F + 1), hop)
    pcm = np.stack([left * env, right * env]).astype(np.float32)
    flo, fhi = float(rng.uniform(100, 600)), float(min(rng.uniform(3000, 7000), 0.45 * fs))
    tag = "mask fs=%d N=%d method=%d alg=%d F=%d" % (fs, N, method, alg, F)
    m = api.FastBinauralMasking(fs, d, flo, fhi, method, alg, fft_size=N)
    cut = int(rng.integers(1, F)) if F > 2 and rng.integers(0, 2) else 0
    if cut:
        oa, da = m.process(pcm[:, :(cut + 1) * hop]); ob, db = m.process(pcm[:, cut * hop:])
        out, dec = np.concatenate([oa[0], ob[0]], axis=1), np.concatenate([da[0], db[0]], axis=0)
    else:
        o_, d_ = m.process(pcm); out, dec = o_[0], d_[0]
    o = po.Masking(fs, N, d, flo, fhi, method, alg)
    ol, orr = o.stream(pcm[0].astype(np.float64), pcm[1].astype(np.float64))
    o2 = po.Masking(fs, N, d, flo, fhi, method, alg)
    X = po.stft_frames(pcm.astype(np.float64), N)
    odec = np.array([o2.process(X[t, 0], X[t, 1])[2] for t in range(F)])
    ndiff = int((dec != odec).sum())
    ref = np.stack([ol, orr])
    err = np.abs(out - ref).max() / (np.abs(ref).max() + 1e-30)
    ok = ndiff <= 2 and (ndiff > 0 or err <= 2e-5)
    m.close()
    return ok, "%s cut=%d decisions differ %d audio err %.1e" % (tag, cut, ndiff, err)


def mvdr_case(rng):
    fs, N = [(8000, 256), (16000, 512), (48000, 1024), (48000, 1024), (96000, 2048)][int(rng.integers(0, 5))]
    M = int(rng.integers(2, 17))
    xs = np.sort(rng.uniform(0, 0.03 * M, M))
    F, A = int(rng.integers(1, 60)), int(rng.integers(1, 4))
    alpha, loading = float(rng.choice([0.0, 0.5, 0.9, 0.95, 0.99])), float(rng.choice([1e-3, 1e-2, 1e-1]))
    hop = N // 2
    pcm = np.stack([synth.noise_source_stream(xs, rng.uniform(-1.3, 1.3), fs, (F + 1) * hop, int(rng.integers(1, 1 << 30)))
                    + synth.noise_source_stream(xs, rng.uniform(-1.3, 1.3), fs, (F + 1) * hop, int(rng.integers(1, 1 << 30)), snr_db=50)
                    for _ in range(A)]).astype(np.float32)
    doa = rng.uniform(-1.4, 1.4, (A, F)).astype(np.float32)
    tag = "mvdr fs=%d N=%d M=%d A=%d F=%d alpha=%.2f loading=%.0e" % (fs, N, M, A, F, alpha, loading)
    bf = api.MvdrBeamformer(fs, xs, N, alpha, loading, max_streams=A)
    cut = int(rng.integers(1, F)) if F > 2 and rng.integers(0, 2) else 0
    if cut:
        ra = bf.process(pcm[:, :, :(cut + 1) * hop], doa[:, :cut], want_spec=True)
        rb = bf.process(pcm[:, :, cut * hop:], doa[:, cut:], want_spec=True)
        out, spec = np.concatenate([ra["out"], rb["out"]], axis=1), np.concatenate([ra["spec"], rb["spec"]], axis=1)
    else:
        r = bf.process(pcm, doa, want_spec=True); out, spec = r["out"], r["spec"]
    worst = 0.0
    for a in range(A):
        o = po.MVDR(fs, N, xs, alpha, loading).stream(pcm[a].astype(np.float64), doa[a].astype(np.float64), want_spec=True)
        sp = o["spec"][:, 0::2] + 1j * o["spec"][:, 1::2]
        worst = max(worst, np.abs(spec[a] - sp).max() / np.abs(sp).max(), np.abs(out[a] - o["out"]).max() / np.abs(o["out"]).max())
    bf.close()
    return worst <= 5e-4, "%s cut=%d worst rel err %.1e" % (tag, cut, worst)


def mvdr_nulls_case(rng):
    """the sources call with soft nulls at the other look directions against its float64 twin (tests/mvdr_nulls_twin.py):
    random geometry, frame size, S, gain and directions, now and then with two directions equal"""
    fs, N = [(8000, 256), (16000, 512), (48000, 1024)][int(rng.integers(0, 3))]
    M, S = int(rng.integers(2, 17)), int(rng.integers(2, 5))
    xs = np.sort(rng.uniform(0, 0.03 * M, M))
    F, A = int(rng.integers(1, 25)), int(rng.integers(1, 4))
    alpha, loading = float(rng.choice([0.0, 0.5, 0.9, 0.95, 0.99])), float(rng.choice([1e-3, 1e-2, 1e-1]))
    gain = float(rng.choice([0.1, 1.0, 10.0, 100.0, rng.uniform(0.0, 100.0)]))
    hop = N // 2
    pcm = np.stack([synth.noise_source_stream(xs, rng.uniform(-1.3, 1.3), fs, (F + 1) * hop, int(rng.integers(1, 1 << 30)))
                    + synth.noise_source_stream(xs, rng.uniform(-1.3, 1.3), fs, (F + 1) * hop, int(rng.integers(1, 1 << 30)), snr_db=50)
                    for _ in range(A)]).astype(np.float32)
    doa = rng.uniform(-1.4, 1.4, (A, F, S)).astype(np.float32)
    same = bool(rng.integers(0, 3) == 0)
    if same:
        doa[:, :, S - 1] = doa[:, :, 0]
    tag = "mvdr nulls fs=%d N=%d M=%d S=%d A=%d F=%d alpha=%.2f loading=%.0e gain=%.3g%s" % (fs, N, M, S, A, F, alpha, loading, gain,
                                                                                            " coincident" if same else "")
    bf = api.MvdrBeamformer(fs, xs, N, alpha, loading, max_streams=A, max_sources=S, null_gain=gain)
    cut = int(rng.integers(1, F)) if F > 2 and rng.integers(0, 2) else 0
    if cut:
        ra = bf.process_sources(pcm[:, :, :(cut + 1) * hop], doa[:, :cut])
        rb = bf.process_sources(pcm[:, :, cut * hop:], doa[:, cut:])
        out, spec = np.concatenate([ra["out"], rb["out"]], axis=2), np.concatenate([ra["spec"], rb["spec"]], axis=2)
    else:
        r = bf.process_sources(pcm, doa); out, spec = r["out"], r["spec"]
    worst = 0.0
    for a in range(A):
        tw = nt.mvdr_nulls_stream(fs, N, xs, pcm[a].astype(np.float64), doa[a], gain, alpha, loading)
        for s_ in range(S):
            worst = max(worst, np.abs(spec[a, s_] - tw["spec"][s_]).max() / np.abs(tw["spec"][s_]).max(),
                        np.abs(out[a, s_] - tw["out"][s_]).max() / np.abs(tw["out"][s_]).max())
    bf.close()
    return bool(np.isfinite(worst) and worst <= 5e-4), "%s cut=%d worst rel err %.1e" % (tag, cut, worst)


def mvdr_geometry_case(rng):
    """the sources call of an XYZ context (mca_hip_mvdr_set_geometry) against the float64 twin (tests/mvdr_geometry_twin.py): random planar
    and 3-D arrays, a random elevation, look directions over the whole circle and up to a turn beyond it, with and without nulls"""
    fs, N = [(8000, 256), (16000, 512), (48000, 1024)][int(rng.integers(0, 3))]
    M, S = int(rng.integers(2, 17)), int(rng.integers(1, 5))
    kind = ["planar", "3d", "uca"][int(rng.integers(0, 3))]
    xyz = synth.uca(M, float(rng.uniform(0.02, 0.1))) if kind == "uca" else rng.uniform(-0.015 * M, 0.015 * M, (M, 3))
    if kind == "planar":
        xyz[:, 2] = 0.0
    el = float(rng.choice([0.0, rng.uniform(-np.pi / 2, np.pi / 2)]))
    F, A = int(rng.integers(1, 17)), int(rng.integers(1, 4))
    alpha, loading = float(rng.choice([0.0, 0.5, 0.9, 0.95, 0.99])), float(rng.choice([1e-3, 1e-2, 1e-1]))
    gain = 0.0 if S == 1 else float(rng.choice([0.0, 1.0, 10.0, 100.0]))
    hop = N // 2
    pcm = np.stack([synth.noise_source_stream_xyz(xyz, rng.uniform(-np.pi, np.pi), fs, (F + 1) * hop, int(rng.integers(1, 1 << 30)), elevation=el)
                    + synth.noise_source_stream_xyz(xyz, rng.uniform(-np.pi, np.pi), fs, (F + 1) * hop, int(rng.integers(1, 1 << 30)), snr_db=50, elevation=el)
                    for _ in range(A)]).astype(np.float32)
    doa = rng.uniform(-3 * np.pi, 3 * np.pi, (A, F, S)).astype(np.float32)
    tag = "mvdr xyz %s fs=%d N=%d M=%d S=%d A=%d F=%d el=%.2f alpha=%.2f loading=%.0e gain=%.3g" % (kind, fs, N, M, S, A, F, el, alpha, loading, gain)
    bf = api.MvdrBeamformer(fs, xyz, N, alpha, loading, max_streams=A, max_sources=S, null_gain=gain, geometry="xyz", elevation_rad=el)
    r = bf.process_sources(pcm, doa)
    worst = 0.0
    for a in range(A):
        with gmt.xyz_mode(el):
            tw = nt.mvdr_nulls_stream(fs, N, xyz, pcm[a].astype(np.float64), doa[a], gain, alpha, loading)
        for s_ in range(S):
            worst = max(worst, np.abs(r["spec"][a, s_] - tw["spec"][s_]).max() / np.abs(tw["spec"][s_]).max(),
                        np.abs(r["out"][a, s_] - tw["out"][s_]).max() / np.abs(tw["out"][s_]).max())
    bf.close()
    return bool(np.isfinite(worst) and worst <= 5e-4), "%s worst rel err %.1e" % (tag, worst)


def mvdr_auto_case(rng):
    """the auto call (masks estimated from the spectra, mca_hip_mvdr_sources_frames_auto_*) against the RTF or the masked call fed
    the masks it returned, bit for bit, and the masks against their own definition: random geometry, frame size, S, band,
    thresholds and number of protected directions"""
    fs, N = [(8000, 256), (16000, 512), (48000, 1024)][int(rng.integers(0, 3))]
    M, S = int(rng.integers(2, 17)), int(rng.integers(1, 5))
    xs = np.sort(rng.uniform(0, 0.03 * M, M))
    F, A, rtf = int(rng.integers(1, 25)), int(rng.integers(1, 4)), bool(rng.integers(0, 2))
    hop = N // 2
    pcm = np.stack([synth.noise_source_stream(xs, rng.uniform(-1.3, 1.3), fs, (F + 1) * hop, int(rng.integers(1, 1 << 30)))
                    + synth.noise_source_stream(xs, rng.uniform(-1.3, 1.3), fs, (F + 1) * hop, int(rng.integers(1, 1 << 30)), snr_db=50)
                    for _ in range(A)]).astype(np.float32)
    doa = rng.uniform(-1.4, 1.4, (A, F, S)).astype(np.float32)
    lo = float(rng.uniform(0.0, 0.5))
    cfg = dict(bin_lo=int(rng.integers(0, 9)), bin_hi=N // 2 - int(rng.integers(0, 9)), coherence_lo=lo, coherence_hi=lo + float(rng.uniform(0.002, 0.5)),
               n_protected=int(rng.integers(0, 5)))
    tag = "mvdr auto fs=%d N=%d M=%d S=%d A=%d F=%d rtf=%d %s" % (fs, N, M, S, A, F, rtf, cfg)
    res = []
    for est in (True, False):
        bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S)
        if rtf:
            bf.set_rtf(True)
        if est:
            bf.set_mask_estimator(True, **cfg)
            res.append(bf.process_sources(pcm, doa, estimate_masks=True))
        else:
            kw = dict(update_mask=res[0]["update_mask"], **(dict(target_mask=res[0]["target_mask"]) if rtf else {}))
            res.append(bf.process_sources(pcm, doa, **kw))
        res[-1]["blob"] = bf.state_save()
        bf.close()
    um, tm = res[0]["update_mask"], res[0]["target_mask"]
    P = S if cfg["n_protected"] == 0 or cfg["n_protected"] > S else cfg["n_protected"]
    ok = bool(np.array_equal(res[0]["spec"].view(np.float32), res[1]["spec"].view(np.float32)) and np.array_equal(res[0]["out"], res[1]["out"])
              and res[0]["blob"] == res[1]["blob"] and np.all((tm >= 0) & (tm <= 1)) and np.all((tm > 0).sum(axis=1) <= 1)
              and np.array_equal(um, np.float32(1) - tm[:, :P].max(axis=1)) and not tm[..., :cfg["bin_lo"]].any() and not tm[..., cfg["bin_hi"] + 1:].any())
    return ok, "%s assigned %.0f %%" % (tag, 100.0 * float((tm > 0).any(axis=1).mean()))


def mvdr_rtf_nulls_case(rng):
    """the RTF call under a null gain (mca_hip_mvdr_set_rtf_nulls) at its exact points: with a target mask of zeros on fresh state the
    bytes of the masked call under the same update mask and gain; with random target masks the bytes do not depend on how the stream
    is cut, the covariances are those of gain 0, and the gain moves the output; random geometry, frame size, S, gain and masks"""
    fs, N = [(8000, 256), (16000, 512), (48000, 1024)][int(rng.integers(0, 3))]
    M, S = int(rng.integers(2, 17)), int(rng.integers(2, 5))
    xs = np.sort(rng.uniform(0, 0.03 * M, M))
    F, A = int(rng.integers(2, 25)), int(rng.integers(1, 4))
    gain = float(rng.choice([0.1, 1.0, 10.0, 100.0, 1000.0, rng.uniform(0.0, 100.0)]))
    hop, K = N // 2, N // 2 + 1
    pcm = np.stack([synth.noise_source_stream(xs, rng.uniform(-1.3, 1.3), fs, (F + 1) * hop, int(rng.integers(1, 1 << 30)))
                    + synth.noise_source_stream(xs, rng.uniform(-1.3, 1.3), fs, (F + 1) * hop, int(rng.integers(1, 1 << 30)), snr_db=50)
                    for _ in range(A)]).astype(np.float32)
    doa = rng.uniform(-1.4, 1.4, (A, F, S)).astype(np.float32)
    upd = rng.choice(np.array([0, 1, 1, .5], dtype=np.float32), size=(A, F, K))
    tm = rng.choice(np.array([0, 0, 1, .5], dtype=np.float32), size=(A, S, F, K))
    pf = bool(rng.integers(0, 2))
    tag = "mvdr rtf nulls fs=%d N=%d M=%d S=%d A=%d F=%d gain=%.3g pf=%d" % (fs, N, M, S, A, F, gain, pf)

    def run(g, rtf, tmask, cut=0):
        bf = api.MvdrBeamformer(fs, xs, N, max_streams=A, max_sources=S, null_gain=g, rtf_nulls=True)
        if pf:
            bf.set_postfilter(True)
        if rtf:
            bf.set_rtf(True, iterations=int(1 + M % 4), ref_mic=int(M // 2))
        kw = (lambda t0, t1: dict(target_mask=np.ascontiguousarray(tmask[:, :, t0:t1]))) if rtf else (lambda t0, t1: {})
        rs = [bf.process_sources(pcm[:, :, t0 * hop:(t1 + 1) * hop].copy(), doa[:, t0:t1].copy(), update_mask=np.ascontiguousarray(upd[:, t0:t1]), **kw(t0, t1))
              for t0, t1 in ([(0, cut), (cut, F)] if cut else [(0, F)])]
        cov = [bf.covariance(a) for a in range(A)]
        bf.close()
        return np.concatenate([r["spec"] for r in rs], axis=2), np.concatenate([r["out"] for r in rs], axis=2), cov

    def same(p, q):
        return bool(np.array_equal(p[0].view(np.float32), q[0].view(np.float32), equal_nan=True) and np.array_equal(p[1], q[1], equal_nan=True)
                    and all(np.array_equal(u, v) for u, v in zip(p[2], q[2])))

    geometric = same(run(gain, True, np.zeros_like(tm)), run(gain, False, None))
    whole, plain = run(gain, True, tm), run(0.0, True, tm)
    cut = same(run(gain, True, tm, int(rng.integers(1, F))), whole)
    state = all(np.array_equal(u, v) for u, v in zip(whole[2], plain[2]))
    moved = gain == 0.0 or not np.array_equal(whole[0], plain[0])
    ok = geometric and cut and state and moved and bool(np.isfinite(whole[1]).all())
    return ok, "%s geometric plane %d cut %d state %d moved %d" % (tag, geometric, cut, state, moved)


def main(cases, seed):
    rng = np.random.default_rng(seed)
    bad = 0
    for case in range(cases):
        for fn in (mask_case, mvdr_case, mvdr_nulls_case, mvdr_auto_case, mvdr_rtf_nulls_case, mvdr_geometry_case):
            try:
                ok, msg = fn(rng)
            except api.MCArrayHipError as e:
                ok, msg = False, "%s raised %s" % (fn.__name__, e)
            print(("ok   " if ok else "FAIL ") + "case %d: %s" % (case, msg), flush=True)
            bad += 0 if ok else 1
    print("%d cases x 6, %d failures" % (cases, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 40, int(sys.argv[2]) if len(sys.argv) > 2 else 0))
