"""Bytes of the MVDR calls of this build against an older build of the library (the yardstick of a refactor of the solve kernels).
usage: python tools/compare_mvdr_builds.py PARENT_LIB

The same inputs go through PARENT_LIB and through mcarray_amd/libmcarray_hip.so, each in a fresh child process (MCA_HIP_LIB names
the library, as for the bench tools) under a time limit of its own; the second child is not started when the first one fails.  A
child binds only the entry points its library has, runs the cases below through the host-pointer calls and leaves one SHA-256 per
case over the spectra, the audio and the covariance read back (the host-layer cases: what they name).  The parent process requires equal digests of every case the older build ran
(exit code 1 otherwise) and never opens the GPU itself.

Cases (N = 64, fs = 16 kHz, 3 streams, two calls of 5 + 4 frames; stream 2 starts with digital silence): 3, 4, 6, 8, 11, 12, 15
and 16 microphones (both forms of every number of row slots) x 1 ... 4 look directions x null_gain 0 and 7.5 (two directions and
more) x no update weights, a weight per frame (zeros, fractions and ones) and a weight per frame and bin x post-filter off and on.
Then one call whose solve takes the pieced tail launch: 1000 streams x 8 frames, 16 microphones, 2 directions (516 workgroups: a
remainder of 4, in 2 pieces).  Then the paths of the host layer (host_layer_cases below) and the cuts the launch plans make under the
workspace cap (plan_cases)."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, N = 16000, 64
HOP, K = N // 2, N // 2 + 1
FRAME_WEIGHTS = (1.0, 0.5, 0.0, 0.0, 1.0, 0.25, 0.0, 1.0, 0.75)
CHILD_SECONDS = 240


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()


def load_lib():
    """(in a child) the library MCA_HIP_LIB names, bound to the entry points it has -> (api, np, has)"""
    import ctypes as C
    import numpy as np
    sys.path.insert(0, ROOT)
    from mcarray_amd import _lib, api
    _lib._pin_single_hip_runtime()
    probe = C.CDLL(_lib.LIB_PATH)
    _lib.SYMBOLS = [sym for sym in _lib.SYMBOLS if hasattr(probe, sym[0])]     # an older build: what it lacks stays unbound
    lib = _lib.load()
    return api, np, lambda name: hasattr(lib, name)


def child(out_path):
    api, np, has = load_lib()
    res = {}

    def run(name, bf, calls, streams):
        parts = []
        for pcm, doa, kw in calls:
            r = bf.process_sources(pcm, doa, **kw) if doa.ndim == 3 else bf.process(pcm, doa, want_spec=True, **kw)
            parts += [r["spec"], r["out"]]
        parts += [bf.covariance(a) for a in streams]
        bf.close()
        res[name] = digest(*parts)

    A, F1, F = 3, 5, 9
    for M in (3, 4, 6, 8, 11, 12, 15, 16):
        rng = np.random.default_rng(100 + M)
        xs = [0.3 / M * m for m in range(M)]
        pcm = rng.standard_normal((A, M, (F + 1) * HOP)).astype(np.float32)
        pcm[2, :, :3 * HOP] = 0.0
        cell = rng.choice(np.array([0.0, 0.0, 1.0, 1.0, 0.3, 0.8], dtype=np.float32), size=(A, F, K))
        frame = np.tile(np.asarray(FRAME_WEIGHTS, dtype=np.float32), (A, 1))
        frame[1] = frame[1, ::-1]
        for S in (1, 2, 3, 4):
            doa = rng.uniform(-1.3, 1.3, (A, F, S)).astype(np.float32)
            for gain in ((0.0,) if S == 1 else (0.0, 7.5)):
                for rule, upd in (("none", None), ("frame", frame), ("cell", cell)):
                    for pf in (False, True):
                        if (gain and not has("mca_hip_mvdr_set_null_gain")) or (pf and not has("mca_hip_mvdr_set_postfilter")) or \
                           (rule == "frame" and not has("mca_hip_mvdr_sources_frames_weighted_host")) or \
                           (rule == "cell" and not has("mca_hip_mvdr_sources_frames_masked_host")) or (S > 1 and not has("mca_hip_mvdr_sources_frames_host")):
                            continue
                        bf = api.MvdrBeamformer(FS, xs, N, max_streams=A, max_sources=S, null_gain=gain)
                        if pf:
                            bf.set_postfilter(True)
                        calls = []
                        for t0, t1 in ((0, F1), (F1, F)):
                            kw = {} if upd is None else {"update" if rule == "frame" else "update_mask": upd[:, t0:t1]}
                            calls.append((pcm[:, :, t0 * HOP:(t1 + 1) * HOP], doa[:, t0:t1] if S > 1 else doa[:, t0:t1, 0], kw))
                        run("M=%d S=%d gain=%g update=%s postfilter=%d" % (M, S, gain, rule, pf), bf, calls, range(A))
    if has("mca_hip_mvdr_sources_frames_host"):
        A, F, M, S = 1000, 8, 16, 2
        rng = np.random.default_rng(7)
        pcm = rng.standard_normal((A, M, (F + 1) * HOP)).astype(np.float32)
        doa = rng.uniform(-1.3, 1.3, (A, F, S)).astype(np.float32)
        bf = api.MvdrBeamformer(FS, [0.3 / M * m for m in range(M)], N, max_streams=A, max_sources=S)
        run("pieced tail launch: 1000 streams x 8 frames, M=16 S=2", bf, [(pcm, doa, {})], (0, 991, 992, 999))
    host_layer_cases(api, np, has, res)
    with open(out_path, "w") as f:
        json.dump(res, f)


def host_layer_cases(api, np, has, res):
    """the paths of the host layer beside the plain calls (the shapes above; 6 microphones, 2 look directions of 3 slots): the RTF
    call and its cut along the frames, the auto call, a change of max_sources under post-filter and RTF down to the state blob,
    the post-filter toggled between calls, the spectrum and a round of the tracks"""
    if not (has("mca_hip_mvdr_sources_frames_rtf_host") and has("mca_hip_mvdr_set_postfilter")):
        return
    A, F1, F, M, S = 3, 5, 9, 6, 2
    rng = np.random.default_rng(4242)
    xs = [0.3 / M * m for m in range(M)]
    pcm = rng.standard_normal((A, M, (F + 1) * HOP)).astype(np.float32)
    pcm[2, :, :3 * HOP] = 0.0
    doa = rng.uniform(-1.3, 1.3, (A, F, S)).astype(np.float32)
    um = rng.choice(np.array([0.0, 0.0, 1.0, 1.0, 0.3, 0.8], dtype=np.float32), size=(A, F, K))
    tm = rng.choice(np.array([0.0, 1.0, 1.0, 0.6], dtype=np.float32), size=(A, S, F, K))

    def new(max_sources=S, gain=0.0, pf=False, rtf=True):
        bf = api.MvdrBeamformer(FS, xs, N, max_streams=A, max_sources=max_sources, null_gain=gain, rtf_nulls=gain != 0.0)
        if pf:
            bf.set_postfilter(True)
        if rtf:
            bf.set_rtf(True)
        return bf

    def call(bf, t0, t1, parts, masks=True, **kw):
        if masks:
            kw.update(update_mask=um[:, t0:t1], target_mask=tm[:, :, t0:t1])
        r = bf.process_sources(pcm[:, :, t0 * HOP:(t1 + 1) * HOP], doa[:, t0:t1], **kw)
        parts += [r[key] for key in ("spec", "out", "update_mask", "target_mask") if key in r]

    def state(bf, parts, slots=S, rtf=True):
        for a in range(A):
            parts.append(bf.covariance(a))
            if rtf:
                for s in range(slots):
                    parts += list(bf.target_covariance(a, s))

    for name, cap in (("RTF call, update and target masks", None), ("RTF call cut into chunks of 2 frames", 2 * A * S * K * M * 8)):
        bf, parts = new(), []
        if cap:
            bf.set_rtf_workspace(cap)                          # 5 frames: 2 + 2 + 1, 4 frames: 2 + 2
        call(bf, 0, F1, parts)
        call(bf, F1, F, parts)
        state(bf, parts)
        bf.close()
        res[name] = digest(*parts)

    if has("mca_hip_mvdr_sources_frames_auto_host"):
        bf, parts = new(), []
        bf.set_mask_estimator(True)
        call(bf, 0, F1, parts, masks=False, estimate_masks=True)
        call(bf, F1, F, parts, masks=False, estimate_masks=True)
        state(bf, parts)
        bf.close()
        res["auto call, both masks handed back"] = digest(*parts)

    bf, parts = new(max_sources=2, gain=7.5, pf=True), []
    bf.set_max_sources(3)
    call(bf, 0, F1, parts)
    bf.set_max_sources(2)
    call(bf, F1, F, parts)
    state(bf, parts)
    parts.append(np.frombuffer(bf.state_save(), dtype=np.uint8))
    bf.close()
    res["set_max_sources 3, call, 2, call, state blob; post-filter, RTF, nulls"] = digest(*parts)

    bf, parts = new(rtf=False), []
    call(bf, 0, F1, parts, masks=False)
    bf.set_postfilter(True)
    call(bf, F1, F1 + 2, parts, masks=False)
    bf.set_postfilter(False)
    call(bf, F1 + 2, F, parts, masks=False)
    state(bf, parts, rtf=False)
    parts.append(np.frombuffer(bf.state_save(), dtype=np.uint8))
    bf.close()
    res["post-filter off, on, off between calls"] = digest(*parts)

    if has("mca_hip_mvdr_spectrum_host") and has("mca_hip_mvdr_tracks_configure"):
        bf, parts = new(), []
        call(bf, 0, F1, parts)
        bf.configure_spectrum(19, n_peaks=2)
        sp = bf.spectrum()
        parts += [sp["spectrum"], sp["peak_doa"], sp["peak_val"]]
        bf.configure_tracks(2, n_own=1)
        bf.seed_tracks(np.array([[0.4, -0.7], [-0.2, 0.9], [1.1, 0.1]], dtype=np.float32))
        for t0, t1 in ((F1, F1 + 2), (F1 + 2, F)):
            call(bf, t0, t1, parts)
            up = bf.update_tracks(want_spectrum=True)
            tr = bf.tracks()
            parts += [up["own_spectrum"], up["own_used"]] + [tr[key] for key in ("theta", "alive", "miss", "gen")]
        bf.close()
        res["spectrum, then tracks configured, seeded, updated and read"] = digest(*parts)
    plan_cases(api, np, has, res)


def plan_cases(api, np, has, res):
    """the cuts the launch plans decide under the workspace cap, which change no byte (4 microphones off the line, 3 streams, 2 look
    directions): an RTF call in chunks of unequal length, a map of 8 x 3 directions a stream a pass, and an update of the map-mode
    tracks with one own track a stream a pass -- each beside the same calls under the default cap, whose digest must be the same"""
    A, F, M, S = 3, 5, 4, 2
    rng = np.random.default_rng(2828)
    xyz = [[0.0, 0.0, 0.0], [0.07, 0.0, 0.0], [0.0, 0.07, 0.0], [0.02, 0.03, 0.06]]
    pcm = rng.standard_normal((A, M, (F + 1) * HOP)).astype(np.float32)
    doa = rng.uniform(-1.3, 1.3, (A, F, S)).astype(np.float32)
    um = rng.choice(np.array([0.0, 1.0, 1.0, 0.3], dtype=np.float32), size=(A, F, K))
    tm = rng.choice(np.array([0.0, 1.0, 1.0, 0.6], dtype=np.float32), size=(A, S, F, K))

    def rtf_call(bf, parts):
        r = bf.process_sources(pcm, doa, update_mask=um, target_mask=tm)
        parts += [r["spec"], r["out"]] + [bf.covariance(a) for a in range(A)]
        for a in range(A):
            for s in range(S):
                parts += list(bf.target_covariance(a, s))

    digests = {}
    for cut in (False, True):
        bf, parts = api.MvdrBeamformer(FS, xyz, N, max_streams=A, max_sources=S), []
        bf.set_rtf(True)
        if cut:
            bf.set_rtf_workspace(2 * A * S * K * M * 8)         # room for 2 of the 5 frames: chunks of 2, 2 and 1
        rtf_call(bf, parts)
        bf.close()
        digests["rtf", cut] = digest(*parts)
    res["plan: RTF call of 5 frames, M=4, whole"] = digests["rtf", False]
    res["plan: RTF call of 5 frames, M=4, cut into 2 + 2 + 1"] = digests["rtf", True]
    assert digests["rtf", False] == digests["rtf", True], "the cut of an RTF call changed bytes"
    if not (has("mca_hip_mvdr_map_host") and has("mca_hip_mvdr_tracks_update_map_host")):
        return
    for cut in (False, True):
        bf, parts = api.MvdrBeamformer(FS, xyz, N, max_streams=A, max_sources=S, geometry="xyz"), []
        bf.set_rtf(True)
        rtf_call(bf, parts)
        bf.configure_spectrum(8, 1, 30)
        bf.map_configure(8, 3, 0.0, 1.0, 1, 30, n_peaks=2)      # 24 directions: 64 lanes, one chunk of bins: 256 floats of partial sums a stream
        if cut:
            bf.set_rtf_workspace(256 * 4)                       # one stream a pass
        mp = bf.map()
        parts += [mp[key] for key in ("map", "peak_az", "peak_el", "peak_val")]
        res["plan: map of 8 x 3 directions, %s" % ("a stream a pass" if cut else "one pass")] = digests["map", cut] = digest(*parts)
        bf.configure_tracks(2, n_own=1)
        bf.configure_tracks_map(0.6, 0.3)
        bf.seed_tracks_map(np.array([[0.4, -0.7], [-0.2, 0.9], [1.1, 0.1]], dtype=np.float32), np.array([[0.2, 0.5], [0.7, 0.1], [0.4, 0.4]], dtype=np.float32))
        if cut:
            bf.set_rtf_workspace(832 * 4)                       # u, flags and partial sums of one own track: 832 floats a stream: one stream a pass (the map: 3)
        up = bf.update_tracks_map(want_map=True)
        tr = bf.tracks_map()
        parts += [up["own_map"], up["own_used"]] + [tr[key] for key in ("theta", "eps", "alive", "miss", "gen")]
        bf.close()
        res["plan: map-mode tracks update, one own track, %s" % ("a stream a pass" if cut else "one pass")] = digests["tracks", cut] = digest(*parts)
    assert digests["map", False] == digests["map", True] and digests["tracks", False] == digests["tracks", True], "the passes of a map call changed bytes"


def run_both(script, parent_lib, seconds=CHILD_SECONDS):
    """`script --child OUT` once per library, the parent's first: each a fresh process under its own time limit, the second not
    started when the first fails -> the two dicts of digests (parent's, this build's).  This process never opens the GPU."""
    got = []
    with tempfile.TemporaryDirectory() as tmp:
        for tag, lib in (("parent", os.path.abspath(parent_lib)), ("this", None)):
            env = dict(os.environ)
            env.pop("MCA_HIP_LIB", None)
            if lib:
                env["MCA_HIP_LIB"] = lib
            out = os.path.join(tmp, tag + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(script), "--child", out], env=env).returncode
            if rc != 0:
                sys.exit("%s build (%s): the child ended with %d; nothing further is started" % (tag, lib or "default", rc))
            got.append(json.load(open(out)))
    return got


def report(par, new, what, parent_lib):
    """prints a line per case the older build ran -> the exit code: 1 on a case this build lacks or on a differing digest"""
    missing = [name for name in par if name not in new]
    if missing:
        print("this build did not run %d of the parent's %d cases: %s ..." % (len(missing), len(par), missing[0]))
        return 1
    bad = [name for name in par if par[name] != new[name]]
    for name in par:
        print("%s  %s  %s" % ("DIFFERENT" if name in bad else "equal    ", new[name][:16], name))
    print("%d cases, %d with different bytes (%s) against %s" % (len(par), len(bad), what, parent_lib))
    return 1 if bad else 0


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    if len(sys.argv) != 2 or not os.path.exists(sys.argv[1]):
        sys.exit(__doc__)
    par, new = run_both(__file__, sys.argv[1])
    sys.exit(report(par, new, "spectra, audio, covariance", sys.argv[1]))


if __name__ == "__main__":
    main()
