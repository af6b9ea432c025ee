"""Device-side cost of S MVDR look directions per frame (16 microphones, N = 1024), on device buffers:

  --mode sources   one mca_hip_mvdr_sources_frames_dev call with S directions on one context (this build)
  --mode separate  S mca_hip_mvdr_frames_dev calls on S contexts: what a user of a library without the sources call does.
                   Binds only the single-look entry points, so MCA_HIP_LIB may name the parent commit's library.
  --ab PARENT_LIB  both, alternating, --runs fresh processes each: the two ranges, their ratio and the per-kernel split

Each run prints one JSON line: ms per step (wall clock over --steps calls after --warmup, events off) and, from a second loop
with the library's HIP events on, the per-kernel milliseconds per step (analysis, solve, synthesis).
Usage: python tools/bench_mvdr_sources_dev.py --ab abtest/lib_parent.so [--streams 256] [--frames 64] [--sources 2] [--runs 5]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("k_mvdr_analyse", "k_mvdr_solve", "k_mvdr_synth")


class Separate:
    """S single-look contexts through the entry points every build has"""

    def __init__(self, fs, xs, N, streams, S):
        from mcarray_amd import _lib
        _lib._pin_single_hip_runtime()
        self.lib = lib = C.CDLL(_lib.LIB_PATH)
        lib.mca_hip_mvdr_create.argtypes = [C.POINTER(_lib.MvdrConfig), C.POINTER(C.c_void_p)]
        lib.mca_hip_mvdr_last_error.restype = C.c_char_p
        lib.mca_hip_mvdr_last_error.argtypes = [C.c_void_p]
        lib.mca_hip_mvdr_destroy.argtypes = [C.c_void_p]
        lib.mca_hip_mvdr_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mca_hip_mvdr_set_timing.argtypes = [C.c_void_p, C.c_int]
        lib.mca_hip_mvdr_get_timing.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        xyz = np.zeros((len(xs), 3))
        xyz[:, 0] = xs
        cfg = _lib.MvdrConfig()
        cfg.struct_size = C.sizeof(_lib.MvdrConfig)
        cfg.device, cfg.sample_rate, cfg.fft_size, cfg.n_mics = 0, fs, N, len(xs)
        cfg.mic_xyz = xyz.ctypes.data_as(_lib.c_dp)
        cfg.alpha, cfg.loading, cfg.max_streams = 0.95, 1e-3, streams
        self.ctx = []
        for _ in range(S):
            h = C.c_void_p()
            rc = lib.mca_hip_mvdr_create(C.byref(cfg), C.byref(h))
            if rc:
                raise RuntimeError("mca_hip_mvdr_create: %s" % lib.mca_hip_mvdr_last_error(None).decode())
            self.ctx.append(h)

    def step(self, pcm, F, doa, out, st):
        # doa [S][streams][F], out [S][streams][F hop]
        for s, h in enumerate(self.ctx):
            rc = self.lib.mca_hip_mvdr_frames_dev(h, pcm.data_ptr(), pcm.stride(0), pcm.stride(1), pcm.shape[0], F, doa[s].data_ptr(),
                                                  out[s].data_ptr(), None, st)
            if rc:
                raise RuntimeError(self.lib.mca_hip_mvdr_last_error(h).decode())

    def set_timing(self, on):
        for h in self.ctx:
            self.lib.mca_hip_mvdr_set_timing(h, int(on))

    def timing(self, kid):
        tot = 0.0
        for h in self.ctx:
            n, ms = C.c_int(0), C.c_double(0)
            self.lib.mca_hip_mvdr_get_timing(h, kid, C.byref(n), C.byref(ms))
            tot += ms.value
        return tot

    def close(self):
        for h in self.ctx:
            self.lib.mca_hip_mvdr_destroy(h)


class Sources:
    def __init__(self, fs, xs, N, streams, S):
        from mcarray_amd import api
        self.bf = api.MvdrBeamformer(fs, xs, N, max_streams=streams, max_sources=S)

    def step(self, pcm, F, doa, out, st):
        # doa [streams][F][S], out [streams][S][F hop]
        self.bf.process_sources_dev(pcm, F, doa, out_pcm=out, stream=st)

    def set_timing(self, on):
        self.bf.set_timing(on)

    def timing(self, kid):
        return self.bf.get_timing(kid)[1]

    def close(self):
        self.bf.close()


def run(a):
    import torch
    from mcarray_amd import synth
    fs, N = 48000, 1024
    hop = N // 2
    xs = [0.32 / a.mics * m for m in range(a.mics)] if a.mics != 16 else list(synth.ULA16)
    dev = torch.device("cuda:0")
    L = (a.frames + 1) * hop
    g = torch.Generator(device=dev); g.manual_seed(1234)
    pcm = (torch.randn((a.streams, a.mics, L), device=dev, generator=g) * 0.1).contiguous()
    look = torch.tensor([0.35, -0.6, 1.1, -0.1][:a.sources], device=dev, dtype=torch.float32)
    if a.mode == "sources":
        eng = Sources(fs, xs, N, a.streams, a.sources)
        doa = look[None, None, :].expand(a.streams, a.frames, a.sources).contiguous()
        out = torch.empty((a.streams, a.sources, a.frames * hop), device=dev, dtype=torch.float32)
    else:
        eng = Separate(fs, xs, N, a.streams, a.sources)
        doa = look[:, None, None].expand(a.sources, a.streams, a.frames).contiguous()
        out = torch.empty((a.sources, a.streams, a.frames * hop), device=dev, dtype=torch.float32)
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(a.warmup):
        eng.step(pcm, a.frames, doa, out, st)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        eng.step(pcm, a.frames, doa, out, st)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    eng.set_timing(True)
    for _ in range(a.steps):
        eng.step(pcm, a.frames, doa, out, st)
    torch.cuda.synchronize()
    res = dict(mode=a.mode, lib=os.environ.get("MCA_HIP_LIB", "default"), sources=a.sources,
               workload="%d streams x %d frames, %d mics, N=%d" % (a.streams, a.frames, a.mics, N), ms_per_step=dt * 1e3,
               checksum=float(out.double().abs().sum().item()))
    for kid, name in enumerate(KERNELS):
        res[name + "_ms"] = eng.timing(kid) / a.steps
    eng.close()
    print(json.dumps(res))


def ab(a):
    base = [sys.executable, os.path.abspath(__file__), "--streams", str(a.streams), "--frames", str(a.frames), "--mics", str(a.mics),
            "--sources", str(a.sources), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    runs = {"separate": [], "sources": []}
    for i in range(a.runs):
        for mode in ("separate", "sources"):
            env = dict(os.environ)
            env.pop("MCA_HIP_LIB", None)
            if mode == "separate":
                env["MCA_HIP_LIB"] = os.path.abspath(a.ab)
            r = subprocess.run(base + ["--mode", mode], env=env, capture_output=True, text=True, timeout=a.child_timeout)
            if r.returncode != 0:                       # nothing more is started on the GPU after a failed run
                sys.stdout.write(r.stdout + r.stderr)
                sys.exit("run %d (%s) ended with status %d" % (i, mode, r.returncode))
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            runs[mode].append(json.loads(line))
    ms = {m: [r["ms_per_step"] for r in v] for m, v in runs.items()}
    med = {m: float(np.median(v)) for m, v in ms.items()}
    summary = dict(workload=runs["sources"][0]["workload"], sources=a.sources, runs=a.runs,
                   separate_ms=[min(ms["separate"]), med["separate"], max(ms["separate"])],
                   sources_ms=[min(ms["sources"]), med["sources"], max(ms["sources"])],
                   ratio_of_medians=med["separate"] / med["sources"],
                   ranges_overlap=bool(max(ms["sources"]) >= min(ms["separate"])))
    for name in KERNELS:
        summary[name + "_ms"] = dict((m, float(np.median([r[name + "_ms"] for r in v]))) for m, v in runs.items())
    print("SUMMARY " + json.dumps(summary), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["sources", "separate"], default="sources")
    ap.add_argument("--ab", metavar="PARENT_LIB", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=120)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--mics", type=int, default=16)
    ap.add_argument("--sources", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.ab:
        ab(a)
    else:
        run(a)


if __name__ == "__main__":
    main()
