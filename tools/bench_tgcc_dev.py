"""Device-side throughput of the time-domain 2-microphone localiser (mca_hip_tgcc_frames_dev) on device buffers:
1024 streams x 32 frames at (44.1 kHz, 0.086 m), (48 kHz, 0.089 m) and (16 kHz, 0.086 m), gate on (the reference).

  python tools/bench_tgcc_dev.py              frames/s (device events, after warm-up), achieved FP64 FLOP/s and HBM bytes
                                              from the shapes, the numpy restatement's frames/s on one CPU core, then the
                                              kernel times of a separate rocprofv3 --kernel-trace --stats run of this tool
  python tools/bench_tgcc_dev.py --no-prof    without the rocprofv3 run
  python tools/bench_tgcc_dev.py --inner      the timed loop only (what the rocprofv3 run executes)

Peaks used for the shares (not measured here): FP64 vector 78.6 TFLOP/s, the figure of AMD's public MI355X datasheet
(256 CUs x 2.4 GHz x 128 FP64 FLOP per CU and clock); HBM 8.0 TB/s datasheet, 6.29 TB/s measured copy rate.
"""
import csv
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

CONFIGS = [(44100, 0.086), (48000, 0.089), (16000, 0.086)]
A, F = 1024, 32
FP64_PEAK = 78.6e12
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def work_model(W, nd):
    """per frame: FP64 FLOP the closed form needs (the 4nd-1 body lags, the tails, the channel statistics) and the FLOP the
    kernel issues (lags padded to 16 per group, W rounded up to 8); HBM bytes read and written."""
    nl = 4 * nd - 1
    tails = 0
    for i in range(nd):
        for n in range(2 * nd + 1):
            tau = n + 2 * i - 2 * nd
            tails += (W - 1 - max(tau, 0)) - min(W - 1 - i, W - 1 - nd + i - tau)
    stats = 2 * 3 * W + 2 * 8 * W                     # sums, then centred sums and energies, both channels
    useful = 2 * nl * W + 2 * tails + stats
    issued = 2 * ((nl + 15) // 16 * 16) * ((W + 7) // 8 * 8) + 2 * tails + stats
    pcm_read = 2 * W * 4                               # both channels of the frame (half of it shared with the next frame)
    written = 6 * 8 * 2 + 4 * 4 + 1                    # per-frame results (written, read by the gate kernel), outputs
    return useful, issued, pcm_read, written


def timed(fs, d, iters):
    import torch
    from mcarray_amd import api, _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    m = api.TemporalGCCBinauralLocalisation(fs, [0.0, d], use_power_floor=True, max_arrays=A)
    W, hop, nd = m.W, m.hop, m.nd
    L = (F - 1) * hop + W
    g = torch.Generator(device=dev).manual_seed(7)
    x = (torch.randn(A, 2, L, device=dev, generator=g) * 1000).round().contiguous()
    doa, prob, power = (torch.empty(A, F, device=dev) for _ in range(3))
    voiced = torch.empty(A, F, dtype=torch.uint8, device=dev)
    k = torch.empty(A, F, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def call():
        rc = lib.mca_hip_tgcc_frames_dev(m.h, C.c_void_p(x.data_ptr()), 2 * L, L, A, F, C.c_void_p(doa.data_ptr()),
                                         C.c_void_p(prob.data_ptr()), C.c_void_p(voiced.data_ptr()), C.c_void_p(power.data_ptr()),
                                         C.c_void_p(k.data_ptr()), None, C.c_void_p(st))
        assert rc == 0, lib.mca_hip_tgcc_last_error(m.h)
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    dt = e0.elapsed_time(e1) / 1e3 / iters
    m.close()
    return W, hop, nd, dt


def twin_rate(fs, d, frames=4):
    """frames/s of tests/tgcc_twin.py's closed form on one CPU core (context only)."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tgcc_twin as tt
    W, hop, nd = tt.geometry(fs, d)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, W)) * 1000
    tt.frame_result(x[0], x[1], nd)
    t0 = time.perf_counter()
    for _ in range(frames):
        tt.frame_result(x[0], x[1], nd)
    return frames / (time.perf_counter() - t0)


def rocprof_run():
    out = tempfile.mkdtemp(prefix="tgcc_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--inner"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        print("rocprofv3 run failed (exit %d):\n%s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
        return
    files = sorted(glob.glob(out + "/**/*kernel_stats.csv", recursive=True))
    if not files:
        print("rocprofv3 wrote no kernel_stats.csv under", out, (r.stdout + r.stderr)[-1500:])
        return
    print("rocprofv3 --kernel-trace --stats (separate run: the three configurations in order, 3 + 20 calls each):")
    print("  %-60s %6s %14s %12s %12s %12s" % ("kernel", "calls", "total ns", "average ns", "min ns", "max ns"))
    for row in csv.DictReader(open(files[0])):
        if "tgcc" in row["Name"]:
            print("  %-60s %6s %14s %12.0f %12s %12s" % (row["Name"][:60], row["Calls"], row["TotalDurationNs"], float(row["AverageNs"]),
                                                       row["MinNs"], row["MaxNs"]))


def main():
    inner = "--inner" in sys.argv
    iters = 20
    results = []
    for fs, d in CONFIGS:
        W, hop, nd, dt = timed(fs, d, iters)
        results.append((fs, d, W, hop, nd, dt))
    if inner:
        return
    print("TemporalGCCBinauralLocalisation, device buffers, %d streams x %d frames per call, gate on, %d timed calls after 3 warm-up" % (A, F, iters))
    for fs, d, W, hop, nd, dt in results:
        useful, issued, rd, wr = work_model(W, nd)
        n = A * F
        print("fs %5d d %.3f (W %5d, hop %4d, nd %2d): %.3f ms per call, %.3f M frames/s" % (fs, d, W, hop, nd, dt * 1e3, n / dt / 1e6))
        print("    FP64: %.1f k FLOP/frame needed, %.1f k issued -> %.2f TFLOP/s needed (%.1f %% of the 78.6 TFLOP/s datasheet peak), "
              "%.2f TFLOP/s issued (%.1f %%)" % (useful / 1e3, issued / 1e3, n * useful / dt / 1e12, 100 * n * useful / dt / FP64_PEAK,
                                                 n * issued / dt / 1e12, 100 * n * issued / dt / FP64_PEAK))
        fp_share, hbm_share = n * issued / dt / FP64_PEAK, n * (rd + wr) / dt / HBM_COPY
        print("    HBM: %.1f KB read + %.0f B written per frame -> %.3f TB/s (%.2f %% of 8.0 TB/s, %.2f %% of the 6.29 TB/s copy rate); "
              "nearer its bound: %s" % (rd / 1e3, wr, n * (rd + wr) / dt / 1e12, 100 * n * (rd + wr) / dt / HBM_PEAK, 100 * hbm_share,
                                        "FP64 issue" if fp_share >= hbm_share else "HBM"))
    if "--no-prof" not in sys.argv:
        rocprof_run()
    try:
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
    except (AttributeError, OSError):
        pass
    for fs, d, W, hop, nd, dt in results:
        print("numpy restatement (tests/tgcc_twin.py closed form), one CPU core, fs %d: %.1f frames/s" % (fs, twin_rate(fs, d)))


if __name__ == "__main__":
    main()
