"""Device-side throughput of the tracked 2-microphone call (mca_hip_gcc2_tracked_frames_dev: the particle-filter DOA tracker
inside the stream call) and of the untracked call (mca_hip_gcc2_frames_dev) on the same context shape, on device buffers:
1, 64 and 4096 arrays x 512 frames at 16 kHz, N = 1024, 61 delays, 500 particles, no gate.

  python tools/bench_gcc2_track_dev.py              frames/s of both calls (device events, after warm-up) against real time
                                                    (31.25 frames/s per array), then the kernel times of a separate
                                                    rocprofv3 --kernel-trace --stats run of the tracked calls
  python tools/bench_gcc2_track_dev.py --no-prof    without the rocprofv3 run
  python tools/bench_gcc2_track_dev.py --inner      the tracked calls only (what the rocprofv3 run executes)
"""
import csv
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

FS, N, F, PARTICLES = 16000, 1024, 512, 500
ARRAYS = (1, 64, 4096)
REAL_TIME = FS / (N // 2)           # frames/s of one live array


def timed(A, tracked, iters):
    import torch
    from mcarray_amd import api, synth, _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    hop = N // 2
    ctx = api.Context(FS, synth.BINAURAL, N, 3.0, 1, max_arrays=A)
    if tracked:
        ctx.gcc2_tracker_attach(seed=1, n_particles=PARTICLES)
    L = (F + 1) * hop
    g = torch.Generator(device=dev).manual_seed(7)
    s = torch.randn(A, 1, L + 8, device=dev, generator=g) * 0.1          # a source 3 samples ahead on one microphone, plus sensor noise
    x = (torch.cat([s[:, :, 3:L + 3], s[:, :, :L]], dim=1) + 0.01 * torch.randn(A, 2, L, device=dev, generator=g)).contiguous()
    idx = torch.empty(A, F, dtype=torch.int32, device=dev)
    doa = torch.empty(A, F, dtype=torch.float32, device=dev)
    prob = torch.empty(A, F, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: C.c_void_p(t.data_ptr())

    def call():
        if tracked:
            rc = lib.mca_hip_gcc2_tracked_frames_dev(ctx.h, p(x), 2 * L, L, A, F, p(idx), p(doa), p(prob), None, None, None, st)
        else:
            rc = lib.mca_hip_gcc2_frames_dev(ctx.h, p(x), 2 * L, L, A, F, p(idx), p(doa), p(prob), None, st)
        assert rc == 0, lib.mca_hip_last_error(ctx.h)
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    dt = e0.elapsed_time(e1) / 1e3 / iters
    spread = float(torch.rad2deg(doa[:, -1]).std()) if A > 1 else 0.0
    last = float(torch.rad2deg(doa[0, -1]))
    ctx.close()
    del x, s
    torch.cuda.empty_cache()
    return dt, last, spread


def rocprof_run():
    out = tempfile.mkdtemp(prefix="gcc2_track_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--inner"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        print("rocprofv3 run failed (exit %d):\n%s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
        return
    files = sorted(glob.glob(out + "/**/*kernel_stats.csv", recursive=True))
    if not files:
        print("rocprofv3 wrote no kernel_stats.csv under", out, (r.stdout + r.stderr)[-1500:])
        return
    print("rocprofv3 --kernel-trace --stats (separate run: the tracked calls of A = %s in order, 2 + 5 calls each):" % (ARRAYS,))
    print("  %-64s %6s %14s %12s %12s %12s" % ("kernel", "calls", "total ns", "average ns", "min ns", "max ns"))
    for row in csv.DictReader(open(files[0])):
        if any(k in row["Name"] for k in ("gcc2", "stft_phat", "srp_gemm", "sum_planes", "k_gate")):
            print("  %-64s %6s %14s %12.0f %12s %12s" % (row["Name"][:64], row["Calls"], row["TotalDurationNs"], float(row["AverageNs"]),
                                                       row["MinNs"], row["MaxNs"]))


def main():
    inner = "--inner" in sys.argv
    iters = 5
    if inner:
        for A in ARRAYS:
            timed(A, True, iters)
        return
    print("FreqGCC stream call with and without the DOA tracker, device buffers, %d frames per call, fs %d, N %d, 61 delays, %d particles, "
          "no gate, %d timed calls after 2 warm-up" % (F, FS, N, PARTICLES, iters))
    for A in ARRAYS:
        dt_u, _, _ = timed(A, False, iters)
        dt_t, last, spread = timed(A, True, iters)
        n = A * F
        print("A %4d: untracked %9.3f ms per call, %10.1f k frames/s | tracked %9.3f ms per call, %10.1f k frames/s = %8.1f x real time "
              "(%.1f k frames/s for %d live arrays); the tracker adds %.3f ms = %.2f us per array-frame; DOA of array 0 at the end %.2f deg "
              "(std over arrays %.2f)" % (A, dt_u * 1e3, n / dt_u / 1e3, dt_t * 1e3, n / dt_t / 1e3, n / dt_t / (A * REAL_TIME),
                                          A * REAL_TIME / 1e3, A, (dt_t - dt_u) * 1e3, (dt_t - dt_u) / n * 1e6, last, spread))
    if "--no-prof" not in sys.argv:
        rocprof_run()


if __name__ == "__main__":
    main()
