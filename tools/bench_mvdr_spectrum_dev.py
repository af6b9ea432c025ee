"""Device-side cost of the Capon spatial spectrum of an MVDR context (mca_hip_mvdr_spectrum_dev) for 256 streams x 16 microphones,
N = 1024, on device buffers:

  D = 361 over all bins (0 ... 512)          D = 181 over bins 8 ... 71

and, in the same process and for scale, the 256 x 64-frame single-look solve call (mca_hip_mvdr_frames_dev) that leaves the
covariance the spectrum reads.

  python tools/bench_mvdr_spectrum_dev.py             wall clock per call (ends in a device synchronise), the library's HIP events
                                                      (kernel_id 3 = both spectrum kernels, 1 = solve), the counted arithmetic, then
                                                      the kernel split of a separate rocprofv3 --kernel-trace --stats run of this tool
  python tools/bench_mvdr_spectrum_dev.py --no-prof   without the rocprofv3 run
  python tools/bench_mvdr_spectrum_dev.py --inner     the timed loops only (what the rocprofv3 run executes)"""
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAMS, MICS, N, FS, FRAMES = 256, 16, 1024, 48000, 64
CONFIGS = [(361, 0, N // 2, "normalised"), (181, 8, 71, "normalised"), (361, 0, N // 2, "power")]
WARMUP, STEPS = 3, 20


def counted_flop(D, lo, hi):
    """per stream: the factorisation (M^3/6 complex MACs a bin) and the forward substitutions (M (M - 1) / 2 complex MACs, M
    phasor products and M squared magnitudes per bin and angle); a complex MAC or product = 8 / 6 FLOP"""
    M, nb = MICS, hi - lo + 1
    return nb * (8 * M ** 3 / 6 + D * (8 * M * (M - 1) / 2 + 6 * M + 4 * M))


def main():
    import torch
    from mcarray_amd import api, synth
    inner = "--inner" in sys.argv
    hop = N // 2
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    pcm = (torch.randn((STREAMS, MICS, (FRAMES + 1) * hop), device=dev, generator=g) * 0.1).contiguous()
    doa = torch.full((STREAMS, FRAMES), 0.35, device=dev, dtype=torch.float32)
    out = torch.empty((STREAMS, FRAMES * hop), device=dev, dtype=torch.float32)
    bf = api.MvdrBeamformer(FS, list(synth.ULA16), N, max_streams=STREAMS)
    st = torch.cuda.current_stream().cuda_stream

    def timed(call, kid):
        for _ in range(WARMUP):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            call()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / STEPS
        n0, ms0 = bf.get_timing(kid)
        bf.set_timing(True)
        for _ in range(STEPS):
            call()
        torch.cuda.synchronize()
        n1, ms1 = bf.get_timing(kid)
        bf.set_timing(False)
        return wall * 1e3, (ms1 - ms0) / STEPS

    wall, ev = timed(lambda: bf.process_dev(pcm, FRAMES, doa, out_pcm=out, stream=st), api.MvdrBeamformer.K_SOLVE)
    if not inner:
        print("MVDR, %d streams x %d microphones, N = %d, device buffers, %d timed calls after %d warm-up" % (STREAMS, MICS, N, STEPS, WARMUP))
        print("frames call, %d frames (analysis + solve + synthesis): %.3f ms per call; its solve kernels (HIP events): %.3f ms" % (FRAMES, wall, ev))
    for D, lo, hi, weighting in CONFIGS:
        bf.configure_spectrum(D, lo, hi, weighting, 4)
        spec = torch.empty((STREAMS, D), device=dev, dtype=torch.float32)
        pd = torch.empty((STREAMS, 4), device=dev, dtype=torch.float32)
        pv = torch.empty((STREAMS, 4), device=dev, dtype=torch.float32)
        wall, ev = timed(lambda: bf.spectrum_dev(STREAMS, spectrum=spec, peak_doa=pd, peak_val=pv, stream=st), api.MvdrBeamformer.K_SPECTRUM)
        if not inner:
            fl = STREAMS * counted_flop(D, lo, hi)
            print("spectrum call, D = %3d, bins %d ... %d, %s: %.3f ms per call; both kernels (HIP events): %.3f ms; %.2f GFLOP counted -> "
                  "%.2f TFLOP/s over the event time; checksum %.6e" % (D, lo, hi, weighting, wall, ev, fl / 1e9, fl / (ev * 1e-3) / 1e12,
                                                                         float(spec.double().sum().item())))
    bf.close()
    if inner or "--no-prof" in sys.argv:
        return
    outdir = tempfile.mkdtemp(prefix="mvdr_spectrum_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--", sys.executable, os.path.abspath(__file__), "--inner"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        print("rocprofv3 run failed (exit %d):\n%s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
        sys.exit(1)
    files = sorted(glob.glob(outdir + "/**/*kernel_stats.csv", recursive=True))
    if not files:
        print("rocprofv3 wrote no kernel_stats.csv under", outdir, (r.stdout + r.stderr)[-1500:])
        sys.exit(1)
    print("rocprofv3 --kernel-trace --stats (separate run: the frames call and the three spectrum configurations in order, %d + 2 x %d calls each):" % (WARMUP, STEPS))
    print("  %-64s %6s %14s %12s %12s %12s" % ("kernel", "calls", "total ns", "average ns", "min ns", "max ns"))
    for row in csv.DictReader(open(files[0])):
        if "mvdr" in row["Name"]:
            print("  %-64s %6s %14s %12.0f %12s %12s" % (row["Name"][:64], row["Calls"], row["TotalDurationNs"], float(row["AverageNs"]),
                                                       row["MinNs"], row["MaxNs"]))


if __name__ == "__main__":
    main()
