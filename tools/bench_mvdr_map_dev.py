"""Device-side cost of the azimuth x elevation Capon map of an MVDR context (mca_hip_mvdr_map_dev) for 16 microphones in XYZ
geometry, N = 1024, all 513 bins, on device buffers:

  72 x 19 = 1368 directions      120 x 17 = 2040 directions      each at 256 streams and at one stream

and, in the same process and for scale, the 1-D spectrum call at 361 angles (mca_hip_mvdr_spectrum_dev: the same scan routine, a
workgroup per (stream, chunk)) and the 256 x 64-frame single-look frames call that leaves the covariance both read.  The yardstick
is the time per (stream, direction, bin) of the map against the spectrum's.

  python tools/bench_mvdr_map_dev.py             wall clock per call (ends in a device synchronise), the library's HIP events
                                                 (kernel_id 8 = both map kernels, 3 = both spectrum kernels, 1 = solve), the counted
                                                 arithmetic, then the kernel split of a separate rocprofv3 --kernel-trace --stats run
  python tools/bench_mvdr_map_dev.py --no-prof   without the rocprofv3 run
  python tools/bench_mvdr_map_dev.py --inner     the timed loops only (what the rocprofv3 run executes)"""
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
MAPS = [(72, 19), (120, 17)]
EL_LO_DEG, EL_HI_DEG = -30.0, 60.0
ANGLES_1D = 361
WARMUP, STEPS = 3, 20
# profiles/r06_mvdr_floor_model.md: a v_pk_fma_f32 costs 2.2 plain-fma slots of 1.33 ... 1.44 ns per wave-instruction and SIMD (the
# two-slot price); a complex multiply-add is two of them per lane; 256 CUs x 4 SIMDs
PK_FMA_NS, SIMDS = 2.2 * 1.385, 256 * 4


def counted_cmac(D, nb):
    """per stream, as DESIGN.md 4.4 counts: M (M + 1) / 2 complex multiply-adds per bin and direction (the forward substitution with
    the phasor product and the squared magnitude of every row)"""
    return D * nb * MICS * (MICS + 1) // 2


def floor_ms(cmac):
    """the time of cmac complex multiply-adds at the packed-fp32 rate of the whole part"""
    return cmac * 2 / 64 * PK_FMA_NS / SIMDS * 1e-6


def main():
    import numpy as np
    import torch
    from mcarray_amd import api
    inner = "--inner" in sys.argv
    hop, nb = N // 2, N // 2 + 1
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    pcm = (torch.randn((STREAMS, MICS, (FRAMES + 1) * hop), device=dev, generator=g) * 0.1).contiguous()
    doa = torch.full((STREAMS, FRAMES), 0.35, device=dev, dtype=torch.float32)
    out = torch.empty((STREAMS, FRAMES * hop), device=dev, dtype=torch.float32)
    xyz = np.random.default_rng(3).uniform(-0.05, 0.05, (MICS, 3))
    bf = api.MvdrBeamformer(FS, xyz, N, max_streams=STREAMS, geometry="xyz")
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

    def line(what, streams, D, wall, ev, checksum):
        cm = streams * counted_cmac(D, nb)
        per = ev * 1e6 / (streams * D * nb)
        print("%s, %3d streams, %4d directions, bins 0 ... %d: %.3f ms per call; both kernels (HIP events): %.3f ms = %.3f ns per (stream, "
              "direction, bin); %.1f M complex multiply-adds counted -> floor %.3f ms at the packed-fp32 rate, %.0f %% of it achieved; checksum %.6e"
              % (what, streams, D, N // 2, wall, ev, per, cm / 1e6, floor_ms(cm), 100.0 * floor_ms(cm) / ev, checksum))
        return per

    wall, ev = timed(lambda: bf.process_dev(pcm, FRAMES, doa, out_pcm=out, stream=st), api.MvdrBeamformer.K_SOLVE)
    if not inner:
        print("MVDR, XYZ geometry, %d microphones, N = %d, device buffers, %d timed calls after %d warm-up" % (MICS, N, STEPS, WARMUP))
        print("frames call, %d streams x %d frames (analysis + solve + synthesis): %.3f ms per call; its solve kernels (HIP events): %.3f ms"
              % (STREAMS, FRAMES, wall, ev))
    per_1d = {}
    bf.configure_spectrum(ANGLES_1D, 0, N // 2, "normalised", 4)
    for streams in (STREAMS, 1):
        spec = torch.empty((streams, ANGLES_1D), device=dev, dtype=torch.float32)
        pk = [torch.empty((streams, 4), device=dev, dtype=torch.float32) for _ in range(2)]
        wall, ev = timed(lambda: bf.spectrum_dev(streams, spectrum=spec, peak_doa=pk[0], peak_val=pk[1], stream=st), api.MvdrBeamformer.K_SPECTRUM)
        if not inner:
            per_1d[streams] = line("spectrum call", streams, ANGLES_1D, wall, ev, float(spec.double().sum().item()))
    for n_az, n_el in MAPS:
        bf.map_configure(n_az, n_el, np.deg2rad(EL_LO_DEG), np.deg2rad(EL_HI_DEG), 0, N // 2, "normalised", 4)
        for streams in (STREAMS, 1):
            m = torch.empty((streams, n_el, n_az), device=dev, dtype=torch.float32)
            pk = [torch.empty((streams, 4), device=dev, dtype=torch.float32) for _ in range(3)]
            wall, ev = timed(lambda: bf.map_dev(streams, map=m, peak_az=pk[0], peak_el=pk[1], peak_val=pk[2], stream=st), api.MvdrBeamformer.K_MAP)
            if not inner:
                per = line("map call %3d x %2d" % (n_az, n_el), streams, n_az * n_el, wall, ev, float(m.double().sum().item()))
                print("    per (stream, direction, bin): %.2f x the spectrum call's at %d streams" % (per / per_1d[streams], streams))
    bf.close()
    if inner or "--no-prof" in sys.argv:
        return
    outdir = tempfile.mkdtemp(prefix="mvdr_map_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--", sys.executable, os.path.abspath(__file__), "--inner"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        print("rocprofv3 run failed (exit %d):\n%s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
        sys.exit(1)
    files = sorted(glob.glob(outdir + "/**/*kernel_stats.csv", recursive=True))
    if not files:
        print("rocprofv3 wrote no kernel_stats.csv under", outdir, (r.stdout + r.stderr)[-1500:])
        sys.exit(1)
    print("rocprofv3 --kernel-trace --stats (separate run: the frames call, the spectrum and the two maps, each at %d streams and at one, %d + 2 x %d calls each):"
          % (STREAMS, WARMUP, STEPS))
    print("  %-64s %6s %14s %12s %12s %12s" % ("kernel", "calls", "total ns", "average ns", "min ns", "max ns"))
    for row in csv.DictReader(open(files[0])):
        if "mvdr" in row["Name"]:
            print("  %-64s %6s %14s %12.0f %12s %12s" % (row["Name"][:64], row["Calls"], row["TotalDurationNs"], float(row["AverageNs"]),
                                                       row["MinNs"], row["MaxNs"]))


if __name__ == "__main__":
    main()
