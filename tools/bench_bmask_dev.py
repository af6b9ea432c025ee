"""Device-side throughput of the filter-bank binaural masking (BinauralMaskingImpl, mca_hip_bmask_frames_dev) on device buffers,
with FastBinauralMasking (mca_hip_mask_frames_dev) at the same shapes beside it as the yardstick: 16 kHz (W = 1024) and
48 kHz (W = 2048), one stream and many streams, and the shapes of tools/bench_mask_dev.py (64 streams, 2^20 / W frames;
8 kHz: W = 512 on the any-length kernels).  Each figure is the median of REPS timed windows of at least 0.2 s after a warm-up.
Run on the GPU box: python tools/bench_bmask_dev.py [--only I] [--profile]   (--only I: shape number I alone; --profile: three
calls per module, no timing, for rocprofv3 --kernel-trace --stats)"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mcarray_amd import api, _lib

REPS = 5
lib = _lib.load()
dev = torch.device("cuda", 0)
profile = "--profile" in sys.argv


def rate(call, frames):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    if profile:
        return 0.0, 0.0, 0.0
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    n = max(2, int(0.2 / max(time.perf_counter() - t0, 1e-6)))
    r = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(n):
            call()
        torch.cuda.synchronize()
        r.append(frames * n / (time.perf_counter() - t0))
    return float(np.median(r)), min(r), max(r)


def shape(fs, W, A, F, lo, hi):
    hop = W // 2
    x = (torch.randn(A, 2, (F + 1) * hop, device=dev) * 0.1).contiguous()
    out = torch.empty(A, 2, F * hop, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    args = (C.c_void_p(x.data_ptr()), 2 * (F + 1) * hop, (F + 1) * hop, A, F, C.c_void_p(out.data_ptr()), None, st)
    bm = api.BinauralMaskingImpl(fs, 0.086, lo, hi, max_streams=A)
    assert bm.W == W
    fm = api.FastBinauralMasking(fs, 0.086, lo, hi, max_streams=A, fft_size=W)

    def call_bm():
        rc = lib.mca_hip_bmask_frames_dev(bm.h, *args)
        assert rc == 0, lib.mca_hip_bmask_last_error(bm.h)

    def call_fm():
        rc = lib.mca_hip_mask_frames_dev(fm.h, *args)
        assert rc == 0, lib.mca_hip_mask_last_error(fm.h)

    b, f = rate(call_bm, A * F), rate(call_fm, A * F)
    if not profile:
        print("fs %5d W %4d, %4d streams x %5d frames: BinauralMaskingImpl %8.3f M frames/s (%.3f..%.3f), FastBinauralMasking %8.3f M frames/s "
              "(%.3f..%.3f), ratio %.2f" % (fs, W, A, F, b[0] / 1e6, b[1] / 1e6, b[2] / 1e6, f[0] / 1e6, f[1] / 1e6, f[2] / 1e6, b[0] / f[0]))
    bm.close()
    fm.close()


SHAPES = []
for fs, W in ((16000, 1024), (48000, 2048)):
    SHAPES += [(fs, W, 1, 4096, 500.0, 5000.0), (fs, W, 512, 256, 500.0, 5000.0)]
for fs, W in ((16000, 1024), (48000, 2048), (8000, 512)):       # tools/bench_mask_dev.py
    SHAPES.append((fs, W, 64, 1024 * 1024 // W, 300.0, min(5000.0, 0.45 * fs)))
only = int(sys.argv[sys.argv.index("--only") + 1]) if "--only" in sys.argv else None
for i, sh in enumerate(SHAPES):
    if only is None or i == only:
        shape(*sh)
