"""Launch time of setProbability at caller-given angles on the device (mca_hip_gcc2_set_probability_dev, k_gcc2_prob) for
A arrays x n particles, timed with device events over 100 launches after warm-up.  The smoothed correlations come from one
gcc2_frames_dev call.  Bytes per launch ~ A (4 D + 8 n): launch / latency bound.
usage (GPU box): python tools/bench_gcc2_prob_dev.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcarray_amd import api  # noqa: E402

dev = torch.device("cuda", 0)
fs, N, F, REPS = 16000, 1024, 64, 100
hop = N // 2
for A in (1, 64, 1024):
    ctx = api.Context(fs, [0.0, 0.086], N, 3.0, 1, max_arrays=A)
    x = (torch.randn(A, 2, (F + 1) * hop, device=dev) * 0.1).contiguous()
    idx = torch.empty(A, F, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev)
    ctx.gcc2_frames_dev(x, F, idx, stream=st.cuda_stream)
    for n in (500, 4096):
        doas = ((torch.rand(A, n, device=dev) - 0.5) * 3.14159).contiguous()
        probs = torch.empty(A, n, dtype=torch.float32, device=dev)
        for _ in range(10):
            ctx.gcc2_set_probability_dev(doas, probs, stream=st.cuda_stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(REPS):
            ctx.gcc2_set_probability_dev(doas, probs, stream=st.cuda_stream)
        e1.record(st)
        e1.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / REPS
        print("gcc2_set_probability_dev: %4d arrays x %4d particles, D %d: %8.2f us per launch, %8.1f M particles/s, %.2f MB moved"
              % (A, n, ctx.D, us, A * n / us, A * (4 * ctx.D + 8 * n) / 1e6))
    ctx.close()
