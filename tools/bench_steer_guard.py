"""Miss-share sweep of the steered delay-and-sum path: 8 arrays x 4 096 frames per call, k of the arrays carry a
source that moves every few frames (their frames miss the predicted bin), the others a stationary one.  Per k, averaged over --reps
repetitions from a reset context: the SECOND call (it steers ahead of its picks: the guard has no report yet; the first call predicts
bin -1) and the THIRD (behind an all-miss first call the guard has switched off: every frame steered after the picks).  Run it on two
builds of the library to compare; a build without the path reports its delay-and-sum kernel's calls under the same columns."""
import argparse
import json
import sys
import os

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcarray_amd import api, synth  # noqa: E402

FS, N, HOP = 48000, 1024, 512


def moving(n_samples, seed, every=5):
    rng = np.random.default_rng(seed)
    parts, n = [], 0
    while n < n_samples:
        ln = int(rng.integers(every - 2, every + 3)) * HOP
        parts.append(synth.noise_source_stream(synth.ULA8, np.deg2rad(float(rng.uniform(-70, 70))), FS, ln, int(rng.integers(1 << 30))))
        n += ln
    return np.concatenate(parts, axis=1)[:, :n_samples]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arrays", type=int, default=8)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ks", default="0,1,2,4,6,8")
    args = ap.parse_args()
    A, F = args.arrays, args.frames
    dev = torch.device("cuda:0")
    L = (3 * F + 1) * HOP
    still = [synth.noise_source_stream(synth.ULA8, np.deg2rad(40.0 - 11 * a), FS, L, 500 + a).astype(np.float32) for a in range(A)]
    moved = [moving(L, 600 + a).astype(np.float32) for a in range(A)]
    ctx = api.Context(FS, synth.ULA8, N, 0.5, 1, srp_precision=api.SRP_ADAPTIVE, max_arrays=A)
    b = torch.empty(A, F, 1, dtype=torch.int32, device=dev); r = torch.empty(A, F, 1, dtype=torch.float32, device=dev)
    q = torch.empty(A, F, 1, dtype=torch.float32, device=dev); o = torch.empty(A, 1, F * HOP, dtype=torch.float32, device=dev)
    for k in [int(x) for x in args.ks.split(",")]:
        pcm = np.stack([moved[a] if a < k else still[a] for a in range(A)])
        x = [torch.from_numpy(np.ascontiguousarray(pcm[:, :, i * F * HOP:((i + 1) * F + 1) * HOP])).to(dev) for i in range(3)]
        ms = [[], [], []]
        stats = None
        for rep in range(args.reps + 3):
            ctx.reset()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            before = ctx.steer_stats() if hasattr(ctx, "steer_stats") else None
            for i in range(3):
                ev[i].record()
                ctx.process_frames_dev(x[i], F, b, r, q, None, o)
            ev[3].record()
            torch.cuda.synchronize()
            if before is not None:
                after = ctx.steer_stats()
                stats = {key: after[key] - before[key] for key in after}
            if rep >= 3:
                for i in range(3):
                    ms[i].append(ev[i].elapsed_time(ev[i + 1]))
        print(json.dumps({"moving_arrays": k, "of": A, "frames_per_call": F, "ms_call1": round(float(np.median(ms[0])), 4),
                          "ms_call2": round(float(np.median(ms[1])), 4), "ms_call3": round(float(np.median(ms[2])), 4),
                          "three_calls": stats}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
