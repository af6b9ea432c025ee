"""The launch plans of the four module contexts (csrc/module_plan.h) on the CPU: tests/cxx/module_plan_cli.cpp is compiled
with the HIP compiler's host pass only (no device code, no HIP call) and prints the plan of every query given to it.  It is built a second time
with the address and undefined-behaviour sanitizers, as a stand-alone program, and the same table goes through both.

Run lengths, frames per workgroup, the scan chunk and the grids change no output bit -- their only effect is speed -- so no comparison of outputs
sees a regression in them; and a launch that asks for more than 64 KiB of dynamic LDS without the attribute fails only on a GPU.  This table sees both.

Expected rows: worked out by hand from the formulas of the host layer before the plans existed (api_mask.hip, api_bmask.hip, api_multiband.hip and
api_tgcc.hip at "MVDR host layer: a launch is a plan; host calls staged in one place") -- never taken from the plan functions.  The constants behind
the LDS sizes: 576 words of scratch per wave of the 512-point transform, 1 344 words of its tables (832 up to the window), rows of 258 words, 4 frames
a pass of the 1024-sample masking kernels, 37 delays of the multiband grid (5 degree steps), 64 + 80 samples of padding round the temporal GCC's second
channel.  attr: the launch sets the function's dynamic-LDS limit, exactly above 64 KiB.  tests/test_gpu_launch_geometry.py restates the run lengths
on its own and checks them on the GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_cli(tmp, name, extra):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc) or shutil.which(hipcc), "no HIP compiler"
    exe = tmp / name
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "mcarray_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "module_plan_cli.cpp"), "-o", str(exe)] + extra)
    return str(exe)


@pytest.fixture(scope="module")
def clis(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("module_plan")
    return [build_cli(tmp, "module_plan_cli", []), build_cli(tmp, "module_plan_cli_san", ["-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def parse(line):
    out = {}
    for tok in line.split():
        k, v = tok.split("=")
        out[k] = tuple(int(x) for x in v.split(",")) if "," in v else (v if k == "form" else int(v))
    return out


def ask(cli, queries):
    text = "".join("%s %s\n" % (stage, " ".join("%s=%r" % kv for kv in q.items())) for stage, q in queries)
    lines = subprocess.run([cli], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(queries)
    return [parse(ln) for ln in lines]


def g(x, y=1, z=1):
    return (x, y, z)


def table():
    """(stage, query, expected fields)"""
    t = []

    def row(stage, want, **q):
        t.append((stage, q, want))

    # ---- the shared rule: the length starts at hi and halves down to lo while streams x ceil(frames / length) < target
    row("run_length", dict(len=16), n_streams=2, n_frames=6, target=512, lo=16, hi=256)                   # never enough workgroups: the minimum
    row("run_length", dict(len=256), n_streams=512, n_frames=300, target=512, lo=16, hi=256)              # 512 * 2 at once: the maximum
    row("run_length", dict(len=256), n_streams=512, n_frames=130, target=512, lo=16, hi=256)              # 512 * 1 = 512 is not fewer than 512
    row("run_length", dict(len=128), n_streams=100, n_frames=1000, target=512, lo=16, hi=256)             # 100 * 4 = 400, 100 * 8 = 800: one step
    row("run_length", dict(len=32), n_streams=128, n_frames=160, target=512, lo=16, hi=256)               # 128, 256, 384, 128 * 5 = 640
    row("run_length", dict(len=4), n_streams=80, n_frames=61, target=1024, lo=2, hi=16)                   # the MVDR synthesis: 320, 640, 1280
    row("fpb", dict(len=8), n_rows=128, n_frames=40, hi=16, lo=4, target=512)                             # 128 * 3 = 384, 128 * 5 = 640
    row("grid_for", dict(grid=g(7)), n=1542, per=256)
    row("grid_for", dict(grid=g(6)), n=1536, per=256)

    # ---- mask.  1024: 4*2*576*8 + 4*3*520*4 + 832*8 + 4*48*8*4 + 520*8 + 528 = 36 864 + 24 960 + 6 656 + 6 144 + 4 160 + 528 = 79 312
    m1024 = dict(form="mask_1024", block=g(512), lds=79312, attr=1)
    row("mask", dict(ft=16, grid=g(1, 2), **m1024), N=1024, n_streams=2, n_frames=6)
    row("mask", dict(ft=32, grid=g(2, 256), **m1024), N=1024, n_streams=256, n_frames=64)                 # 256, 256, 256, 256 * 2 = 512
    row("mask", dict(ft=128, grid=g(8, 100), **m1024), N=1024, n_streams=100, n_frames=1000)
    row("mask", dict(ft=256, grid=g(2, 512), **m1024), N=1024, n_streams=512, n_frames=300)
    row("mask", dict(ft=40, grid=g(1, 2), **m1024), N=1024, noisy_first=1, n_streams=2, n_frames=40)      # NOISY's first call: one chunk
    row("mask", dict(ft=16, grid=g(3, 2), **m1024), N=1024, noisy_first=0, n_streams=2, n_frames=40)      # ... and its later calls
    # 2048: (16*258 + 8*576 + 832) * 8 + 2*48*8*4 = 76 544 + 3 072 = 79 616
    m2048 = dict(form="mask_2048", block=g(512), lds=79616, attr=1)
    row("mask", dict(ft=16, grid=g(3, 2), **m2048), N=2048, n_streams=2, n_frames=40)
    row("mask", dict(ft=40, grid=g(1, 2), **m2048), N=2048, noisy_first=1, n_streams=2, n_frames=40)
    row("mask", dict(ft=32, grid=g(5, 128), **m2048), N=2048, n_streams=128, n_frames=160)
    # any length, N = 512: 2*257*8 + (3*257 + 512 + 384) * 4 = 4 112 + 6 668 = 10 780; 256 threads; min(163 840 / 10 780 = 15, 2048 / 256 = 8) = 8 a CU:
    # the runs halve while there are fewer than 2048 of them
    gen512 = dict(form="mask_gen", nthr=256, per_cu=8, block=g(256), lds=10780, attr=0)
    row("mask", dict(ft=16, grid=g(3, 2), **gen512), N=512, n_streams=2, n_frames=40)
    row("mask", dict(ft=256, grid=g(2, 1024), **gen512), N=512, n_streams=1024, n_frames=300)             # 1024 * 2 = 2048
    row("mask", dict(ft=128, grid=g(2, 1024), **gen512), N=512, n_streams=1024, n_frames=256)             # 1024 < 2048 (under a bound of 512: 256)
    row("mask", dict(ft=40, grid=g(1, 2), **gen512), N=512, noisy_first=1, n_streams=2, n_frames=40)
    row("mask", dict(form="mask_gen", nthr=256, per_cu=8, lds=2 * 33 * 8 + (99 + 64 + 384) * 4, attr=0), N=64, n_streams=2, n_frames=6)
    # N = 4096: 2*2049*8 + (6147 + 4096 + 384) * 4 = 32 784 + 42 508 = 75 292: 2 a CU by LDS, 512 threads
    row("mask", dict(form="mask_gen", ft=16, nthr=512, per_cu=2, grid=g(1, 3), block=g(512), lds=75292, attr=1), N=4096, n_streams=3, n_frames=5)
    # N = 8192: 65 552 + (12 291 + 8192 + 384) * 4 = 149 020: 1 a CU, so the bound is 256 runs (under 512: ft 128)
    row("mask", dict(form="mask_gen", ft=256, nthr=512, per_cu=1, grid=g(1, 256), lds=149020, attr=1), N=8192, n_streams=256, n_frames=256)

    # ---- bmask.  1024: (4*2*576 + 832) * 8 = 43 520, the synthesis + 4*48*8 = 45 056; 4 frames a workgroup of the analysis; the scan: a workgroup of 1024 a stream
    row("bmask", dict(form="bmask_1024", ft=16, n_runs=1, analyse_grid=g(2, 2), analyse_block=g(512), analyse_lds=43520, analyse_attr=0, scan_grid=g(2), scan_block=g(1024),
                      scan_lds=0, synth_grid=g(1, 2), synth_block=g(512), synth_lds=45056, synth_attr=0), N=1024, n_streams=2, n_frames=6)
    row("bmask", dict(form="bmask_1024", ft=32, n_runs=5, analyse_grid=g(40, 128), synth_grid=g(5, 128), scan_grid=g(128)), N=1024, n_streams=128, n_frames=160)
    row("bmask", dict(form="bmask_1024", ft=256, n_runs=2, analyse_grid=g(75, 512), synth_grid=g(2, 512)), N=1024, n_streams=512, n_frames=300)
    # 2048: 76 544, the synthesis + 2*48*8 = 77 312; 2 frames a workgroup of the analysis
    row("bmask", dict(form="bmask_2048", ft=16, n_runs=3, analyse_grid=g(20, 3), analyse_block=g(512), analyse_lds=76544, analyse_attr=1, scan_grid=g(3), scan_block=g(1024),
                      synth_grid=g(3, 3), synth_block=g(512), synth_lds=77312, synth_attr=1), N=2048, n_streams=3, n_frames=40)
    # any length: 2 * (N/2 + 1) * 8, the synthesis + 2 * (N/2) * 4 + 48*8; a frame a workgroup of the analysis
    row("bmask", dict(form="bmask_gen", ft=16, n_runs=1, analyse_grid=g(3, 1), analyse_block=g(256), analyse_lds=65552, analyse_attr=1, scan_grid=g(1), synth_grid=g(1, 1),
                      synth_block=g(256), synth_lds=98704, synth_attr=1), N=8192, n_streams=1, n_frames=3)
    row("bmask", dict(form="bmask_gen", analyse_lds=32784, analyse_attr=0, synth_lds=49552, synth_attr=0), N=4096, n_streams=1, n_frames=3)
    row("bmask", dict(form="bmask_gen", ft=16, n_runs=3, analyse_grid=g(40, 2), analyse_lds=2064, synth_grid=g(3, 2), synth_lds=2064 + 1024 + 384, synth_attr=0), N=256, n_streams=2,
        n_frames=40)

    # ---- multiband analysis.  1024: 8*576*8 + 4*520*12 + 1344*8 + 64 = 36 864 + 24 960 + 10 752 + 64 = 72 640; fpb 16 halved down to 4
    b1024 = dict(form="mb_1024", block=g(512), lds=72640, attr=1)
    row("mb_analyse", dict(fpb=4, grid=g(2, 2), **b1024), N=1024, n_arrays=2, n_frames=6)
    row("mb_analyse", dict(fpb=8, grid=g(5, 128), **b1024), N=1024, n_arrays=128, n_frames=40)
    row("mb_analyse", dict(fpb=16, grid=g(2, 512), **b1024), N=1024, n_arrays=512, n_frames=32)
    # 512: 76 544 + 64 = 76 608; fpb 32 halved down to 8
    b512 = dict(form="mb_512", block=g(512), lds=76608, attr=1)
    row("mb_analyse", dict(fpb=8, grid=g(1, 2), **b512), N=512, n_arrays=2, n_frames=6)
    row("mb_analyse", dict(fpb=16, grid=g(7, 100), **b512), N=512, n_arrays=100, n_frames=100)            # 100 * 4 = 400, 100 * 7 = 700
    row("mb_analyse", dict(fpb=32, grid=g(2, 512), **b512), N=512, n_arrays=512, n_frames=64)
    # any length: 2 * (N/2 + 1) * 8 + (N/2 + 1) * 12 + 32; a frame a workgroup
    row("mb_analyse", dict(form="mb_gen", grid=g(6, 2), block=g(256), lds=2064 + 1032 + 516 + 32, attr=0), N=256, n_arrays=2, n_frames=6)
    row("mb_analyse", dict(form="mb_gen", grid=g(40, 3), block=g(256), lds=65552 + 32776 + 16388 + 32, attr=1), N=8192, n_arrays=3, n_frames=40)
    # ---- multiband scan, 37 delays.  32 frames a chunk while 32 * (37 nb + 37 + nb) * 4 <= 81 920: nb = 15 gives 77 696, nb = 16 gives 82 560
    row("mb_scan", dict(chunk=32, grid=g(2, 2), block=g(576), lds=32 * (555 + 37) * 4 + 32 * 15 * 4, attr=1), nbins=15, D=37, n_arrays=2, n_frames=40)
    assert 32 * (555 + 37) * 4 + 32 * 15 * 4 == 77696
    row("mb_scan", dict(chunk=16, grid=g(3, 2), block=g(640), lds=16 * (592 + 37) * 4 + 16 * 16 * 4, attr=0), nbins=16, D=37, n_arrays=2, n_frames=40)
    row("mb_scan", dict(chunk=32, grid=g(1, 2), block=g(192), lds=29056, attr=0), nbins=5, D=37, n_arrays=2, n_frames=6)
    row("mb_scan", dict(chunk=16, grid=g(1, 3), block=g(1024), lds=16 * (999 + 37) * 4 + 16 * 27 * 4, attr=1), nbins=27, D=37, n_arrays=3, n_frames=16)      # 68 032
    row("mb_summary", dict(grid=g(3), block=g(256), lds=0, attr=0), n_arrays=3)

    # ---- temporal GCC.  The hook's workspace: (8*16 + 4*16 + 16 + 2*32 + 8 + nd (2 nd + 1) + 1) doubles, rounded down to even; the stream kernel adds both
    # channels in fp32, the second one padded by 64 + 80 samples.  0.2 m at 48 kHz: nd = 27, W = 7200: 8 * 1766 + 4 * (14 400 + 144) = 72 304
    row("tgcc", dict(frames_grid=g(2, 1), frames_block=g(256), frames_lds=72304, frames_attr=1, gate_grid=g(1), gate_block=g(64), gate_lds=0, hook_grid=g(1), hook_block=g(256),
                     hook_lds=8 * 1766, hook_attr=0), W8=7200, nd=27, n_arrays=1, n_frames=2)
    # at 16 kHz: nd = 9, W = 2400: 8 * 452 + 4 * (4800 + 144) = 23 392
    row("tgcc", dict(frames_grid=g(40, 3), frames_lds=23392, frames_attr=0, hook_lds=3616, gate_grid=g(1)), W8=2400, nd=9, n_arrays=3, n_frames=40)
    row("tgcc", dict(gate_grid=g(2), frames_grid=g(1, 65)), W8=2400, nd=9, n_arrays=65, n_frames=1)
    # the largest: 32 delay pairs, 96 kHz (W = 14 400): 8 * 2360 + 4 * (28 800 + 144) = 134 656, inside the 160 KiB of a CU
    row("tgcc", dict(frames_lds=134656, frames_attr=1, hook_lds=18880, hook_attr=0), W8=14400, nd=32, n_arrays=1, n_frames=1)
    return t


def test_the_plans_of_the_table(clis):
    t = table()
    for cli in clis:
        for (stage, q, want), got in zip(t, ask(cli, [(s, q) for s, q, _ in t])):
            print(stage, q, "->", got)
            assert {k: got.get(k) for k in want} == want, (stage, q)


def test_the_unconditional_attribute_sets_that_went_were_all_above_64_kib(clis):
    """k_mb_analyse_1024, k_mb_analyse_512 and k_mask_stream_2048 set the attribute whatever the size before the one launcher; their LDS does not depend on the call"""
    qs = [("mb_analyse", dict(N=1024, n_arrays=a, n_frames=f)) for a, f in ((1, 1), (3, 40), (512, 64))]
    qs += [("mb_analyse", dict(N=512, n_arrays=a, n_frames=f)) for a, f in ((1, 1), (3, 40), (512, 64))]
    qs += [("mask", dict(N=2048, noisy_first=n, n_streams=a, n_frames=f)) for n in (0, 1) for a, f in ((1, 1), (3, 40), (512, 64))]
    for ans in ask(clis[0], qs):
        assert ans["attr"] == 1 and ans["lds"] > 64 * 1024, ans
