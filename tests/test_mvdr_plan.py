"""The launch plans of the MVDR path (csrc/mvdr_plan.h) on the CPU: tests/cxx/mvdr_plan_cli.cpp is compiled with
the HIP compiler's host pass only (no device code, no HIP call) and prints the plan of every query given to it.  It is built a second time
with the address and undefined-behaviour sanitizers, as a stand-alone program, and the same table goes through both.

Frames per workgroup, the pieced tail launch of the solve, the chunks of an RTF call, the passes of the map and the grids change no output
bit -- their only effect is speed and workspace size -- so no comparison of outputs sees a regression in them.  This table does.

Expected rows: worked out by hand from the formulas of the host layer before the plans existed (api_mvdr.hip at "MVDR: tracks in azimuth
and elevation, fed by the Capon map") -- never taken from the plan functions.  The constants behind the LDS sizes: 576 words of the
512-point transform's scratch, 1 344 words of its tables (832 up to the window), chunks of 64 bins, tiles of
128 directions.  tests/test_gpu_launch_geometry.py restates three of the formulas on its own and checks them on the GPU."""
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
                           os.path.join(ROOT, "tests", "cxx", "mvdr_plan_cli.cpp"), "-o", str(exe)] + extra)
    return str(exe)


@pytest.fixture(scope="module")
def clis(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mvdr_plan")
    return [build_cli(tmp, "mvdr_plan_cli", []), build_cli(tmp, "mvdr_plan_cli_san", ["-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def parse(line):
    out = {}
    for tok in line.split():
        k, v = tok.split("=")
        out[k] = tuple(int(x) for x in v.split(",")) if "," in v else (v if k in ("form", "weight") else int(v))
    return out


def ask(cli, queries):
    """queries: (stage, dict) -> the parsed answer per query"""
    text = "".join("%s %s\n" % (stage, " ".join("%s=%r" % kv for kv in q.items())) for stage, q in queries)
    lines = subprocess.run([cli], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(queries)
    return [parse(ln) for ln in lines]


def g(x, y=1, z=1):
    return (x, y, z)


def ceil_div(a, b):
    return (a + b - 1) // b


def table():
    """(stage, query, expected fields)"""
    t = []

    def row(stage, want, **q):
        t.append((stage, q, want))

    # ---- analysis.  1024: fpb 8 halved while streams x ceil(frames / fpb) < 1024; (8 * 580 + TW_WORDS) * 8 bytes with the 1 344 words of
    # the 512-point transform's tables (fft512.h; not the 1 152 of the 1024-point table): 47 872
    row("analyse", dict(form="analyse_1024", fpb=8, grid=g(8, 256), block=g(512), lds=(8 * 580 + 1344) * 8, attr=0), N=1024, M=8, n_streams=256, n_frames=64)
    row("analyse", dict(form="analyse_1024", fpb=1, grid=g(5, 3), lds=47872), N=1024, M=8, n_streams=3, n_frames=5)
    # 512: 40 x 61: 40 * 8 = 320, 40 * 16 = 640, 40 * 31 = 1240 -> 2; 64 x 61: 64 * 8 = 512, 64 * 16 = 1024 -> 4; 128 x 61: 128 * 8 = 1024 -> 8
    # (16 * 258 + 8 * 576 + 832) * 8 = 76 544 bytes: above 64 KiB, the attribute is needed
    for n, fpb, grid in ((40, 2, g(31, 40)), (64, 4, g(16, 64)), (128, 8, g(8, 128))):
        row("analyse", dict(form="analyse_512", fpb=fpb, grid=grid, block=g(512), lds=76544, attr=1), N=512, M=8, n_streams=n, n_frames=61)
    row("analyse", dict(form="analyse_gen", grid=g(5, 3), block=g(256), lds=3 * 33 * 8, attr=0), N=64, M=3, n_streams=3, n_frames=5)
    # 8 * 4096 / 8 = 4096 work items: 256 threads doubled while 2 t <= items, 1024 at the most; 8 * 2049 * 8 bytes
    row("analyse", dict(form="analyse_gen", grid=g(7, 2), block=g(1024), lds=131136, attr=1), N=4096, M=8, n_streams=2, n_frames=7)
    row("analyse", dict(form="analyse_gen", block=g(512), lds=2 * 1025 * 8, attr=0), N=2048, M=2, n_streams=2, n_frames=7)      # 2 * 256 items: doubled while 2 t <= 512

    # ---- solve split.  K = 257, 128 streams: 32 896 problems, 514 workgroups, remainder 2
    row("solve_split", dict(n_prob=32896, pieces=8, main_prob=32768, tail_prob=128, scratch=1, grid=g(512), tail_grid=g(16), block=g(256)), N=512, M=8, n_streams=128, n_loop=61)
    row("solve_split", dict(pieces=4, main_prob=32768, tail_prob=128, scratch=1, grid=g(512), tail_grid=g(8)), N=512, M=8, n_streams=128, n_loop=19)      # 19 / 8 = 2 < 4
    row("solve_split", dict(pieces=1, main_prob=40 * 257, tail_prob=0, scratch=0, grid=g(161)), N=512, M=8, n_streams=40, n_loop=61)
    row("solve_split", dict(pieces=1, main_prob=64 * 257, tail_prob=0, scratch=0, grid=g(257)), N=512, M=8, n_streams=64, n_loop=61)
    row("solve_split", dict(n_prob=33000, pieces=2, main_prob=32768, tail_prob=232, scratch=1, grid=g(512), tail_grid=g(8)), N=64, M=16, n_streams=1000, n_loop=8)      # 516 workgroups, 8 / 4 = 2 < 4
    row("solve_split", dict(n_prob=131328, pieces=8, main_prob=131072, tail_prob=256, scratch=1, grid=g(2048), tail_grid=g(32)), N=1024, M=8, n_streams=256, n_loop=64)   # 2052 workgroups
    n129 = next(n for n in range(64, 100000) if ceil_div(513 * n, 64) % 512 == 129)     # past a whole round, a remainder of 129 workgroups: too many for a tail
    row("solve_split", dict(pieces=1, scratch=0, grid=g(ceil_div(513 * n129, 64)), main_prob=513 * n129), N=1024, M=8, n_streams=n129, n_loop=64)
    for n in (64, 128):                                                                 # K = 512: exactly 512 and 1024 workgroups
        row("solve_split", dict(pieces=1, scratch=0, grid=g(8 * n), tail_prob=0), N=1022, M=8, n_streams=n, n_loop=64)
    row("solve_split", dict(pieces=1, scratch=0, grid=g(514)), N=512, M=8, n_streams=128, n_loop=7)      # 7 / 2 = 3 < 4: no piece is worth it

    # ---- solve choice
    for M, Q, full in ((3, 1, 0), (4, 1, 1), (15, 4, 0), (16, 4, 1)):
        row("solve_choice", dict(form="solve_hand", Q=Q, full=full, S=1, nulls=0, weight="none", noise=0, have=1, lds=0), N=64, M=M, n_sources=1)
        row("solve_choice", dict(form="solve_template", Q=Q, full=full, S=1, nulls=0, weight="frame", noise=1, have=1, lds=0), N=64, M=M, n_sources=1, pf_on=1)
    # nulls: one instantiation serves M = 4Q and M < 4Q; u parked in LDS, 256 * 8 Q S bytes, + 256 * 12 S where the directions take two passes (Q = 4, S = 4)
    row("solve_choice", dict(form="solve_template", Q=1, full=0, S=2, nulls=1, weight="none", noise=0, have=1, lds=4096), N=64, M=4, n_sources=2, null_gain=7.5)
    row("solve_choice", dict(form="solve_template", Q=4, full=0, S=4, nulls=1, weight="cell", noise=1, have=1, lds=256 * (128 + 48)), N=64, M=16, n_sources=4, null_gain=7.5,
        update=1, masked=1, pf_on=1)
    row("solve_choice", dict(form="solve_template", Q=1, full=1, S=2, nulls=0, weight="none", noise=0, have=1, lds=0), N=64, M=4, n_sources=2, null_gain=1e-50)
    row("solve_choice", dict(form="solve_template", S=1, nulls=0, weight="frame", noise=0, have=1), N=64, M=4, n_sources=1, null_gain=7.5, update=1)      # one direction: nothing to null
    row("solve_choice", dict(form="solve_template", weight="cell", noise=0, have=1), N=64, M=6, n_sources=1, update=1, masked=1)
    row("solve_choice", dict(form="solve_template", weight="none", noise=0, have=1), N=64, M=6, n_sources=2, masked=1)      # masked without a mask: all 1
    for pf in (0, 1):
        row("solve_choice", dict(form="solve_rtf", Q=2, full=0, S=2, nulls=0, weight="cell", noise=pf, have=1, lds=0), N=64, M=6, rtf=1, n_sources=2, masked=1, pf_on=pf)
        row("solve_choice", dict(form="solve_rtf", Q=2, full=1, S=1, nulls=0, weight="cell", noise=pf, have=1, lds=0), N=64, M=8, rtf=1, n_sources=1, update=1, masked=1, pf_on=pf, null_gain=7.5)
        row("solve_choice", dict(form="solve_rtf_nulls", Q=1, full=0, S=2, nulls=1, weight="cell", noise=pf, have=1, lds=4096), N=64, M=4, rtf=1, n_sources=2, masked=1, pf_on=pf, null_gain=7.5)

    # ---- RTF chunks: 3 streams x 2 directions x 33 bins x 4 microphones = 792 cells a frame; 198 problems: 4 workgroups
    rtf = dict(N=64, M=4, n_streams=3, n_sources=2, n_frames=9)
    row("rtf", dict(fc=9, grid=g(4), block=g(256), lds=0), cap_cells=9 * 792, **rtf)
    row("rtf", dict(fc=3), cap_cells=4 * 792 + 791, **rtf)     # room for 4 frames: 3 chunks of 3
    row("rtf", dict(fc=5), cap_cells=8 * 792, **rtf)           # room for 8: 5 + 4
    row("rtf", dict(fc=1, grid=g(4)), cap_cells=100, **rtf)    # room for less than one frame
    row("estmask", dict(grid=g(8), block=g(256), lds=0), N=64, M=4, n_streams=3, n_frames=5)             # 495 cells, 64 a workgroup
    row("postfilter", dict(grid=g(1), block=g(256), lds=0), N=64, M=4, n_streams=3, n_sources=2)         # 198 cells, 256 a workgroup
    row("postfilter", dict(grid=g(1026)), N=1024, M=8, n_streams=256, n_sources=2)                       # 262 656 cells = 1026 x 256
    row("postfilter", dict(grid=g(7)), N=512, M=8, n_streams=3, n_sources=2)                             # 1 542 cells = 6 x 256 + 6

    # ---- synthesis: 80 outputs: 80 * 4 = 320, 80 * 8 = 640, 80 * 16 = 1280 -> ft 4
    row("synth", dict(ft=4, grid=g(16, 80), block=g(256), lds=257 * 8 + 256 * 4, attr=0), N=512, M=8, n_streams=40, n_sources=2, n_frames=61)
    row("synth", dict(ft=16, grid=g(4, 512), block=g(256), lds=513 * 8 + 512 * 4), N=1024, M=8, n_streams=256, n_sources=2, n_frames=64)
    row("synth", dict(ft=2, grid=g(3, 3), block=g(512), lds=1025 * 8 + 1024 * 4), N=2048, M=8, n_streams=3, n_sources=1, n_frames=5)

    # ---- scans.  LDS of the Capon scans: 64 * (tri * 8 + 4); N = 1024: 17 + 32 phasors a microphone
    whole = dict(N=1024, bin_lo=0, bin_hi=512, Dpad=384)
    row("spectrum", dict(chunk0=0, n_chunks=9, n_slices=36, nhi=17, nph=49, pass_=5, lds=64 * (136 * 8 + 4), attr=1, per_part=9 * 4 * 384, scan_grid=g(45)), M=16, n_streams=5, **whole)
    assert 64 * (136 * 8 + 4) == 69888
    row("spectrum", dict(lds=18688, attr=0), M=8, n_streams=5, **whole)
    row("spectrum", dict(chunk0=1, n_chunks=1, n_slices=4, scan_grid=g(5)), N=1024, M=8, bin_lo=70, bin_hi=100, Dpad=384, n_streams=5)      # inside one chunk
    row("spectrum", dict(chunk0=1, n_chunks=2, scan_grid=g(10)), N=1024, M=8, bin_lo=64, bin_hi=128, Dpad=384, n_streams=5)                 # both ends on chunk boundaries
    row("spectrum", dict(chunk0=1, n_chunks=1), N=1024, M=8, bin_lo=64, bin_hi=127, Dpad=384, n_streams=5)
    row("tracks", dict(n_chunks=9, pass_=5, per_part=2 * 9 * 4 * 384, per_u=0, per_f=0, tables_grid=g(10), scan_grid=g(90)), M=8, n_own=2, n_streams=5, **whole)
    # the map: 2048 directions at N = 1024: 16 tiles, 9 * 4 * 2048 floats (288 KiB) a stream
    row("map", dict(n_chunks=9, n_tiles=16, pass_=3, per_part=73728, scan_grid=g(432), lds=18688), N=1024, M=8, bin_lo=0, bin_hi=512, Dpad=2048, n_streams=3, cap_cells=1 << 27)
    small = dict(N=64, M=4, bin_lo=0, bin_hi=32, Dpad=64, n_streams=5)       # 8 x 3 directions: one chunk, one tile, 256 floats a stream
    row("map", dict(n_chunks=1, n_tiles=1, nhi=2, nph=34, pass_=5, per_part=256, scan_grid=g(5), last_scan_grid=g(5)), cap_cells=1 << 27, **small)
    row("map", dict(pass_=2, scan_grid=g(2), last_scan_grid=g(1)), cap_cells=256, **small)       # 512 floats under the cap: 2 of 5
    row("map", dict(pass_=2), cap_cells=383, **small)
    row("map", dict(pass_=1, scan_grid=g(1)), cap_cells=1, **small)                              # below one stream
    # map-mode tracks, one own track: U 64 * 4 float2, F 64 ints, part 256 floats: 2 * 256 + 64 + 256 = 832 floats a stream
    row("tracks_map", dict(pass_=5, per_u=256, per_f=64, per_part=256, tables_grid=g(5), vectors_grid=g(5), scan_grid=g(5)), n_own=1, cap_cells=1 << 27, **small)
    row("tracks_map", dict(pass_=2, tables_grid=g(2), last_scan_grid=g(1)), n_own=1, cap_cells=832, **small)
    row("tracks_map", dict(pass_=1), n_own=1, cap_cells=831, **small)
    row("tracks_map", dict(pass_=1), n_own=1, cap_cells=1, **small)
    row("tracks_map", dict(pass_=5, per_u=0, per_f=0, per_part=0), n_own=0, cap_cells=1, **small)      # no own track: one pass of all streams, no workspace
    row("tracks_map", dict(n_chunks=9, n_tiles=16, per_u=2 * 9 * 64 * 8, per_f=2 * 9 * 64, per_part=2 * 73728, pass_=3, vectors_grid=g(54), scan_grid=g(864)), N=1024, M=8, bin_lo=0,
        bin_hi=512, Dpad=2048, n_own=2, n_streams=3, cap_cells=1 << 27)
    return t


def test_the_plans_of_the_table(clis):
    t = table()
    for cli in clis:
        for (stage, q, want), got in zip(t, ask(cli, [(s, q) for s, q, _ in t])):
            print(stage, q, "->", got)
            want = {("pass" if k == "pass_" else k): v for k, v in want.items()}
            assert {k: got.get(k) for k in want} == want, (stage, q)


def sweep():
    """every solve a call can ask for: the facts mvdr_frames_dev derives, over every microphone count and number of look directions"""
    qs = []
    for M in range(2, 17):
        for S in (1, 2, 3, 4):
            for gain in (0.0, 7.5):
                for pf in (0, 1):
                    for update, masked in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        qs.append(("solve_choice", dict(N=64, M=M, n_sources=S, null_gain=gain, update=update, masked=masked, pf_on=pf)))
                    for update in (0, 1):                                 # (the RTF and auto calls: masked always)
                        qs.append(("solve_choice", dict(N=64, M=M, rtf=1, n_sources=S, null_gain=gain, update=update, masked=1, pf_on=pf)))
    return qs


def test_the_rows_built_are_the_rows_reachable(clis):
    cli = clis[0]
    text = subprocess.run([cli], input="rows\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert text[-1] == "end"
    keys = ("form", "Q", "full", "S", "nulls", "weight", "noise")
    built = {tuple(parse(ln)[k] for k in keys) for ln in text[:-1]}
    # 8 hand-written kernels; per (weight, noise) 4 x (2 x 4 without nulls + 3 with) = 44 rows less the 8 single-look rows without weights; the RTF
    # kernels 4 x 2 x 4 and 4 x 3 with nulls, each with and without the noise plane
    assert len(built) == 8 + (44 - 8) + 4 * 44 + 2 * 32 + 2 * 12
    qs = sweep() + [(s, q) for s, q, _ in table() if s == "solve_choice"]
    reached = set()
    for ans in ask(cli, qs):
        assert ans["have"] == 1, ans                                    # the plan returned a choice the build lacks
        reached.add(tuple(ans[k] for k in keys))
    print("built %d rows, reached %d, built and never launched: %s" % (len(built), len(reached), sorted(built - reached)))
    assert reached == built
