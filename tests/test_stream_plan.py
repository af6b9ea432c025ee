"""The launch plans of the stream path (csrc/stream_plan.h) on the CPU: tests/cxx/stream_plan_cli.cpp is compiled
with the HIP compiler's host pass only (no device code, no HIP call) and prints the plan of every query given to it.  It is built a second
time with the address and undefined-behaviour sanitizers, as a stand-alone program, and the same table goes through both.

Frames per wave, the skew of the resident round, the K split and the grids change no output bit -- their only effect is speed -- so no
comparison of outputs sees a regression in them.  This table does.

Expected rows: worked out by hand from the formulas of the host layer before the plans existed (api.hip at "Stream path: a call's
decisions travel in a call record") with 256 compute units, and confirmed against that build's dispatch trace
(profiles/r25_launch_plan_dispatch.log) -- never taken from the plan functions.  The constants behind the LDS sizes: 1 152 words of the
1024-point transform's table and of a wave's scratch, 576 words of the 512-point scratch, its tables 1 344 (832 up to the window).

The shape of a context is what mca_hip_create derives from a configuration; shape() repeats those rules (uniformly spaced microphones)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32, FP16X3, FP16, ADAPTIVE = 0, 1, 2, 3


def round_up(v, m):
    return (v + m - 1) // m * m


def shape(M, N=1024, D=361, S=1, prec=ADAPTIVE, ula=None, gate=0, no_phat=0, fold=None, n_cu=256):
    ula = (M > 2) if ula is None else ula
    P = M * (M - 1) // 2
    G = M - 1 if ula else P
    K, H = N // 2 + 1, N // 2
    Dp = 64 if (D <= 64 and prec != FP32) else round_up(D, 192)
    n512, n2048, generic = int(N == 512 and M <= 8), int(N == 2048), int(N != 1024)
    merged = int(bool(ula) and (not generic or n2048) and not n512 and M in (4, 8) and prec in (ADAPTIVE, FP16) and Dp % 64 == 0)
    n_merged = int(np.unique(np.outer(np.arange(K), np.arange(1, G + 1))).size) if merged else 0
    fold = (merged and N == 1024 and D % 2 == 1 and Dp == 384) if fold is None else fold
    return dict(M=M, P=P, G=G, D=D, Dp=Dp, K=K, N=N, H=H, Kp=round_up(G * K * 2, 32), S=S, prec=prec, ula=int(ula), generic=generic, n512=n512, n2048=n2048,
                merged=merged, n_merged=n_merged, Kp_m=2 * round_up(n_merged, 64), fold=int(bool(fold)), tab_planes=2 if prec in (FP16X3, ADAPTIVE) else 1,
                n_cu=n_cu, bf_pairs=M if n2048 else (M + 1) // 2, gate=gate, no_phat=no_phat)


def build_cli(tmp, name, extra):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc) or shutil.which(hipcc), "no HIP compiler"
    exe = tmp / name
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "mcarray_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "stream_plan_cli.cpp"), "-o", str(exe)] + extra)
    return str(exe)


@pytest.fixture(scope="module")
def clis(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("plan")
    return [build_cli(tmp, "stream_plan_cli", []), build_cli(tmp, "stream_plan_cli_san", ["-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def parse(line):
    line, _, why = line.partition(" why=")
    out = {}
    for tok in line.split():
        k, v = tok.split("=")
        out[k] = tuple(int(x) for x in v.split(",")) if "," in v else (v if k == "form" else int(v))
    if why:
        out["why"] = why
    return out


def ask(cli, queries):
    """queries: (stage, dict) -> the parsed answer per query"""
    text = "".join("%s %s\n" % (stage, " ".join("%s=%d" % kv for kv in q.items())) for stage, q in queries)
    lines = subprocess.run([cli], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(queries)
    return [parse(ln) for ln in lines]


FORM_KEYS = {"pick": ("pl", "mode"), "repick": ("pl", "patch"), "gemm_f16": ("split", "bn"), "gemm_repair": ("bn",), "bf_wave_ms": ("npt", "odd"), "bf_wave": ("odd",),
             "bf_ola": ("cpw", "occ")}
STFT_KEYS = ("mt", "ula", "f32", "pl2", "power", "nophat", "merge", "cand", "fuse")


def form_of(ans):
    f = ans["form"]
    return (f,) + tuple(ans[k] for k in (STFT_KEYS if f.startswith("stft_") else FORM_KEYS.get(f, ())))


U8 = shape(8)                      # the flagship: 8-microphone ULA, N = 1024, D = 361, Dp = 384, 1 962 merged terms, folding
STFT0 = dict(mt=0, ula=0, f32=0, pl2=0, power=0, nophat=0, merge=0, cand=0, fuse=0)


def stft(family, **kw):
    return dict(STFT0, form="stft_" + family, have=1, **kw)


def g(x, y=1, z=1):
    return (x, y, z)


def table():
    """(stage, query, expected fields)"""
    t = []

    def analysis(sh, want, **q):
        t.append(("analysis", dict(sh, **q), want))
    # ---- the issue's rows
    mf = dict(fl_merged=1, steer=1)
    analysis(U8, dict(stft("wave", mt=8, ula=1, merge=1, fuse=1), fpb=16, skew=3, grid=g(8, 64), block=g(256), lds=(1152 + 898 + 4 * 1984 + 4 * 56) * 8, steers=1), n_arrays=8, n_frames=4096, **mf)
    analysis(shape(8, gate=1), dict(stft("wave", mt=8, ula=1, merge=1, power=1), fpb=16, skew=3, grid=g(8, 64), block=g(256), lds=79888, steers=0), n_arrays=8, n_frames=4096, fl_merged=1, power=1)
    analysis(U8, dict(stft("wave", mt=8, ula=1, merge=1, fuse=1), fpb=16, skew=3, grid=g(128, 4), block=g(256), lds=81680), n_arrays=128, n_frames=256, **mf)
    analysis(U8, dict(stft("wave", mt=8, ula=1, merge=1, fuse=1), fpb=16, skew=0, grid=g(64, 8), block=g(256), lds=81680), n_arrays=8, n_frames=4095, **mf)
    analysis(shape(8, prec=FP32), dict(stft("wave", mt=8, ula=1, f32=1), fpb=1, skew=0, grid=g(16, 2), block=g(256), lds=(1152 + 4608 + 16) * 8, steers=0), f32=1, n_arrays=2, n_frames=64)
    for cand in (0, 1):
        analysis(shape(4), dict(stft("wave", mt=4, ula=1, pl2=1, cand=cand), fpb=1, skew=0, grid=g(100, 1), block=g(256), lds=46144), planes=2, n_arrays=8, n_frames=4096,
                 list_groups=100, list_cap=512, cand_on=cand)
    # ---- 16-microphone ULA on k_stft_phat_wave16, with and without the skew: (1152 + 4 * 1152 + 64 fpa) * 8 + (1024 + 4 fpa) * 4, fpa = fpb + skew
    analysis(shape(16), dict(stft("wave16", ula=1), fpb=16, skew=3, grid=g(8, 64), block=g(256), lds=60208), n_arrays=8, n_frames=4096)
    analysis(shape(16), dict(stft("wave16", ula=1), fpb=16, skew=0, grid=g(64, 8), block=g(256), lds=58624), n_arrays=8, n_frames=4095)
    # ---- 512-sample frames: (2 * 8 * 258 + 8 * 576 + 832 + fpb M) * 8 + 32 fpb; runs wanted: 512, two frames at least
    analysis(shape(4, N=512, prec=FP16), dict(stft("512", mt=4, ula=1), fpb=2, grid=g(80, 2), block=g(512), lds=76672), n_arrays=2, n_frames=160)
    analysis(shape(8, N=512, prec=FP32), dict(stft("512", mt=8, ula=1, f32=1), fpb=8, grid=g(512, 8), block=g(512), lds=77312), f32=1, n_arrays=8, n_frames=4096)
    analysis(shape(3, N=512, prec=FP16), dict(stft("512", mt=0, ula=1), fpb=2, grid=g(80, 2), block=g(512), lds=76656), n_arrays=2, n_frames=160)
    # ---- 2048-sample frames: (fp mr 1026 + 1152 + 8 * 1152 + fpb M) * 8 + 32 fpb, fp mr = 8; the merged index at 4 / 8 microphones of a ULA's one plane
    analysis(shape(4, N=2048, prec=FP16), dict(stft("2048", mt=4, ula=1, merge=1), fpb=2, grid=g(80, 2), block=g(512), lds=148736), n_arrays=2, n_frames=160, fl_merged=1)
    analysis(shape(8, N=2048, prec=FP32), dict(stft("2048", mt=8, ula=1, f32=1), fpb=16, grid=g(256, 8), block=g(512), lds=150144), f32=1, n_arrays=8, n_frames=4096)
    analysis(shape(3, N=2048, prec=FP16X3), dict(stft("2048", mt=0, ula=1), fpb=2, grid=g(80, 2), block=g(512), lds=148720), planes=2, n_arrays=2, n_frames=160)
    analysis(shape(8, N=2048, prec=ADAPTIVE), dict(stft("2048", mt=8, ula=1, merge=1), fpb=16, grid=g(256, 8), block=g(512), lds=150144), n_arrays=8, n_frames=4096, fl_merged=1)
    analysis(shape(8, N=2048, prec=ADAPTIVE), dict(stft("2048", mt=8, ula=1), fpb=4, grid=g(100, 1), block=g(512), lds=(8208 + 1152 + 9216 + 32) * 8 + 128), planes=2, n_arrays=8,
             n_frames=4096, list_groups=100, list_cap=512)
    # ---- 2 microphones: k_stft_phat_few at 1024 ((8 * 576 + 1344 + 2 fpb) * 8 + 32 fpb, 256 runs wanted), the sub-sequence kernel at 2048 / 4096
    analysis(shape(2, prec=FP32), dict(stft("few", mt=2, f32=1), fpb=1, grid=g(160, 2), block=g(512), lds=47664), f32=1, n_arrays=2, n_frames=160)
    analysis(shape(2, N=2048, prec=FP16), dict(stft("sub2", mt=4), fpb=2, grid=g(80, 2), block=g(512), lds=76672), n_arrays=2, n_frames=160)
    analysis(shape(2, N=4096, prec=FP32), dict(stft("sub2", mt=8, f32=1), fpb=8, grid=g(32, 128), block=g(512), lds=76672), f32=1, n_arrays=128, n_frames=256)
    # ---- any length: a frame per workgroup, M (H + 1) * 8 + 16 bytes, 256 / 1024 / 1024 threads
    analysis(shape(4, N=256, prec=FP16), dict(stft("gen"), grid=g(160, 2), block=g(256), lds=4144), n_arrays=2, n_frames=160)
    analysis(shape(3, N=4096, prec=FP32), dict(stft("gen", f32=1), grid=g(64, 2), block=g(1024), lds=49192), f32=1, n_arrays=2, n_frames=64)
    # ---- the block kernel: exact rows of 16 microphones, any other count; list mode takes REPAIR_GROUP frames per unit
    analysis(shape(16), dict(stft("block", mt=16, ula=1), fpb=4, grid=g(512, 1), block=g(512), lds=(16 * 576 + 1344 + 64) * 8 + 128), planes=2, n_arrays=8, n_frames=4096,
             list_groups=8000, list_cap=512)
    analysis(shape(5, prec=FP32), dict(stft("block", mt=0, ula=1, f32=1), fpb=16, grid=g(256, 8), block=g(512), lds=(5 * 576 + 1344 + 80) * 8 + 512), f32=1, n_arrays=8, n_frames=4096)

    def contraction(sh, want, planes, rows):
        t.append(("contraction", dict(sh, planes=planes, rows=rows, rows_planned=rows, rows_planned_chunk=rows), dict(want, have=1)))
    v = dict(block=g(512), lds=163840)
    contraction(U8, dict(form="gemm_fold", ksplit=2, grid=g(128, 2), block=g(512), lds=4 * 448 * 64), 1, 32768)
    contraction(U8, dict(form="gemm_fold", ksplit=2, grid=g(64, 2), block=g(512), lds=114688), 1, 16384)
    contraction(U8, dict(v, form="gemm_v3", ksplit=1, grid=g(256, 1)), 1, 65536)
    contraction(U8, dict(v, form="gemm_v2", ksplit=2, grid=g(128, 2)), 2, 32768)
    contraction(shape(16, prec=FP16), dict(form="gemm_f16", split=0, bn=192, ksplit=16, grid=g(1, 2, 16), block=g(256), lds=0), 1, 128)
    # 16 microphones, 15 392 terms: quarters below 32 768 rows; the merged rows of 2048-sample frames (7 936 deep) too
    contraction(shape(16), dict(v, form="gemm_v3", ksplit=4, grid=g(64, 4)), 1, 16384)
    assert shape(8, N=2048)["Kp_m"] == 7936
    contraction(shape(8, N=2048), dict(v, form="gemm_v3", ksplit=4, grid=g(64, 4)), 1, 16384)
    contraction(shape(8, fold=0), dict(v, form="gemm_v3", ksplit=2, grid=g(64, 2)), 1, 16384)
    # a 5-degree grid (D = 37, Dp = 64): 3 row tiles, 512 / 3 workgroups wanted, at least 8 K steps each: 3 968 / 32 / 8 = 15; two planes of 7 200: 16 at most
    contraction(shape(8, D=37, prec=FP16), dict(form="gemm_f16", split=0, bn=64, ksplit=15, grid=g(3, 1, 15), block=g(256), lds=0), 1, 320)
    contraction(shape(8, D=37, prec=FP16X3), dict(form="gemm_f16", split=1, bn=64, ksplit=16, grid=g(3, 1, 16), block=g(256), lds=0), 2, 320)
    contraction(shape(8, prec=FP32), dict(form="gemm_f32", ksplit=4, grid=g(64, 2, 4), block=g(256), lds=0), 1, 8192)
    t.append(("repair_contraction", dict(U8, pass_rows=4096, repair_ksplit=32), dict(form="gemm_repair", bn=192, have=1, col_tiles=2, grid=g(768), block=g(256), patch_grid=g(2048), patch_block=g(128))))
    t.append(("repair_contraction", dict(shape(8, D=37), pass_rows=128, repair_ksplit=8), dict(form="gemm_repair", bn=64, have=1, col_tiles=1, grid=g(8), block=g(256), patch_grid=g(128), patch_block=g(128))))

    # ---- picks: 8 x 4096 frames are 128 chunks per array
    big = dict(n_arrays=8, n_chunks=128)
    t.append(("pick", dict(U8, adaptive=1, **big), dict(form="pick", pl=6, mode=1, have=1, grid=g(128, 8), block=g(512), lds=32 * 392 * 4)))
    t.append(("repick", dict(U8, patch=1, **big), dict(form="repick", pl=6, patch=1, have=1, grid=g(512), block=g(512), lds=50176 + (1152 + 8 * 1152) * 8, may_patch=1)))
    t.append(("repick", dict(U8, patch=0, **big), dict(form="repick", pl=6, patch=0, have=1, grid=g(256), block=g(512), lds=50176)))
    for D, pl in ((130, 2), (131, 6), (386, 6), (387, 8)):
        t.append(("pick", dict(shape(8, D=D), adaptive=0, **big), dict(pl=pl, mode=0, have=1, lds=32 * (round_up(D, 192) + 8) * 4, block=g(512))))
        t.append(("repick", dict(shape(8, D=D), patch=0, n_arrays=1, n_chunks=4), dict(pl=pl, grid=g(4), may_patch=int(pl != 8))))
    t.append(("pick", dict(shape(8, D=37), adaptive=1, **big), dict(pl=2, mode=1, lds=32 * 72 * 4, block=g(512), grid=g(128, 8))))
    t.append(("pick", dict(shape(8, D=513, prec=FP32), adaptive=0, **big), dict(pl=8, block=g(576), lds=32 * 584 * 4)))
    t.append(("repick", dict(shape(8, D=451), patch=0, **big), dict(pl=8, patch=0, block=g(512), grid=g(256), lds=32 * 584 * 4, may_patch=0)))

    # ---- beamformers
    t.append(("steer", dict(U8, n_arrays=8, np=4096), dict(ft=16, synth_grid=g(64, 8), patch_grid=g(512), block=g(256), lds=46080)))
    t.append(("steer", dict(U8, n_arrays=2, np=160), dict(ft=2, synth_grid=g(20, 2), patch_grid=g(40), block=g(256), lds=46080)))

    def beamform(sh, want, n_arrays, n_frames, table=1, **q):
        t.append(("beamform", dict(sh, table=table, n_arrays=n_arrays, n_frames=n_frames, **q), dict(dict(have=1, unsupported=0), **want)))
    beamform(U8, dict(form="bf_wave", odd=0, ft=17, skew=3, grid=g(8, 62, 1), block=g(256), lds=54272), 8, 4096)
    beamform(shape(5), dict(form="bf_wave", odd=1, ft=2, skew=0, grid=g(23, 2, 1), block=g(256), lds=54272), 2, 160)
    # several sources up to 8 microphones: 46 080 + 4 S * 512 * 4 bytes, 2048 runs wanted, two frames at least
    beamform(shape(8, S=2), dict(form="bf_wave_ms", npt=4, odd=0, ft=16, grid=g(64, 8), block=g(256), lds=62464), 8, 4096)
    beamform(shape(5, S=2), dict(form="bf_wave_ms", npt=3, odd=1, ft=2, grid=g(20, 2), block=g(256), lds=62464), 2, 160)
    beamform(shape(2, S=2), dict(form="bf_wave_ms", npt=1, odd=0), 2, 160)
    # 16 microphones, 3 sources: one beamformed slot; (16 + 3) * 576 * 8 + 3 * 16 * 49 * 8 + 1344 * 8 + 16 * 4 * 8 + 5 * 3 * 8
    beamform(shape(16, S=3), dict(form="bf_ola", cpw=2, occ=2, ft=4, nb=1, grid=g(40, 2), block=g(512), lds=117752), 2, 160)
    beamform(U8, dict(form="bf_ola", cpw=1, occ=4, ft=64, nb=4, grid=g(64, 8), block=g(512), lds=(8 + 4) * 4608 + 8 * 49 * 8 + 10752 + 4 * 8 * 2 * 8 + 65 * 8), 8, 4096, table=0)
    # 512-sample frames: (2 * 8 * 258 + 8 * 576 + 832 + 2 S M 41) * 8 + 16 S = 81 808 <= 80 KiB: two workgroups per CU, 512 runs wanted
    beamform(shape(8, N=512), dict(form="bf_512", ft=64, grid=g(64, 8), block=g(512), lds=81808), 8, 4096)
    # any length, 16 microphones at 2048 samples, 4 sources: M + 2 spectra fit a CU; 20 * 1025 * 8 + 4 * 4096 = 180 384 bytes want one workgroup per CU
    beamform(shape(16, N=2048, S=4), dict(form="bf_gen", ft=4, s_pass=2, grid=g(40, 2), block=g(512), lds=18 * 8200 + 8192 + 80 + 8), 2, 160, table=0)
    beamform(shape(8, N=2048), dict(form="bf_wave_2048", ft=17, grid=g(62, 8, 1), block=g(256), lds=(1152 + 4608 + 2048) * 8), 8, 4096)
    beamform(shape(8, N=2048), dict(form="bf_gen", s_pass=1, block=g(512)), 8, 4096, out_aligned=0)
    # the two limits (shapes mca_hip_create refuses or never builds: the plan is asked directly)
    beamform(shape(4, N=8192), dict(form="bf_gen", unsupported=1, why="fft_size x n_mics exceeds the 160 KiB LDS of a CU"), 2, 160, table=0)
    beamform(shape(24, S=4), dict(form="bf_ola", unsupported=1, why="n_mics/n_sources combination exceeds the 160 KiB LDS of a CU"), 2, 160, table=0)
    return t


def test_the_plans_of_the_table(clis):
    t = table()
    for cli in clis:
        for (stage, q, want), got in zip(t, ask(cli, [(s, q) for s, q, _ in t])):
            print(stage, {k: q[k] for k in q if k not in U8 or q[k] != U8[k]}, "->", got)
            assert {k: got.get(k) for k in want} == want, (stage, q)


# k_scan_repick<8, true> is built and never launched: the patching second pick is refused from D - 2 > 384 on (repick_may_patch), which is
# where PL = 8 begins
UNREACHABLE = {("repick", 8, 1)}


def sweep():
    """every launch api.hip can ask for over a sweep of contexts and small calls, with the flags its call sites derive"""
    qs = []
    calls = [(1, 1), (1, 64), (2, 160), (3, 100), (8, 512), (8, 4096), (128, 256), (64, 1024)]
    for M in (2, 3, 4, 5, 6, 7, 8, 16):
        for ula in ((0, 1) if M > 2 else (0,)):
            for N in (256, 512, 1024, 2048, 4096):
                for prec in (FP32, FP16X3, FP16, ADAPTIVE):
                    for gate in (0, 1):
                        for no_phat in ((0, 1) if prec == FP32 and N == 1024 and M in (4, 8) else (0,)):
                            for D in (37, 361, 451):
                                if D != 361 and (N != 1024 or gate):
                                    continue
                                sh = shape(M, N=N, D=D, prec=prec, ula=ula, gate=gate, no_phat=no_phat)
                                for S in ((1, 2, 3) if D == 361 else ()):
                                    shs = dict(sh, S=S)
                                    for a, f in calls[:4]:
                                        qs.append(("beamform", dict(shs, table=1, n_arrays=a, n_frames=f)))
                                        qs.append(("beamform", dict(shs, table=0, n_arrays=a, n_frames=f)))
                                adaptive = prec == ADAPTIVE and M > 2 and (N == 1024 or (N in (512, 2048) and M <= 8))
                                # (... and a ULA whose float delays fail the proportionality check of build_merged_tables keeps the per-group index)
                                for sh in ([sh, dict(sh, merged=0, n_merged=0, Kp_m=0, fold=0)] if sh["merged"] and D == 361 else [sh]):
                                  for a, f in calls:
                                      for planes in ((1,) if prec in (FP32, FP16) else (2,) if not adaptive else (1, 2)):
                                          fl = dict(power=gate, fl_merged=int(sh["merged"] and planes == 1), fl_no_phat=no_phat)
                                          for steer in ((0, 1) if fl["fl_merged"] and not gate and M == 8 and N == 1024 else (0,)):
                                              qs.append(("analysis", dict(sh, f32=int(prec == FP32), planes=planes, n_arrays=a, n_frames=f, steer=steer, **fl)))
                                          qs.append(("contraction", dict(sh, planes=planes, rows=a * f, rows_planned=a * f, rows_planned_chunk=a * f)))
                                      if adaptive:
                                          lazy = M in (4, 8) and N == 1024 and not gate
                                          for cand in ((0, 1) if lazy else (0,)):
                                              qs.append(("analysis", dict(sh, planes=2, n_arrays=a, n_frames=f, list_groups=(f + 3) // 4 * a, list_cap=512, cand_on=cand)))
                                          qs.append(("repair_contraction", dict(sh, pass_rows=128, repair_ksplit=8)))
                                      n_chunks = (f + 31) // 32
                                      qs.append(("pick", dict(sh, adaptive=int(adaptive), n_arrays=a, n_chunks=n_chunks)))
                                      if adaptive:
                                          steered = M == 8 and ula and N == 1024 and not gate and sh["merged"] and (D - 2 <= 384)      # (steer_applies, repick_may_patch)
                                          for patch in ((0, 1) if steered else (0,)):
                                              qs.append(("repick", dict(sh, patch=patch, n_arrays=a, n_chunks=n_chunks)))
    return qs


def test_the_rows_built_are_the_rows_reachable(clis):
    cli = clis[0]
    text = subprocess.run([cli], input="rows\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert text[-1] == "end"
    built = {form_of(parse(ln)) for ln in text[:-1]}
    assert len({f for f in built if f[0] == "stft_wave"}) == 41 and len({f for f in built if f[0] == "stft_2048"}) == 14 and len({f for f in built if f[0] == "stft_512"}) == 12
    qs = sweep() + [(s, q) for s, q, _ in table()[:-2]]                # (not the two shapes beyond mca_hip_create's limits)
    reached = set()
    for stage, ans in zip((s for s, _ in qs), ask(cli, qs)):
        assert ans.get("have", 1) == 1, ans                           # the plan returned a form the build lacks
        if stage == "repick" and ans["patch"]:
            assert ans["may_patch"] == 1
        if "form" in ans:                                             # (the steered passes: two kernels without template arguments)
            reached.add(form_of(ans))
    fixed = {f for f in reached if f[0] in ("gemm_f32", "gemm_v2", "gemm_v3", "gemm_fold", "bf_wave_2048", "bf_512", "bf_gen")}      # families of one kernel: no lookup
    reached -= fixed
    print("built %d rows, reached %d, built and never launched: %s" % (len(built), len(reached), sorted(built - reached)))
    assert reached <= built, sorted(reached - built)
    assert built - reached == UNREACHABLE
