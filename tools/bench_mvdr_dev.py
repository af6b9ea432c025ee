"""Device-side throughput of the MVDR path (BASELINE.json configs[3]: 16 microphones, 256 concurrent streams x 64 frames)
on device buffers, with the per-kernel split from the library's HIP events and a parity spot check of stream 0
against the CPU oracle.  Usage: python tools/bench_mvdr_dev.py [--streams 256] [--frames 64] [--mics 16] [--steps 10]
With --sources S (2 ... 4) it times the sources call with S look directions per frame instead, under --null-gain g (soft nulls
at the other look directions; 0, the default, is the plain sources call), and the spot check goes against the float64 twin of
that call (tests/mvdr_nulls_twin.py).  --update ones / half passes per-frame covariance update weights (the weighted solve kernel):
all 1, or every second run of 8 frames frozen (weight 0; the frames a noise-only covariance freezes, and where the solve reuses
its factor); the spot check then goes against tests/mvdr_gate_twin.py.  The weighted row of DESIGN.md 4.5 is k_mvdr_solve_ms of
--update none, ones and half.  --postfilter enables the decision-directed Wiener post-filter (defaults of
mca_hip_mvdr_set_postfilter): the solve then also writes the noise plane, k_mvdr_postfilter runs behind it, the result carries its
time and its traffic (20 B per cell and the state once each way) as a rate, and the spot check goes against
tests/mvdr_postfilter_twin.py on the scale of the twin's unfiltered audio.  --mask times the table of DESIGN.md 4.7
instead, one JSON line per row: for one and for three look directions the unweighted call, the per-frame weighted call (every second
run of 8 frames frozen) and the masked call (update_mask [streams][F][K]) under a mask of ones, that per-frame pattern along the
bins, blocks of 4 frames x 16 bins half of them open, and independent random binary cells (the worst divergence of the quads of a
wave); a build without the masked entry points (MCA_HIP_LIB) runs the first two rows only.  --rtf times the table of DESIGN.md 4.8, one
JSON line for one and one for two look directions: k_mvdr_rtf, the solve that reads the steering plane beside the masked (CELL) solve
under the same update mask, and both calls' totals; update mask and target masks are complementary blocks of 4 frames x 16 bins.  --estmask times the table of DESIGN.md 4.9, one JSON line for one and one for two look directions: k_mvdr_estmask against its own
traffic (X and T read, S + 1 masks written) as a share of the measured float4 copy rate, and the auto call's total beside the RTF
call fed the masks the auto call returned.  --rtf-nulls times the table of DESIGN.md 4.10, one JSON line for two look directions: the solve
of the RTF call at null gain 0 (k_mvdr_solve_rtf_t) and 100 (k_mvdr_solve_rtf_nulls_t, mca_hip_mvdr_set_rtf_nulls), the CELL nulls solve
of the masked call at gain 100 under the same update mask, and the calls' totals; masks as in --rtf.  --tracks-map times the table of DESIGN.md 4.21, one JSON line for n_own = 1 and one for 2: the update of the tracks in
map mode on a 72 x 19 map, without and with the whole own map, beside the map call and the auto call.  MCA_HIP_LIB may name an older build of the library (the yardstick of a comparison): the entry
points it lacks are left unbound, --null-gain must then stay 0, --update none and --postfilter off (as far as the build lacks them)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mcarray_amd import _lib, api, synth  # noqa: E402

LOOK = [0.35, -0.15, 0.8, -0.45]       # look directions of --sources (radians): the first two 0.5 rad apart


def bind_what_the_library_has():
    """an older build side by side (MCA_HIP_LIB): leave the entry points it lacks unbound"""
    import ctypes as C
    _lib._pin_single_hip_runtime()
    probe = C.CDLL(_lib.LIB_PATH)
    _lib.SYMBOLS = [sym for sym in _lib.SYMBOLS if hasattr(probe, sym[0])]


def mask_table(a, fs, N, xs, pcm, st):
    """the rows of DESIGN.md 4.7: solve kernel and whole call per update rule, for one and three look directions"""
    hop, K = N // 2, N // 2 + 1
    dev = pcm.device
    rng = np.random.default_rng(7)
    frame = np.ones((a.streams, a.frames), dtype=np.float32)
    frame[:, (np.arange(a.frames) // 8) % 2 == 1] = 0.0
    blocks = (rng.random((a.streams, (a.frames + 3) // 4, (K + 15) // 16)) < 0.5).astype(np.float32)
    blocks = np.repeat(np.repeat(blocks, 4, axis=1), 16, axis=2)[:, :a.frames, :K]
    rules = [("unweighted", {}), ("per-frame weights", dict(update=torch.from_numpy(frame).to(dev)))]
    if hasattr(_lib.load(), "mca_hip_mvdr_sources_frames_masked_dev"):
        masks = (("mask of ones", np.ones((a.streams, a.frames, K), dtype=np.float32)),
                 ("mask constant along the bins", np.repeat(frame[:, :, None], K, axis=2)),
                 ("mask of 4 x 16 blocks", blocks),
                 ("mask of random cells", (rng.random((a.streams, a.frames, K)) < 0.5).astype(np.float32)))
        rules += [(name, dict(update_mask=torch.from_numpy(np.ascontiguousarray(m)).to(dev))) for name, m in masks]
    for S in (1, 3):
        look = torch.tensor(LOOK[:S], device=dev, dtype=torch.float32)
        doa = look[None, None, :].expand(a.streams, a.frames, S).contiguous()
        out = torch.empty((a.streams, S, a.frames * hop), device=dev, dtype=torch.float32)
        for name, kw in rules:
            bf = api.MvdrBeamformer(fs, xs, N, max_streams=a.streams, max_sources=S)
            if a.postfilter:
                bf.set_postfilter(True)
            step = lambda: bf.process_sources_dev(pcm, a.frames, doa, out_pcm=out, stream=st, **kw)
            for _ in range(a.warmup):
                step()
            bf.set_timing(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / a.steps
            n, ms = bf.get_timing(bf.K_SOLVE)
            print(json.dumps(dict(rule=name, sources=S, postfilter=bool(a.postfilter), lib=os.environ.get("MCA_HIP_LIB", "default"),
                                  workload="%d streams x %d frames, %d mics, N=%d" % (a.streams, a.frames, a.mics, N),
                                  k_mvdr_solve_ms=ms / max(n, 1), ms_per_step=dt * 1e3)), flush=True)
            bf.close()


def rtf_table(a, fs, N, xs, pcm, st):
    """the rows of DESIGN.md 4.8: the masked call and the RTF call under the same update mask, for one and two look directions"""
    hop, K = N // 2, N // 2 + 1
    dev = pcm.device
    rng = np.random.default_rng(7)
    for S in (1, 2):
        blocks = (rng.random((a.streams, S, (a.frames + 3) // 4, (K + 15) // 16)) < 0.5 / S).astype(np.float32)
        tm = np.ascontiguousarray(np.repeat(np.repeat(blocks, 4, axis=2), 16, axis=3)[:, :, :a.frames, :K])       # the targets' cells
        upd = torch.from_numpy(np.ascontiguousarray(1.0 - tm.max(axis=1))).to(dev)                                  # the noise learns elsewhere
        tmask = torch.from_numpy(tm).to(dev)
        look = torch.tensor(LOOK[:S], device=dev, dtype=torch.float32)
        doa = look[None, None, :].expand(a.streams, a.frames, S).contiguous()
        out = torch.empty((a.streams, S, a.frames * hop), device=dev, dtype=torch.float32)
        row = dict(sources=S, postfilter=bool(a.postfilter), workload="%d streams x %d frames, %d mics, N=%d" % (a.streams, a.frames, a.mics, N),
                   steering_plane_MB=a.streams * S * a.frames * K * a.mics * 8 / 1e6)
        for name, kw in (("masked", dict(update_mask=upd)), ("rtf", dict(update_mask=upd, target_mask=tmask))):
            bf = api.MvdrBeamformer(fs, xs, N, max_streams=a.streams, max_sources=S)
            if a.postfilter:
                bf.set_postfilter(True)
            if name == "rtf":
                bf.set_rtf(True)
            step = lambda: bf.process_sources_dev(pcm, a.frames, doa, out_pcm=out, stream=st, **kw)
            for _ in range(a.warmup):
                step()
            bf.set_timing(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize()
            row[name + "_ms_per_step"] = (time.perf_counter() - t0) / a.steps * 1e3
            n, ms = bf.get_timing(bf.K_SOLVE)
            row[("k_mvdr_solve_cell" if name == "masked" else "k_mvdr_solve_rtf") + "_ms"] = ms / max(n, 1)
            if name == "rtf":
                n, ms = bf.get_timing(bf.K_RTF)
                row["k_mvdr_rtf_ms"] = ms / max(n, 1)
            bf.close()
        print(json.dumps(row), flush=True)


def rtf_nulls_table(a, fs, N, xs, pcm, st, gain=100.0):
    """the row of DESIGN.md 4.10: the RTF call without and with nulls at the estimated vectors beside the masked call with geometric
    nulls, two look directions, the masks of rtf_table()"""
    hop, K = N // 2, N // 2 + 1
    dev = pcm.device
    rng = np.random.default_rng(7)
    S = 2
    blocks = (rng.random((a.streams, S, (a.frames + 3) // 4, (K + 15) // 16)) < 0.5 / S).astype(np.float32)
    tm = np.ascontiguousarray(np.repeat(np.repeat(blocks, 4, axis=2), 16, axis=3)[:, :, :a.frames, :K])
    upd = torch.from_numpy(np.ascontiguousarray(1.0 - tm.max(axis=1))).to(dev)
    tmask = torch.from_numpy(tm).to(dev)
    look = torch.tensor(LOOK[:S], device=dev, dtype=torch.float32)
    doa = look[None, None, :].expand(a.streams, a.frames, S).contiguous()
    out = torch.empty((a.streams, S, a.frames * hop), device=dev, dtype=torch.float32)
    row = dict(sources=S, null_gain=gain, postfilter=bool(a.postfilter), workload="%d streams x %d frames, %d mics, N=%d" % (a.streams, a.frames, a.mics, N))
    for name, g, kw in (("rtf_g0", 0.0, dict(update_mask=upd, target_mask=tmask)), ("rtf_nulls", gain, dict(update_mask=upd, target_mask=tmask)),
                        ("masked_nulls", gain, dict(update_mask=upd))):
        bf = api.MvdrBeamformer(fs, xs, N, max_streams=a.streams, max_sources=S, null_gain=g, rtf_nulls=True)
        if a.postfilter:
            bf.set_postfilter(True)
        if name != "masked_nulls":
            bf.set_rtf(True)
        step = lambda: bf.process_sources_dev(pcm, a.frames, doa, out_pcm=out, stream=st, **kw)
        for _ in range(a.warmup):
            step()
        bf.set_timing(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        row[name + "_ms_per_step"] = (time.perf_counter() - t0) / a.steps * 1e3
        n, ms = bf.get_timing(bf.K_SOLVE)
        row[name + "_solve_ms"] = ms / max(n, 1)
        bf.close()
    print(json.dumps(row), flush=True)


COPY_TBPS = 6.29       # the measured float4 copy rate of the MI355X


def estmask_table(a, fs, N, xs, pcm, st):
    """the rows of DESIGN.md 4.9: k_mvdr_estmask against its traffic, the auto call beside the RTF call fed its masks"""
    hop, K = N // 2, N // 2 + 1
    dev = pcm.device
    nph = N // 64 + 33
    for S in (1, 2):
        look = torch.tensor(LOOK[:S], device=dev, dtype=torch.float32)
        doa = look[None, None, :].expand(a.streams, a.frames, S).contiguous()
        out = torch.empty((a.streams, S, a.frames * hop), device=dev, dtype=torch.float32)
        cells = a.streams * a.frames * K
        traffic = cells * a.mics * 8.0 + a.streams * a.frames * S * a.mics * nph * 8.0 + cells * (S + 1) * 4.0
        row = dict(sources=S, postfilter=bool(a.postfilter), workload="%d streams x %d frames, %d mics, N=%d" % (a.streams, a.frames, a.mics, N),
                   k_mvdr_estmask_bytes=traffic)
        masks = None
        for name in ("auto", "rtf"):
            bf = api.MvdrBeamformer(fs, xs, N, max_streams=a.streams, max_sources=S)
            if a.postfilter:
                bf.set_postfilter(True)
            bf.set_rtf(True)
            if name == "auto":
                # one look direction: absolute thresholds; two: the second is the competitor
                bf.set_mask_estimator(True, coherence_lo=0.2 if S == 1 else 0.0, coherence_hi=0.4 if S == 1 else 0.05, n_protected=1)
                masks = bf.process_sources_dev(pcm, a.frames, doa, out_pcm=out, stream=st, estimate_masks=True)
                # the timed step hands no masks back: they stay in the workspace
                step = lambda: bf._check(bf._lib.mca_hip_mvdr_sources_frames_auto_dev(bf.h, *api.pcm_layout(pcm), a.streams, a.frames, S, api._ptr(doa), None,
                                                                                     None, api._ptr(out), None, st))
            else:
                step = lambda: bf.process_sources_dev(pcm, a.frames, doa, out_pcm=out, stream=st, **masks)
            for _ in range(a.warmup):
                step()
            bf.set_timing(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize()
            row[name + "_ms_per_step"] = (time.perf_counter() - t0) / a.steps * 1e3
            for kid, kname in ((bf.K_ANALYSE, "k_mvdr_analyse"), (bf.K_RTF, "k_mvdr_rtf"), (bf.K_SOLVE, "k_mvdr_solve_rtf")):
                n, ms = bf.get_timing(kid)
                row["%s_%s_ms" % (name, kname)] = ms / max(n, 1)
            if name == "auto":
                n, ms = bf.get_timing(bf.K_ESTMASK)
                row["k_mvdr_estmask_ms"] = ms / max(n, 1)
                row["k_mvdr_estmask_TBps"] = traffic / (ms / max(n, 1) * 1e-3) / 1e12 if ms > 0 else 0.0
                row["k_mvdr_estmask_share_of_copy_rate"] = row["k_mvdr_estmask_TBps"] / COPY_TBPS
                row["protected_cells_share"] = float((masks["update_mask"] < 1).float().mean())
            bf.close()
        print(json.dumps(row), flush=True)


def tracks_table(a, fs, N, xs, pcm, st):
    """the rows of DESIGN.md 4.11: the update of the tracks beside the spectrum call of the same process and beside the auto call that
    feeds it, 361 angles, two look directions of which n_own = 1 and 2 follow their own target covariance"""
    hop = N // 2
    dev = pcm.device
    S = 2
    look = torch.tensor(LOOK[:S], device=dev, dtype=torch.float32)
    doa = look[None, None, :].expand(a.streams, a.frames, S).contiguous()
    out = torch.empty((a.streams, S, a.frames * hop), device=dev, dtype=torch.float32)
    peaks = torch.empty((2, a.streams, S), device=dev, dtype=torch.float32)
    for n_own in (1, 2):
        bf = api.MvdrBeamformer(fs, xs, N, max_streams=a.streams, max_sources=S)
        bf.set_rtf(True)
        bf.set_mask_estimator(True, n_protected=1)
        bf.configure_spectrum(361, n_peaks=S)
        bf.configure_tracks(S, n_own, max_step_rad=0.1, min_sep_rad=0.1, hold=3)
        bf.seed_tracks(np.tile(np.asarray(LOOK[:S], dtype=np.float32), (a.streams, 1)))
        auto = lambda: bf._check(bf._lib.mca_hip_mvdr_sources_frames_auto_dev(bf.h, *api.pcm_layout(pcm), a.streams, a.frames, S, api._ptr(doa), None, None,
                                                                             api._ptr(out), None, st))
        steps = dict(auto=auto, spectrum=lambda: bf.spectrum_dev(a.streams, peak_doa=peaks[0], peak_val=peaks[1], stream=st),
                     update=lambda: bf.update_tracks_dev(a.streams, stream=st))
        row = dict(n_own=n_own, workload="%d streams x %d frames, %d mics, N=%d, 361 angles" % (a.streams, a.frames, a.mics, N))
        for name in ("auto", "spectrum", "update"):
            for _ in range(a.warmup):
                steps[name]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                steps[name]()
            torch.cuda.synchronize()
            row[name + "_ms_per_step"] = (time.perf_counter() - t0) / a.steps * 1e3
        bf.set_timing(True)
        for _ in range(a.steps):
            steps["update"]()
        for kid, kname in ((bf.K_SPECTRUM, "update_capon_kernels_ms"), (bf.K_TRACKS, "update_track_kernels_ms")):
            n, ms = bf.get_timing(kid)
            row[kname] = ms / max(n, 1)
        tr = bf.tracks()
        row["own_tracks_with_a_match"] = float((tr["miss"][:, :n_own] == 0).mean())
        bf.close()
        print(json.dumps(row), flush=True)


def tracks_map_table(a, fs, N, st):
    """the rows of DESIGN.md 4.21: the update of the tracks in map mode beside the map call of the same process and beside the auto
    call that feeds it; a cube of 10 cm, a 72 x 19 map over elevations 0 ... 90 degrees, two look directions of which n_own = 1 and 2
    follow their own target covariance; without and with the whole own map taken (the tile skip)"""
    hop = N // 2
    dev = torch.device("cuda:0")
    S, n_az, n_el = 2, 72, 19
    xyz = np.random.default_rng(3).uniform(-0.05, 0.05, (a.mics, 3))
    L = (a.frames + 1) * hop
    g = torch.Generator(device=dev); g.manual_seed(1234)
    pcm = (torch.randn((a.streams, a.mics, L), device=dev, generator=g) * 0.1).contiguous()
    look_el = [0.5, 0.2]
    p0 = (synth.noise_source_stream_xyz(xyz, LOOK[0], fs, L, 77, elevation=look_el[0]) + synth.noise_source_stream_xyz(xyz, LOOK[1], fs, L, 78, elevation=look_el[1]))
    pcm[0] = torch.from_numpy(p0.astype(np.float32)).to(dev)
    look = torch.tensor(LOOK[:S], device=dev, dtype=torch.float32)
    doa = look[None, None, :].expand(a.streams, a.frames, S).contiguous()
    out = torch.empty((a.streams, S, a.frames * hop), device=dev, dtype=torch.float32)
    peaks = torch.empty((3, a.streams, S), device=dev, dtype=torch.float32)
    for n_own in (1, 2):
        bf = api.MvdrBeamformer(fs, xyz, N, max_streams=a.streams, max_sources=S, geometry="xyz")
        bf.set_rtf(True)
        bf.set_mask_estimator(True, n_protected=1)
        bf.configure_spectrum(n_az, n_peaks=S)
        bf.map_configure(n_az, n_el, 0.0, np.pi / 2, n_peaks=S)
        bf.set_elevations(np.tile(np.asarray(look_el, dtype=np.float32), (a.streams, 1)))
        auto = lambda: bf._check(bf._lib.mca_hip_mvdr_sources_frames_auto_dev(bf.h, *api.pcm_layout(pcm), a.streams, a.frames, S, api._ptr(doa), None, None,
                                                                             api._ptr(out), None, st))
        auto()
        bf.configure_tracks(S, n_own, max_step_rad=0.1, min_sep_rad=0.1, hold=3)
        bf.configure_tracks_map(max_step_el_rad=0.1, min_sep_el_rad=0.1)
        bf.seed_tracks_map(np.tile(np.asarray(LOOK[:S], dtype=np.float32), (a.streams, 1)), np.tile(np.asarray(look_el, dtype=np.float32), (a.streams, 1)))
        own_map = torch.empty((a.streams, n_own, n_el, n_az), device=dev, dtype=torch.float32)
        steps = dict(auto=auto, map=lambda: bf.map_dev(a.streams, peak_az=peaks[0], peak_el=peaks[1], peak_val=peaks[2], stream=st),
                     update=lambda: bf.update_tracks_map_dev(a.streams, stream=st),
                     update_with_own_map=lambda: bf.update_tracks_map_dev(a.streams, own_map=own_map, stream=st))
        row = dict(n_own=n_own, workload="%d streams x %d frames, %d mics, N=%d, %d x %d map" % (a.streams, a.frames, a.mics, N, n_az, n_el))
        for name in ("auto", "map", "update", "update_with_own_map"):
            for _ in range(a.warmup):
                steps[name]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                steps[name]()
            torch.cuda.synchronize()
            row[name + "_ms_per_step"] = (time.perf_counter() - t0) / a.steps * 1e3
        bf.set_timing(True)
        for _ in range(a.steps):
            steps["update"]()
        for kid, kname in ((bf.K_MAP, "update_map_kernels_ms"), (bf.K_TRACKS_MAP, "update_trk2_kernels_ms")):
            n, ms = bf.get_timing(kid)
            row[kname] = ms / max(n, 1)
        tr = bf.tracks_map()
        row["own_tracks_with_a_match"] = float((tr["miss"][:, :n_own] == 0).mean())
        bf.close()
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--mics", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", type=int, default=1)
    ap.add_argument("--sources", type=int, default=0, help="time the sources call with this many look directions per frame")
    ap.add_argument("--null-gain", type=float, default=0.0, help="gain of the soft nulls of the sources call")
    ap.add_argument("--update", choices=["none", "ones", "half"], default="none", help="covariance update weights of the call")
    ap.add_argument("--postfilter", action="store_true", help="enable the Wiener post-filter (its defaults)")
    ap.add_argument("--mask", action="store_true", help="time the table of the time-frequency update masks (DESIGN.md 4.7)")
    ap.add_argument("--rtf", action="store_true", help="time the table of the estimated steering vectors (DESIGN.md 4.8)")
    ap.add_argument("--estmask", action="store_true", help="time the table of the mask estimator (DESIGN.md 4.9)")
    ap.add_argument("--rtf-nulls", action="store_true", help="time the table of the nulls at estimated steering vectors (DESIGN.md 4.10)")
    ap.add_argument("--tracks", action="store_true", help="time the update of the tracks beside the spectrum call and the auto call (DESIGN.md 4.11)")
    ap.add_argument("--tracks-map", action="store_true", help="time the update of the tracks in map mode beside the map call and the auto call (DESIGN.md 4.21)")
    ap.add_argument("--geometry", choices=["linear_x", "xyz"], default="linear_x",
                    help="xyz: an XYZ context (mca_hip_mvdr_set_geometry) on a uniform circular array of --mics microphones, radius 5 cm (DESIGN.md 4.12)")
    ap.add_argument("--elevation", type=float, default=0.0, help="the elevation of --geometry xyz (radians)")
    a = ap.parse_args()
    if a.null_gain != 0.0 and a.sources < 2:
        ap.error("--null-gain needs --sources 2 ... 4")
    xyz = a.geometry == "xyz"
    if xyz and (a.mask or a.rtf or a.estmask or a.rtf_nulls or a.tracks or a.postfilter or a.update != "none"):
        ap.error("--geometry xyz times the plain calls (with --sources and --null-gain)")
    if os.environ.get("MCA_HIP_LIB"):
        bind_what_the_library_has()
    fs, N = 48000, 1024
    hop, K = N // 2, N // 2 + 1
    if a.tracks_map:
        return tracks_map_table(a, fs, N, torch.cuda.current_stream().cuda_stream)
    xs = [0.32 / a.mics * m for m in range(a.mics)] if a.mics != 16 else synth.ULA16
    if xyz:
        xs = synth.uca(a.mics, 0.05)
    geo = dict(geometry="xyz", elevation_rad=a.elevation) if xyz else {}
    dev = torch.device("cuda:0")
    L = (a.frames + 1) * hop
    g = torch.Generator(device=dev); g.manual_seed(1234)
    pcm = (torch.randn((a.streams, a.mics, L), device=dev, generator=g) * 0.1).contiguous()
    if a.check:
        if xyz:
            p0 = (synth.noise_source_stream_xyz(xs, np.deg2rad(20.0), fs, L, 77, elevation=a.elevation)
                  + synth.noise_source_stream_xyz(xs, np.deg2rad(-150.0), fs, L, 78, snr_db=60, elevation=a.elevation))
        else:
            p0 = synth.noise_source_stream(xs, np.deg2rad(20.0), fs, L, 77) + synth.noise_source_stream(xs, np.deg2rad(-50.0), fs, L, 78, snr_db=60)
        pcm[0] = torch.from_numpy(p0.astype(np.float32)).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    if a.mask:
        return mask_table(a, fs, N, xs, pcm, st)
    if a.rtf:
        return rtf_table(a, fs, N, xs, pcm, st)
    if a.estmask:
        return estmask_table(a, fs, N, xs, pcm, st)
    if a.rtf_nulls:
        return rtf_nulls_table(a, fs, N, xs, pcm, st)
    if a.tracks:
        return tracks_table(a, fs, N, xs, pcm, st)
    upd = None
    if a.update != "none":
        w = np.ones((a.streams, a.frames), dtype=np.float32)
        if a.update == "half":
            w[:, (np.arange(a.frames) // 8) % 2 == 1] = 0.0
        upd = torch.from_numpy(w).to(dev)
    if a.sources:
        look = torch.tensor(LOOK[:a.sources], device=dev, dtype=torch.float32)
        doa = look[None, None, :].expand(a.streams, a.frames, a.sources).contiguous()
        out = torch.empty((a.streams, a.sources, a.frames * hop), device=dev, dtype=torch.float32)
        bf = api.MvdrBeamformer(fs, xs, N, max_streams=a.streams, max_sources=a.sources, **geo)
        if a.null_gain != 0.0:
            bf.set_null_gain(a.null_gain)
        step = lambda: bf.process_sources_dev(pcm, a.frames, doa, out_pcm=out, stream=st, **({} if upd is None else {"update": upd}))
    else:
        doa = torch.full((a.streams, a.frames), float(np.deg2rad(20.0)), device=dev, dtype=torch.float32)
        out = torch.empty((a.streams, a.frames * hop), device=dev, dtype=torch.float32)
        bf = api.MvdrBeamformer(fs, xs, N, max_streams=a.streams, **geo)
        step = lambda: bf.process_dev(pcm, a.frames, doa, out_pcm=out, stream=st, **({} if upd is None else {"update": upd}))
    if a.postfilter:
        bf.set_postfilter(True)
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    res = {}
    if a.check and a.postfilter:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import mvdr_postfilter_twin as pt
        bf.reset()
        step()
        torch.cuda.synchronize()
        tw = pt.mvdr_postfilter_stream(fs, N, xs, pcm[0].cpu().numpy().astype(np.float64), doa[0].cpu().numpy(), a.null_gain,
                                       None if upd is None else upd[0].cpu().numpy())
        o0 = out[0].cpu().numpy().reshape(tw["out"].shape)
        res["audio_err_of_unfiltered_peak_max"] = float(max(np.abs(o0[s] - tw["out"][s]).max() / np.abs(tw["raw_out"][s]).max() for s in range(o0.shape[0])))
    elif a.check and upd is not None:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import mvdr_gate_twin as gt
        bf.reset()
        step()
        torch.cuda.synchronize()
        tw = gt.mvdr_gate_stream(fs, N, xs, pcm[0].cpu().numpy().astype(np.float64), doa[0].cpu().numpy(), a.null_gain, upd[0].cpu().numpy())
        o0 = out[0].cpu().numpy().reshape(tw["out"].shape)
        res["audio_err_rel_max"] = float(max(np.abs(o0[s] - tw["out"][s]).max() / np.abs(tw["out"][s]).max() for s in range(o0.shape[0])))
    elif a.check and xyz:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import mvdr_geometry_twin as gmt
        import mvdr_nulls_twin as nt
        bf.reset()
        step()
        torch.cuda.synchronize()
        S = max(a.sources, 1)
        with gmt.xyz_mode(a.elevation):
            tw = nt.mvdr_nulls_stream(fs, N, xs, pcm[0].cpu().numpy().astype(np.float64), doa[0].cpu().numpy().reshape(a.frames, S), a.null_gain)
        o0 = out[0].cpu().numpy().reshape(tw["out"].shape)
        res["audio_err_rel_max"] = float(max(np.abs(o0[s] - tw["out"][s]).max() / np.abs(tw["out"][s]).max() for s in range(S)))
    elif a.check and a.sources:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import mvdr_nulls_twin as nt
        bf.reset()
        step()
        torch.cuda.synchronize()
        tw = nt.mvdr_nulls_stream(fs, N, xs, pcm[0].cpu().numpy().astype(np.float64), doa[0].cpu().numpy(), a.null_gain)
        res["audio_err_rel_max"] = float(max(np.abs(out[0, s].cpu().numpy() - tw["out"][s]).max() / np.abs(tw["out"][s]).max()
                                             for s in range(a.sources)))
    elif a.check:
        from oracle import pyoracle as po
        bf.reset()
        step()
        torch.cuda.synchronize()
        o = po.MVDR(fs, N, xs).stream(pcm[0].cpu().numpy().astype(np.float64), np.full(a.frames, float(np.float32(np.deg2rad(20.0)))))
        err = np.abs(out[0].cpu().numpy() - o["out"]).max() / np.abs(o["out"]).max()
        res["audio_err_rel_max"] = float(err)
    bf.set_timing(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    frames = a.streams * a.frames
    if a.sources:
        res.update(dict(sources=a.sources, null_gain=a.null_gain))
    if xyz:
        res.update(dict(geometry="xyz", elevation=a.elevation))
    res.update(dict(update=a.update, lib=os.environ.get("MCA_HIP_LIB", "default")))
    res.update(dict(workload="%d streams x %d frames, %d mics, N=%d" % (a.streams, a.frames, a.mics, N), ms_per_step=dt * 1e3,
                    frames_per_s=frames / dt, algorithmic_GBps=frames / dt * (a.mics * hop * 4 + hop * 4) / 1e9))
    for kid, name in ((0, "k_mvdr_analyse"), (1, "k_mvdr_solve"), (2, "k_mvdr_synth")):
        n, ms = bf.get_timing(kid)
        res[name + "_ms"] = ms / max(n, 1)
    if a.postfilter:
        n, ms = bf.get_timing(bf.K_POSTFILTER)
        slots = max(a.sources, 1)
        traffic = 20.0 * a.streams * slots * a.frames * K + 2 * 4.0 * a.streams * slots * K
        res.update(dict(postfilter=True, k_mvdr_postfilter_ms=ms / max(n, 1), k_mvdr_postfilter_bytes=traffic,
                        k_mvdr_postfilter_GBps=traffic / (ms / max(n, 1) * 1e-3) / 1e9 if ms > 0 else 0.0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
