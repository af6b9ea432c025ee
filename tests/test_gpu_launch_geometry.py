"""GPU: the launch shapes the host code picks from the batch size, at the sizes where it leaves the minimum.

api_mvdr.hip picks the frames per analysis block (fpb), the frames per synthesis block (ft) and the cut of the tail solve launch
along the frames (pieces) from the stream and frame counts; api_mask.hip, api_bmask.hip and api_multiband.hip pick their run
length ft and their fpb the same way.  The module tests stay at batches for which all of them are at their minimum (except the
single-look MVDR audio of test_mvdr_full_size_properties).  Here the batches are large enough to move them, made of copies of 3
distinct signals: the 3 distinct streams, a middle one and the last one go against the module's reference under the module's own
bar (imported), and every copy must have the bits of the first stream with its signal -- wherever it sits in the grid, and, for
a stream in the tail launch of the MVDR solve, whether its frames were cut into pieces or not."""
import functools

import numpy as np
import pytest

from mcarray_amd import api, synth
from oracle import pyoracle as po

import mvdr_nulls_twin as nt

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------
# MVDR
# ---------------------------------------------------------------------------------------------------------------------------
import test_gpu_mvdr as tv                    # noqa: E402  SPEC_TOL, AUDIO_TOL, COV_TOL for the plain solve
import test_gpu_mvdr_nulls as tn              # noqa: E402  the bar test_gpu_mvdr_nulls.py uses for its gains (the same three figures)

FS, N, HOP, K = 16000, 512, 256, 257
CALLS = (61, 19)                              # frames of the first and the second call on one context
FT = sum(CALLS)


def _mvdr_shapes(n_streams, n_frames, n_sources):
    """(fpb, ft, pieces) as mca_hip_mvdr_sources_frames_dev derives them at N = 512 (api_mvdr.hip):
         fpb = 8;  while fpb > 1 and streams * ceil(F / fpb) < 1024: fpb /= 2
         ft = 16;  while ft > 2 and streams * sources * ceil(F / ft) < 1024: ft /= 2
         n_wg = ceil(streams * K / 64), rem = n_wg % 512; pieces = 1; if n_wg > 512 and 0 < rem <= 128:
             while pieces < 8 and rem * pieces * 2 <= 512 and F / (pieces * 2) >= 4: pieces *= 2"""
    fpb = 8
    while fpb > 1 and n_streams * -(-n_frames // fpb) < 1024:
        fpb >>= 1
    ft = 16
    while ft > 2 and n_streams * n_sources * -(-n_frames // ft) < 1024:
        ft >>= 1
    n_wg = -(-n_streams * K // 64)
    rem, pieces = n_wg % 512, 1
    if n_wg > 512 and 0 < rem <= 128:
        while pieces < 8 and rem * pieces * 2 <= 512 and n_frames // (pieces * 2) >= 4:
            pieces *= 2
    return fpb, ft, pieces


def test_the_shapes_these_batches_reach():
    """(no GPU work) 40 / 64 / 128 streams x 61 frames: fpb = 2 / 4 / 8 and, with two sources, ft = 4 / 8 / 16.  128 streams x 257
    bins = 514 solve workgroups: the 2 behind the 512 resident ones go in the tail launch, cut into 8 pieces of the 61 frames (no
    multiple of 8) and into 4 pieces of the 19 frames of the second call; 40 and 64 streams (161 and 257 workgroups) never take it."""
    assert [_mvdr_shapes(a, 61, 2) for a in (40, 64, 128)] == [(2, 4, 1), (4, 8, 1), (8, 16, 8)]
    assert _mvdr_shapes(128, 19, 2)[2] == 4 and _mvdr_shapes(128, 61, 4)[2] == 8 and _mvdr_shapes(128, 61, 1) == (8, 8, 8)
    assert [-(-a * K // 64) for a in (40, 64, 128)] == [161, 257, 514]
    # what the module tests reach (64 streams x 10 frames of 1024 samples, two sources): the minimum of each, and two pieces
    assert (1, 2) == _mvdr_shapes(64, 10, 2)[:2]


def _xs(M):
    return {8: synth.ULA8, 16: synth.ULA16}.get(M, tn._irregular(M))


@functools.lru_cache(maxsize=None)
def _mvdr_reference(M, S, gain):
    """the 3 scenes through the reference in the two calls -> pcm [3][M][...], doa [3][FT][S], per scene and call dict(spec [S][F][K],
    out [S][F*hop], phi, skip): po.MVDR per look direction for gain 0 (its stream() restarts the overlap-add per call: skip = the
    first hop of the second call), the twin of the dense definition otherwise.  Computed once per (M, S, gain), shared by the
    batch sizes, never written."""
    xs = _xs(M)
    pcm = np.stack([nt.scene(xs, FS, N, FT, a) for a in range(3)])
    doa = nt.drifting_doa(3, FT, max(S, 1))
    refs = []
    for a in range(3):
        per_call, t0, state = [], 0, None
        ogs = [po.MVDR(FS, N, xs) for _ in range(max(S, 1))]
        for i, n in enumerate(CALLS):
            x = pcm[a, :, t0 * HOP:(t0 + n + 1) * HOP].astype(np.float64)
            if gain:
                state = nt.mvdr_nulls_stream(FS, N, xs, x, doa[a, t0:t0 + n], gain, state=state)
                per_call.append(dict(spec=state["spec"], out=state["out"], phi=state["phi"], skip=0))
            else:
                o = [og.stream(x, doa[a, t0:t0 + n, s].astype(np.float64), want_spec=True) for s, og in enumerate(ogs)]
                per_call.append(dict(spec=np.stack([tv._ospec(q) for q in o]), out=np.stack([q["out"] for q in o]),
                                     phi=ogs[0].covariance().copy(), skip=HOP if i else 0))
            t0 += n
        refs.append(per_call)
    for v in (pcm, doa):
        v.setflags(write=False)
    return pcm, doa, refs


def _mvdr_case(M, S, gain, A):
    """S = 0: the single-look entry point"""
    pcm3, doa3, refs = _mvdr_reference(M, S, gain)
    spec_tol, audio_tol, cov_tol = (tn.SPEC_TOL, tn.AUDIO_TOL, tn.COV_TOL) if gain else (tv.SPEC_TOL, tv.AUDIO_TOL, tv.COV_TOL)
    pick = np.arange(A) % 3
    pcm = pcm3[pick]
    bf = api.MvdrBeamformer(FS, _xs(M), N, max_streams=A, max_sources=max(S, 1), null_gain=gain)
    sample = sorted({0, 1, 2, A // 2, A - 1})
    t0 = 0
    for i, n in enumerate(CALLS):
        x = np.ascontiguousarray(pcm[:, :, t0 * HOP:(t0 + n + 1) * HOP])
        if S:
            r = bf.process_sources(x, np.ascontiguousarray(doa3[pick, t0:t0 + n]))
        else:
            r = bf.process(x, np.ascontiguousarray(doa3[pick, t0:t0 + n, 0]), want_spec=True)
            r = dict(out=r["out"][:, None], spec=r["spec"][:, None])
        assert np.isfinite(r["out"]).all() and np.isfinite(r["spec"].view(np.float32)).all()
        cov = [bf.covariance(a) for a in range(A)]
        for a in sample:
            ref = refs[pick[a]][i]
            for s in range(max(S, 1)):
                es = np.abs(r["spec"][a, s] - ref["spec"][s]).max() / np.abs(ref["spec"][s]).max()
                ea = np.abs(r["out"][a, s, ref["skip"]:] - ref["out"][s, ref["skip"]:]).max() / np.abs(ref["out"][s]).max()
                print("M %d S %d gain %g A %d call %d stream %d source %d: spectra %.2e audio %.2e of the peak" % (M, S, gain, A, i, a, s, es, ea))
                assert es <= spec_tol and ea <= audio_tol, (i, a, s, es, ea)
            ec = np.abs(cov[a] - ref["phi"]).max() / np.abs(ref["phi"]).max()
            print("call %d stream %d: covariance %.2e" % (i, a, ec))
            assert ec <= cov_tol, (i, a, ec)
        # every copy of a scene has the bits of its first copy: across the blocks of the analysis and the synthesis, and -- the last
        # streams of 128 -- between the tail launch, cut along the frames, and the main launch
        for a in range(3, A):
            b = pick[a]
            assert r["spec"][a].tobytes() == r["spec"][b].tobytes(), ("spectra", i, a)
            assert r["out"][a].tobytes() == r["out"][b].tobytes(), ("audio", i, a)
            assert cov[a].tobytes() == cov[b].tobytes(), ("covariance", i, a)
        t0 += n
    bf.close()


@pytest.mark.parametrize("A", [40, 64, 128])
@pytest.mark.parametrize("gain", [0.0, 100.0])
@pytest.mark.parametrize("M,S", [(2, 2), (5, 3), (8, 4), (16, 4)])
def test_mvdr_sources_batches_that_move_the_launch_shapes(M, S, gain, A):
    """k_mvdr_solve_t without (gain 0) and with NULLS (gain 100) behind an analysis that writes one steering table per look
    direction with fpb = 2 / 4 / 8 frames per block, in front of a synthesis of ft = 4 ... 16 frames per block; A = 128: the tail
    launch in 8 and then 4 pieces ((16, 4): the two-pass instantiation inside a pieced launch).  The second call continues the
    covariances and the overlap-add tails the first one left."""
    _mvdr_case(M, S, gain, A)


def test_mvdr_single_look_pieced_launch_leaves_the_covariance_of_the_unpieced_one():
    """what test_mvdr_full_size_properties leaves out: the covariance a pieced tail launch hands over (moved from the scratch
    copy), and the call that continues from it -- 128 streams of 5 microphones"""
    _mvdr_case(5, 0, 0.0, 128)


# ---------------------------------------------------------------------------------------------------------------------------
# run lengths of the masking modules
# ---------------------------------------------------------------------------------------------------------------------------
MASK_FRAMES = 256                             # per call, two calls
MASK_SEEDS = {1024: (101, 102, 104), 2048: (104, 107, 110)}       # fixed on the CPU, see test_fast_binaural_masking_run_lengths


def _mask_ft(n_streams, n_frames):
    """api_mask.hip / api_bmask.hip: ft = 256; while ft > 16 and streams * ceil(F / ft) < 512: ft /= 2"""
    ft = 256
    while ft > 16 and n_streams * -(-n_frames // ft) < 512:
        ft >>= 1
    return ft


def _mask_signal(Nm, seed, F):
    hop = Nm // 2
    n = (F + 1) * hop
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(n) * 0.1
    left = src + rng.standard_normal(n) * 0.003
    right = np.roll(src, 1 + seed % 3) * 0.9 + rng.standard_normal(n) * 0.003
    env = np.repeat(rng.choice([1.0, 0.2, 0.05, 0.6], F + 1), hop)
    return np.stack([left * env, right * env]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _fast_mask_reference(fs, Nm):
    F = 2 * MASK_FRAMES
    flo, fhi = 300.0, min(5000.0, 0.45 * fs)
    pcm = np.stack([_mask_signal(Nm, seed, F) for seed in MASK_SEEDS[Nm]])
    refs = []
    for a in range(3):
        ol, orr = po.Masking(fs, Nm, 0.086, flo, fhi, api.RELATIVE, api.BOTH).stream(pcm[a, 0].astype(np.float64), pcm[a, 1].astype(np.float64))
        o2 = po.Masking(fs, Nm, 0.086, flo, fhi, api.RELATIVE, api.BOTH)
        X = po.stft_frames(pcm[a].astype(np.float64), Nm)
        refs.append((np.stack([ol, orr]), np.array([o2.process(X[t, 0], X[t, 1])[2] for t in range(F)])))
    pcm.setflags(write=False)
    return pcm, refs


def _two_calls(m, pcm, hop, F):
    ra = m.process(np.ascontiguousarray(pcm[:, :, :(F + 1) * hop]))
    rb = m.process(np.ascontiguousarray(pcm[:, :, F * hop:]))
    return np.concatenate([ra[0], rb[0]], axis=2), np.concatenate([ra[1], rb[1]], axis=1)


def _copies_have_the_same_bits(out, dec, pick):
    for a in range(3, len(pick)):
        assert out[a].tobytes() == out[pick[a]].tobytes() and dec[a].tobytes() == dec[pick[a]].tobytes(), a


@pytest.mark.parametrize("A", [3, 64, 128])
@pytest.mark.parametrize("fs,Nm", [(16000, 1024), (48000, 2048)])
def test_fast_binaural_masking_run_lengths(fs, Nm, A):
    """256 frames per call: 3 streams run at ft = 16, 64 at ft = 32, 128 at ft = 64 (the module tests stay at 16).  Decisions
    against the oracle with at most 2 differing cells per stream, audio on every hop whose own and previous frame agree
    (tests/test_gpu_fft_sizes.py).  The seeds were fixed on the CPU before any GPU run, from the oracle against itself: the
    oracle exposes no threshold to move, so every bin of both channels' spectra was scaled by 1 + 1e-4 x a normal deviate (two
    draws) and by 1 + 1e-5 x one (which moves every band quantity against its thresholds by about that much, 100 and 10 times
    what fp32 does), and one channel by 1 +- 1e-4 as a whole.  Of the seeds 100 ... 123 the ones kept change no decision cell
    of their 23 040 under any of these at their frame length (at 2048 samples most others change 1 ... 12), so the cap of 2 is
    not spent on the oracle's own ties."""
    from test_gpu_fft_sizes import MASK_MAX_CELLS, assert_masking_audio_where_decisions_agree
    assert [_mask_ft(a, MASK_FRAMES) for a in (3, 64, 128)] == [16, 32, 64]
    pcm3, refs = _fast_mask_reference(fs, Nm)
    pick = np.arange(A) % 3
    hop = Nm // 2
    m = api.FastBinauralMasking(fs, 0.086, 300.0, min(5000.0, 0.45 * fs), api.RELATIVE, api.BOTH, fft_size=Nm, max_streams=A)
    out, dec = _two_calls(m, pcm3[pick], hop, MASK_FRAMES)
    m.close()
    assert np.isfinite(out).all()
    for a in sorted({0, 1, 2, A - 1}):
        ref, odec = refs[pick[a]]
        ndiff = int((dec[a] != odec).sum())
        assert ndiff <= MASK_MAX_CELLS, (a, ndiff)
        compared = assert_masking_audio_where_decisions_agree(out[a], ref, dec[a], odec, hop)
        assert compared >= 2 * MASK_FRAMES - 2 * MASK_MAX_CELLS
    _copies_have_the_same_bits(out, dec, pick)


@functools.lru_cache(maxsize=None)
def _bmask_reference():
    import bmask_twin as bt
    import test_gpu_bmask as tb
    pcm = np.stack([bt.parity_input(seed, tb.FS, 2 * MASK_FRAMES) for seed in sorted(bt.PARITY)])
    tws = [bt.Twin(tb.FS, tb.D, tb.LO, tb.HI, bt.RELATIVE).stream(pcm[a]) for a in range(3)]
    pcm.setflags(write=False)
    return pcm, tws


@pytest.mark.parametrize("A", [3, 64, 128])
def test_binaural_masking_impl_run_lengths(A):
    """the filter-bank masking at 16 kHz, 256 frames per call: ft = 16 / 32 / 64.  The bar is tests/test_gpu_bmask.py's: decisions
    differ only on the twin's own near-tie cells, audio on every hop whose frames agree; the inputs are that file's parity
    signals (seeds 41 ... 43), made longer."""
    import bmask_twin as bt
    import test_gpu_bmask as tb
    pcm3, tws = _bmask_reference()
    pick = np.arange(A) % 3
    m = api.BinauralMaskingImpl(tb.FS, tb.D, tb.LO, tb.HI, bt.RELATIVE, max_streams=A)
    out, dec = _two_calls(m, pcm3[pick], m.hop, MASK_FRAMES)
    m.close()
    assert np.isfinite(out).all()
    for a in sorted({0, 1, 2, A - 1}):
        tb._check_stream("A %d stream %d" % (A, a), out[a], dec[a], tws[pick[a]])
    _copies_have_the_same_bits(out, dec, pick)


# ---------------------------------------------------------------------------------------------------------------------------
# frames per block of the multiband localiser
# ---------------------------------------------------------------------------------------------------------------------------
MB_CALLS = (61, 35)


def _mb_fpb(Nm, n_arrays, n_frames):
    """api_multiband.hip: N = 1024: fpb = 16, minimum 4; N = 512: fpb = 32, minimum 8; halved while arrays * ceil(F / fpb) < 512"""
    fpb, lo = (16, 4) if Nm == 1024 else (32, 8)
    while fpb > lo and n_arrays * -(-n_frames // fpb) < 512:
        fpb >>= 1
    return fpb


@functools.lru_cache(maxsize=None)
def _mb_input(fs, Nm):
    Ft = sum(MB_CALLS)
    pcm = np.stack([synth.noise_source_stream(synth.BINAURAL, np.deg2rad(-55.0 + 45.0 * a), fs, (Ft + 1) * Nm // 2, 40 + a) for a in range(3)]).astype(np.float32)
    pcm.setflags(write=False)
    return pcm


@pytest.mark.parametrize("A", [16, 256])
@pytest.mark.parametrize("fs,Nm", [(48000, 1024), (16000, 512)])
def test_multiband_frames_per_block(fs, Nm, A):
    """16 arrays keep fpb at its minimum (4 at N = 1024, 8 at N = 512), 256 arrays run at 16 and 32 frames per block, in both calls
    (61 + 35 frames: the counts are no multiple of either).  The 3 distinct streams and the last one against the oracle under
    tests/test_gpu_multiband.py's rules; every copy has the bits of its first."""
    import test_gpu_multiband as tm
    assert [_mb_fpb(Nm, a, f) for a in (16, 256) for f in MB_CALLS] == ([4, 4, 16, 16] if Nm == 1024 else [8, 8, 32, 32])
    pcm3 = _mb_input(fs, Nm)
    pick = np.arange(A) % 3
    pcm = pcm3[pick]
    hop, n1 = Nm // 2, MB_CALLS[0]
    loc = api.MultibandBinarualLocalisation(fs, synth.BINAURAL, 15, False, fft_size=Nm, max_arrays=A)
    ra = loc.process(np.ascontiguousarray(pcm[:, :, :(n1 + 1) * hop]), want_bands=True)
    rb = loc.process(np.ascontiguousarray(pcm[:, :, n1 * hop:]), want_bands=True)
    r = {k: np.concatenate([ra[k], rb[k]], axis=1) for k in ra}
    flagged = 0
    sample = sorted({0, 1, 2, A - 1})
    for a in sample:
        flagged += tm._compare(loc, po.Multiband(fs, synth.BINAURAL, Nm + 2, 15, False), pcm[a], Nm, r, a)
    assert flagged <= 0.1 * len(sample) * sum(MB_CALLS), flagged
    for a in range(3, A):
        for k in r:
            assert r[k][a].tobytes() == r[k][pick[a]].tobytes(), (k, a)
    loc.close()
