"""GPU, library level: the folded coarse contraction (k_srp_gemm_f16_fold behind planar merged rows, csrc/fold_table.h) inside
the ADAPTIVE path.  16 384 rows is the smallest call that reaches the kernel: 4 arrays x 4 096 frames and 64 arrays x 256 frames of the
8-microphone array, even arrays with one stationary source, odd arrays with a source that jumps half-way through the stream.

  * the ADAPTIVE picks equal the FP16X3 picks, except frames that the classifier of parity_helpers (the bar of the parity tests) calls
    ties on the FP16X3 energy row;
  * the separated audio of the first 512 frames of an array against the CPU oracle, on the hops whose bins agree;
  * the same stream in one call and in two ragged calls (neither of which reaches the 256-row tiles: the full-width kernels on the
    same planar rows and folded values) gives the same bins, angles and audio, array_equal;
  * a context whose step gives an even D under Dp = 384 (180 / 361 degrees: D = 362) does not fold and passes the same checks."""
import numpy as np
import pytest

from mcarray_amd import api, synth
from oracle import pyoracle as po
from parity_helpers import assert_audio_where_bins_agree, assert_bins, classify_bins

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FS, N, HOP, XS = 48000, 1024, 512, synth.ULA8
ORACLE_FRAMES = 512


@pytest.fixture(autouse=True)
def no_back_off(monkeypatch):
    monkeypatch.setenv("MCA_HIP_ADAPT_FALLBACK", "0")        # read by mca_hip_create: the test is about coarse + repair itself


_PCM = {}


def streams(A, F):
    """[A][8][(F + 1) * 512] float32, computed once per shape and left unchanged"""
    if (A, F) not in _PCM:
        L = (F + 1) * HOP
        rows = []
        for a in range(A):
            th0 = np.deg2rad(-70.0 + 140.0 * (a + 0.5) / A)
            x = synth.noise_source_stream(XS, th0, FS, L, 7000 + a, snr_db=25.0 - 15.0 * (a % 3) / 2)
            if a & 1:                                                        # the source jumps by 35 degrees half-way through
                cut = (F // 2) * HOP + 137
                x[:, cut:] = synth.noise_source_stream(XS, th0 - np.sign(th0) * np.deg2rad(35.0), FS, L - cut, 9000 + a, snr_db=20.0)
            rows.append(x)
        pcm = np.stack(rows)
        pcm.setflags(write=False)
        _PCM[(A, F)] = pcm
    return _PCM[(A, F)]


def run(ctx, pcm_dev, calls):
    """calls: frame counts that add up to F; -> bin, doa, prob, energy, out (cuda tensors of the whole stream)"""
    A = pcm_dev.shape[0]
    parts, f0 = [], 0
    for nf in calls:
        piece = pcm_dev[:, :, f0 * HOP:(f0 + nf + 1) * HOP].contiguous()
        b = torch.empty(A, nf, ctx.S, dtype=torch.int32, device=pcm_dev.device)
        r, p = torch.empty_like(b, dtype=torch.float32), torch.empty_like(b, dtype=torch.float32)
        e = torch.empty(A, nf, ctx.D, dtype=torch.float32, device=pcm_dev.device)
        o = torch.empty(A, ctx.S, nf * HOP, dtype=torch.float32, device=pcm_dev.device)
        ctx.process_frames_dev(piece, nf, b, r, p, e, o)
        parts.append((b, r, p, e, o))
        f0 += nf
    torch.cuda.synchronize()
    return [torch.cat([q[i] for q in parts], dim=2 if i == 4 else 1).cpu().numpy() for i in range(5)]


@pytest.mark.parametrize("step,D", [(0.5, 361), (180.0 / 361.0, 362)], ids=["folds", "even_grid_does_not_fold"])
@pytest.mark.parametrize("A,F", [(4, 4096), (64, 256)])
def test_adaptive_on_the_folded_contraction(A, F, step, D):
    pcm = streams(A, F)
    dev = torch.device("cuda:0")
    pcm_dev = torch.from_numpy(pcm.copy()).to(dev)
    res = {}
    for name, prec, calls in (("x3", api.SRP_FP16X3, (F,)), ("adaptive", api.SRP_ADAPTIVE, (F,)), ("ragged", api.SRP_ADAPTIVE, (F // 4 + 7, F - F // 4 - 7))):
        ctx = api.Context(FS, XS, N, step, 1, srp_precision=prec, max_arrays=A)
        assert ctx.D == D
        res[name] = run(ctx, pcm_dev, calls)
        if name == "adaptive":
            st, P = ctx.repair_stats(), ctx.P
        ctx.close()
    assert st["frames"] == A * F and st["flagged"] < 0.5 * A * F, st              # the coarse + repair mode ran, and most frames were left to the coarse map

    # ADAPTIVE picks = FP16X3 picks except ties under the shared bar
    n_ties = 0
    for a in range(A):
        ties, bad = classify_bins(res["adaptive"][0][a], res["x3"][0][a], res["x3"][3][a].astype(np.float64), P)
        assert not bad, (a, bad[:4], res["adaptive"][0][a][bad[0]].tolist(), res["x3"][0][a][bad[0]].tolist())
        n_ties += len(ties)
    print("A %d F %d D %d: flagged %d of %d frames, %d tie(s) against FP16X3" % (A, F, D, st["flagged"], A * F, n_ties))
    assert n_ties <= max(2, A * F // 4096)

    # one call = two ragged calls
    for i, key in ((0, "bin"), (1, "doa"), (4, "out")):
        assert np.array_equal(res["adaptive"][i], res["ragged"][i]), key

    # audio (and bins) of an array with a jump inside the oracle's reach (64 x 256) or a stationary one (4 x 4 096) against the oracle
    a = 1 if F <= ORACLE_FRAMES else 0
    nf = min(F, ORACLE_FRAMES)
    o = po.ssl_stream(FS, N, XS, pcm[a][:, :(nf + 1) * HOP].astype(np.float64), 1, step, want_map=True)
    assert_bins(res["adaptive"][0][a][:nf], o["bin"], o["energy"], P, max_ties=3)
    compared = assert_audio_where_bins_agree(res["adaptive"][4][a][:, :nf * HOP], o["out"], res["adaptive"][0][a][:nf], o["bin"], HOP)
    assert compared > 0.9 * nf
