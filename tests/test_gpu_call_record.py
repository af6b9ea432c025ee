"""What a stream call decides belongs to that call: API traffic between two calls that is neutral to the stream --
rejected calls of every stream entry point, a reservation of a larger shape, the statistics, a graph created and destroyed without a
launch -- changes no byte of what the calls return, nor of the state they leave.

Context A runs three mca_hip_process_frames_dev calls (64, 160 and 64 frames, 2 of 3 arrays, 8-microphone ULA at 1024 samples); its
twin B runs the same calls with that traffic in between.  All outputs and the final state blobs must be byte-equal, for FP16 (the
steered path) and for ADAPTIVE (coarse + repair with lazy tails, candidate columns and the steered tail; pinned to the mode)."""
import numpy as np
import pytest

from mcarray_amd import api, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FS, N, HOP = 48000, 1024, 512
XS = synth.ULA8
A_MAX, A = 3, 2
CALLS = (64, 160, 64)
INVALID_ARGUMENT = -1


@pytest.fixture(scope="module")
def pcm():
    total = sum(CALLS)
    x = np.stack([synth.noise_source_stream(XS, np.deg2rad(-35.0 + 50 * a), FS, (total + 1) * HOP, 900 + a, snr_db=12.0) for a in range(A)]).astype(np.float32)
    x.setflags(write=False)
    return x


def _outputs(n_arrays, F, D, dev):
    return [torch.zeros((n_arrays, F, 1), dtype=torch.int32, device=dev), torch.zeros((n_arrays, F, 1), device=dev), torch.zeros((n_arrays, F, 1), device=dev),
            torch.zeros((n_arrays, F, D), device=dev), torch.zeros((n_arrays, 1, F * HOP), device=dev)]


def _rejected(call):
    with pytest.raises(api.MCArrayHipError) as e:
        call()
    assert "error %d:" % INVALID_ARGUMENT in str(e.value), str(e.value)


def _neutral_traffic(ctx, dev):
    """every one of these leaves the streams of the context where they are"""
    F = 64
    many = torch.zeros((A_MAX + 1, 8, (F + 1) * HOP), device=dev)                   # more arrays than the context has
    r = _outputs(A_MAX + 1, F, ctx.D, dev)
    _rejected(lambda: ctx.process_frames_dev(many, F, *r))
    _rejected(lambda: ctx.process_frames_dev(many, F, *r[:4], separate=False))      # mca_hip_localise_frames_dev
    _rejected(lambda: ctx.process_frames_dev(many, F, *r, localise=False))          # mca_hip_separate_frames_dev
    _rejected(lambda: ctx.process_frames_dev(many, F, *r, localise=False, bins_are_grid=True))   # mca_hip_separate_frames_bins_dev
    _rejected(lambda: ctx.graph_create(many, F, *r))
    _rejected(lambda: ctx.process_frames_host(np.zeros((A_MAX + 1, 8, (F + 1) * HOP), dtype=np.float32)))
    two = torch.zeros((A, 8, (F + 1) * HOP), device=dev)
    _rejected(lambda: ctx.gcc2_frames_dev(two[:, :2], F, torch.zeros((A, F), dtype=torch.int32, device=dev)))   # not a 2-microphone context
    ctx.reserve(A_MAX, 256)
    ctx.repair_stats()
    ctx.steer_stats()
    ok = _outputs(A, F, ctx.D, dev)
    ctx.graph_create(two, F, *ok).close()


def _run(prec, pcm, monkeypatch, traffic):
    monkeypatch.setenv("MCA_HIP_ADAPT_CAND", "1")          # read by mca_hip_create: candidate columns wherever the call's shape allows
    monkeypatch.delenv("MCA_HIP_ADAPT_FALLBACK", raising=False)
    dev = torch.device("cuda:0")
    ctx = api.Context(FS, XS, N, 0.5, 1, srp_precision=prec, max_arrays=A_MAX, adaptive_fallback=False, adaptive_min_rows=64)
    parts, t0 = [], 0
    for F in CALLS:
        if traffic:
            _neutral_traffic(ctx, dev)
        r = _outputs(A, F, ctx.D, dev)
        ctx.process_frames_dev(torch.from_numpy(pcm[:, :, t0 * HOP:(t0 + F + 1) * HOP].copy()).to(dev), F, *r)
        torch.cuda.synchronize()
        parts += [t.cpu().numpy() for t in r]
        t0 += F
    if traffic:
        _neutral_traffic(ctx, dev)
    parts.append(np.frombuffer(ctx.state_save(), dtype=np.uint8))
    ctx.close()
    return parts


@pytest.mark.parametrize("prec", [api.SRP_FP16, api.SRP_ADAPTIVE], ids=["FP16", "ADAPTIVE"])
def test_neutral_traffic_between_calls_changes_no_byte(prec, pcm, monkeypatch):
    plain = _run(prec, pcm, monkeypatch, traffic=False)
    busy = _run(prec, pcm, monkeypatch, traffic=True)
    assert len(plain) == len(busy) == 5 * len(CALLS) + 1
    names = ("bin", "doa", "prob", "energy", "out")
    for i, (p, b) in enumerate(zip(plain, busy)):
        what = "the state blob" if i == 5 * len(CALLS) else "%s of call %d" % (names[i % 5], i // 5)
        assert p.shape == b.shape and p.tobytes() == b.tobytes(), what
    assert np.isfinite(plain[4]).all() and np.abs(plain[4]).max() > 0            # (the calls really produced audio)
