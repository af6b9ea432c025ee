"""GPU: the life of the MVDR context's per-source arrays with every one of them live at once -- the overlap-add tails, the
post-filter's A, Psi and cpsi -- through mca_hip_mvdr_set_max_sources and through destroy / create.

The slot rule (include/mcarray_hip.h): a change of max_sources keeps the slots both layouts have and starts the others at zero,
and a call clears the slots it leaves out.  So a context that goes 2 -> 4 -> 2 slots between calls of 2 look directions holds, in
its first two slots, what a context that stayed at 2 holds: same kernels, same inputs, and the slot stride enters no arithmetic.
Every comparison is np.array_equal (bytes).

Shapes: N = 64; 5 irregular microphones (two row slots per lane, the second partly filled); max_streams = 4 with 3 streams per
call (a size taken from n_streams instead of max_streams shows); 4 frames per call; post-filter, RTF, RTF nulls under a null gain
of 7.5 and tracks (one own track, which reads Psi at the slot stride) all enabled."""
import numpy as np
import pytest

from mcarray_amd import api

pytestmark = pytest.mark.gpu

FS, N, M, A_MAX, A, F, S, GAIN = 16000, 64, 5, 4, 3, 4, 2, 7.5
HOP, K = N // 2, N // 2 + 1
N_CALLS = 4                                                    # three calls of 2 look directions and the single-look one
XS = np.sort(np.random.default_rng(M).uniform(0.0, 0.04 * M, M))        # the irregular array of tests/test_gpu_mvdr_nulls.py

_rng = np.random.default_rng(2024)
PCM = _rng.standard_normal((A, M, (N_CALLS * F + 1) * HOP)).astype(np.float32)
PCM[2, :, :3 * HOP] = 0.0                                      # stream 2 starts with digital silence
DOA = _rng.uniform(-1.3, 1.3, (A, N_CALLS * F, S)).astype(np.float32)
UPDATE = _rng.choice(np.array([0.0, 0.0, 1.0, 1.0, 0.3, 0.8], dtype=np.float32), size=(A, N_CALLS * F, K))
TARGET = _rng.choice(np.array([0.0, 1.0, 1.0, 0.6], dtype=np.float32), size=(A, S, N_CALLS * F, K))
SEED = np.array([[0.4, -0.7], [-0.2, 0.9], [1.1, 0.1]], dtype=np.float32)


def _ctx(max_sources=S):
    """everything on"""
    bf = api.MvdrBeamformer(FS, XS, N, max_streams=A_MAX, max_sources=max_sources, null_gain=GAIN, rtf_nulls=True)
    bf.set_postfilter(True)
    bf.set_rtf(True)
    bf.configure_spectrum(19, n_peaks=2)
    bf.configure_tracks(2, n_own=1)
    bf.seed_tracks(SEED)
    return bf


def _call(bf, i, n_sources=S, tracks=True):
    """call i of the stream: frames 4 i ... 4 i + 3, the RTF call with both masks, audio and spectra; then one update of the tracks"""
    t0, t1 = i * F, (i + 1) * F
    r = bf.process_sources(PCM[:, :, t0 * HOP:(t1 + 1) * HOP], DOA[:, t0:t1, :n_sources], update_mask=UPDATE[:, t0:t1],
                           target_mask=TARGET[:, :n_sources, t0:t1])
    assert r["out"].shape == (A, n_sources, F * HOP) and r["spec"].shape == (A, n_sources, F, K)
    if tracks:
        bf.update_tracks(A)
        r.update(bf.tracks(A))
    return r


def _same(r, q, what):
    assert set(r) == set(q), what
    for key in r:
        assert np.array_equal(r[key].view(np.float32) if key == "spec" else r[key], q[key].view(np.float32) if key == "spec" else q[key],
                              equal_nan=key in ("spec", "out", "theta")), (what, key)


def _same_state(a, b, n_slots, what):
    for stream in range(A_MAX):
        assert np.array_equal(a.covariance(stream), b.covariance(stream)), (what, "covariance", stream)
        for slot in range(n_slots):
            (pa, ca), (pb, cb) = a.target_covariance(stream, slot), b.target_covariance(stream, slot)
            assert np.array_equal(pa, pb) and np.array_equal(ca, cb), (what, "target covariance", stream, slot)
    assert a.state_save() == b.state_save(), (what, "state blob")


def test_reslot_with_every_per_source_array_live():
    """A stays at 2 slots over three calls of 2 look directions; B takes the first call, goes to 4 slots for the second and back
    to 2 for the third: outputs, tracks, covariances, target covariances and the state blob are A's.  Then both go to 1 slot (which
    disables the tracks: fewer slots than tracks) and take a single-look call."""
    a, b = _ctx(), _ctx()
    try:
        for i in range(3):
            if i == 1:
                b.set_max_sources(4)
            if i == 2:
                b.set_max_sources(2)
            ra, rb = _call(a, i), _call(b, i)
            assert np.all(np.isfinite(ra["spec"])) and np.all(np.isfinite(ra["out"])) and np.abs(ra["out"]).max() > 0.0
            _same(ra, rb, "call %d" % i)
            if i == 1:
                # B's slots 2 and 3 were never used: a call of 2 look directions leaves them cleared
                for stream in range(A_MAX):
                    for slot in (2, 3):
                        psi, cpsi = b.target_covariance(stream, slot)
                        assert not psi.any() and not cpsi.any(), (stream, slot)
        psi, cpsi = a.target_covariance(0, 1)
        assert cpsi.any() and psi.any()                        # the comparison below is not one of zeros
        _same_state(a, b, S, "after three calls")
        for bf in (a, b):
            bf.set_max_sources(1)
            assert not bf.get_tracks_config()["enable"]
        _same(_call(a, 3, 1, tracks=False), _call(b, 3, 1, tracks=False), "single-look call at 1 slot")
        _same_state(a, b, 1, "at 1 slot")
    finally:
        a.close()
        b.close()


def test_recreate_at_the_same_size():
    """create, everything on, one call, close -- three times at the same size: every round gives the bytes of the first"""
    first = None
    for n in range(3):
        bf = _ctx(4)
        try:
            r = _call(bf, 0)
            blob = bf.state_save()
        finally:
            bf.close()
        if first is None:
            first = (r, blob)
        _same(first[0], r, "round %d" % n)
        assert first[1] == blob, n
