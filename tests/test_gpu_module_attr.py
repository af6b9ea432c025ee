"""GPU: the limit of dynamic LDS is a property of a kernel FUNCTION, shared by every context of the process.

Two contexts of one module live in one process and are called alternately, A, B, A: A's launches ask for more than 64 KiB of dynamic LDS, B's for
less, through the same kernels.  Under the one rule of the launcher (host_common.h) each launch sets what it needs, so every call's outputs must equal,
bit for bit, those of a fresh context of the same configuration fed the same calls alone -- whatever the other context did to the function in between.
The reference runs first, with one context alive at a time (A fed both its calls and closed, then B), so nothing of it alternates.

  temporal GCC: A 0.2 m at 48 kHz (27 delay pairs, a window of 7 200 samples: 72 304 bytes), B the same pair at 16 kHz (23 392 bytes); 1 array x 2 frames
  bmask:        A frames of 8192 samples (65 552 and 98 704 bytes), B frames of 256 samples; 1 stream x 3 frames

These are the smallest shapes at which a wrong rule shows (tests/test_module_plan.py holds the byte counts on the CPU)."""
import numpy as np
import pytest

from mcarray_amd import api

pytestmark = pytest.mark.gpu

PAIR = [[-0.1, 0.0, 0.0], [0.1, 0.0, 0.0]]       # 0.2 m


def _noise(shape, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def _alone(make, feed, which, n_calls):
    """a fresh context of configuration `which`, the only one alive, fed its calls -> the arrays of each call"""
    m = make(which)
    got = [feed(m, which, call) for call in range(n_calls)]
    m.close()
    return got


def _alternate(make, feed):
    """make(which) -> a context, feed(ctx, which, call) -> the arrays of one call.  The reference first, one context alive at a time: A fed
    its two calls and closed, then B fed its one.  Then A, B, A on two live contexts, each call against the reference's call"""
    ref_a = _alone(make, feed, "A", 2)
    ref_b = _alone(make, feed, "B", 1)
    alone = [ref_a[0], ref_b[0], ref_a[1]]
    a, b = make("A"), make("B")
    both = [feed(a, "A", 0), feed(b, "B", 0), feed(a, "A", 1)]
    a.close()
    b.close()
    for i, (x, y) in enumerate(zip(both, alone)):
        assert len(x) == len(y)
        for j, (u, v) in enumerate(zip(x, y)):
            assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), "call %d, output %d" % (i, j)
    return both


def test_tgcc_two_contexts_alternate():
    fs = dict(A=48000, B=16000)

    def make(which):
        m = api.TemporalGCCBinauralLocalisation(fs[which], PAIR, use_power_floor=False)
        assert (m.nd, m.W) == dict(A=(27, 7200), B=(9, 2400))[which]
        return m

    def feed(m, which, call):
        r = m.process(_noise((1, 2, m.hop + m.W), 10 * call + (which == "B")), want_index=True)          # 2 frames
        return [r[k] for k in ("doa", "prob", "voiced", "power", "delay_idx", "index")]

    both = _alternate(make, feed)
    assert all(np.isfinite(x).all() for call in both for x in call)


def test_bmask_two_contexts_alternate():
    fs = dict(A=160000, B=5000)          # frames of 2^round(log2(0.05 fs)) samples

    def make(which):
        m = api.BinauralMaskingImpl(fs[which], 0.2, 100.0, 2000.0)
        assert m.W == dict(A=8192, B=256)[which]
        return m

    def feed(m, which, call):
        out, dec = m.process(_noise((1, 2, 4 * m.hop), 20 + 10 * call + (which == "B")))                  # 3 frames
        return [out, dec]

    both = _alternate(make, feed)
    assert all(np.isfinite(call[0]).all() and np.abs(call[0]).max() > 0 for call in both)
