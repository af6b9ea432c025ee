"""No GPU: the stride helper of the device-pointer binding (mcarray_amd.api.pcm_layout) and the index arithmetic of the poisoned
and guarded buffers the GPU layout tests use (tests/dev_layout_helpers.py), on CPU tensors."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mcarray_amd import api

import dev_layout_helpers as dl


def _ptr(t):
    return t.data_ptr()


def test_layout_of_a_contiguous_tensor():
    x = torch.zeros(3, 4, 100)
    p, sa, sc = api.pcm_layout(x)
    assert (p.value, sa, sc) == (_ptr(x), 400, 100)


def test_layout_of_a_padded_view():
    whole = torch.zeros(3 * (4 * 106 + 10))
    v = torch.as_strided(whole, (3, 4, 100), (4 * 106 + 10, 106, 1), 0)
    p, sa, sc = api.pcm_layout(v)
    assert (p.value, sa, sc) == (_ptr(whole), 434, 106)


def test_layout_of_a_view_offset_by_two_floats():
    whole = torch.zeros(2 + 3 * 400)
    v = torch.as_strided(whole, (3, 4, 100), (400, 100, 1), 2)
    p, sa, sc = api.pcm_layout(v)
    assert (p.value, sa, sc) == (_ptr(whole) + 8, 400, 100)


def test_layout_of_rows_longer_than_needed():
    x = torch.zeros(3, 4, 100)
    v = x[:, :, 10:60]                      # the call needs 50 samples of rows 100 apart
    p, sa, sc = api.pcm_layout(v)
    assert (p.value, sa, sc) == (_ptr(x) + 40, 400, 100)
    assert api.pcm_layout(x[1:])[0].value == _ptr(x) + 1600


def test_layout_refuses_inner_stride_two_float64_and_other_ranks():
    x = torch.zeros(3, 4, 100)
    with pytest.raises(api.MCArrayHipError):
        api.pcm_layout(x[:, :, ::2])
    with pytest.raises(api.MCArrayHipError):
        api.pcm_layout(x.double())
    with pytest.raises(api.MCArrayHipError):
        api.pcm_layout(x.to(torch.int32))
    with pytest.raises(api.MCArrayHipError):
        api.pcm_layout(x[0])


@pytest.mark.parametrize("A,C_,L", [(3, 8, 64), (1, 2, 12), (3, 5, 1000)])
def test_strided_pcm_holds_the_source_and_nothing_but_poison(A, C_, L):
    rng = np.random.default_rng(L)
    x = rng.standard_normal((A, C_, L)).astype(np.float32)
    v, whole = dl.strided_pcm(x, device="cpu")
    assert v.shape == (A, C_, L) and v.stride() == (C_ * (L + 6) + 10, L + 6, 1)
    assert v.data_ptr() == whole.data_ptr() + 8
    assert (L + 6) % 4 == 2                               # (the pitch that leaves every other row 8-byte aligned only)
    assert np.array_equal(v.numpy(), x)
    p, sa, sc = api.pcm_layout(v)
    assert (p.value, sa, sc) == (whole.data_ptr() + 8, C_ * (L + 6) + 10, L + 6)
    # the address formula of the header, sample by sample, and NaN everywhere else
    w = whole.numpy()
    idx = (2 + np.arange(A)[:, None, None] * sa + np.arange(C_)[None, :, None] * sc + np.arange(L)[None, None, :])
    assert np.array_equal(w[idx], x)
    mask = np.ones(len(w), dtype=bool)
    mask[idx.reshape(-1)] = False
    assert np.isnan(w[mask]).all() and mask.sum() == len(w) - A * C_ * L
    assert np.isnan(w[idx.max() + 1:]).all() and len(w) - (idx.max() + 1) >= L       # more than a frame of poison behind the last row
    assert np.isnan(w[:2]).all()


def test_strided_pcm_other_pads():
    x = np.arange(2 * 2 * 8, dtype=np.float32).reshape(2, 2, 8)
    v, whole = dl.strided_pcm(x, row_pad=2, array_pad=4, lead=0, device="cpu")
    assert v.stride() == (24, 10, 1) and v.data_ptr() == whole.data_ptr()
    assert np.array_equal(v.numpy(), x) and int(np.isnan(whole.numpy()).sum()) == len(whole) - 32


@pytest.mark.parametrize("shape,dtype", [((3, 21, 1), torch.int32), ((3, 2, 13 * 512), torch.float32), ((3, 21), torch.uint8),
                                         ((3, 8, 257, 2), torch.float32), ((2, 5, 7), torch.float64)])
def test_guarded_margins(shape, dtype):
    g = dl.guarded(shape, dtype, device="cpu")
    assert tuple(g.t.shape) == shape and g.t.dtype == dtype and g.t.is_contiguous()
    row_bytes = int(np.prod(shape[1:])) * g.t.element_size()
    assert g.margin >= row_bytes and g.margin % 512 == 0
    assert g.t.data_ptr() == g.raw.data_ptr() + g.margin
    g.assert_guards_intact()
    g.t.zero_()                                          # writing the whole output leaves the guards alone
    g.assert_guards_intact()
    assert int((g.raw != dl.GUARD_BYTE).sum()) == g.nbytes
    g.raw[g.margin + g.nbytes] = 0                       # one byte behind it does not
    with pytest.raises(AssertionError):
        g.assert_guards_intact()
    g.raw[g.margin + g.nbytes] = dl.GUARD_BYTE
    g.raw[g.margin - 1] = 1
    with pytest.raises(AssertionError):
        g.assert_guards_intact()
