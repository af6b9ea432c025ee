"""Buffers for the tests of the device-pointer ABI (tests/test_gpu_dev_layout.py, tests/test_dev_layout_cpu.py).

strided_pcm() puts PCM into a poisoned allocation at padded strides: whatever a kernel reads outside the samples it was promised
is NaN and ends up in a result.  guarded() carves an output out of a larger buffer whose margins hold a fixed bit pattern: whatever
a kernel writes outside its output changes them.  Both work on CPU tensors as well (the index arithmetic is checked there)."""
import numpy as np
import torch

ROW_PAD, ARRAY_PAD, LEAD = 6, 10, 2      # a pitch of L + 6 == 2 (mod 4) for L a multiple of 4: every other row is only 8-byte aligned
GUARD_BYTE = 0xA5                        # float32 0xA5A5A5A5 = -2.87e-16, int32 -1515870811: finite, and nothing a kernel would write


def strided_pcm(x, row_pad=ROW_PAD, array_pad=ARRAY_PAD, lead=LEAD, device="cuda"):
    """x: contiguous [A][C][L] float32 (numpy or torch) -> (view, whole): `whole` is one NaN-filled allocation, `view` the [A][C][L]
    view of it that starts `lead` floats in, with rows L + row_pad apart and arrays C * (L + row_pad) + array_pad apart, holding x.
    A whole row of NaN (L + row_pad floats: more than a frame) stays behind the last row."""
    x = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x)
    assert x.dim() == 3 and x.dtype == torch.float32
    A, C_, L = x.shape
    pitch = L + row_pad
    a_stride = C_ * pitch + array_pad
    total = lead + A * a_stride + pitch
    whole = torch.full((total,), float("nan"), dtype=torch.float32, device=device)
    view = torch.as_strided(whole, (A, C_, L), (a_stride, pitch, 1), lead)
    view.copy_(x.to(device))
    return view, whole


class Guarded:
    """`.t`: a contiguous tensor of `shape` inside a larger allocation; assert_guards_intact(): the margins before and behind it
    still hold the bit pattern they were filled with."""

    def __init__(self, shape, dtype, device="cuda"):
        item = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(shape))
        row = int(np.prod(shape[1:])) if len(shape) > 1 else n           # one output row: everything of one array / stream
        # (a multiple of 512 bytes: the view is aligned like a fresh allocation, so a kernel choice that depends on the alignment
        # of an output is the same for both)
        self.margin = -(-max(row, 1) * item // 512) * 512
        self.nbytes = n * item
        self.raw = torch.full((2 * self.margin + self.nbytes,), GUARD_BYTE, dtype=torch.uint8, device=device)
        self.t = self.raw[self.margin:self.margin + self.nbytes].view(dtype).view(*shape)

    def assert_guards_intact(self, what=""):
        before = self.raw[:self.margin]
        behind = self.raw[self.margin + self.nbytes:]
        for name, g in (("before", before), ("behind", behind)):
            bad = torch.nonzero(g != GUARD_BYTE)
            assert bad.numel() == 0, "%s: %d guard bytes %s the output were overwritten, the first at offset %d" % (
                what, bad.numel(), name, int(bad[0]))


def guarded(shape, dtype, device="cuda"):
    return Guarded(tuple(int(s) for s in shape), dtype, device)
