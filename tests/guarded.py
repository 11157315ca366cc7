"""Poison-guarded output buffers, shared by the GPU sweeps
(tests/test_gpu_query_sweep.py, tests/test_gpu_given_sweep.py): a kernel's
output is a view into a byte buffer filled with a poison byte; the bytes before
and after it must stay poison, and a cell the kernel skipped differs from the
reference under one of the two poisons every call is run with."""
import numpy as np

POISONS = (0xA5, 0x5A)
LEAD = 64                  # guard bytes before and after an output


class Guarded:
    """An output tensor of ``dtype`` and ``shape`` inside a byte buffer filled
    with ``poison``, LEAD + ``skew`` bytes in (``skew`` 0: 16-byte aligned)."""

    def __init__(self, dev, dtype, shape, poison, skew=0):
        import torch
        size = torch.empty((), dtype=dtype).element_size()
        self.lead, self.n, self.poison = LEAD + skew, int(np.prod(shape)) * size, poison
        self.buf = torch.full((self.lead + self.n + LEAD,), poison, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 16 == 0 and self.lead % size == 0
        self.out = self.buf[self.lead:self.lead + self.n].view(dtype).view(shape)
        assert self.out.data_ptr() % 16 == skew % 16

    def check(self, want, what):
        """The guards are intact and the output is ``want`` (numpy), exactly."""
        buf = self.buf.cpu().numpy()
        assert (buf[:self.lead] == self.poison).all(), (what, "bytes before the output written")
        assert (buf[self.lead + self.n:] == self.poison).all(), (what, "bytes after it written")
        same(self.out, want, what)


def same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} cells differ, first at {bad[:5].tolist()}: got "
                             f"{got[tuple(bad[0])]}, reference {want[tuple(bad[0])]}")
