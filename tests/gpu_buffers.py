"""Device buffers with canary bytes and the bit-for-bit comparison of the GPU pins (test_gpu_calib.py, test_gpu_train.py): every output and
every statistic or gradient slot a kernel writes sits between 64 canary bytes, and take() asserts that they survived."""
import numpy as np
import pytest
import torch

F32 = np.float32
CB, PAD = 0x55, 64


class Buf:
    """nbytes of device memory `off` bytes past a 64-byte boundary, canary bytes in front and behind; `data` (any array) fills it,
    `fill` (a float32) otherwise."""

    def __init__(self, dev, nbytes, off=0, data=None, fill=None):
        self.n, self.a = nbytes, PAD + off
        h = np.full(self.a + nbytes + PAD, CB, np.uint8)
        if data is not None:
            raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            assert raw.size == nbytes
            h[self.a:self.a + nbytes] = raw
        elif fill is not None:
            h[self.a:self.a + nbytes] = np.full(nbytes // 4, fill, F32).view(np.uint8)
        t = torch.empty(h.size + 64, dtype=torch.uint8, device=dev)
        skip = -t.data_ptr() % 64
        self.t = t[skip:skip + h.size]
        self.t.copy_(torch.from_numpy(h))
        assert self.t.data_ptr() % 64 == 0
        self.ptr = self.t.data_ptr() + self.a

    def dev_view(self, dtype):
        """The payload as a device tensor of `dtype` (writes go straight to the buffer)."""
        return self.t[self.a:self.a + self.n].view(dtype)

    def take(self, dtype, what):
        h = self.t.cpu().numpy()
        assert np.all(h[:self.a] == CB), "canary in front of %s changed" % what
        assert np.all(h[self.a + self.n:] == CB), "canary behind %s changed" % what
        return h[self.a:self.a + self.n].copy().view(dtype)


class Slots:
    """n one-float statistic slots, each with 64 canary bytes in front of it and behind it."""
    W = 33

    def __init__(self, dev, n, init):
        h = np.full((n, self.W), CB, np.uint8).repeat(4, axis=1).view(F32).copy()
        h[:, 16] = init
        self.n = n
        self.t = torch.from_numpy(h).to(dev)

    def ptr(self, i):
        return self.t.data_ptr() + (i * self.W + 16) * 4

    def take(self, what):
        h = self.t.cpu().numpy()
        keep = np.ones(self.W, bool)
        keep[16] = False
        assert np.all(np.ascontiguousarray(h[:, keep]).view(np.uint8) == CB), "canary around a statistic slot of %s changed" % what
        return h[:, 16].copy()


def _bits(v):
    v = np.asarray(v)
    return "0x%0*x" % (2 * v.dtype.itemsize, int(v.view({2: np.uint16, 4: np.uint32}[v.dtype.itemsize])))


def same(got, want):
    """Elementwise: NaN where the oracle has NaN, == elsewhere (+0 == -0: the project documents that the zeros may swap sign)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return (np.isnan(got) & np.isnan(want)) | (got == want)


def check_bits(got, want, x, what):
    """Bit for bit (NaN exactly where the oracle has one); names the first differing (row, column)."""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F32, (what, got.shape, want.shape)
    ng, nw = np.isnan(got), np.isnan(want)
    bad = np.argwhere((ng != nw) | (~nw & ~ng & (got.view(np.uint32) != want.view(np.uint32))))
    if len(bad):
        r, c = (int(v) for v in bad[0])
        xv = np.atleast_2d(x)[r, c] if x is not None else F32(0)
        pytest.fail("%s: %d of %d differ, first at (row %d, col %d): got %r (%s) want %r (%s), input %r (%s)"
                    % (what, len(bad), got.size, r, c, float(got[r, c]), _bits(got[r, c]), float(want[r, c]), _bits(want[r, c]), float(xv), _bits(xv)))
