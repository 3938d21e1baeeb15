"""Guarded buffers for the tests that call the C ABI through ctypes (plain helper, no test in it; tests/test_guarded_buffers.py checks it
on the CPU).

Every buffer a test hands to an entry is a window inside one larger allocation of 32-bit words: PAD words, the window, PAD words.  The
pads — and the elements of the window a test declares to be no payload, the gaps of a leading dimension larger than its matrix — are
filled with one word, chosen by the buffer's role:

  output (also in-place and scratch): SENTINEL_WORD.  ``get()`` asserts that every such word is bitwise what it was: a store outside
      the payload fails an assertion and, being inside memory the test owns, cannot fault the device.
  input: POISON_WORD = 0x7fc07fc0, a NaN read as float32 and a NaN in both halves read as float16 (so it also poisons DM3D_FMT_H2
      operands).  A read outside the payload that reaches a result makes that result non-finite.  ``unchanged()`` asserts that the whole
      allocation still holds what was uploaded: an input must not be written at all.

PAD is 4096 elements on each side: the widest tile an entry stores is 64 channels x 8 voxels = 512 elements, so an overrun of several
tiles stays inside the allocation.  4096 words are 16 KiB, so the window keeps the 16-byte alignment of the allocation.

Also here: the numpy coder of DM3D_FMT_H2 (include/dm3d.h: each run of 16 consecutive k of a row is one 64-byte record
[hi k0-7 | hi k8-15 | lo k0-7 | lo k8-15] of float16), so that tests build and read such operands without a kernel of the library."""
import numpy as np
import torch

PAD = 4096
POISON_WORD = 0x7FC07FC0
SENTINEL_WORD = 0xC7F12000               # the float32 -123456.0

IN, OUT = "in", "out"


def _i32(word):
    return int(np.array([word], np.uint32).view(np.int32)[0])


class Guarded:
    """``arr`` (numpy, 4- or 8-byte elements) between two pads on ``device``.  ``valid``: boolean array of arr's shape, False where an
    element is a gap (filled like the pads; what ``arr`` holds there is ignored)."""

    def __init__(self, arr, device, role, valid=None):
        assert role in (IN, OUT)
        a = np.ascontiguousarray(arr)
        assert a.dtype.itemsize in (4, 8), a.dtype
        self.dtype, self.shape, self.role = a.dtype, a.shape, role
        per = a.dtype.itemsize // 4
        words = a.reshape(-1).view(np.int32).copy()
        self.fill = _i32(POISON_WORD if role == IN else SENTINEL_WORD)
        self.gap = None
        if valid is not None:
            v = np.ascontiguousarray(np.broadcast_to(valid, a.shape)).reshape(-1)
            self.gap = np.repeat(~v, per)
            words[self.gap] = self.fill
        self.n = words.size
        host = np.full(self.n + 2 * PAD, self.fill, np.int32)
        host[PAD:PAD + self.n] = words
        self.host = host
        self.t = torch.from_numpy(host.copy()).to(device)
        self.ptr = self.t.data_ptr() + PAD * 4
        assert self.ptr % 16 == 0, "the window is not 16-byte aligned"

    @classmethod
    def matrix(cls, mat, ld, device, role):
        """[rows, cols] (or [batch, rows, cols]) payload with leading dimension ld >= cols: the columns cols..ld-1 of every row are a gap."""
        m = np.asarray(mat)
        assert ld >= m.shape[-1]
        full = np.zeros(m.shape[:-1] + (ld,), m.dtype)
        full[..., :m.shape[-1]] = m
        valid = np.zeros(full.shape, bool)
        valid[..., :m.shape[-1]] = True
        return cls(full, device, role, valid)

    def _words(self):
        if self.t.is_cuda:
            torch.cuda.synchronize()
        return self.t.cpu().numpy()

    def get(self):
        """The window as an array of the original dtype and shape, after checking that pads and gaps are intact."""
        w = self._words()
        assert (w[:PAD] == self.fill).all(), f"{int((w[:PAD] != self.fill).sum())} words of the pad in front of the buffer were overwritten"
        assert (w[PAD + self.n:] == self.fill).all(), f"{int((w[PAD + self.n:] != self.fill).sum())} words of the pad behind the buffer were overwritten"
        win = w[PAD:PAD + self.n]
        if self.gap is not None:
            assert (win[self.gap] == self.fill).all(), f"{int((win[self.gap] != self.fill).sum())} words of a leading-dimension gap were overwritten"
        return win.copy().view(self.dtype).reshape(self.shape)

    def unchanged(self):
        """Asserts that the allocation (pads, gaps, payload) is bitwise what was uploaded."""
        w = self._words()
        assert np.array_equal(w, self.host), f"{int((w != self.host).sum())} words of an input buffer were written"


def poison_reads():
    """The poison word as float32 and as its two float16 halves."""
    w = np.array([POISON_WORD], np.uint32)
    return float(w.view(np.float32)[0]), float(w.view(np.float16)[0]), float(w.view(np.float16)[1])


# ---- DM3D_FMT_H2 ----------------------------------------------------------------------------------------------------------------------
def h2_encode(x):
    """float32 [..., k] (k % 16 == 0) -> uint32 words [..., k]: per 16 k one record of float16 (hi k0-7, hi k8-15, lo k0-7, lo k8-15) with
    hi = float16(x), lo = float16(x - hi)."""
    x = np.asarray(x, np.float32)
    k = x.shape[-1]
    assert k % 16 == 0
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    rec = np.stack([hi.reshape(x.shape[:-1] + (k // 16, 2, 8)), lo.reshape(x.shape[:-1] + (k // 16, 2, 8))], -3)     # [..., k/16, (hi, lo), 2, 8]
    return np.ascontiguousarray(rec).view(np.uint32).reshape(x.shape[:-1] + (k,))


def h2_decode(words):
    """uint32 / int32 / float32-typed words [..., k] -> float64 [..., k]: hi + lo."""
    w = np.ascontiguousarray(words)
    k = w.shape[-1]
    assert k % 16 == 0 and w.dtype.itemsize == 4
    rec = w.view(np.float16).reshape(w.shape[:-1] + (k // 16, 2, 2, 8)).astype(np.float64)
    return (rec[..., 0, :, :] + rec[..., 1, :, :]).reshape(w.shape[:-1] + (k,))
