"""The guarded buffers of tests/guarded_buffers.py on CPU tensors: alignment, the pads and gaps, what get() and unchanged() notice, the
poison word, and the DM3D_FMT_H2 coder."""
import math

import numpy as np
import pytest
import torch

import guarded_buffers as gb

CPU = torch.device("cpu")


def test_poison_word_is_nan_in_all_three_readings():
    as_f32, half_lo, half_hi = gb.poison_reads()
    assert math.isnan(as_f32) and math.isnan(half_lo) and math.isnan(half_hi)
    assert gb.PAD == 4096 and gb.PAD * 4 % 16 == 0


@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.uint32, np.float64, np.uint64])
@pytest.mark.parametrize("role", [gb.IN, gb.OUT])
def test_window_is_aligned_and_round_trips(dtype, role):
    arr = (np.arange(3 * 5).reshape(3, 5) * 7 - 11).astype(dtype)
    b = gb.Guarded(arr, CPU, role)
    assert b.ptr % 16 == 0 and b.ptr == b.t.data_ptr() + gb.PAD * 4
    assert b.t.numel() == arr.size * (arr.dtype.itemsize // 4) + 2 * gb.PAD
    got = b.get()
    assert got.dtype == arr.dtype and np.array_equal(got, arr)
    b.unchanged()
    fill = gb.POISON_WORD if role == gb.IN else gb.SENTINEL_WORD
    assert int(b.t[0]) & 0xFFFFFFFF == fill and int(b.t[-1]) & 0xFFFFFFFF == fill


@pytest.mark.parametrize("where", [0, gb.PAD - 1, -gb.PAD, -1])
def test_get_raises_when_a_pad_word_changes(where):
    b = gb.Guarded(np.ones(8, np.float32), CPU, gb.OUT)
    b.get()
    b.t[where] += 1                                          # one bit of one word
    with pytest.raises(AssertionError, match="pad"):
        b.get()
    with pytest.raises(AssertionError, match="written"):
        b.unchanged()


def test_payload_stores_are_allowed_for_outputs_and_noticed_for_inputs():
    b = gb.Guarded(np.zeros(8, np.float32), CPU, gb.IN)
    b.t[gb.PAD + 3] = 5
    b.get()                                                  # the pads are intact
    with pytest.raises(AssertionError, match="written"):
        b.unchanged()


def test_matrix_gaps_are_filled_and_checked():
    m = np.arange(12, dtype=np.float32).reshape(3, 4)
    out = gb.Guarded.matrix(m, 6, CPU, gb.OUT)
    assert out.shape == (3, 6) and np.array_equal(out.get()[:, :4], m)
    assert (out.get()[:, 4:].view(np.uint32) == gb.SENTINEL_WORD).all()
    inp = gb.Guarded.matrix(m, 6, CPU, gb.IN)
    assert np.isnan(inp.get()[:, 4:]).all() and np.array_equal(inp.get()[:, :4], m)
    out.t[gb.PAD + 1] = 9                                    # payload: fine
    out.get()
    out.t[gb.PAD + 6 + 5] = 9                                # row 1, column 5: a gap
    with pytest.raises(AssertionError, match="gap"):
        out.get()
    batched = gb.Guarded.matrix(np.zeros((2, 3, 4), np.float32), 8, CPU, gb.OUT)
    assert batched.shape == (2, 3, 8) and int(batched.gap.sum()) == 2 * 3 * 4


def test_h2_coder():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((5, 48)) * 100).astype(np.float32)
    w = gb.h2_encode(x)
    assert w.shape == x.shape and w.dtype == np.uint32
    assert np.abs(gb.h2_decode(w) - x).max() <= 2.0 ** -21 * np.abs(x).max()
    rec = w[0, :16].view(np.float16)                         # the record layout of include/dm3d.h
    hi = x[0, :16].astype(np.float16)
    assert np.array_equal(rec[:16], hi) and np.array_equal(rec[16:], (x[0, :16] - hi.astype(np.float32)).astype(np.float16))
    poison = np.full((1, 16), gb.POISON_WORD, np.uint32)
    assert np.isnan(gb.h2_decode(poison)).all()
