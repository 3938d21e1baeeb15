"""The pad step of the Winograd-x conv (dm3d_conv_h3w.hip) after the fold: tap pair 3 = (0, 2) | pad runs two passes on ONE mixed A fragment
(lane half 0: the hi piece of tap (0, 2), half 1: the lo piece of the same records) against a weight slice whose pad half repeats the hi pieces
of (0, 2) over zero lo pieces — mixed.bh = ah.bh + al.bh in one MFMA, mixed.bl = ah.bl.

Reference: the float64 conv of tests/test_gpu_wino.py; bar: the per-kernel 2e-5 of max|ref|.  Inputs and weights are
random float32 that float16 cannot hold (lo != 0): a lost al.bh term is a relative error of about 2^-11 = 5e-4 of the (0, 2) tap's share.
Every case runs with three weight patterns: all taps, only (dz, dy) = (0, 2) (the folded step alone), only (1, 2) (the voxels the pad half
used to read against zeros: a leak of the repeated bh into that tap shows here).  The packer test reads the image itself.

Measured max|err| / max|ref| on MI355X (profiles/wino_fold_gpu_run.log, parent and this kernel side by side): 1.6e-7 .. 5.6e-7 for both; the
fold moves a case by at most 6e-8."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from test_gpu_wino import _ref_conv, _rel          # noqa: E402  (the float64 reference and the error measure of the Winograd suite)

pytestmark = pytest.mark.gpu
BAR = 2e-5
PATTERNS = ("all taps", "only (0,2)", "only (1,2)")


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


@pytest.fixture()
def small_grids(monkeypatch):
    """The policy keeps small launches on the direct kernel; the knobs (read per call) admit the test shapes."""
    monkeypatch.setenv("DM3D_CONV_WIDE_WGS", "1")
    monkeypatch.setenv("DM3D_CONV_WINO_MINCHUNKS", "1")


def _kernel(cin, cout, pattern, dev, scale=0.05):
    k = torch.randn(3, 3, 3, cin, cout, device=dev) * scale
    if pattern != "all taps":
        dz = 0 if pattern == "only (0,2)" else 1
        keep = torch.zeros_like(k)
        keep[dz, 2] = k[dz, 2]
        k = keep
    return k


def _pro(c, dev):
    return torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev) * 0.1


def _is_wino(y_wino, y_direct):
    assert not torch.equal(y_wino, y_direct), "the Winograd form did not run (its results differ from the direct kernel's in the last bits)"


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("cin", [32, 48])
def test_fold_mode1_prologue(dev, small_grids, cin, pattern):
    from dm3d_amd import ops, _lib
    torch.manual_seed(11)
    x = torch.randn(1, 8, 8, 8, cin, device=dev)
    k = _kernel(cin, 64, pattern, dev)
    wpk, w_exp = ops.pack_weights_h3(k)
    wino = ops.pack_weights_h3w(k, w_exp)
    bias, ps = torch.randn(64, device=dev) * 0.1, _pro(cin, dev)
    kw = dict(bias=bias, pro_scale=ps[0], pro_shift=ps[1], precision=_lib.PREC_H3, w_exp=w_exp)
    y = ops.conv3d(x, wpk, 64, 3, wpk_wino=wino, **kw)
    _is_wino(y, ops.conv3d(x, wpk, 64, 3, **kw))
    e = _rel(y, _ref_conv(x, k, bias, ps))
    print(f"fold MODE 1 prologue Cin={cin} {pattern}: {e:.2e}")
    assert e < BAR


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("cin", [32, 48])
def test_fold_mode2_behind_h2_hand_off(dev, small_grids, cin, pattern):
    """The producer's side of the hand-off is its DM3D_FMT_H2 buffer: an activation split into float16 (hi, lo) pairs (dm3d_split_h2 — a conv
    writes that format for whole 64-channel tiles only, and these shapes have 32 and 48); the consumer (kernel MODE 2) rebuilds float32,
    transforms and splits again.  Its reference is the float64 conv of exactly the values stored (hi + lo, decoded on the host)."""
    from dm3d_amd import ops, _lib
    torch.manual_seed(12)
    act = torch.randn(1, 8, 8, 8, cin, device=dev)
    act = act * torch.sigmoid(act)
    a = ops.split_h2(act.reshape(-1, cin)).reshape(1, 8, 8, 8, cin)
    mid = ops.h2_to_f32(a.reshape(-1, cin), cin).reshape(1, 8, 8, 8, cin)
    assert float((mid - mid.half().float()).abs().max()) > 0, "the hand-off carries no lo part"
    k = _kernel(cin, 64, pattern, dev)
    wpk, w_exp = ops.pack_weights_h3(k)
    wino = ops.pack_weights_h3w(k, w_exp)
    kw = dict(precision=_lib.PREC_H3, w_exp=w_exp, x1_h2_channels=cin)
    y = ops.conv3d(a, wpk, 64, 3, wpk_wino=wino, **kw)
    _is_wino(y, ops.conv3d(a, wpk, 64, 3, **kw))
    e = _rel(y, _ref_conv(mid, k))
    print(f"fold MODE 2 hand-off Cin={cin} {pattern}: {e:.2e}")
    assert e < BAR


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("cin", [32, 48])
def test_fold_with_fused_skip_tail(dev, small_grids, cin, pattern):
    from dm3d_amd import ops, _lib
    torch.manual_seed(13)
    h = torch.randn(1, 8, 8, 8, cin, device=dev)
    sx = torch.randn(1, 8, 8, 8, 40, device=dev)
    k = _kernel(cin, 64, pattern, dev)
    ks = torch.randn(1, 1, 1, 40, 64, device=dev) * 0.05
    w_exp = ops.h3_weight_exponent(k.cpu(), ks.cpu())
    wpk, _ = ops.pack_weights_h3(k, w_exp=w_exp)
    wino = ops.pack_weights_h3w(k, w_exp)
    swpk, sfrag = ops.pack_weights_skip_h3p(ks, w_exp), ops.pack_weights_skip_h3f(ks, w_exp)
    bias, ps = torch.randn(64, device=dev) * 0.1, _pro(cin, dev)
    kw = dict(bias=bias, pro_scale=ps[0], pro_shift=ps[1], precision=_lib.PREC_H3, w_exp=w_exp)
    y = ops.conv3d(h, wpk, 64, 3, wpk_wino=wino, skip=(sx, None, swpk, sfrag), **kw)
    _is_wino(y, ops.conv3d(h, wpk, 64, 3, skip=(sx, None, swpk), **kw))
    yr = _ref_conv(h, k, bias, ps) + torch.einsum("bdhwc,co->bdhwo", sx.double(), ks.double()[0, 0, 0])
    e = _rel(y, yr)
    print(f"fold + skip tail Cin={cin} {pattern}: {e:.2e}")
    assert e < BAR


@pytest.mark.parametrize("pattern", PATTERNS)
def test_fold_cin64_two_way_split(dev, small_grids, monkeypatch, pattern):
    """Cin = 64 as two parts of two chunks (DM3D_CONV_WINO_SPLIT_MINCHUNKS admits it): the parts meet behind the shared chunk loop."""
    from dm3d_amd import ops, _lib
    monkeypatch.setenv("DM3D_CONV_WINO_SPLIT_MINCHUNKS", "4")
    torch.manual_seed(14)
    x = torch.randn(1, 8, 8, 8, 64, device=dev)
    k = _kernel(64, 64, pattern, dev)
    wpk, w_exp = ops.pack_weights_h3(k)
    wino = ops.pack_weights_h3w(k, w_exp)
    bias, ps = torch.randn(64, device=dev) * 0.1, _pro(64, dev)
    kw = dict(bias=bias, pro_scale=ps[0], pro_shift=ps[1], precision=_lib.PREC_H3, w_exp=w_exp, wpk_wino=wino)
    y = ops.conv3d(x, wpk, 64, 3, **kw)
    whole = ops.conv3d(x, wpk, 64, 3, split=False, **kw)
    assert not torch.equal(y, whole), "the launch did not split"
    e, e1 = _rel(y, _ref_conv(x, k, bias, ps)), _rel(whole, _ref_conv(x, k, bias, ps))
    print(f"fold Cin=64 two-way split {pattern}: {e:.2e} (unsplit {e1:.2e})")
    assert e < BAR and e1 < BAR


@pytest.mark.parametrize("pattern", PATTERNS)
def test_fold_persistent_workgroups_walk_item_lists(dev, small_grids, monkeypatch, pattern):
    """B = 2 at 16^3 = 16 items on 8 workgroups: every workgroup stages its second item's first steps during its first item's last chunk."""
    from dm3d_amd import ops, _lib
    monkeypatch.setenv("DM3D_CONV_WINO_GRID", "8")
    torch.manual_seed(15)
    x = torch.randn(2, 16, 16, 16, 32, device=dev)
    k = _kernel(32, 64, pattern, dev)
    wpk, w_exp = ops.pack_weights_h3(k)
    wino = ops.pack_weights_h3w(k, w_exp)
    bias, ps = torch.randn(64, device=dev) * 0.1, _pro(32, dev)
    kw = dict(bias=bias, pro_scale=ps[0], pro_shift=ps[1], precision=_lib.PREC_H3, w_exp=w_exp)
    y = ops.conv3d(x, wpk, 64, 3, wpk_wino=wino, **kw)
    _is_wino(y, ops.conv3d(x, wpk, 64, 3, **kw))
    e = _rel(y, _ref_conv(x, k, bias, ps))
    print(f"fold persistent B=2 16^3 {pattern}: {e:.2e}")
    assert e < BAR


def test_packer_pad_half_repeats_tap_02_hi(dev):
    """The (Cin = 32, Cout = 64) image, [chunk][virtual tap = 2 (5 term + pair) + half][64 positions][4 slots of 8 halfs, slot ^ position
    swizzle]: the pad half of pair 3 is tap (0, 2)'s hi pieces over zero lo pieces for every chunk, term and column; every other record is
    the split of the F(2,3)-transformed weight, bit for bit; no negative zero, nothing that is not finite."""
    from dm3d_amd import ops
    import lds_model
    torch.manual_seed(16)
    cin, cout = 32, 64
    k = torch.randn(3, 3, 3, cin, cout, device=dev) * 0.05
    _, w_exp = ops.pack_weights_h3(k)
    img = ops.pack_weights_h3w(k, w_exp).cpu()
    assert img.numel() == 2 * 40 * 64 * 32
    bits = img.view(torch.int16)
    assert int((bits == -32768).sum()) == 0 and bool(torch.isfinite(img.float()).all())
    rec = img.reshape(2, 40, 64, 4, 8)
    pos = torch.arange(64)
    sw = (pos >> 2) & 3
    pieces = torch.stack([rec[:, :, pos, j ^ sw] for j in range(4)], 3)          # [chunk][tap][pos][logical piece: hi 0-7, hi 8-15, lo 0-7, lo 8-15][8]
    hi, lo = pieces[:, :, :, 0:2].reshape(2, 40, 64, 16), pieces[:, :, :, 2:4].reshape(2, 40, 64, 16)
    # the expected image from the kernel in float32, the packer's operations in its order
    inv = {lds_model.pi_pos(c): c for c in range(16)}
    co = torch.tensor([4 * inv[p & 15] + (p >> 4) for p in range(64)])
    kc = k.cpu()
    g0, g1, g2 = kc[:, :, 0], kc[:, :, 1], kc[:, :, 2]                            # [dz][dy][cin][cout]
    u = torch.stack([g0, 0.5 * ((g0 + g2) + g1), 0.5 * ((g0 + g2) - g1), g2]) * (2.0 ** w_exp)
    pairs = [((0, 0), (0, 1)), ((1, 0), (1, 1)), ((2, 0), (2, 1)), ((0, 2), None), ((1, 2), (2, 2))]
    for t in range(4):
        for p, taps in enumerate(pairs):
            for h, tap in enumerate(taps):
                vt = 2 * (5 * t + p) + h
                if tap is None:
                    assert torch.equal(hi[:, vt], hi[:, vt - 1]), f"term {t}: the pad half's hi pieces are not tap (0,2)'s"
                    assert int((lo[:, vt].view(torch.int16) != 0).sum()) == 0, f"term {t}: the pad half's lo pieces are not zero"
                    continue
                v = u[t, tap[0], tap[1]].reshape(2, 16, cout)[:, :, co].permute(0, 2, 1)      # [chunk][pos][k]
                e_hi = v.half()
                e_lo = (v - e_hi.float()).half()
                assert torch.equal(hi[:, vt], e_hi) and torch.equal(lo[:, vt], e_lo), f"term {t} pair {p} half {h}"
    assert float(lo.float().abs().max()) > 0
