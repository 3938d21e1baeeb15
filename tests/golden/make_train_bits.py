"""Records tests/golden/train_bits.npz: the bits the training entries with a bitwise contract leave on the GPU (dm3d_adam_ema,
dm3d_adam_scaled, dm3d_grad_scale, dm3d_objective_loss_grad, dm3d_guide_update with a rescale), so that a change to their kernels can be
held against a build made before it.  tests/test_gpu_train_bits.py replays every case through ``run_case`` below and wants the same bits.

    python tests/golden/make_train_bits.py [--root TREE] [--out FILE]

``--root TREE`` imports the package of another tree (a worktree of the commit to record, built there); the cases and the guarded buffers
are this tree's.  Inputs are not stored: every case draws them from ``numpy.random.default_rng(seed)`` and the file keeps the seed.
Outputs are stored as uint32 / uint64 views, or, where ``digest`` is set, as the SHA-256 of their bytes (32 uint8).  Needs a GPU.
"""
import argparse
import ctypes
import hashlib
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))                    # tests/: guarded_buffers
from guarded_buffers import IN, OUT, Guarded  # noqa: E402

B1, B2, EPS = 0.9, 0.999, 1e-7
ADAM_LR = 0.5
RATES = (1.0, 0.25, 0.0)                                     # test_adam_ema_kernel's three steps
SCALE = 0.3717
BIG = 4 * (4096 * 256 + 1001)                                # past the cap of the Adam grid (4096 blocks) and of grad_sqnorm's (1024)
ADAM_SIZES = (4, 1004, BIG)
NORM_SIZES = (4, 1004, 4 * (3 * 256 + 7), BIG)
LOSS_PARTS, GUIDE_PARTS, NORM_PARTS = 64, 256, 1024          # DM3D_*_PARTIAL_BLOCKS
LOSS_SIZES = (4, 1004, 4 * (256 * LOSS_PARTS + 5))
GUIDE_SIZES = (4, 1004, 4 * (256 * GUIDE_PARTS + 5))
LOSS_ROWS = np.array([[0.8, -0.6, 1.0, 0.0], [0.31, 0.95, 0.37, 0.0]], np.float32)       # (a_z, a_0, w, unused) per sample
LOSS_INV = 1.0 / 4096.0 / 3.0
GUIDE_W, GUIDE_PHI = np.array([2.5, -0.7], np.float32), np.array([0.7, 0.4], np.float32)


def _cases():
    c = {}
    for n in ADAM_SIZES:
        for variant in ("ema", "scaled_ema", "scaled_plain", "scaled_skip"):
            c[f"adam_{variant}-n{n}"] = dict(kind="adam", variant=variant, n=n, digest=n == BIG)
    for n in NORM_SIZES:
        for clip in (1.0, float("inf")):
            for pre in (1.0, 0.5):
                c[f"grad_scale-n{n}-clip{clip}-pre{pre}"] = dict(kind="grad_scale", n=n, clip=clip, pre=pre, digest=n == BIG)
    for per in LOSS_SIZES:
        c[f"objective-per{per}"] = dict(kind="objective", per=per, digest=per == LOSS_SIZES[-1])
    for per in GUIDE_SIZES:
        c[f"guide-per{per}"] = dict(kind="guide", per=per, digest=True)
    return c


CASES = _cases()


def seed_of(case_id):
    return zlib.crc32(case_id.encode())


def pack(arr, digest=False):
    """The bits of ``arr`` as unsigned words of its element size, or the SHA-256 of its bytes."""
    a = np.ascontiguousarray(arr)
    if digest:
        return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8).copy()
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).copy()


def _call(name, *args):
    from dm3d_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args, None), name)


# ---- inputs (also what the CPU check of the recording reads) ---------------------------------------------------------------------------
def adam_inputs(n, seed):
    rng = np.random.default_rng(seed)

    def f(scale, power=1):
        return (rng.standard_normal(n) ** power * scale).astype(np.float32)

    start = dict(w=f(0.1), m=f(0.1), v=f(0.01, 2), ema=f(0.1))                  # non-zero moments; v >= 0
    grads = [f(1.0) for _ in RATES]
    lr_ts = [float(np.float32(ADAM_LR * np.sqrt(1 - B2 ** t) / (1 - B1 ** t))) for t in range(1, len(RATES) + 1)]
    return start, grads, lr_ts


def adam_state(variant):
    """The 16-byte state dm3d_adam_scaled reads: (norm, factor, non-finite flag, 0)."""
    return np.array([7.0, SCALE if variant == "scaled_ema" else 1.0, 1.0 if variant == "scaled_skip" else 0.0, 0.0], np.float32)


def norm_inputs(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


# ---- one case on the device: {output name: packed bits} ----------------------------------------------------------------------------------
def _adam(dev, seed, variant, n, digest):
    start, grads, lr_ts = adam_inputs(n, seed)
    with_ema = variant != "scaled_plain"
    buf = {k: Guarded(start[k], dev, OUT) for k in ("w", "m", "v")}
    if with_ema:
        buf["ema"] = Guarded(start["ema"], dev, OUT)
    state = None if variant == "ema" else Guarded(adam_state(variant), dev, IN)
    for g, lr_t, rate in zip(grads, lr_ts, RATES):
        bg = Guarded(g, dev, IN)
        args = (buf["w"].ptr, bg.ptr, buf["m"].ptr, buf["v"].ptr, buf["ema"].ptr if with_ema else None, n, lr_t, B1, B2, EPS, rate)
        if variant == "ema":
            _call("dm3d_adam_ema", *args)
        else:
            _call("dm3d_adam_scaled", *args, state.ptr)
        buf["w"].get()                                       # (synchronises, and checks the pads, before g is read back)
        bg.unchanged()
    if state is not None:
        state.unchanged()
    return {k: pack(b.get(), digest) for k, b in buf.items()}


def _grad_scale(dev, seed, n, clip, pre, digest):
    from dm3d_amd import _lib
    g = Guarded(norm_inputs(n, seed), dev, IN)
    parts, state = Guarded(np.full(NORM_PARTS, np.nan), dev, OUT), Guarded(np.full(4, np.nan, np.float32), dev, OUT)
    d = _lib.GradScaleDesc()
    d.g, d.n, d.partials, d.state, d.clip_norm, d.pre_scale = g.ptr, n, parts.ptr, state.ptr, clip, pre
    _call("dm3d_grad_scale", ctypes.byref(d))
    out = dict(partials=pack(parts.get(), digest), state=pack(state.get()))
    g.unchanged()
    return out


def _objective(dev, seed, per, digest):
    from dm3d_amd import _lib
    rng = np.random.default_rng(seed)
    B = len(LOSS_ROWS)
    pred, noise, x0 = (Guarded(rng.standard_normal((B, per)).astype(np.float32), dev, IN) for _ in range(3))
    coef = Guarded(LOSS_ROWS, dev, IN)
    dpred = Guarded(np.full((B, per), np.nan, np.float32), dev, OUT)
    parts = Guarded(np.full((B, LOSS_PARTS), np.nan), dev, OUT)
    rows, loss = Guarded(np.full(B, np.nan), dev, OUT), Guarded(np.full(1, np.nan), dev, OUT)
    d = _lib.LossDesc()
    d.pred, d.noise, d.x0, d.coef, d.dpred = pred.ptr, noise.ptr, x0.ptr, coef.ptr, dpred.ptr
    d.partials, d.loss_rows, d.loss = parts.ptr, rows.ptr, loss.ptr
    d.batch, d.per_sample, d.inv_divisor = B, per, LOSS_INV
    _call("dm3d_objective_loss_grad", ctypes.byref(d))
    used = min(-(-(per // 4) // 256), LOSS_PARTS)
    out = dict(partials=pack(parts.get()[:, :used]), loss_rows=pack(rows.get()), loss=pack(loss.get()), dpred=pack(dpred.get(), digest))
    for b in (pred, noise, x0, coef):
        b.unchanged()
    return out


def _guide(dev, seed, per, digest):
    from dm3d_amd import _lib
    rng = np.random.default_rng(seed)
    B = len(GUIDE_W)
    ep = Guarded((rng.standard_normal((B, per)) + 0.5).astype(np.float32), dev, IN)
    en = Guarded(rng.standard_normal((B, per)).astype(np.float32), dev, IN)
    scale, rescale = Guarded(GUIDE_W, dev, IN), Guarded(GUIDE_PHI, dev, IN)
    out = Guarded(np.full((B, per), np.nan, np.float32), dev, OUT)
    parts = Guarded(np.full((B, GUIDE_PARTS, 4), np.nan), dev, OUT)
    for mode in (0, 1):                                      # the combine with its sums, then the rescale that reads them
        d = _lib.GuideDesc()
        d.mode, d.batch, d.per_sample, d.out, d.rescale, d.partials = mode, B, per, out.ptr, rescale.ptr, parts.ptr
        if mode == 0:
            d.eps_pos, d.eps_neg, d.scale = ep.ptr, en.ptr, scale.ptr
        _call("dm3d_guide_update", ctypes.byref(d))
    used = min(-(-(per // 4) // 256), GUIDE_PARTS)
    res = dict(partials=pack(parts.get()[:, :used]), out=pack(out.get(), digest))
    for b in (ep, en, scale, rescale):
        b.unchanged()
    return res


def run_case(dev, case_id, seed):
    spec = dict(CASES[case_id])
    return {"adam": _adam, "grad_scale": _grad_scale, "objective": _objective, "guide": _guide}[spec.pop("kind")](dev, seed, **spec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT, help="the tree whose package is imported")
    ap.add_argument("--out", default=os.path.join(HERE, "train_bits.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import dm3d_amd  # noqa: F401
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    assert (_lib.LOSS_PARTIAL_BLOCKS, _lib.GUIDE_PARTIAL_BLOCKS, _lib.GRADNORM_PARTIAL_BLOCKS) == (LOSS_PARTS, GUIDE_PARTS, NORM_PARTS)
    rec = {}
    for case_id in CASES:
        seed = seed_of(case_id)
        first, again = run_case(dev, case_id, seed), run_case(dev, case_id, seed)
        for k, v in first.items():
            assert np.array_equal(v, again[k]), f"{case_id}: {k} does not repeat"
            rec[f"{case_id}/{k}"] = v
        rec[f"{case_id}/seed"] = np.asarray(seed, np.uint32)
        print(case_id, {k: v.shape for k, v in first.items()}, flush=True)
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {len(CASES)} cases, {os.path.getsize(args.out)} bytes (library {_lib.LIB_PATH})")


if __name__ == "__main__":
    main()
