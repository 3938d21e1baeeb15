"""GPU parity of the sampler entries of the C ABI — the kernels that run between the U-Net and the next step of every non-DDPM chain —
one kernel at a time, called through ctypes as a host would, with EVERY device buffer inside guard bands (tests/guarded_buffers.py).

Two references, both in oracle/ref_kernels.py.  order="f32" restates an entry as individually rounded float32 operations in the order
include/dm3d.h states; the kernels are held to it BITWISE (noise injected).  order="f64" is the same formula in float64; the kernels are
held to it at the project's bars (KERNEL_BAR x coefficient mass for the updates, 2e-6 for the edit kernel, tests/test_gpu_guidance.py's
2^-22 M / 2^-21 M f for the guidance, tests/test_gpu_objective.py's 1e-10 / 1e-5 for the loss), so that a restatement that copied a
misreading of the header's order does not pass on its own.  tests/test_ref_kernels.py ties the restatements to the paper forms.

What the guard bands see.  Outputs, in-place buffers, t_idx, bound, partials and scratch sit between 4096 sentinel words and start out
full of the sentinel: a store outside the payload fails `get()`, and an element a grid-stride loop skipped still holds the sentinel and
fails the bitwise comparison.  Everything `const` in the header sits between 4096 NaN words and is asserted unwritten, tables included.

Tables are made by hand: an unrelated random O(1) value in every column an entry reads, the poison word (a NaN) in every column the
header calls unread in that call — columns 6 and 7 of `coef` (7 for the SDE table), columns 0 and 1 with a frame table, columns 2 and
3 of a frame row for the DPM kernels and the threshold, everything but 0, 1 and 5 (5 with a frame) for the threshold, column 3 of the
level table — and the rows that switch a branch (c_1 == 0, clip == 0 / != 0, c_z == 0, sigma == 0, sqrt(1-a') == 0, the row to clean).
Each update kernel also runs once on the host's own tables of a 5-step schedule (DiffusionModel._ddim_table / _dpm_table /
_dpm_sde_table, schedules.frame_table), so the hand-made layout cannot drift from the host's.

Sizes (per_sample): 4 (one float4), 1004 (one partial block), 2060 (two blocks and 3 float4), 263180 (the 256-block cap and a second
trip of one full and one partial block; batch 2), 2 105 356 for the threshold alone (its 256 x 2048-float4 grid wraps there; batch 1),
131084 for the loss (its 64-block cap).  dm3d_edit_update needs channels | per_sample: channels 3, 6 and 8 run at 24, 1008, 2064 and
263184 (= 4 (65536 + 256 + 4)) instead, the same paths.

Entries and cases
  dm3d_ddim_update / dm3d_dpm_update / dm3d_dpm_sde_update and their _frame forms: modes 0 and 1 (mode 1 in place, out / x0_out handed
      over as sentinels that must stay), with and without a frame table and a dynamic bound; x0_out NULL; hist NULL on c_1 != 0 rows
      (bitwise the c_1 = 0 table); t_idx NULL and set; pos outside [0, rows) against its clamp, bitwise; x0_bound all ones against NULL;
      hist all-NaN on first-order rows, noise all-NaN on no-noise rows; dpm_sde on a c_z = 0 table against dm3d_dpm_update;
      *_frame(d, NULL) against the plain entry; the clip fraction of every clipping row between 0.2 and 0.8.
  in-kernel Philox (ddim, dpm_sde, edit): the draw recovered through a unit row and injected into a general row equals the drawn
      result bitwise; seed_dev; other seeds, other tau, the other kernels differ; (4, P) read flat equals (1, 4P) (one side wraps the
      grid); mean and variance at tests/test_gpu_ddim.py's bars.  Against the host reference oracle/ref_philox.py (Philox4x32-10 from
      the paper, the float32 uniforms restated exactly, Box-Muller in float64), EVERY element within philox_cases.Z_BAR: the four
      sizes; seven seeds up to 2^64 - 1 by value and through seed_dev written as the int64 a chain writes, and a flipped bit 40 of
      the key; a table of three timesteps under pos = [2, 0, 1]; the _frame kernels bitwise the plain ones (the wrapped grid too);
      edit mode 1 under a mask of 0, 1 and fractions at channels 1, 3 and 8 (the surviving elements hold the z of their own index);
      a seeded call on general rows against the float64 update fed the reference z.  tests/test_gpu_philox.py does the same for
      dm3d_randn, dm3d_ddpm_update and the Python layer.
  dm3d_x0_threshold / _scratch_bytes: ranks 0, N-2, N-1, past the end, negative; frac 0 and general; smax binding and not; a
      non-clipping row and an all-non-clipping call (scratch: cleared histograms, everything else untouched); frame; two calls on one
      scratch; a heavy tie at the large size.  The bound is bitwise np.sort's.
  dm3d_edit_update: channels 1, 2, 3, 6, 8; w with exact 0, exact 1 and fractions, runs of each; w == 0 everywhere with x0 and noise
      all-NaN; mode 0 with x and w NULL.
  dm3d_guide_update: mode 0 apart and in place, rescale NULL, partial slots (unused ones keep the sentinel), w = 0 / 1 rows with the
      unread operand all-NaN; mode 1 on those partials (phi == 0 rows untouched); mode 2 with and without t_idx.
  dm3d_pred_to_eps: out NULL, apart, == pred, == x; t_idx clamped.   dm3d_objective_loss_grad: dpred NULL and set, loss / loss_rows
      written over the sentinel, partial slots past the grid untouched.

Not covered, and why.  The factor f of the guidance rescale and the float64 loss sums are reductions whose order numpy does not share:
f is held to the float64 bar and to "the output is bitwise f' x eps_g for a float32 f' within one ulp of the reference f"; the loss to
1e-10.  A read outside a payload whose value is masked afterwards cannot be seen.  A NaN bound / more NaNs than ranks in the threshold
(tests/test_gpu_threshold.py), batch > 6, per_sample near 2^31, and refused arguments (DM3D_EINVAL: the host tests) are not repeated.
Of the Philox stream: the high word of the float4 index (more than 2^34 elements: tests/test_philox_host.py checks it in the reference
only) and the tail of the normal beyond what these counters reach (max |z| about 5.3).
A miscount in the threshold's wave-aggregated counting shows at the large tied volume only: at the small sizes two lanes of a wave
rarely share a digit under the selected prefix (docs/EXPERIMENTS.md, mutation (c)).

The worst error per entry is printed at the end of the module (docs/EXPERIMENTS.md records a run)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import philox_cases as pc
from guarded_buffers import IN, OUT, POISON_WORD, SENTINEL_WORD, Guarded
from oracle import ref_kernels as rk
from oracle import ref_philox as rp

pytestmark = pytest.mark.gpu

KERNEL_BAR = 2e-6        # tests/test_gpu_dpm.py's kernel bar, scaled by the coefficient mass of the row
EDIT_BAR = 2e-6          # tests/test_gpu_edit.py's
SIZES = [4, 1004, 2060, 263180]
BIG = 263180
EDIT_SIZES = {1: SIZES, 2: SIZES, 3: [24, 1008, 2064, 263184], 6: [24, 1008, 2064, 263184], 8: [24, 1008, 2064, 263184]}
THRESH_BIG = 2105356
LOSS_SIZES = [4, 1004, 2060, 131084]
POISON = np.array([POISON_WORD], np.uint32).view(np.float32)[0]
SENT = np.array([SENTINEL_WORD], np.uint32).view(np.float32)[0]
SENT_I32 = int(np.array([SENTINEL_WORD], np.uint32).view(np.int32)[0])
SENT_F64 = np.array([SENTINEL_WORD, SENTINEL_WORD], np.uint32).view(np.float64)[0]
WORST = {}


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    yield torch.device("cuda:0")
    for name in sorted(WORST):
        print(f"worst error {name}: {WORST[name]:.2e}")


@pytest.fixture()
def rng(request):
    return np.random.default_rng(sum(map(ord, request.node.name)))


def _lib_():
    from dm3d_amd import _lib
    return _lib


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype.itemsize == 4 else np.int64)


def _same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    diff = _bits(got) != _bits(want)
    assert not diff.any(), f"{name}: {int(diff.sum())} of {diff.size} elements differ bitwise, first at {np.argwhere(diff)[0].tolist()}"
    WORST.setdefault(f"{name} (bitwise)", 0.0)


def _close(name, got, ref, bar):
    """max |got - ref| per sample against the per-sample absolute bar(s)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), name
    err = np.abs(got - ref).reshape(len(got), -1).max(1)
    bar = np.broadcast_to(np.asarray(bar, np.float64), err.shape)
    worst = float((err / bar).max())
    WORST[f"{name} (float64, fraction of the bar)"] = max(WORST.get(f"{name} (float64, fraction of the bar)", 0.0), worst)
    print(f"{name}: max err {float(err.max()):.2e}, {worst:.2f} of the bar")
    assert (err < bar).all(), (name, err.tolist(), bar.tolist())


def _f32(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def _mag(rng, lo, hi, *shape):
    """Random values of magnitude in [lo, hi] and random sign."""
    return (rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def _gin(dev, arr):
    return Guarded(arr, dev, IN)


def _gout(dev, arr):
    return Guarded(arr, dev, OUT)


def _sentinels(*shape):
    return np.full(shape, SENT, np.float32)


def _seed_dev(seed_dev):
    """The 8 bytes behind seed_dev: an int as uint64, or the int64 array a chain would write (philox_cases.seed_words)."""
    return seed_dev if isinstance(seed_dev, np.ndarray) else np.array([seed_dev], np.uint64)


def _check_inputs(bufs):
    for b in bufs.values():
        if b.role == IN:
            b.unchanged()


# ======================================================================================================================================
# 1. The three update kernels
# ======================================================================================================================================
# rows of the hand-made tables.  DDIM: (a_x0, a_eps, sigma, clip); DPM / SDE: (c_x, c_0, c_1, clip, c_z).  None: a random value.
DDIM_ROWS = [(None, None, None, 1.0), (None, None, None, 0.0), (None, None, 0.0, 1.0), (None, None, 0.0, 0.0), (1.0, 0.0, 0.0, 1.0),
             (None, None, None, 2.5)]
DPM_ROWS = [(None, None, None, 1.0, None), (None, None, None, 0.0, None), (None, None, 0.0, 1.0, None), (None, None, None, 1.0, 0.0),
            (None, None, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 1.0, 0.0), (None, None, None, -3.0, None)]
KINDS = ["ddim", "dpm", "sde"]
NAMES = {"ddim": "ddim", "dpm": "dpm", "sde": "dpm_sde"}


def _coef(rng, kind, frame=False):
    """[rows][8]: random O(1) values where the entry reads, the poison word where the header says it does not."""
    spec = DDIM_ROWS if kind == "ddim" else DPM_ROWS
    t = np.full((len(spec), 8), POISON, np.float32)
    if not frame:
        t[:, 0], t[:, 1] = _mag(rng, 0.6, 1.0, len(spec)), _mag(rng, 0.7, 1.3, len(spec))
    for r, row in enumerate(spec):
        vals = [float(_mag(rng, 0.5, 1.5)) if v is None else v for v in row]
        t[r, 2:6] = vals[:4]
        if kind == "sde":
            t[r, 6] = vals[4]
    return t


def _frame(rng, rows, kind):
    f = _mag(rng, 0.9, 1.4, rows, 4)
    if kind != "ddim":
        f[:, 2:] = POISON                                                    # the solver needs no eps: columns 2 and 3 are not read
    return f


def _run_update(dev, kind, x, eps, coef, pos, *, mode=0, noise=None, hist=None, x0_out=True, frame=None, via_frame=False, bound=None,
                tau=None, t_next=None, t_idx=False, seed=0, seed_dev=None):
    """One guarded launch.  Returns res (out, or x in mode 1), x0 (x0_out, or hist in mode 1; None for ddim) and t_idx."""
    lib = _lib_()
    B, per = x.shape
    d = {"ddim": lib.DdimDesc, "dpm": lib.DpmDesc, "sde": lib.DpmSdeDesc}[kind]()
    bufs = dict(x=Guarded(x, dev, OUT if mode == 1 else IN), eps=_gin(dev, eps), coef=_gin(dev, coef), pos=_gin(dev, np.asarray(pos, np.int32)),
                out=_gout(dev, _sentinels(B, per)))
    d.x, d.eps, d.coef, d.pos, d.out = (bufs[k].ptr for k in ("x", "eps", "coef", "pos", "out"))
    d.rows, d.batch, d.per_sample, d.mode = len(coef), B, per, mode
    if kind != "ddim":
        if hist is not None:
            bufs["hist"] = Guarded(hist, dev, OUT if mode == 1 else IN)
            d.hist = bufs["hist"].ptr
        if x0_out:
            bufs["x0_out"] = _gout(dev, _sentinels(B, per))
            d.x0_out = bufs["x0_out"].ptr
    if kind != "dpm":
        bufs["tau"] = _gin(dev, np.asarray(tau, np.int32))
        d.tau, d.seed = bufs["tau"].ptr, seed
        if noise is not None:
            bufs["noise"] = _gin(dev, noise)
            d.noise = bufs["noise"].ptr
        if seed_dev is not None:
            bufs["seed_dev"] = _gin(dev, _seed_dev(seed_dev))
            d.seed_dev = bufs["seed_dev"].ptr
    if bound is not None:
        bufs["bound"] = _gin(dev, np.asarray(bound, np.float32))
        d.x0_bound = bufs["bound"].ptr
    if t_next is not None:
        bufs["t_next"] = _gin(dev, np.asarray(t_next, np.int32))
        d.t_next = bufs["t_next"].ptr
    if t_idx:
        bufs["t_idx"] = _gout(dev, np.full(B, SENT_I32, np.int32))
        d.t_idx = bufs["t_idx"].ptr
    name = {"ddim": "dm3d_ddim_update", "dpm": "dm3d_dpm_update", "sde": "dm3d_dpm_sde_update"}[kind]
    if frame is not None or via_frame:
        if frame is not None:
            bufs["frame"] = _gin(dev, frame)
        lib.check(getattr(lib.lib(), name + "_frame")(C.byref(d), bufs["frame"].ptr if frame is not None else None, None), name + "_frame")
    else:
        lib.check(getattr(lib.lib(), name)(C.byref(d), None), name)
    r = SimpleNamespace(res=None, x0=None, t_idx=None)
    out = bufs["out"].get()
    if mode == 1:
        assert (_bits(out) == SENT_I32).all(), "mode 1 wrote to out"
        if "x0_out" in bufs:
            assert (_bits(bufs["x0_out"].get()) == SENT_I32).all(), "mode 1 wrote to x0_out"
        r.res = bufs["x"].get()
        r.x0 = bufs["hist"].get() if "hist" in bufs else None
    else:
        r.res = out
        r.x0 = bufs["x0_out"].get() if "x0_out" in bufs else None
    if t_idx:
        r.t_idx = bufs["t_idx"].get()
    _check_inputs(bufs)
    return r


def _ref_update(kind, order, x, eps, coef, pos, noise=None, hist=None, frame=None, bound=None):
    if kind == "ddim":
        return rk.ddim_update(x, eps, coef, pos, noise, frame, bound, order), None
    if kind == "dpm":
        return rk.dpm_update(x, eps, coef, pos, hist, frame, bound, order)
    return rk.dpm_sde_update(x, eps, coef, pos, hist, noise, frame, bound, order)


def _bars(kind, coef, pos, frame, zmax):
    """Per sample: KERNEL_BAR x the row's coefficient mass for the result (tests/test_gpu_dpm.py, tests/test_gpu_dpm_sde.py: the noise
    coefficient counts with max |z|), and x the mass of the linear map that gives the x0 estimate."""
    r = np.clip(pos, 0, len(coef) - 1)
    c = np.abs(coef[r].astype(np.float64))
    if kind == "ddim":
        mass = c[:, 2] + c[:, 3] + c[:, 4] * zmax
    else:
        mass = c[:, 2] + c[:, 3] + c[:, 4] + (c[:, 6] * zmax if kind == "sde" else 0.0)
    if frame is None:
        mass0 = (1 + c[:, 1]) / c[:, 0]
    else:
        mass0 = np.abs(frame[r, :2].astype(np.float64)).sum(1)
    return KERNEL_BAR * np.maximum(1.0, mass), KERNEL_BAR * np.maximum(1.0, mass0)


def _clip_fraction_ok(x, eps, coef, pos, frame, bound):
    """On the reference side: the raw estimate leaves the bound on 20 % to 80 % of the elements of every clipping row."""
    raw, _ = rk.x0_estimate(x, eps, coef, pos, frame)
    r = np.clip(pos, 0, len(coef) - 1)
    for b in range(len(r)):
        if coef[r[b], 5] != 0:
            frac = float((np.abs(raw[b]) > (1.0 if bound is None else bound[b])).mean())
            assert 0.2 < frac < 0.8, (b, frac)


def _update_inputs(rng, kind, per):
    rows = len(DDIM_ROWS if kind == "ddim" else DPM_ROWS)
    if per == BIG:                                                           # batch 2: general rows and branch rows in two launches
        poses = [np.array([0, 2]), np.array([1, 3])]
    else:
        poses = [rng.permutation(rows)]
    B = len(poses[0])
    x, eps, hist, z = (_f32(rng, B, per) for _ in range(4))
    tau, t_next = rng.integers(0, 1000, rows).astype(np.int32), rng.integers(0, 1000, rows).astype(np.int32)
    return rows, poses, x, eps, hist, z, tau, t_next


@pytest.mark.parametrize("per", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_update_modes_frames_and_bounds(dev, rng, kind, per):
    """Modes 0 and 1, with and without a frame table and a dynamic bound, every sample on a row of its own: bitwise the float32
    restatement, within the bars of the float64 one; mode 1 is mode 0's result in place and t_idx receives t_next[row]."""
    rows, poses, x, eps, hist, z, tau, t_next = _update_inputs(rng, kind, per)
    B = x.shape[0]
    zmax = float(np.abs(z).max())
    for pos in poses:
        for with_frame in (False, True):
            coef = _coef(rng, kind, with_frame)
            frame = _frame(rng, rows, kind) if with_frame else None
            for bound in (None, rng.uniform(1.05, 1.3, B).astype(np.float32)):
                if per >= 1004:
                    _clip_fraction_ok(x, eps, coef, pos, frame, bound)
                kw = dict(noise=z, hist=hist, frame=frame, bound=bound)
                want, want0 = _ref_update(kind, "f32", x, eps, coef, pos, **kw)
                ref, ref0 = _ref_update(kind, "f64", x, eps, coef, pos, **kw)
                assert float(np.abs(ref).max()) < 40                         # O(1) values: the bars are absolute
                got = _run_update(dev, kind, x, eps, coef, pos, mode=0, tau=tau, **kw)
                tag = f"dm3d_{NAMES[kind]}_update" + ("_frame" if with_frame else "")
                _same(tag, got.res, want)
                bar, bar0 = _bars(kind, coef, pos, frame, zmax)
                _close(tag, got.res, ref, bar)
                if kind != "ddim":
                    _same(tag + " x0", got.x0, want0)
                    _close(tag + " x0", got.x0, ref0, bar0)
                step = _run_update(dev, kind, x, eps, coef, pos, mode=1, tau=tau, t_next=t_next, t_idx=True, **kw)
                _same(tag + " mode 1", step.res, want)
                if kind != "ddim":
                    _same(tag + " mode 1 hist", step.x0, want0)
                assert step.t_idx.tolist() == t_next[pos].tolist()


@pytest.mark.parametrize("kind", KINDS)
def test_update_optional_pointers_and_unread_operands(dev, rng, kind):
    per = 1004
    rows, (pos,), x, eps, hist, z, tau, t_next = _update_inputs(rng, kind, per)
    B = x.shape[0]
    coef = _coef(rng, kind)
    kw = dict(noise=z, hist=hist, tau=tau)
    base = _run_update(dev, kind, x, eps, coef, pos, **kw)
    tag = f"dm3d_{NAMES[kind]}_update"
    # *_frame(d, NULL) is the plain entry
    _same(tag + " frame NULL", _run_update(dev, kind, x, eps, coef, pos, via_frame=True, **kw).res, base.res)
    # x0_bound: all ones is the static clamp, bitwise
    ones = _run_update(dev, kind, x, eps, coef, pos, bound=np.ones(B, np.float32), **kw)
    _same(tag + " bound 1", ones.res, base.res)
    # pos outside [0, rows) is clamped before any table is indexed (the tables' neighbours are poison); t_idx with it
    p_out, p_in = np.array([-5, 0, rows - 1, rows + 3]), np.array([0, 0, rows - 1, rows - 1])
    a = _run_update(dev, kind, x[:4], eps[:4], coef, p_out, mode=1, noise=z[:4], hist=hist[:4], tau=tau, t_next=t_next, t_idx=True)
    b = _run_update(dev, kind, x[:4], eps[:4], coef, p_in, mode=1, noise=z[:4], hist=hist[:4], tau=tau, t_next=t_next, t_idx=True)
    _same(tag + " clamped pos", a.res, b.res)
    _same(tag + " clamped pos", a.res, _ref_update(kind, "f32", x[:4], eps[:4], coef, p_in, z[:4], hist[:4])[0])
    assert a.t_idx.tolist() == b.t_idx.tolist() == t_next[p_in].tolist()
    nan = np.full((B, per), np.nan, np.float32)
    if kind != "ddim":
        _same(tag + " x0", ones.x0, base.x0)
        _same(tag + " clamped pos hist", a.x0, b.x0)
        # x0_out NULL
        _same(tag + " x0_out NULL", _run_update(dev, kind, x, eps, coef, pos, x0_out=False, **kw).res, base.res)
        # hist NULL: every row is first order, bitwise the table with c_1 = 0
        first = coef.copy()
        first[:, 4] = 0
        assert (coef[pos, 4] != 0).sum() >= 3
        no_hist = _run_update(dev, kind, x, eps, coef, pos, noise=z, tau=tau)
        _same(tag + " hist NULL", no_hist.res, _run_update(dev, kind, x, eps, first, pos, **kw).res)
        _same(tag + " hist NULL", no_hist.res, _ref_update(kind, "f32", x, eps, coef, pos, z, None)[0])
        # an all-NaN history on first-order rows is not read
        p1 = np.array([r for r in range(rows) if coef[r, 4] == 0] * 2)[:3]
        got = _run_update(dev, kind, x[:3], eps[:3], coef, p1, noise=z[:3], hist=nan[:3], tau=tau)
        _same(tag + " NaN hist unread", got.res, _ref_update(kind, "f32", x[:3], eps[:3], coef, p1, z[:3], hist[:3])[0])
    if kind != "dpm":
        # all-NaN noise on rows without a noise term is not read
        col = 4 if kind == "ddim" else 6
        p0 = np.array([r for r in range(rows) if coef[r, col] == 0] * 2)[:3]
        got = _run_update(dev, kind, x[:3], eps[:3], coef, p0, noise=nan[:3], hist=hist[:3], tau=tau)
        assert np.isfinite(got.res).all()
        _same(tag + " NaN noise unread", got.res, _ref_update(kind, "f32", x[:3], eps[:3], coef, p0, z[:3], hist[:3])[0])
    if kind == "sde":
        # c_z = 0 everywhere: dm3d_dpm_update on the same buffers, bitwise (its table has the poison in column 6)
        ode, dpm = coef.copy(), coef.copy()
        ode[:, 6], dpm[:, 6] = 0, POISON
        for mode in (0, 1):
            s = _run_update(dev, "sde", x, eps, ode, pos, mode=mode, noise=nan, hist=hist, tau=tau)
            o = _run_update(dev, "dpm", x, eps, dpm, pos, mode=mode, hist=hist)
            _same("dm3d_dpm_sde_update c_z 0 is dm3d_dpm_update", s.res, o.res)
            _same("dm3d_dpm_sde_update c_z 0 is dm3d_dpm_update", s.x0, o.x0)


@pytest.mark.parametrize("kind", KINDS)
def test_update_on_the_hosts_own_tables(dev, rng, kind):
    """The rows DiffusionModel writes for a 5-step schedule of T = 1000 (eta = 0.7 where there is one), eps frame and v frame."""
    import dm3d_amd
    from dm3d_amd import schedules
    from dm3d_amd.diffusion import DiffusionModel
    T, per = 1000, 1004
    ab = dm3d_amd.Betas(T).alpha_bar
    host = SimpleNamespace(b=SimpleNamespace(alpha_bar=ab))
    src = schedules.ddim_timesteps(T, 5)[::-1].copy()
    dst, prev = np.append(src[1:], -1), np.append(-1, src[:-1])
    if kind == "ddim":
        coef = DiffusionModel._ddim_table(host, src, dst, 0.7, True).numpy()
    elif kind == "dpm":
        coef = DiffusionModel._dpm_table(host, src, dst, prev, 2, True).numpy()
    else:
        coef = DiffusionModel._dpm_sde_table(host, src, dst, prev, 2, True, 0.7).numpy()
    assert coef.shape == (5, 8) and coef.dtype == np.float32
    noisy = 4 if kind == "ddim" else 6
    assert (coef[:4, noisy] != 0).all() == (kind != "dpm") and coef[4, noisy] == 0 and (coef[:, 5] == 1).all()
    if kind != "ddim":
        assert coef[0, 4] == 0 and (coef[1:4, 4] != 0).all() and coef[4].tolist()[2:5] == [0.0, 1.0, 0.0]
    frame_v = schedules.frame_table(ab, "v")[src]
    x, eps, hist, z = (_f32(rng, 5, per) for _ in range(4))
    pos = np.arange(5)
    zmax = float(np.abs(z).max())
    for frame in (None, frame_v):
        kw = dict(noise=z, hist=hist, frame=frame)
        got = _run_update(dev, kind, x, eps, coef, pos, tau=src.astype(np.int32), **kw)
        want, want0 = _ref_update(kind, "f32", x, eps, coef, pos, **kw)
        ref, ref0 = _ref_update(kind, "f64", x, eps, coef, pos, **kw)
        tag = f"dm3d_{NAMES[kind]}_update host tables"
        _same(tag, got.res, want)
        bar, _ = _bars(kind, coef, pos, frame, zmax)
        _close(tag, got.res, ref, bar)
        if kind != "ddim":
            _same(tag + " x0", got.x0, want0)
            _close(tag + " x0", got.x0, ref0, _bars(kind, coef, pos, frame, zmax)[1])


# ======================================================================================================================================
# 2. dm3d_edit_update
# ======================================================================================================================================
def _levels(rng, rows=4):
    """(sqrt(a'), sqrt(1-a'), level timestep, -): magnitudes in [0.3, 0.9]; row 1 is clean."""
    t = np.full((rows, 4), POISON, np.float32)
    t[:, 0], t[:, 1], t[:, 2] = _mag(rng, 0.3, 0.9, rows), _mag(rng, 0.3, 0.9, rows), rng.integers(0, 1000, rows)
    t[1, :3] = (0.8, 0.0, -1)
    return t


def _run_edit(dev, x0, levels, pos, *, mode=0, noise=None, x=None, w=None, channels=1, seed=0, seed_dev=None):
    lib = _lib_()
    B, per = x0.shape
    d = lib.EditDesc()
    bufs = dict(x0=_gin(dev, x0), levels=_gin(dev, levels), pos=_gin(dev, np.asarray(pos, np.int32)), out=_gout(dev, _sentinels(B, per)))
    d.x0, d.levels, d.pos, d.out = (bufs[k].ptr for k in ("x0", "levels", "pos", "out"))
    d.rows, d.batch, d.per_sample, d.channels, d.mode, d.seed = len(levels), B, per, channels, mode, seed
    if noise is not None:
        bufs["noise"] = _gin(dev, noise)
        d.noise = bufs["noise"].ptr
    if seed_dev is not None:
        bufs["seed_dev"] = _gin(dev, _seed_dev(seed_dev))
        d.seed_dev = bufs["seed_dev"].ptr
    if mode == 1:
        bufs["x"], bufs["w"] = _gout(dev, x), _gin(dev, w)
        d.x, d.w = bufs["x"].ptr, bufs["w"].ptr
    lib.check(lib.lib().dm3d_edit_update(C.byref(d), None), "dm3d_edit_update")
    out = bufs["out"].get()
    if mode == 1:
        assert (_bits(out) == SENT_I32).all(), "mode 1 wrote to out"
        out = bufs["x"].get()
    _check_inputs(bufs)
    return out


def _weights(rng, B, vox):
    """Keep weights with exact 0, exact 1 and fractions: a run of zeros, a run of ones (whole lanes skip / copy), then a mix."""
    w = rng.choice(np.array([0.0, 1.0, 0.25, 0.7, 0.999], np.float32), (B, vox))
    w[:, :vox // 4], w[:, vox // 4:vox // 2] = 0.0, 1.0
    return w


@pytest.mark.parametrize("size", range(4))
@pytest.mark.parametrize("channels", [1, 2, 3, 6, 8])
def test_edit_update(dev, rng, channels, size):
    """Inputs are clipped to |v| <= 3 and the level coefficients are below 0.9, so |known_t| <= 5.4: its three roundings stay below
    2 x 2^-24 x 2.7 + 2^-24 x 5.4, the blend's four add at most as much again: 1.2e-6 in all, inside the 2e-6 bar."""
    per = EDIT_SIZES[channels][size]
    B = 2 if per > 4096 else 4
    levels = _levels(rng)
    pos = np.array([0, 2]) if B == 2 else np.array([3, 1, 0, 2])
    x0, z, x = (np.clip(_f32(rng, B, per), -3, 3) for _ in range(3))
    w = _weights(rng, B, per // channels)
    tag = "dm3d_edit_update"
    got = _run_edit(dev, x0, levels, pos, mode=0, noise=z, channels=channels)        # x and w NULL
    _same(tag + " mode 0", got, rk.edit_update(x0, levels, pos, z))
    _close(tag + " mode 0", got, rk.edit_update(x0, levels, pos, z, order="f64"), EDIT_BAR)
    got = _run_edit(dev, x0, levels, pos, mode=1, noise=z, x=x, w=w, channels=channels)
    _same(tag + " mode 1", got, rk.edit_update(x0, levels, pos, z, 1, x, w, channels))
    _close(tag + " mode 1", got, rk.edit_update(x0, levels, pos, z, 1, x, w, channels, order="f64"), EDIT_BAR)
    # w == 0 everywhere: x bitwise untouched, x0 and noise (all-NaN) not read
    nan = np.full((B, per), np.nan, np.float32)
    got = _run_edit(dev, nan, levels, pos, mode=1, noise=nan, x=x, w=np.zeros_like(w), channels=channels)
    _same(tag + " w 0", got, x)
    if B == 4:                                                               # the clean row writes x0 bitwise and reads no noise
        got = _run_edit(dev, x0, levels, [1, 1, 1, 1], mode=0, noise=nan, channels=channels)
        _same(tag + " clean", got, x0)


# ======================================================================================================================================
# 3. The in-kernel Philox of ddim, dpm_sde and edit
# ======================================================================================================================================
P_SMALL, P_FLAT = 65796, 4 * 65796                                           # (4, P) does not wrap the 256-block grid, (1, 4P) does
TAU, SEED = 517, 987654321


def _draw(dev, kind, shape, seed=SEED, tau=TAU, seed_dev=None, pos=None, frame=None):
    """The draw itself through a unit row: a_x0 = a_eps = 0, sigma = 1 / c_x = c_0 = c_1 = 0, c_z = 1 / sqrt(a') = 0, sqrt(1-a') = 1.
    `tau`: one timestep (a table of one row) or one per row of the table, every row a unit row; `pos` (default all 0) picks each
    sample's row; `frame`: a frame table, through the _frame kernels (x = p = 0, so the estimate is 0 whatever the row holds)."""
    B, per = shape
    zero = np.zeros(shape, np.float32)
    taus = np.atleast_1d(np.asarray(tau, np.int64))
    pos = [0] * B if pos is None else pos
    if kind == "edit":
        levels = np.array([[0, 1, t, POISON] for t in taus], np.float32)
        return _run_edit(dev, zero, levels, pos, seed=seed, seed_dev=seed_dev)
    coef = np.full((len(taus), 8), POISON, np.float32)
    coef[:, :6] = (1, 1, 0, 0, 1, 0) if kind == "ddim" else (1, 1, 0, 0, 0, 0)
    if kind == "sde":
        coef[:, 6] = 1
    if frame is not None:
        coef[:, :2] = POISON
    return _run_update(dev, kind, zero, zero, coef, pos, tau=taus.astype(np.int32), seed=seed, seed_dev=seed_dev, x0_out=False, frame=frame).res


@pytest.mark.parametrize("kind", ["ddim", "sde", "edit"])
def test_philox_draws(dev, rng, kind):
    z = _draw(dev, kind, (4, P_SMALL))
    assert np.isfinite(z).all()
    # the counter is the flat float4 index: one tau for all samples makes (4, P) read flat the draws of (1, 4P)
    _same(f"philox {kind} flat counter", _draw(dev, kind, (1, P_FLAT)).reshape(4, P_SMALL), z)
    mean, std = float(z.astype(np.float64).mean()), float(z.astype(np.float64).std())
    print(f"philox {kind}: mean {mean:+.2e}, std {std:.5f}")
    assert abs(mean) < 1e-2 and abs(std - 1) < 1e-2                           # tests/test_gpu_ddim.py's bars
    # seed_dev holding s is seed = s; another seed, another tau and the other kernels draw something else
    _same(f"philox {kind} seed_dev", _draw(dev, kind, (4, P_SMALL), seed=5, seed_dev=SEED), z)
    for other in (_draw(dev, kind, (4, P_SMALL), seed=SEED + 1), _draw(dev, kind, (4, P_SMALL), tau=TAU + 1)):
        assert float((z.astype(np.float64) - other).std()) > 1.0              # independent: var(a - b) = 2
    for k2 in {"ddim", "sde", "edit"} - {kind}:
        assert float((z[:1, :1004].astype(np.float64) - _draw(dev, k2, (1, 1004))).std()) > 1.0
    # the draw injected as `noise` into a general row gives the drawn result bitwise
    B, per = 4, 1004
    zs = _draw(dev, kind, (B, per))
    _same(f"philox {kind} prefix", zs.reshape(-1)[:per], z.reshape(-1)[:per])
    x, eps, hist = (_f32(rng, B, per) for _ in range(3))
    if kind == "edit":
        levels = _levels(rng)
        levels[:, 2] = TAU
        pos = [0, 2, 3, 0]
        a = _run_edit(dev, x, levels, pos, seed=SEED)
        b = _run_edit(dev, x, levels, pos, noise=zs)
    else:
        coef = _coef(rng, kind)
        pos = [0, 1, 0, 1]
        tau = np.full(len(coef), TAU, np.int32)
        a = _run_update(dev, kind, x, eps, coef, pos, hist=hist, tau=tau, seed=SEED).res
        b = _run_update(dev, kind, x, eps, coef, pos, hist=hist, tau=tau, noise=zs).res
    _same(f"philox {kind} drawn is injected", a, b)


# ---- the stream against its host reference (oracle/ref_philox.py): every element, at philox_cases.Z_BAR ------------------------------
PHILOX_KINDS = ["ddim", "sde", "edit"]
REF_Z = {"ddim": rp.ddim, "sde": rp.dpm_sde, "edit": rp.edit}
TAU_TABLE, TAU_POS = [3, 517, 999], [2, 0, 1]                               # pos is no identity and no row index is a timestep


def _z_close(name, got, ref, bar=pc.Z_BAR):
    pc.z_close(WORST, name, got, ref, bar)


@pytest.mark.parametrize("per", SIZES)
@pytest.mark.parametrize("kind", PHILOX_KINDS)
def test_philox_reference_sizes(dev, kind, per):
    """One float4, a partial block, two blocks, the wrapped grid (batch 2: the second sample's counters start at per / 4)."""
    B = 2 if per == BIG else 3
    z = _draw(dev, kind, (B, per), seed=pc.SEED64)
    _z_close(kind, z, REF_Z[kind](B, per, TAU, pc.SEED64))


@pytest.mark.parametrize("seed", pc.SEEDS, ids=hex)
@pytest.mark.parametrize("kind", PHILOX_KINDS)
def test_philox_reference_seeds(dev, kind, seed):
    """Both key words, by value and through seed_dev written as the int64 a chain writes (negative from 2^63 up)."""
    shape = (2, 1004)
    ref = REF_Z[kind](*shape, TAU, seed)
    z = _draw(dev, kind, shape, seed=seed)
    _z_close(kind, z, ref)
    _same(f"philox {kind} seed_dev int64", _draw(dev, kind, shape, seed=5, seed_dev=pc.seed_words(seed)), z)
    assert pc.independent(z, _draw(dev, kind, shape, seed=seed ^ (1 << 40)))  # a bit of the key's high word


@pytest.mark.parametrize("kind", PHILOX_KINDS)
def test_philox_reference_tau_of_the_row(dev, rng, kind):
    """Three rows with three timesteps and pos = [2, 0, 1]: word 2 is tau[pos[b]] (the level of row pos[b]), not tau[b], not the row
    index; the _frame kernels draw the same z bitwise."""
    shape = (3, 1004)
    want_tau = [TAU_TABLE[p] for p in TAU_POS]
    ref = REF_Z[kind](*shape, want_tau, pc.SEED64)
    assert pc.independent(ref, REF_Z[kind](*shape, TAU_TABLE, pc.SEED64)) and pc.independent(ref, REF_Z[kind](*shape, TAU_POS, pc.SEED64))
    z = _draw(dev, kind, shape, seed=pc.SEED64, tau=TAU_TABLE, pos=TAU_POS)
    _z_close(f"{kind} tau table", z, ref)
    if kind != "edit":
        for per in (1004, BIG):
            B = 2 if per == BIG else 3
            plain = z if per == 1004 else _draw(dev, kind, (B, per), seed=pc.SEED64, tau=TAU_TABLE, pos=TAU_POS[:B])
            framed = _draw(dev, kind, (B, per), seed=pc.SEED64, tau=TAU_TABLE, pos=TAU_POS[:B], frame=_frame(rng, 3, kind))
            _same(f"philox {kind} frame kernel", framed, plain)


@pytest.mark.parametrize("channels", [1, 3, 8])
def test_philox_reference_edit_mask(dev, rng, channels):
    """Mode 1 on the unit level (known_t = z): an element with w = 1 holds the reference z of ITS OWN index — the skipped ones around
    it shifted no counter, and the 3-channel path (a lane's four elements on two voxels) indexes as the others do; w = 0 keeps x
    bitwise.  Where 0 < w < 1 the element is fl(fl(w z) + fl((1-w) x)) with 1-w exact (w >= 0.25), three roundings of at most
    2^-24 (|w z| + |(1-w) x|) each way, so z recovered as (out - (1-w) x) / w carries at most 2^-23 (|z| + (1-w) |x| / w) more than the
    bar: added per element."""
    per = EDIT_SIZES[channels][2]
    B = 3
    x = np.clip(_f32(rng, B, per), -3, 3)
    w = _weights(rng, B, per // channels)
    levels = np.array([[0, 1, t, POISON] for t in TAU_TABLE], np.float32)
    got = _run_edit(dev, np.zeros((B, per), np.float32), levels, TAU_POS, mode=1, x=x, w=w, channels=channels, seed=pc.SEED64)
    ref = rp.edit(B, per, [TAU_TABLE[p] for p in TAU_POS], pc.SEED64)
    we = np.repeat(w, channels, axis=1)
    assert (we == 0).sum() > per // 4 and (we == 1).sum() > per // 4 and ((we > 0) & (we < 1)).sum() > per // 4
    assert np.array_equal(_bits(got)[we == 0], _bits(x)[we == 0]), "an element with w = 0 was written"
    _z_close(f"edit mode 1 w = 1, channels {channels}", got[we == 1], ref[we == 1])
    mid = (we > 0) & (we < 1)
    w64, x64 = we[mid].astype(np.float64), x[mid].astype(np.float64)
    one_m_w = (np.float32(1) - we[mid]).astype(np.float64)
    z_mid = (got[mid].astype(np.float64) - one_m_w * x64) / w64
    bar = pc.Z_BAR + 2.0 ** -23 * (np.abs(ref[mid]) + one_m_w * np.abs(x64) / w64)
    _z_close(f"edit mode 1 0 < w < 1 (recovered), channels {channels}", z_mid, ref[mid], bar)


@pytest.mark.parametrize("kind", PHILOX_KINDS)
def test_philox_reference_general_row(dev, rng, kind):
    """A seeded call on general rows against the float64 update fed the REFERENCE z: host arithmetic end to end, nothing of the device's
    own draw injected.  The bar is the entry's own plus |coefficient of z| x the z bar."""
    B, per = 4, 1004
    x, eps, hist = (_f32(rng, B, per) for _ in range(3))
    if kind == "edit":
        levels = _levels(rng)
        levels[:, 2] = [3, -1, 517, 999]
        pos = np.array([3, 1, 0, 2])
        z = rp.edit(B, per, levels[pos, 2].astype(np.int64), pc.SEED64)
        got = _run_edit(dev, x, levels, pos, seed=pc.SEED64)
        ref = rk.edit_update(x, levels, pos, z, order="f64")
        bar = EDIT_BAR + np.abs(levels[pos, 1].astype(np.float64)) * pc.Z_BAR
    else:
        coef = _coef(rng, kind)
        col = 4 if kind == "ddim" else 6
        noisy = [r for r in range(len(coef)) if coef[r, col] != 0]           # rows with a noise term
        pos = np.array(noisy[::-1] + noisy)[:B]
        assert len(noisy) >= 3
        tau = (np.arange(len(coef)) * 37 + 11).astype(np.int32)
        z = REF_Z[kind](B, per, tau[pos], pc.SEED64)
        got = _run_update(dev, kind, x, eps, coef, pos, hist=hist, tau=tau, seed=pc.SEED64).res
        ref, _ = _ref_update(kind, "f64", x, eps, coef, pos, noise=z, hist=hist)
        bar = _bars(kind, coef, pos, None, float(np.abs(z).max()))[0] + np.abs(coef[pos, col].astype(np.float64)) * pc.Z_BAR
    _close(f"dm3d_{NAMES.get(kind, 'edit')}_update seeded, reference z", got, ref, bar)


# ======================================================================================================================================
# 4. dm3d_x0_threshold
# ======================================================================================================================================
HIST_WORDS = 4096 + 2 * 1024 + 2 * 512


def _thresh_bufs(dev, x, eps):
    lib = _lib_()
    B, per = x.shape
    nbytes = lib.lib().dm3d_x0_threshold_scratch_bytes(B, per)
    assert nbytes >= 4 * B * (per + HIST_WORDS) and nbytes % 16 == 0
    assert lib.lib().dm3d_x0_threshold_scratch_bytes(0, per) == 0 and lib.lib().dm3d_x0_threshold_scratch_bytes(B, 0) == 0
    return dict(x=_gin(dev, x), eps=_gin(dev, eps), scratch=_gout(dev, np.full(nbytes // 4, SENT_I32, np.int32)))


def _run_thresh(dev, shared, coef, pos, rank, frac, smax, frame=None):
    """One guarded launch on the shared x / eps / scratch buffers; returns the bounds."""
    lib = _lib_()
    B, per = shared["x"].shape
    bufs = dict(coef=_gin(dev, coef), pos=_gin(dev, np.asarray(pos, np.int32)), rank=_gin(dev, np.asarray(rank, np.int32)),
                frac=_gin(dev, np.asarray(frac, np.float32)), smax=_gin(dev, np.asarray(smax, np.float32)), bound=_gout(dev, _sentinels(B)))
    d = lib.ThreshDesc()
    d.x, d.eps, d.scratch = shared["x"].ptr, shared["eps"].ptr, shared["scratch"].ptr
    d.coef, d.pos, d.rank, d.frac, d.smax, d.bound = (bufs[k].ptr for k in ("coef", "pos", "rank", "frac", "smax", "bound"))
    d.rows, d.batch, d.per_sample = len(coef), B, per
    if frame is not None:
        bufs["frame"] = _gin(dev, frame)
        d.frame = bufs["frame"].ptr
    lib.check(lib.lib().dm3d_x0_threshold(C.byref(d), None), "dm3d_x0_threshold")
    out = bufs["bound"].get()
    shared["scratch"].get()                                                  # the pads around the scratch are intact
    _check_inputs(bufs)
    return out


def _thresh_coef(rng, rows, frame=False):
    """Only columns 0, 1 and 5 are read (5 with a frame); row 0 does not clip."""
    t = np.full((rows, 8), POISON, np.float32)
    if not frame:
        t[:, 0], t[:, 1] = _mag(rng, 0.6, 1.0, rows), _mag(rng, 0.7, 1.3, rows)
    t[:, 5] = rng.choice([1.0, -2.0, 0.5], rows)
    t[0, 5] = 0.0
    return t


def _ranks(n):
    return [0, n - 2, n - 1, n + 5, -3]


@pytest.mark.parametrize("per", SIZES)
def test_x0_threshold(dev, rng, per):
    """Batch 6: the five ranks (past the end and negative ones clamped) and a non-clipping row, frac general and 0, smax binding (the
    top ranks) and not, without and with a frame table, twice on one scratch."""
    B, rows = 6, 7
    x, eps = _f32(rng, B, per) * 2, _f32(rng, B, per)
    shared = _thresh_bufs(dev, x, eps)
    rank = _ranks(per) + [per // 2]
    pos = np.array([3, 1, 6, 2, 5, 0])                                       # sample 5 sits on the row that does not clip
    for with_frame in (False, True):
        coef = _thresh_coef(rng, rows, with_frame)
        frame = _frame(rng, rows, "dpm") if with_frame else None
        for frac, smax in ((rng.uniform(0.05, 0.95, B), np.full(B, 1e9)), (np.zeros(B), np.full(B, 1e9)),
                           (rng.uniform(0.05, 0.95, B), rng.uniform(1.5, 2.5, B))):
            want = rk.x0_bound(x, eps, coef, pos, rank, frac, smax, frame)
            got = _run_thresh(dev, shared, coef, pos, rank, frac, smax, frame)
            _same("dm3d_x0_threshold", got, want)
            _same("dm3d_x0_threshold repeat", _run_thresh(dev, shared, coef, pos, rank, frac, smax, frame), want)
            assert got[5] == 1.0                                             # the row that does not clip
            if per >= 1004:                                                  # the smallest magnitude is below 1, the largest above 2.5
                assert got[0] == 1.0 and got[4] == 1.0 and (got[1:4] > 1.0).all() and ((got[1:4] == np.asarray(smax, np.float32)[1:4]).all() == (smax[0] < 1e8))
    shared["x"].unchanged(), shared["eps"].unchanged()
    # no row clips: every bound is 1 and the scratch holds nothing but the cleared histograms
    fresh = _thresh_bufs(dev, x, eps)
    coef = _thresh_coef(rng, rows)
    coef[:, 5] = 0.0
    got = _run_thresh(dev, fresh, coef, pos, rank, np.zeros(B), np.full(B, 1e9))
    _same("dm3d_x0_threshold no clip", got, np.ones(B, np.float32))
    words = fresh["scratch"].get()
    assert int((words == 0).sum()) == B * HIST_WORDS and int((words == SENT_I32).sum()) == words.size - B * HIST_WORDS


def test_x0_threshold_wrapped_grid(dev, rng):
    """per_sample = 4 (256 x 2048 + 2048 + 3), batch 1: block 0 takes a second trip and the last wave of it is partial.  Plain data at
    the five ranks, then a heavy tie: every other float4 holds one value, so a wave's counting sees its aggregated path (the lanes that
    share the leader's digit) and its single-lane path together, on the wrapped trip too."""
    per = THRESH_BIG
    x, eps = _f32(rng, 1, per) * 2, _f32(rng, 1, per)
    coef = _thresh_coef(rng, 2)
    shared = _thresh_bufs(dev, x, eps)
    raw, _ = rk.x0_estimate(x, eps, coef, [1])
    v = np.sort(np.abs(raw[0]))
    f = np.float32(0.37)

    def want(i, smax=np.float32(1e9)):
        i = min(max(i, 0), per - 1)
        s = v[i] + f * (v[min(i + 1, per - 1)] - v[i])
        return np.array([min(max(s, np.float32(1)), smax)], np.float32)

    for i in _ranks(per) + [per // 2, int(0.9 * per)]:
        _same("dm3d_x0_threshold wrapped grid", _run_thresh(dev, shared, coef, [1], [i], [f], [1e9]), want(i))
    _same("dm3d_x0_threshold wrapped grid", _run_thresh(dev, shared, coef, [1], [per - 1], [f], [2.25]), want(per - 1, np.float32(2.25)))
    shared["x"].unchanged(), shared["eps"].unchanged()
    # the tie: x = 1.75 sqrt(a), eps = 0 on every other float4 (x0 = 1.75 after one exact-or-not division: whatever it is, it repeats)
    x4, e4 = x.reshape(-1, 4).copy(), eps.reshape(-1, 4).copy()
    x4[::2], e4[::2] = np.float32(1.75) * coef[1, 0], 0.0
    x, eps = x4.reshape(1, per), e4.reshape(1, per)
    shared = _thresh_bufs(dev, x, eps)
    raw, _ = rk.x0_estimate(x, eps, coef, [1])
    v = np.sort(np.abs(raw[0]))
    tie = np.abs(raw[0, 0])
    lo, hi = int(np.searchsorted(v, tie, "left")), int(np.searchsorted(v, tie, "right"))
    assert hi - lo >= per // 2 and tie > 1
    for i in (lo - 1, lo, (lo + hi) // 2, hi - 1, hi, per - 1):
        _same("dm3d_x0_threshold heavy tie", _run_thresh(dev, shared, coef, [1], [i], [f], [1e9]), want(i))
    shared["x"].unchanged(), shared["eps"].unchanged()


# ======================================================================================================================================
# 5. dm3d_guide_update
# ======================================================================================================================================
PARTS = 256


def _run_guide(dev, mode, *, ep=None, en=None, out=None, scale=None, rescale=None, partials=None, in_place=False, x=None, t_idx=None):
    """One guarded launch.  mode 0: returns (out, partials); mode 1: `out` and `partials` are what mode 0 left; mode 2: (x, t_idx)."""
    lib = _lib_()
    d = lib.GuideDesc()
    d.mode = mode
    bufs = {}
    if mode == 2:
        B2, per = x.shape
        bufs["x"] = _gout(dev, x)
        d.x, d.batch, d.per_sample = bufs["x"].ptr, B2 // 2, per
        if t_idx is not None:
            bufs["t_idx"] = _gout(dev, np.asarray(t_idx, np.int32))
            d.t_idx = bufs["t_idx"].ptr
    else:
        B, per = (ep if mode == 0 else out).shape
        d.batch, d.per_sample = B, per
        if rescale is not None:
            bufs["rescale"] = _gin(dev, np.asarray(rescale, np.float32))
            d.rescale = bufs["rescale"].ptr
        if mode == 0:
            bufs["ep"] = _gout(dev, ep) if in_place else _gin(dev, ep)
            bufs["en"], bufs["scale"] = _gin(dev, en), _gin(dev, np.asarray(scale, np.float32))
            bufs["out"] = bufs["ep"] if in_place else _gout(dev, _sentinels(B, per))
            d.eps_pos, d.eps_neg, d.scale = bufs["ep"].ptr, bufs["en"].ptr, bufs["scale"].ptr
            if partials:
                bufs["partials"] = _gout(dev, np.full((B, PARTS, 4), SENT_F64, np.float64))
                d.partials = bufs["partials"].ptr
        else:
            bufs["out"], bufs["partials"] = _gout(dev, out), _gin(dev, partials)
            d.partials = bufs["partials"].ptr
        d.out = bufs["out"].ptr
    lib.check(lib.lib().dm3d_guide_update(C.byref(d), None), "dm3d_guide_update")
    if mode == 2:
        res = (bufs["x"].get(), bufs["t_idx"].get() if t_idx is not None else None)
    else:
        res = (bufs["out"].get(), bufs["partials"].get() if mode == 0 and partials else None)
    _check_inputs(bufs)
    return res


@pytest.mark.parametrize("per", SIZES)
def test_guide_combine_and_rescale(dev, rng, per):
    big = per == BIG
    w = np.array([2.5, 1.0] if big else [2.5, 0.0, 1.0, -0.7, 1.0], np.float32)
    phi = np.array([0.7, 0.4] if big else [0.7, 0.3, 0.0, 1.0, 0.5], np.float32)
    B = len(w)
    ep, en = _f32(rng, B, per) + np.float32(0.5), _f32(rng, B, per)
    g32, f32_, out32 = rk.guide_update(ep, en, w, phi)
    g64, f64_, out64 = rk.guide_update(ep, en, w, phi, order="f64")
    M = (np.abs(en.astype(np.float64)) + np.abs(w.astype(np.float64))[:, None] * np.abs(ep.astype(np.float64) - en)).max(1)
    # mode 0, rescale NULL; the operand a w = 0 / w = 1 row does not read is all-NaN
    ep_nan, en_nan = ep.copy(), en.copy()
    ep_nan[w == 0], en_nan[w == 1] = np.nan, np.nan
    got, _ = _run_guide(dev, 0, ep=ep_nan, en=en_nan, scale=w)
    _same("dm3d_guide_update combine", got, g32)
    _close("dm3d_guide_update combine", got, g64, 2.0 ** -22 * M)            # tests/test_gpu_guidance.py's bar
    # mode 0 with partials: the same eps_g, and one slot of float64 sums per block of the rows with phi != 0
    got, parts = _run_guide(dev, 0, ep=ep, en=en, scale=w, rescale=phi, partials=True)
    _same("dm3d_guide_update combine", got, g32)
    nblocks = min(-(-(per // 4) // 256), PARTS)
    for b in range(B):
        used = nblocks if phi[b] != 0 else 0
        assert (_bits(parts[b, used:]) == _bits(np.array(SENT_F64))).all(), f"row {b}: a partial slot past block {used} was written"
        if used:
            a, c = ep[b].astype(np.float64), g32[b].astype(np.float64)
            sums = np.array([a.sum(), (a * a).sum(), c.sum(), (c * c).sum()])
            assert np.abs(parts[b, :used].sum(0) - sums).max() < 1e-11 * per, b
    # in place (out == eps_pos): the same bits; a row with w == 1 is eps_pos already
    got, _ = _run_guide(dev, 0, ep=ep, en=en, scale=w, rescale=phi, partials=True, in_place=True)
    _same("dm3d_guide_update combine in place", got, g32)
    # mode 1 on the partials mode 0 left: rows with phi == 0 are not touched; f within the float64 bar, and the output is one
    # float32 factor within an ulp of the reference's times eps_g, bitwise
    got, _ = _run_guide(dev, 1, out=g32, rescale=phi, partials=parts)
    fmax = np.maximum(f64_.astype(np.float64), 1.0)
    _close("dm3d_guide_update rescale", got, out64, 2.0 ** -21 * M * fmax)
    for b in range(B):
        if phi[b] == 0:
            _same("dm3d_guide_update rescale phi 0", got[b], g32[b])
        else:
            cands = [f32_[b], np.nextafter(f32_[b], np.float32(9)), np.nextafter(f32_[b], np.float32(-9))]
            assert any(np.array_equal(_bits(got[b]), _bits(fc * g32[b])) for fc in cands), f"row {b}: the output is not one factor times eps_g"
    WORST.setdefault("dm3d_guide_update rescale = f x eps_g (bitwise, f within an ulp)", 0.0)


@pytest.mark.parametrize("with_t", [False, True])
@pytest.mark.parametrize("per", SIZES)
def test_guide_mirror(dev, rng, per, with_t):
    B = 2 if per == BIG else 3
    x = _f32(rng, 2 * B, per)
    t = rng.integers(0, 1000, 2 * B).astype(np.int32) if with_t else None
    gx, gt = _run_guide(dev, 2, x=x, t_idx=t)
    _same("dm3d_guide_update mirror", gx, np.concatenate([x[:B], x[:B]]))
    if with_t:
        assert gt.tolist() == np.concatenate([t[:B], t[:B]]).tolist()


# ======================================================================================================================================
# 6. dm3d_pred_to_eps and dm3d_objective_loss_grad
# ======================================================================================================================================
@pytest.mark.parametrize("per", SIZES)
def test_pred_to_eps(dev, rng, per):
    lib = _lib_()
    T = 7
    B = 2 if per == BIG else 4
    t_out, t_in = ([T + 5, -3], [T - 1, 0]) if B == 2 else ([-3, 2, T + 5, 6], [0, 2, T - 1, 6])
    table = _mag(rng, 0.5, 1.5, T, 2)
    pred, x = _f32(rng, B, per), _f32(rng, B, per)
    want = rk.pred_to_eps(pred, x, table, t_in)
    ref = rk.pred_to_eps(pred, x, table, t_in, order="f64")
    for form in ("NULL", "apart", "pred", "x"):
        for t in (t_in, t_out):
            bufs = dict(pred=Guarded(pred, dev, OUT if form in ("NULL", "pred") else IN), x=Guarded(x, dev, OUT if form == "x" else IN),
                        table=_gin(dev, table), t=_gin(dev, np.asarray(t, np.int32)))
            if form == "apart":
                bufs["out"] = _gout(dev, _sentinels(B, per))
            d = lib.PredDesc()
            d.pred, d.x, d.table, d.t_idx = (bufs[k].ptr for k in ("pred", "x", "table", "t"))
            d.batch, d.per_sample, d.timesteps = B, per, T
            res = {"NULL": "pred", "apart": "out", "pred": "pred", "x": "x"}[form]
            d.out = None if form == "NULL" else bufs[res].ptr
            lib.check(lib.lib().dm3d_pred_to_eps(C.byref(d), None), "dm3d_pred_to_eps")
            got = bufs[res].get()
            _check_inputs(bufs)
            _same(f"dm3d_pred_to_eps out {form}", got, want)
    _close("dm3d_pred_to_eps", got, ref, KERNEL_BAR * np.abs(table[t_in].astype(np.float64)).sum(1))


@pytest.mark.parametrize("with_dpred", [True, False])
@pytest.mark.parametrize("per", LOSS_SIZES)
def test_objective_loss_grad(dev, rng, per, with_dpred):
    lib = _lib_()
    B, inv, LP = 3, 1.0 / (4 * 2 * 4 ** 4), 64
    coef = np.full((B, 4), POISON, np.float32)
    coef[:, :3] = _mag(rng, 0.5, 1.5, B, 3)
    coef[:, 2] = np.abs(coef[:, 2])
    pred, noise, x0 = (_f32(rng, B, per) for _ in range(3))
    bufs = dict(pred=_gin(dev, pred), noise=_gin(dev, noise), x0=_gin(dev, x0), coef=_gin(dev, coef),
                partials=_gout(dev, np.full((B, LP), SENT_F64, np.float64)), loss_rows=_gout(dev, np.full(B, SENT_F64, np.float64)),
                loss=_gout(dev, np.full(1, SENT_F64, np.float64)))
    d = lib.LossDesc()
    d.pred, d.noise, d.x0, d.coef, d.partials, d.loss_rows, d.loss = (bufs[k].ptr for k in ("pred", "noise", "x0", "coef", "partials", "loss_rows", "loss"))
    d.batch, d.per_sample, d.inv_divisor = B, per, inv
    if with_dpred:
        bufs["dpred"] = _gout(dev, _sentinels(B, per))
        d.dpred = bufs["dpred"].ptr
    lib.check(lib.lib().dm3d_objective_loss_grad(C.byref(d), None), "dm3d_objective_loss_grad")
    want_g, want_rows, want_loss = rk.objective_loss(pred, noise, x0, coef, inv)
    ref_g, ref_rows, ref_loss = rk.objective_loss(pred, noise, x0, coef, inv, order="f64")
    rows, loss, parts = bufs["loss_rows"].get(), bufs["loss"].get(), bufs["partials"].get()
    _check_inputs(bufs)
    if with_dpred:
        got = bufs["dpred"].get()
        _same("dm3d_objective_loss_grad dpred", got, want_g)
        _close("dm3d_objective_loss_grad dpred", got, ref_g, 1e-5 * np.abs(ref_g).max(1))
    # written, not accumulated into (the buffers held the sentinel, -5e36 as a float64); tests/test_gpu_objective.py's bars
    rel = np.abs(rows - want_rows) / want_rows
    rel_loss = abs(float(loss[0]) - want_loss) / want_loss
    rel64 = max(float((np.abs(rows - ref_rows) / ref_rows).max()), abs(float(loss[0]) - ref_loss) / ref_loss)
    print(f"loss per_sample {per}: rows {rel.max():.2e}, total {rel_loss:.2e} against the float32 d; {rel64:.2e} against float64")
    assert rel.max() < 1e-10 and rel_loss < 1e-10 and rel64 < 1e-5
    assert float(loss[0]) == float(rows[0]) + float(rows[1]) + float(rows[2])                     # in index order
    nblocks = min(-(-(per // 4) // 256), LP)
    assert (_bits(parts[:, nblocks:]) == _bits(np.array(SENT_F64))).all(), "a partial slot past the grid was written"
    assert np.isfinite(parts[:, :nblocks]).all() and (parts[:, :nblocks] >= 0).all()
    WORST["dm3d_objective_loss_grad loss (relative)"] = max(WORST.get("dm3d_objective_loss_grad loss (relative)", 0.0), float(rel.max()), rel_loss)
