"""GPU tier of global-norm clipping and gradient accumulation: dm3d_grad_scale against float64 numpy and against itself (bitwise),
dm3d_adam_scaled against dm3d_adam / dm3d_adam_ema (bitwise), the clipped and the skipped step through Trainer and train_step, and
the accumulation cycle.  Every buffer an entry writes sits between the sentinel pads of tests/guarded_buffers.py.  Model shapes are
those of test_gpu_train.py::test_train_step_public_api (8^3 x 4ch latents, B = 2, T = 20, real widths)."""
import warnings
from collections import Counter
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from guarded_buffers import IN, OUT, Guarded

pytestmark = pytest.mark.gpu

ULP2 = 2.0 ** -22                        # two float32 ulps, relative: the final rounding and the sqrt (the float64 sum's error is far below)
LAYER_TOL = 2e-5                         # test_gpu_train.py's bound for what the float atomics' reordering does to a gradient
SIZES = [4, 1004, 4 * (4096 * 256 + 1001)]         # test_adam_ema_kernel's: one float4; a ragged last block; past the cap of the grid
NORM_SIZES = SIZES + [4 * (3 * 256 + 7)]           # and several blocks under the cap, so slots past the grid exist beside more than one used
B1, B2, EPS = 0.9, 0.999, 1e-7
T, B, LC = 20, 2, 4
SHAPE = (B, 8, 8, 8, LC)
LR = 2e-4


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _call(name, *args):
    from dm3d_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args, None), name)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _grad_scale(g, partials, state, clip, pre):
    from dm3d_amd import _lib
    d = _lib.GradScaleDesc()
    d.g, d.n, d.partials, d.state, d.clip_norm, d.pre_scale = g.ptr, int(np.prod(g.shape)), partials.ptr, state.ptr, clip, pre
    _call("dm3d_grad_scale", d)


def _parts(dev, fill=None):
    from dm3d_amd import _lib
    n = _lib.GRADNORM_PARTIAL_BLOCKS
    return Guarded(np.full(n, np.nan) if fill is None else fill(n), dev, OUT)


def _state(dev):
    return Guarded(np.full(4, np.nan, np.float32), dev, OUT)


def _gradient(n):
    return (np.random.default_rng(n % 1000).standard_normal(n) * 1e-3).astype(np.float32)


# ---- 1. the norm and the factor ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NORM_SIZES)
def test_norm_and_factor(dev, n):
    """state[0] = pre * |g| and state[1] = pre * min(1, clip / (pre |g|)) within two float32 ulps of float64 numpy, for a clip under
    the norm, one above it and +inf, at pre_scale 1 and 0.25; the factor is exactly 1.0f when nothing clips at pre_scale 1; flags 0; a
    repeated launch is bitwise the same in state and partials, and garbage left in partials changes nothing."""
    g = _gradient(n)
    norm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    gb = Guarded(g, dev, IN)
    for pre in (1.0, 0.25):
        for which, clip in (("under", float(np.float32(0.5 * pre * norm))), ("above", float(np.float32(2.0 * pre * norm))), ("inf", float("inf"))):
            want0 = pre * norm
            want1 = pre * (clip / want0 if want0 > clip else 1.0)
            pa, sa = _parts(dev), _state(dev)
            _grad_scale(gb, pa, sa, clip, pre)
            st, parts = sa.get(), pa.get()
            e0, e1 = abs(float(st[0]) - want0) / want0, abs(float(st[1]) - want1) / want1
            print(f"grad_scale n={n} pre={pre} clip {which}: norm error {e0:.2e}, factor error {e1:.2e} (bound {ULP2:.2e})")
            assert e0 <= ULP2 and e1 <= ULP2
            assert (which == "under") == (float(st[1]) < pre)
            if which != "under" and pre == 1.0:
                assert _same(st[1], np.float32(1.0))
            assert _same(st[2:], np.zeros(2, np.float32))
            # (every slot is a chain of under 100 float64 additions of exact products and numpy adds pairwise: 1e-14 at the worst)
            assert np.isfinite(parts).all() and abs(float(parts.sum()) - norm ** 2) <= 1e-12 * norm ** 2
            _grad_scale(gb, pa, sa, clip, pre)                                   # the same buffers again
            assert _same(sa.get(), st) and np.array_equal(pa.get().view(np.uint64), parts.view(np.uint64))
            junk, sj = _parts(dev, lambda k: np.random.default_rng(k).standard_normal(k) * 1e30), _state(dev)
            junk.t[junk.t.numel() // 2] = -1                                     # (and a NaN pattern among them)
            _grad_scale(gb, junk, sj, clip, pre)
            assert _same(sj.get(), st) and np.array_equal(junk.get().view(np.uint64), parts.view(np.uint64))
    gb.unchanged()


# ---- 2. a gradient that is not finite ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NORM_SIZES)
def test_non_finite_gradient_sets_the_flag_and_the_step_is_skipped(dev, n):
    """One inf, and one NaN, in the first block, in the last ragged block and at the last element: state[2] = 1, state[3] = 0, and
    dm3d_adam_scaled on that state stores nothing: w, m, v and ema are bitwise what they were."""
    g = _gradient(n)
    rng = np.random.default_rng(7)
    w0, ema0 = (rng.standard_normal(n) * 0.1).astype(np.float32), (rng.standard_normal(n) * 0.1).astype(np.float32)
    m0, v0 = (rng.standard_normal(n) * 1e-3).astype(np.float32), (rng.standard_normal(n) ** 2 * 1e-6).astype(np.float32)
    for pos in sorted({min(1, n - 1), max(n - 7, 0), n - 1}):
        for value in (np.inf, np.nan):
            bad = g.copy()
            bad[pos] = value
            gb, pa, sa = Guarded(bad, dev, IN), _parts(dev), _state(dev)
            _grad_scale(gb, pa, sa, 1.0, 1.0)
            st = sa.get()
            assert float(st[2]) == 1.0 and float(st[3]) == 0.0, (pos, value, st)
            pa.get()
            for ema in (ema0, None):
                bw, bm, bv = Guarded(w0, dev, OUT), Guarded(m0, dev, OUT), Guarded(v0, dev, OUT)
                be = Guarded(ema, dev, OUT) if ema is not None else None
                _call("dm3d_adam_scaled", bw.ptr, gb.ptr, bm.ptr, bv.ptr, be.ptr if be else None, n, 1e-3, B1, B2, EPS, 0.25, sa.ptr)
                assert _same(bw.get(), w0) and _same(bm.get(), m0) and _same(bv.get(), v0) and (be is None or _same(be.get(), ema0)), (pos, value)
            assert _same(sa.get(), st)
            gb.unchanged()


# ---- 3. bitwise against the unscaled kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_adam_scaled_is_bitwise_the_parent_kernels(dev, n):
    """state = (., 1, 0, 0): dm3d_adam_ema's w, m, v, ema, and with ema = NULL dm3d_adam's w, m, v.  state[1] = s: dm3d_adam_ema's on
    the buffer float32(s) * g (one float32 multiply on the host).  g and state are left as they are."""
    rng = np.random.default_rng(n % 1000 + 1)
    g = rng.standard_normal(n).astype(np.float32)
    w0, ema0 = (rng.standard_normal(n) * 0.1).astype(np.float32), (rng.standard_normal(n) * 0.1).astype(np.float32)
    m0, v0 = (rng.standard_normal(n) * 0.1).astype(np.float32), (rng.standard_normal(n) ** 2 * 0.01).astype(np.float32)
    lr_t, rate = 0.05, 0.25
    gb = Guarded(g, dev, IN)

    def run(entry, grad, ema, state=None):
        bw, bm, bv = Guarded(w0, dev, OUT), Guarded(m0, dev, OUT), Guarded(v0, dev, OUT)
        be = Guarded(ema0, dev, OUT) if ema else None
        if entry == "dm3d_adam":
            _call(entry, bw.ptr, grad.ptr, bm.ptr, bv.ptr, n, lr_t, B1, B2, EPS)
        elif entry == "dm3d_adam_ema":
            _call(entry, bw.ptr, grad.ptr, bm.ptr, bv.ptr, be.ptr, n, lr_t, B1, B2, EPS, rate)
        else:
            _call(entry, bw.ptr, grad.ptr, bm.ptr, bv.ptr, be.ptr if be else None, n, lr_t, B1, B2, EPS, rate, state.ptr)
        out = [bw.get(), bm.get(), bv.get()] + ([be.get()] if ema else [])
        assert not _same(out[0], w0) and all(np.isfinite(o).all() for o in out)
        return out

    for s in (1.0, 0.25, 0.3717):
        sb = Guarded(np.array([7.0, s, 0.0, 0.0], np.float32), dev, IN)
        scaled = gb if s == 1.0 else Guarded(np.float32(s) * g, dev, IN)
        for ema in ((True, False) if s == 1.0 else (True,)):
            got, want = run("dm3d_adam_scaled", gb, ema, sb), run("dm3d_adam_ema" if ema else "dm3d_adam", scaled, ema)
            for name, a, b in zip("wmve", got, want):
                assert _same(a, b), f"n={n} s={s} ema={ema}: {name} differs in {int((_bits(a) != _bits(b)).sum())} elements"
        sb.unchanged()
    gb.unchanged()


# ---- the tiny model ---------------------------------------------------------------------------------------------------------------------
def _args():
    return SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B)


@pytest.fixture(scope="module")
def weights():
    import dm3d_amd
    return dm3d_amd.synthetic_weights(dm3d_amd.UNetConfig(img_size=8, img_channels=4), seed=1)


@pytest.fixture(scope="module")
def batches():
    g = torch.Generator().manual_seed(5)
    return [dict(lat=torch.randn(*SHAPE, generator=g), noise=torch.randn(*SHAPE, generator=g), t=torch.randint(0, T, (B,), generator=g),
                 ctx=torch.randint(0, 2, (B, 1, 1), generator=g)) for _ in range(3)]


def _model(weights, **compile_kw):
    from dm3d_amd.networks import conditional_dm3d as cdm
    m = cdm.DiffusionModel(8, 1024, 4, None, _args(), weights=weights)
    m.compile(loss="mse_sum", optimizer=SimpleNamespace(learning_rate=LR), **compile_kw)
    return m


def _step(m, b, **kw):
    return m.train_step((None, None, b["ctx"]), latents=b["lat"], t=b["t"], noise=kw.get("noise", b["noise"]))


def _loss_and_grad(tr, b, dev, **kw):
    import dm3d_amd
    from dm3d_amd.betas import BETAS_FIELDS
    tab = dm3d_amd.Betas(T).device_tables(dev)
    betas = (tab[BETAS_FIELDS.index("sqrt_alpha_bar")], tab[BETAS_FIELDS.index("sqrt_one_minus_alpha_bar")])
    return tr.loss_and_grad(b["lat"].to(dev), b["t"], b["noise"].to(dev), b["ctx"].reshape(-1).numpy(), betas, T, B, LC, **kw)


def _flat(tr):
    torch.cuda.synchronize()
    return SimpleNamespace(theta=tr.theta.cpu().numpy(), m=tr.m.cpu().numpy(), v=tr.v.cpu().numpy(), grad=tr.grad.cpu().numpy(),
                           ema=None if tr.ema is None else tr.ema.cpu().numpy(), step_count=tr.step_count, ema_updates=tr.ema_updates)


def _lr_t(tt, lr=LR):
    return lr * (1.0 - B2 ** tt) ** 0.5 / (1.0 - B1 ** tt)


def _plain_adam(dev, before, grad, tt):
    """What dm3d_adam makes of copies of the recorded buffers ``before`` fed ``grad`` at step ``tt``."""
    bw, bm, bv, bg = Guarded(before.theta, dev, OUT), Guarded(before.m, dev, OUT), Guarded(before.v, dev, OUT), Guarded(grad, dev, IN)
    _call("dm3d_adam", bw.ptr, bg.ptr, bm.ptr, bv.ptr, grad.size, _lr_t(tt), B1, B2, EPS)
    return bw.get(), bm.get(), bv.get()


def _assert_step(dev, tr, before, tt, label):
    """theta, m, v of ``tr`` are bitwise dm3d_adam's on ``before`` with the gradient float32(state[1]) * (the buffer tr holds)."""
    now = _flat(tr)
    factor = tr.clip_state.cpu().numpy()[1]
    w, m, v = _plain_adam(dev, before, np.float32(factor) * now.grad, tt)
    assert not _same(now.theta, before.theta), label
    assert _same(now.theta, w) and _same(now.m, m) and _same(now.v, v), label
    return now, float(factor)


# ---- 4. Trainer level ---------------------------------------------------------------------------------------------------------------------
def test_trainer_clipped_step(dev, weights, batches):
    """After loss_and_grad the buffer is copied to the host; the clipped adam_step at half its float64 norm reports that norm within two
    ulps and leaves theta, m, v bitwise dm3d_adam's on the recorded buffers fed float32(state[1]) * grad; at ten times the norm they are
    bitwise the plain step's.  (Recorded buffers, never a second backward: dm3d_wgrad's float atomics do not repeat bitwise.)"""
    import dm3d_amd
    from dm3d_amd.train import Trainer
    tr = Trainer(dm3d_amd.UNetConfig(img_size=8, img_channels=4), weights, dev, lr=LR)
    _loss_and_grad(tr, batches[0], dev)
    tr.adam_step()                                                       # a plain first step: the moments are no longer zero
    assert tr.finish_step() is False and tr.clip_state is None and tr.grad_norm is None
    for tt, b, mult in ((2, batches[1], 0.5), (3, batches[2], 10.0)):
        _loss_and_grad(tr, b, dev)
        before = _flat(tr)
        norm = float(np.sqrt(np.sum(before.grad.astype(np.float64) ** 2)))
        assert np.isfinite(norm) and norm > 0
        tr.set_clipping(global_clipnorm=mult * norm)
        tr.adam_step()
        assert tr.finish_step() is False and tr.step_count == tt and tr.skipped_steps == 0
        print(f"trainer step {tt}: grad_norm {tr.grad_norm:.9e} vs host {norm:.9e}")
        assert abs(tr.grad_norm - norm) <= ULP2 * norm
        now, factor = _assert_step(dev, tr, before, tt, f"clip at {mult} x norm")
        assert _same(now.grad, before.grad)
        if mult < 1:
            assert abs(factor - mult) <= 4 * ULP2 * mult              # (the clip itself was rounded to float32 on its way in)
        else:
            assert factor == 1.0
            w, m, v = _plain_adam(dev, before, before.grad, tt)
            assert _same(now.theta, w) and _same(now.m, m) and _same(now.v, v)


# ---- 5. accumulation ----------------------------------------------------------------------------------------------------------------------
def _compare_grads(got, ref, tol, label=""):
    """test_gpu_train.py's rule: per tensor, max |g - ref| <= tol * max(|ref| of that tensor, 1e-3 * the largest gradient entry overall)."""
    gmax = max(float(np.abs(v).max()) for v in ref.values())
    worst = ("", 0.0)
    for name, r in ref.items():
        scale = max(float(np.abs(r).max()), 1e-3 * gmax)
        e = float(np.abs(got[name].astype(np.float64) - r).max()) / scale
        if e > worst[1]:
            worst = (name, e)
    print(f"{label} worst gradient error {worst[1]:.3e} at {worst[0]} (largest gradient entry {gmax:.3e})")
    assert worst[1] < tol, worst


def test_accumulation_cycle(dev, weights, batches):
    """compile(grad_accum_steps=2): the first train_step leaves theta, m, v and step_count untouched and the buffer filled; the second
    applies float32(0.5) * (the sum of the two micro-batches' gradients); the third starts a new cycle from a zeroed buffer."""
    import dm3d_amd
    from dm3d_amd.train import Trainer
    ref = Trainer(dm3d_amd.UNetConfig(img_size=8, img_channels=4), weights, dev, lr=LR)       # same weights; no step is ever taken on it
    single = []
    for b in batches[:2]:
        _loss_and_grad(ref, b, dev)
        torch.cuda.synchronize()
        single.append({k: v.astype(np.float64) for k, v in ref.grads().items()})
    m = _model(weights, grad_accum_steps=2)
    tr = m.trainer
    start = _flat(tr)
    out = _step(m, batches[0])
    mid = _flat(tr)
    assert set(out) == {"loss"} and m.loss_tracker.count == 1
    assert _same(mid.theta, start.theta) and _same(mid.m, start.m) and _same(mid.v, start.v) and tr.step_count == 0 and tr.ema_updates == 0
    assert np.abs(mid.grad).max() > 0 and tr.clip_state is None and tr.grad_norm is None
    _step(m, batches[1])
    assert tr.step_count == 1 and m.loss_tracker.count == 2 and tr.skipped_steps == 0
    _compare_grads(tr.grads(), {k: single[0][k] + single[1][k] for k in single[0]}, LAYER_TOL, "sum of two micro-batches:")
    now, factor = _assert_step(dev, tr, start, 1, "accumulated step")
    assert _same(np.float32(factor), np.float32(0.5))
    norm = 0.5 * float(np.sqrt(np.sum(now.grad.astype(np.float64) ** 2)))
    assert abs(tr.grad_norm - norm) <= ULP2 * norm
    _step(m, batches[0])                                                 # a new cycle: the buffer is zeroed first
    third = _flat(tr)
    assert tr.step_count == 1 and _same(third.theta, now.theta) and _same(third.m, now.m) and m.loss_tracker.count == 3
    ref.theta.copy_(tr.theta)                                            # batch 0's gradient alone, at the weights the step left
    _loss_and_grad(ref, batches[0], dev)
    torch.cuda.synchronize()
    # a buffer that was not zeroed would hold the old sum as well, whose largest entry is of the order of the largest gradient entry
    # itself: 1e-3 of it tells the two apart with two orders of magnitude to either side of the atomics' 2e-5
    _compare_grads(tr.grads(), {k: v.astype(np.float64) for k, v in ref.grads().items()}, 1e-3, "first micro-batch of the next cycle:")


# ---- 6. the skipped step through the public path ----------------------------------------------------------------------------------------
def test_skipped_step_through_train_step(dev, weights, batches):
    """compile(global_clipnorm=1.0, ema_decay=0.99): a good step; a step whose noise holds one inf raises nothing, warns, counts in
    skipped_steps and leaves theta, m, v, ema, step_count and ema_updates as the good step left them; the next good step is step 2,
    with step 2's bias correction."""
    m = _model(weights, global_clipnorm=1.0, ema_decay=0.99)
    _step(m, batches[0])
    tr = m.trainer
    good = _flat(tr)
    assert (good.step_count, good.ema_updates, tr.skipped_steps) == (1, 1, 0) and np.isfinite(tr.grad_norm)
    noise = batches[1]["noise"].clone()
    noise.view(-1)[123] = float("inf")
    with pytest.warns(UserWarning, match="skipped"):
        out = _step(m, batches[1], noise=noise)
    assert set(out) == {"loss"}
    after = _flat(tr)
    assert tr.skipped_steps == 1 and (after.step_count, after.ema_updates) == (1, 1)
    assert not np.isfinite(after.grad).all() and not np.isfinite(tr.grad_norm)
    for name in ("theta", "m", "v", "ema"):
        assert _same(getattr(after, name), getattr(good, name)), name
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*skipped.*")          # no such warning on a good step
        _step(m, batches[2])
    assert (tr.step_count, tr.ema_updates, tr.skipped_steps) == (2, 2, 1)
    now, factor = _assert_step(dev, tr, good, 2, "the step after a skipped one")
    assert 0 < factor <= 1.0 and np.isfinite(now.ema).all() and not _same(now.ema, good.ema)
    w3, _, _ = _plain_adam(dev, good, np.float32(factor) * now.grad, 3)
    assert not _same(now.theta, w3)                                      # (the check tells step 2's lr_t from step 3's)


# ---- a model compiled without the new keywords launches what it launched before ---------------------------------------------------------
def test_without_the_keywords_the_launches_are_the_old_ones(dev, weights, batches, monkeypatch):
    import dm3d_amd.train as train
    real, calls = train.lib(), Counter()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)

            def counted(*a):
                calls[name] += 1
                return fn(*a)
            return counted

    monkeypatch.setattr(train, "lib", lambda: Spy())
    m = _model(weights)
    _step(m, batches[0])
    tr = m.trainer
    assert (calls["dm3d_adam"], calls["dm3d_adam_ema"], calls["dm3d_grad_scale"], calls["dm3d_adam_scaled"]) == (1, 0, 0, 0)
    assert tr.clip_state is None and tr.clip_partials is None and tr.grad_norm is None and tr.skipped_steps == 0
    m.compile(loss="mse_sum", optimizer=SimpleNamespace(learning_rate=LR), ema_decay=0.9)
    _step(m, batches[1])
    assert (calls["dm3d_adam"], calls["dm3d_adam_ema"], calls["dm3d_grad_scale"], calls["dm3d_adam_scaled"]) == (1, 1, 0, 0)
    assert tr.clip_state is None
    m.compile(loss="mse_sum", optimizer=SimpleNamespace(learning_rate=LR), ema_decay=0.9, global_clipnorm=1.0)     # re-read at the next step
    _step(m, batches[2])
    assert (calls["dm3d_adam"], calls["dm3d_adam_ema"], calls["dm3d_grad_scale"], calls["dm3d_adam_scaled"]) == (1, 1, 1, 1)
    assert tr.clip_state is not None and tr.step_count == 3 and tr.ema_updates == 2 and np.isfinite(tr.grad_norm)
