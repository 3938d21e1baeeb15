"""GPU tier of the training extensions: dm3d_adam_ema against dm3d_adam (bitwise) and a float64 lerp, the weight average through
train_step / use_ema() / checkpoints, context dropout and the null-context default of guidance.  The float64 references are written
here; shapes are those of test_gpu_train.py::test_train_step_public_api (8^3 x 4ch latents, B = 2, T = 20)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ELEM_TOL = 1e-6                          # the elementwise bar of test_gpu_train_kernels.py
PAD = 64                                 # sentinel elements on each side of a buffer (a multiple of 4: pointers stay 16-byte aligned)
SENTINEL = -123456.0
T, B, LC = 20, 2, 4
SHAPE = (B, 8, 8, 8, LC)
LR, DECAY = 2e-4, 0.9


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


class Buf:
    """A device buffer holding `arr` between two runs of sentinel elements."""

    def __init__(self, arr, dev):
        a = np.ascontiguousarray(arr, np.float32)
        self.n = a.size
        self.t = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=dev)
        self.t[PAD:PAD + self.n] = torch.from_numpy(a.reshape(-1)).to(dev)
        self.ptr = self.t.data_ptr() + PAD * 4
        assert self.ptr % 16 == 0

    def get(self):
        torch.cuda.synchronize()
        assert bool((self.t[:PAD] == SENTINEL).all()) and bool((self.t[PAD + self.n:] == SENTINEL).all()), "sentinel padding overwritten"
        return self.t[PAD:PAD + self.n].cpu().numpy()


def _call(name, *args):
    from dm3d_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args, None), name)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("n", [4, 1004, 4 * (4096 * 256 + 1001)])       # one float4; a ragged last block; past the cap of the grid
def test_adam_ema_kernel(dev, n):
    """Three steps at rates 1, 0.25 and 0: w, m and v bitwise those of dm3d_adam on copies, ema within 1e-6 of the float64 lerp towards
    the device's own new weights, bitwise the new weights at rate 1 and bitwise untouched at rate 0; g and the sentinels survive."""
    rng = np.random.default_rng(n % 1000)
    b1, b2, eps, lr = 0.9, 0.999, 1e-7, 0.5
    w0 = (rng.standard_normal(n) * 0.1).astype(np.float32)
    ema0 = (rng.standard_normal(n) * 0.1).astype(np.float32)             # unrelated to w: the lerp has something to do
    zeros = np.zeros(n, np.float32)
    bw, bm, bv, be = Buf(w0, dev), Buf(zeros, dev), Buf(zeros, dev), Buf(ema0, dev)
    cw, cm, cv = Buf(w0, dev), Buf(zeros, dev), Buf(zeros, dev)          # the plain optimizer's copies
    ema_prev = ema0
    for t, rate in ((1, 1.0), (2, 0.25), (3, 0.0)):
        g = rng.standard_normal(n).astype(np.float32)
        lr_t = float(np.float32(lr * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)))
        bg = Buf(g, dev)
        _call("dm3d_adam", cw.ptr, bg.ptr, cm.ptr, cv.ptr, n, lr_t, b1, b2, eps)
        _call("dm3d_adam_ema", bw.ptr, bg.ptr, bm.ptr, bv.ptr, be.ptr, n, lr_t, b1, b2, eps, rate)
        w_new, ema = bw.get(), be.get()
        assert np.array_equal(_bits(w_new), _bits(cw.get())), f"w differs from dm3d_adam at step {t}"
        assert np.array_equal(_bits(bm.get()), _bits(cm.get())), f"m differs from dm3d_adam at step {t}"
        assert np.array_equal(_bits(bv.get()), _bits(cv.get())), f"v differs from dm3d_adam at step {t}"
        assert not np.array_equal(w_new, w0) and np.isfinite(ema).all()
        ref = ema_prev.astype(np.float64) + rate * (w_new.astype(np.float64) - ema_prev.astype(np.float64))
        err = float(np.abs(ema - ref).max() / np.abs(ref).max())
        print(f"dm3d_adam_ema n={n} rate={rate}: ema error {err:.2e}")
        assert err < ELEM_TOL
        if rate == 1.0:
            assert np.array_equal(_bits(ema), _bits(w_new))
        if rate == 0.0:
            assert np.array_equal(_bits(ema), _bits(ema_prev))
        assert np.array_equal(_bits(bg.get()), _bits(g))
        ema_prev = ema


def _args():
    return SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B)


def _batch(g):
    return dict(lat=torch.randn(*SHAPE, generator=g), noise=torch.randn(*SHAPE, generator=g), t=torch.randint(0, T, (B,), generator=g),
                ctx=torch.randint(0, 2, (B, 1, 1), generator=g))


@pytest.fixture(scope="module")
def trained(dev):
    """A model trained for three steps with compile(ema_decay=0.9) (warm-up on), and after every step the live weights and the
    average read back from its Trainer."""
    import dm3d_amd
    from dm3d_amd.networks import conditional_dm3d as cdm
    cfg = dm3d_amd.UNetConfig(img_size=8, img_channels=4)
    W = dm3d_amd.synthetic_weights(cfg, seed=1)
    m = cdm.DiffusionModel(8, 1024, 4, None, _args(), weights=W)
    m.compile(loss="mse_sum", optimizer=SimpleNamespace(learning_rate=LR), ema_decay=DECAY)
    g = torch.Generator().manual_seed(5)
    history = []
    for _ in range(3):
        b = _batch(g)
        m.train_step((None, None, b["ctx"]), latents=b["lat"], t=b["t"], noise=b["noise"])
        history.append((m.trainer.state_dict(), m.trainer.ema_state_dict(), m.trainer.ema_updates))
    return SimpleNamespace(model=m, W=W, history=history, gen=g)


def _rel(a, ref):
    a, ref = torch.as_tensor(a).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def test_average_follows_the_recurrence_and_the_sampler_switches(dev, trained):
    """After each of three train steps ema_state_dict() is the float64 recurrence ema += (1 - decay_t) (w - ema), decay_t = 0.1, 2/11,
    3/12 (warm-up under 0.9), over the live weights read back after that step, at 1e-6 of each tensor's largest entry; its moving
    statistics are the live ones.  Under use_ema(True) network([x, t, c]) is the oracle's forward on the averaged weights at the 1e-3
    bar of test_train_step_public_api, under use_ema(False) on the live ones.  At lr 2e-4 the oracle's two outputs differ by 1.7e-1
    of the largest entry (CPU oracle on its own trajectory: 170 times the bar), so an ignored switch fails; the test asserts >= 1e-2."""
    from dm3d_amd.train import is_trainable
    from oracle import ref_torch as rt
    m = trained.model
    ref = {k: np.asarray(v, np.float64) for k, v in trained.W.items() if is_trainable(k)}
    assert m.trainer.ema_updates == 3 and m.trainer.step_count == 3
    worst = 0.0
    for n, (live, ema, updates) in enumerate(trained.history):
        assert updates == n + 1 and set(ema) == set(live) == set(trained.W)
        decay = min(DECAY, (1 + n) / (10 + n))
        for k in live:
            assert ema[k].shape == live[k].shape == trained.W[k].shape and ema[k].dtype == np.float32
            if not is_trainable(k):
                assert np.array_equal(_bits(ema[k]), _bits(live[k])), k
                continue
            ref[k] = ref[k] + (1.0 - decay) * (live[k].astype(np.float64) - ref[k])
            err = float(np.abs(ema[k] - ref[k]).max() / max(float(np.abs(ref[k]).max()), 1e-30))
            worst = max(worst, err)
            assert err < 1e-6, (n, k, err)
    print(f"average vs float64 recurrence over three steps: worst {worst:.2e}")
    live = trained.history[-1][0]
    assert max(float(np.abs(ref[k] - live[k]).max()) for k in ref) > 1e-5                 # the average is not the live weights
    ocfg = rt.UNetConfig(img_size=8, img_channels=4)
    x = torch.randn(*SHAPE, generator=torch.Generator().manual_seed(11))
    tt, cc = torch.tensor([1, 7]), torch.tensor([[[1]], [[0]]])
    o_live = rt.unet_forward({k: torch.from_numpy(v) for k, v in live.items()}, ocfg, x, tt, cc)
    o_avg = rt.unet_forward({k: torch.from_numpy(ref[k].astype(np.float32) if k in ref else v) for k, v in live.items()}, ocfg, x, tt, cc)
    gap = _rel(o_avg, o_live)
    print(f"oracle, averaged against live weights: {gap:.3e}")
    assert gap >= 1e-2
    assert m.use_ema(True) is False
    e_avg = m.network([x.to(dev), tt, cc])
    print(f"network under use_ema(True) against the oracle on the averaged weights: {_rel(e_avg, o_avg):.3e}")
    assert _rel(e_avg, o_avg) < 1e-3
    assert m.use_ema(False) is True
    e_live = m.network([x.to(dev), tt, cc])
    assert _rel(e_live, o_live) < 1e-3


def _chain(model, **kw):
    return model.generate(SHAPE, context_value=[1, 0], seed=3, sampler="ddim", num_steps=4, **kw)


def test_switch_drops_the_captured_graphs(dev, trained):
    m = trained.model
    m.use_ema(False)
    a = _chain(m)
    m.use_ema(True)
    b = _chain(m)
    assert m.use_ema(False) is True
    c = _chain(m)
    torch.cuda.synchronize()
    assert torch.isfinite(b).all() and torch.equal(a, c) and not torch.equal(a, b)


def test_inference_only_load_samples_from_the_average(dev, trained, tmp_path):
    from dm3d_amd.networks import conditional_dm3d as cdm
    m = trained.model
    path = str(tmp_path / "trained.npz")
    m.use_ema(True)
    m.save_weights(path)                                                                   # the live weights and ema/..., whatever the switch says
    want = _chain(m)
    m.use_ema(False)
    live_out = _chain(m)
    saved = dict(np.load(path))
    live = trained.history[-1][0]
    assert all(np.array_equal(_bits(saved[k]), _bits(live[k])) for k in live)
    assert int(saved["ema/num_updates"]) == 3 and "optimizer/iter" in saved
    other = cdm.DiffusionModel(8, 1024, 4, None, _args(), weights=None, seed=9)
    other.load_weights(path)
    assert torch.equal(_chain(other), live_out)
    assert other.use_ema(True) is False
    got = _chain(other)
    torch.cuda.synchronize()
    assert other.weights.trainer is None
    assert torch.equal(got, want) and not torch.equal(got, live_out)
    # a resumed run continues the average where it stopped
    other.compile(optimizer=SimpleNamespace(learning_rate=LR), ema_decay=DECAY)
    assert other.trainer.ema_updates == 3 and other.weights.pending_ema is None
    ema = other.trainer.ema_state_dict()
    assert all(np.array_equal(_bits(ema[k]), _bits(trained.history[-1][1][k])) for k in ema)


def test_context_dropout_trains_the_null_row_and_guidance_defaults_to_it(dev, trained):
    """context_dim = 2 with the spare id 2 as the null context: a dropped sample's gradient lands in the table's row 2 and nowhere
    else; generate(guidance_scale=) without negative_context is the call with negative_context=2."""
    import dm3d_amd
    from dm3d_amd.networks import conditional_dm3d as cdm
    cfg = dm3d_amd.UNetConfig(img_size=8, img_channels=4, context_dim=2)
    m = cdm.DiffusionModel(8, 1024, 4, None, _args(), weights=dm3d_amd.synthetic_weights(cfg, seed=2), context_dim=2)
    m.compile(optimizer=SimpleNamespace(learning_rate=LR), context_dropout=0.5, null_context=2)
    b = _batch(torch.Generator().manual_seed(7))
    ctx = torch.tensor([[[1]], [[0]]])
    for drop, zero_row, live_row in (([True, False], 1, 2), ([False, False], 2, 1)):
        m.train_step((None, None, ctx), latents=b["lat"], t=b["t"], noise=b["noise"], drop=torch.tensor(drop))
        table = m.trainer.grads()["ctx_embed.table"]
        assert table.shape[0] == 3
        assert not table[zero_row].any(), (drop, table[zero_row])
        assert table[live_row].any() and table[0].any(), drop
    kw = dict(context_value=[1, 0], seed=4, sampler="ddim", num_steps=2, guidance_scale=2.0)
    out = m.generate(SHAPE, **kw)
    assert torch.equal(out, m.generate(SHAPE, negative_context=2, **kw))
    assert not torch.equal(out, m.generate(SHAPE, negative_context=0, **kw))
    with pytest.raises(ValueError, match="no reserved null context"):
        trained.model.generate(SHAPE, **kw)
    with pytest.raises(ValueError):
        trained.model.train_step((None, None, ctx), latents=b["lat"], t=b["t"], noise=b["noise"], drop=torch.tensor([True, False]))
