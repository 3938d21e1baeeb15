"""The in-kernel N(0,1) stream of dm3d_randn and dm3d_ddpm_update, and of the Python layer above all five drawing entries, against the
host reference oracle/ref_philox.py: EVERY element of every draw within philox_cases.Z_BAR of the float64 evaluation (the stream of
dm3d_ddim_update, dm3d_dpm_sde_update and dm3d_edit_update is held to the same reference in section 3 of
tests/test_gpu_sampler_kernels.py).  The entries are called through ctypes with every device buffer inside guard bands
(tests/guarded_buffers.py): outputs start out full of the sentinel, so an element a grid-stride loop skipped fails the comparison.

dm3d_randn     n = 4, 1004, 2060 and RANDN_WRAP: its grid is min(ceil(n4 / 256), 2048) blocks of 256 lanes (grid_for in dm3d_elem.hip), so
               n4 = 2048 x 256 + 256 + 3 float4 sends block 0 on a second trip of one full block and block 1 on one of 3 lanes; the seven
               seeds (both key words); stream_id 0, 0x7ffffffe, 0x7fffffff, 0xffffffff (word 2 is unsigned).
dm3d_ddpm_update  the draw through a hand-made unit row (alpha_bar_prev = 0, beta = 1, alpha_bar = 0: var = 1, sigma = expf(0.5 logf(1)) = 1,
               and x = eps = 0 gives mean = 0, so x <- z): the four sizes (the last at batch 2 wraps the 256-block grid); the seeds by
               value and through seed_dev as the int64 a chain writes; t = 1, 517, T-1 in one launch next to t = 0, which draws nothing;
               a seeded step on the real tables against the float64 update fed the reference z.
Python layer   ops.randn; a Sampler started under a key >= 2^63 (x_T is stream 0x7fffffff, seed_buf holds the key modulo 2^64);
               q_sample (it draws under the edit kernel's stream at word 2 = t; train_step's own noise is dm3d_randn under stream_id
               0x7ffffffe and a fresh key nobody outside can name, so that id is pinned at the entry, above); ddim_step and dpm_step
               under seed= against the same call with noise= the reference z at word 2 = t, the timestep stepped from, one t per sample:
               this pins the tau the Python layer hands over.

Not covered: the high word of the float4 index (more than 2^34 elements; tests/test_philox_host.py checks it in the reference) and the tail
of the normal beyond what these counters reach (max |z| about 5.3)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import philox_cases as pc
from guarded_buffers import IN, OUT, SENTINEL_WORD, Guarded
from oracle import ref_kernels as rk
from oracle import ref_philox as rp
from oracle import ref_torch as rt

pytestmark = pytest.mark.gpu

SIZES = [4, 1004, 2060, 263180]           # tests/test_gpu_sampler_kernels.py's: one float4, a partial block, two blocks, the wrapped grid
BIG = 263180
RANDN_WRAP = 4 * (2048 * 256 + 256 + 3)
T = 1000
ELEM_TOL = 1e-6                           # tests/test_gpu_infer_kernels.py's bar of dm3d_ddpm_update, relative to max |ref|
EDIT_BAR = 2e-6                           # tests/test_gpu_edit.py's
SENT = np.array([SENTINEL_WORD], np.uint32).view(np.float32)[0]
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


def _z_close(name, got, ref, bar=pc.Z_BAR):
    pc.z_close(WORST, name, got, ref, bar)


def _bitwise(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


# ======================================================================================================================================
# 1. dm3d_randn
# ======================================================================================================================================
def _randn(dev, n, seed, stream_id):
    lib = _lib_()
    buf = Guarded(np.full(n, SENT, np.float32), dev, OUT)
    lib.check(lib.lib().dm3d_randn(buf.ptr, n, seed, stream_id, None), "randn")
    return buf.get()


@pytest.mark.parametrize("n", [4, 1004, 2060, RANDN_WRAP])
def test_randn_sizes(dev, n):
    _z_close("randn", _randn(dev, n, pc.SEED64, 3), rp.randn(n, pc.SEED64, 3))


@pytest.mark.parametrize("seed", pc.SEEDS, ids=hex)
def test_randn_seeds(dev, seed):
    z = _randn(dev, 2060, seed, 0x7FFFFFFF)
    _z_close("randn", z, rp.randn(2060, seed, 0x7FFFFFFF))
    assert pc.independent(z, _randn(dev, 2060, seed ^ (1 << 40), 0x7FFFFFFF))       # a bit of the key's high word


@pytest.mark.parametrize("stream_id", [0, 0x7FFFFFFE, 0x7FFFFFFF, 0xFFFFFFFF], ids=hex)
def test_randn_stream_ids(dev, stream_id):
    _z_close("randn", _randn(dev, 1004, pc.SEED64, stream_id), rp.randn(1004, pc.SEED64, stream_id))


# ======================================================================================================================================
# 2. dm3d_ddpm_update
# ======================================================================================================================================
TABLES = ("beta", "sqrt_alpha", "alpha_bar", "alpha_bar_prev", "sqrt_alpha_bar", "sqrt_alpha_bar_prev", "sqrt_one_minus_alpha_bar")
# every row: alpha_bar_prev = 0, beta = 1, alpha_bar = 0 -> var = (1 - 0) 1 / (1 - 0) = 1 and c1 = c2's operands finite; x = eps = 0 -> mean = 0
UNIT_ROW = dict(beta=1.0, sqrt_alpha=1.0, alpha_bar=0.0, alpha_bar_prev=0.0, sqrt_alpha_bar=1.0, sqrt_alpha_bar_prev=0.0, sqrt_one_minus_alpha_bar=0.0)


def _unit_tables(timesteps):
    return SimpleNamespace(**{k: np.full(timesteps, v, np.float32) for k, v in UNIT_ROW.items()})


def _ddpm_step(dev, tab, x, eps, t, seed=0, seed_dev=None):
    """One guarded mode-1 launch without injected noise; returns x."""
    lib = _lib_()
    B, per = x.shape
    bufs = dict(x=Guarded(x, dev, OUT), eps=Guarded(eps, dev, IN), t=Guarded(np.asarray(t, np.int32), dev, IN))
    d = lib.DdpmDesc()
    d.x, d.eps, d.t, d.batch, d.per_sample, d.mode, d.seed = bufs["x"].ptr, bufs["eps"].ptr, bufs["t"].ptr, B, per, 1, seed
    for name in TABLES:
        bufs[name] = Guarded(np.asarray(getattr(tab, name), np.float32), dev, IN)
        setattr(d, name, bufs[name].ptr)
    d.timesteps = len(np.asarray(tab.beta))
    if seed_dev is not None:
        bufs["seed_dev"] = Guarded(seed_dev, dev, IN)
        d.seed_dev = bufs["seed_dev"].ptr
    lib.check(lib.lib().dm3d_ddpm_update(C.byref(d), None), "ddpm_update")
    out = bufs["x"].get()
    for b in bufs.values():
        if b.role == IN:
            b.unchanged()
    return out


def _ddpm_draw(dev, shape, t, seed=0, seed_dev=None):
    zero = np.zeros(shape, np.float32)
    return _ddpm_step(dev, _unit_tables(T), zero, zero, t, seed, seed_dev)


@pytest.mark.parametrize("per", SIZES)
def test_ddpm_sizes(dev, per):
    B = 2 if per == BIG else 3
    _z_close("ddpm", _ddpm_draw(dev, (B, per), [517] * B, pc.SEED64), rp.ddpm(B, per, 517, pc.SEED64))


@pytest.mark.parametrize("seed", pc.SEEDS, ids=hex)
def test_ddpm_seeds(dev, seed):
    shape, t = (2, 1004), [517, 517]
    z = _ddpm_draw(dev, shape, t, seed)
    _z_close("ddpm", z, rp.ddpm(*shape, 517, seed))
    assert _bitwise(_ddpm_draw(dev, shape, t, 5, seed_dev=pc.seed_words(seed)), z)
    assert pc.independent(z, _ddpm_draw(dev, shape, t, seed ^ (1 << 40)))


def test_ddpm_timesteps(dev):
    """Word 2 is each sample's own t; t = 0 draws nothing (x = clip(mean) = 0 stays 0)."""
    t = [1, 0, 517, T - 1]
    z = _ddpm_draw(dev, (4, 1004), t, pc.SEED64)
    assert (z[1] == 0).all()
    _z_close("ddpm", z, rp.ddpm(4, 1004, t, pc.SEED64))


def test_ddpm_general_row(dev, rng):
    """A seeded step on the real tables against the float64 update fed the REFERENCE z: the entry's own bar (1e-6 of max |ref|) plus
    sigma <= 1 times the z bar."""
    tab, B, per = rt.Betas(50), 4, 1004
    x, eps = (rng.standard_normal((B, per)).astype(np.float32) for _ in range(2))
    t = [49, 0, 17, 1]
    z = rp.ddpm(B, per, t, pc.SEED64)
    ref = rk.ddpm_update(tab, x, eps, t, z)[2].numpy()
    np_tab = SimpleNamespace(**{k: getattr(tab, k).numpy() for k in TABLES})
    got = _ddpm_step(dev, np_tab, x, eps, t, pc.SEED64)
    assert np.isfinite(got).all()
    err = float(np.abs(got - ref).max())
    bar = ELEM_TOL * float(np.abs(ref).max()) + pc.Z_BAR
    print(f"dm3d_ddpm_update seeded, reference z: {err:.2e} (bar {bar:.2e})")
    WORST["dm3d_ddpm_update seeded, reference z (fraction of the bar)"] = err / bar
    assert err < bar


# ======================================================================================================================================
# 3. The Python layer
# ======================================================================================================================================
SHAPE = (2, 8, 8, 8, 4)
PER = 8 * 8 * 8 * 4


@pytest.fixture(scope="module")
def model(dev):
    import dm3d_amd
    from dm3d_amd.networks import conditional_dm3d as cdm
    W = dm3d_amd.synthetic_weights(dm3d_amd.UNetConfig(img_size=8, img_channels=4), seed=0)
    return cdm.DiffusionModel(8, 1024, 4, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=2), weights=W)


def _np(t):
    return t.detach().cpu().numpy()


def test_ops_randn(dev):
    from dm3d_amd import ops
    seed = (1 << 63) + 12345
    z = ops.randn((3, 5, 4), seed, 7)
    assert z.shape == (3, 5, 4) and z.dtype == torch.float32
    _z_close("ops.randn", _np(z).reshape(-1), rp.randn(60, seed, 7))


def test_sampler_start_under_a_key_above_2_63(dev, model):
    seed = (1 << 63) + 12345
    smp = model.sampler(SHAPE, torch.tensor([[[1]], [[0]]]), seed=seed)
    smp.reset()
    _z_close("Sampler x_T", _np(smp.x).reshape(-1), rp.randn(2 * PER, seed, rp.STREAM_ID_X_T))
    assert int(smp.plan.seed_buf.cpu().numpy().view(np.uint64)[0]) == seed
    assert np.array_equal(smp.plan.seed_buf.cpu().numpy(), pc.seed_words(seed))


def test_q_sample_seeded(dev, model, rng):
    """sqrt(a) x0 + sqrt(1-a) z in float64 on the float32 alpha_bar table, z the edit stream's at word 2 = t; a clean level (-1)
    returns x0.  |x0| <= 3: tests/test_gpu_edit.py's 2e-6, plus sqrt(1-a) <= 1 times the z bar."""
    x0 = np.clip(rng.standard_normal(SHAPE), -3, 3).astype(np.float32)
    t, seed = np.array([700, 33]), pc.SEED64
    ab = np.asarray(model.b.alpha_bar, np.float64)[t].reshape(2, 1)
    z = rp.edit(2, PER, t, seed)
    want = np.sqrt(ab) * x0.reshape(2, PER) + np.sqrt(1 - ab) * z
    got = _np(model.q_sample(torch.from_numpy(x0), torch.from_numpy(t), seed=seed)).reshape(2, PER)
    _z_close("q_sample (result)", got, want, EDIT_BAR + pc.Z_BAR)


@pytest.mark.parametrize("step", ["ddim_step", "dpm_step"])
def test_step_seeded_is_the_step_with_the_reference_noise(dev, model, rng, step):
    """seed=s against noise= the reference z at word 2 = t (one t per sample, neither the row index nor t_prev).  Both calls run the same
    kernel on the same x, eps and row; they differ by c (z_device - z_ref32) with c the row's noise coefficient, |c| <= 1: the z bar,
    the float32 rounding of the injected z (2^-24 x 6) and one ulp each of the product and the sum (2^-23 max |out|)."""
    x, eps = (torch.from_numpy(rng.standard_normal(SHAPE).astype(np.float32)) for _ in range(2))
    t, t_prev, seed = np.array([500, 300]), np.array([480, 250]), pc.SEED64
    fn = rp.ddim if step == "ddim_step" else rp.dpm_sde
    z = torch.from_numpy(fn(2, PER, t, seed).astype(np.float32).reshape(SHAPE))
    if step == "ddim_step":
        a = model.ddim_step(x, eps, t, t_prev, 1.0, seed=seed)
        b = model.ddim_step(x, eps, t, t_prev, 1.0, noise=z)
        none = model.ddim_step(x, eps, t, t_prev, 1.0, noise=torch.zeros(SHAPE))
    else:
        a = model.dpm_step(x, eps, t, t_prev, sde_eta=1.0, seed=seed)[0]
        b = model.dpm_step(x, eps, t, t_prev, sde_eta=1.0, noise=z)[0]
        none = model.dpm_step(x, eps, t, t_prev, sde_eta=1.0, noise=torch.zeros(SHAPE))[0]
    a, b, none = _np(a), _np(b), _np(none)
    assert float(np.abs(b - none).std()) > 0.05                             # the row has a noise term worth the name
    bar = pc.Z_BAR + 2.0 ** -24 * 6 + 2.0 ** -23 * float(np.abs(b).max())
    _z_close(f"{step} seeded against reference noise (result)", a, b.astype(np.float64), bar)
