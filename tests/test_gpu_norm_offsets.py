"""GPU parity of every kernel that turns a tensor into a mean and a variance, on tensors whose mean is up to 1000 times their spread
(tests/norm_offset_cases.py: inputs, float32 models, bars; tests/test_norm_offsets_host.py: the models against float64 on the CPU).

Raw C ABI through ctypes on guarded buffers (tests/guarded_buffers.py); the two conv launches and the one Trainer layer go through the
wrappers the tests they are taken from use.  Seven entries:

  dm3d_groupnorm_stats -> dm3d_batchnorm_finalize     the accumulator filled by the kernel that fills it in training; bar LAYER_TOL at every r
  dm3d_groupnorm_stats x 2 -> dm3d_groupnorm_finalize two inputs at chan_off; bar LAYER_TOL at every r
  dm3d_groupnorm_partials -> dm3d_groupnorm_finalize2 float32 slots: bar max(LAYER_TOL, 4 x the slot model's error on the input); the partials
                                                      themselves against the float64 slot sums at LAYER_TOL (a sum's own error does not grow)
  gn_stats of a conv launch -> finalize2              a fused launch and a Cin-split launch, bias = +-r x std of the bias-free output
  dm3d_layernorm3, _h2, dm3d_layernorm_bwd            per-row offsets; bar max(ROW_TOL, 4 x the two-pass model's error)
  dm3d_bn_act_bwd                                     on the statistics the chain above produced; bar from the float32 model of x*scale + shift
  Trainer.bn_act, forward and backward                one layer at r = 30 at the bars of tests/test_gpu_train.py

Every comparison asserts finiteness first and prints error / model error / bar; the worst per (entry, r) is printed at the end of the
module (docs/EXPERIMENTS.md records a run)."""
import numpy as np
import pytest
import torch

import norm_offset_cases as nc
from guarded_buffers import IN, OUT, PAD, Guarded, h2_decode
from norm_offset_cases import EPS, LAYER_TOL, MOMENTUM, ROW_TOL, R_VALUES

pytestmark = pytest.mark.gpu

TABLE = {}


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    yield torch.device("cuda:0")
    print("entry | r | measured | model | bar")
    for (entry, r) in sorted(TABLE):
        e, m, b = TABLE[(entry, r)]
        print(f"{entry} | {r} | {e:.2e} | {m:.2e} | {b:.2e}")


def _call(name, *args):
    from dm3d_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args, None), name)


def _hold(entry, r, what, got, ref, bar, model=0.0, final=True):
    """One comparison; final=False keeps an intermediate (sums, partials, a conv's output) out of the table printed at the end."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), f"{entry} {what} r={r}: non-finite output"
    e = nc.err(got, ref)
    print(f"{entry} {what} r={r}: {e:.2e} (model {model:.2e}, bar {bar:.2e})")
    if final:
        w = TABLE.get((entry, r), (0.0, 0.0, 0.0))
        TABLE[(entry, r)] = (max(w[0], e), max(w[1], model), max(w[2], bar))
    assert e < bar, f"{entry} {what} r={r}: {e:.3e} >= {bar:.3e}"


def _zeros(dev, *shape, dtype=np.float32):
    return Guarded(np.zeros(shape, dtype), dev, OUT)


def _stats(dev, x, c1, acc):
    """dm3d_groupnorm_stats of x [B, V, c] as one input, or as two at chan_off 0 and c1.  Returns the input buffers."""
    B, V, c = x.shape
    bufs = []
    for lo, hi in ((0, c1), (c1, c)) if c1 < c else ((0, c),):
        b = Guarded(x[..., lo:hi], dev, IN)
        _call("dm3d_groupnorm_stats", b.ptr, B, V, hi - lo, acc.ptr, c, lo)
        bufs.append(b)
    return bufs


# ---- dm3d_groupnorm_stats -> dm3d_batchnorm_finalize ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", R_VALUES)
@pytest.mark.parametrize("shape", nc.BN_SHAPES, ids=nc.shape_id)
def test_stats_into_batchnorm_finalize(dev, shape, r):
    entry = "groupnorm_stats -> batchnorm_finalize"
    B, V, c = shape
    x, gamma, beta = nc.stats_input(B, V, c, r)
    mov = nc.moving_input(c)
    bg, bb = Guarded(gamma, dev, IN), Guarded(beta, dev, IN)
    acc = _zeros(dev, B, c, 2, dtype=np.float64)
    moments = nc.rk.moments_acc(nc._t64(x)).numpy()
    bx = Guarded(x, dev, IN)
    for unbiased in (1, 0):
        for moving in (True, False):
            _call("dm3d_groupnorm_stats", bx.ptr, B, V, c, acc.ptr, c, 0)
            got = acc.get()
            _hold(entry, r, "sums", got[..., 0], moments[..., 0], LAYER_TOL, final=False)
            _hold(entry, r, "sums of squares", got[..., 1], moments[..., 1], LAYER_TOL, final=False)
            ref = nc.bn_reference(x, gamma, beta, mov if moving else None, unbiased)
            outs = [_zeros(dev, c) for _ in range(4)]
            bmm, bmv = Guarded(mov[0], dev, OUT), Guarded(mov[1], dev, OUT)
            _call("dm3d_batchnorm_finalize", acc.ptr, B, V, c, EPS, bg.ptr, bb.ptr, *(o.ptr for o in outs), bmm.ptr if moving else None,
                  bmv.ptr if moving else None, MOMENTUM, unbiased)
            for o, f, what in zip(outs, ref, nc.BN_OUTPUTS):
                _hold(entry, r, what, o.get(), f, LAYER_TOL)
            if moving:
                _hold(entry, r, "moving_mean", bmm.get(), ref[4], LAYER_TOL)
                _hold(entry, r, "moving_var", bmv.get(), ref[5], LAYER_TOL)
            else:
                assert np.array_equal(bmm.get(), mov[0]) and np.array_equal(bmv.get(), mov[1])
            assert not acc.get().any(), "acc must be zero again"
    bx.unchanged(), bg.unchanged(), bb.unchanged()


# ---- GroupNormalization: stats (two inputs) -> finalize, partials -> finalize2 ---------------------------------------------------------------
GN_RUNS = nc.GN_RUNS
GN_IDS = [f"r{r}{'' if m == 'mixed' else m}" for r, m in GN_RUNS]


@pytest.mark.parametrize("r,mode", GN_RUNS, ids=GN_IDS)
@pytest.mark.parametrize("shape", nc.GN_SHAPES, ids=nc.shape_id)
def test_stats_into_groupnorm_finalize(dev, shape, r, mode):
    entry = "groupnorm_stats x 2 -> groupnorm_finalize" + ("" if mode == "mixed" else f" ({mode})")
    B, V, c1, c2, groups = shape
    c = c1 + c2
    x, gamma, beta = nc.stats_input(B, V, c, r, groups, mode)
    ref = nc.gn_reference(x, groups, gamma, beta)
    bg, bb = Guarded(gamma, dev, IN), Guarded(beta, dev, IN)
    acc = _zeros(dev, B, c, 2, dtype=np.float64)
    bufs = _stats(dev, x, c1, acc)
    moments = nc.rk.moments_acc(nc._t64(x)).numpy()
    got = acc.get()
    _hold(entry, r, "sums", got[..., 0], moments[..., 0], LAYER_TOL, final=False)
    _hold(entry, r, "sums of squares", got[..., 1], moments[..., 1], LAYER_TOL, final=False)
    scale, shift = _zeros(dev, B, c), _zeros(dev, B, c)
    _call("dm3d_groupnorm_finalize", acc.ptr, B, V, c, groups, EPS, bg.ptr, bb.ptr, scale.ptr, shift.ptr)
    _hold(entry, r, "scale", scale.get(), ref[0], LAYER_TOL)
    _hold(entry, r, "shift", shift.get(), ref[1], LAYER_TOL)
    assert not acc.get().any(), "acc must be zero again"
    for b in bufs + [bg, bb]:
        b.unchanged()


@pytest.mark.parametrize("r,mode", GN_RUNS, ids=GN_IDS)
@pytest.mark.parametrize("shape", nc.GN_SHAPES, ids=nc.shape_id)
def test_partials_into_groupnorm_finalize2(dev, shape, r, mode):
    entry = "groupnorm_partials -> groupnorm_finalize2" + ("" if mode == "mixed" else f" ({mode})")
    B, V, c1, c2, groups = shape
    c, slots = c1 + c2, -(-V // 64)
    x, gamma, beta = nc.stats_input(B, V, c, r, groups, mode)
    ref = nc.gn_reference(x, groups, gamma, beta)
    bar, model = nc.slot_bar(x, c1, groups, gamma, beta)
    bg, bb = Guarded(gamma, dev, IN), Guarded(beta, dev, IN)
    parts, bufs = [], []
    for lo, hi in ((0, c1), (c1, c)):
        bx = Guarded(x[..., lo:hi], dev, IN)
        p = Guarded(np.full((B, slots, hi - lo, 2), np.nan, np.float32), dev, OUT)          # every slot must be written
        _call("dm3d_groupnorm_partials", bx.ptr, B, V, hi - lo, p.ptr)
        _hold(entry, r, "partials", p.get(), nc.slot_partials(x[..., lo:hi], "f64"), LAYER_TOL, final=False)
        parts.append(p), bufs.append(bx)
    scale, shift = _zeros(dev, B, c), _zeros(dev, B, c)
    _call("dm3d_groupnorm_finalize2", parts[0].ptr, c1, parts[1].ptr, c2, B, V, groups, EPS, bg.ptr, bb.ptr, scale.ptr, shift.ptr)
    _hold(entry, r, "scale", scale.get(), ref[0], bar, model)
    _hold(entry, r, "shift", shift.get(), ref[1], bar, model)
    for b in bufs + [bg, bb]:
        b.unchanged()


# ---- gn_stats of a conv launch ------------------------------------------------------------------------------------------------------------------
def _ref_conv(x, k):
    import torch.nn.functional as F
    return F.conv3d(x.double().permute(0, 4, 1, 2, 3), k.double().permute(4, 3, 0, 1, 2), padding=1).permute(0, 2, 3, 4, 1)


# B, edge, cin, cout, must split: the smallest fused case of test_gpu_round4.py::test_conv_sums_groupnorm_statistics_of_its_output and the
# smallest Cin-split case of test_gpu_round5.py::test_cin_split_hand_over_against_float64 (direct kernel 16-way, B = 1)
CONV_CASES = [("fused", 2, 8, 32, 64, False), ("cin_split", 1, 8, 256, 256, True)]


@pytest.mark.parametrize("r", nc.CONV_R)
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_gn_stats_of_an_offset_output(dev, monkeypatch, case, r):
    from dm3d_amd import _lib, ops
    name, B, e, cin, cout, must_split = case
    entry = f"conv gn_stats ({name}) -> groupnorm_finalize2"
    for v in ("DM3D_CONV_WIDE_WGS", "DM3D_CONV_WINO_MINCHUNKS", "DM3D_CONV_WINO", "DM3D_CONV_WINO_SPLIT", "DM3D_CONV_KSPLIT", "DM3D_CONV_WINO_GRID"):
        monkeypatch.delenv(v, raising=False)
    groups, vox = 8, e ** 3
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, e, e, e, cin, generator=g)
    k = torch.randn(3, 3, 3, cin, cout, generator=g) * 0.05
    y0 = _ref_conv(x, k)                                                        # the bias-free output in float64
    std = y0.reshape(-1, cout).std(0, unbiased=False)
    sign = torch.where((torch.arange(cout) // (cout // groups)) % 2 == 1, -1.0, 1.0).double()      # constant within a group
    bias = (sign * r * std).float()
    wpk, w_exp = ops.pack_weights_h3(k.to(dev))
    slots = -(-vox // 64)
    gn = Guarded(np.full((B, slots, cout, 2), np.nan, np.float32), dev, OUT)     # every slot must be written
    gn_t = gn.t[PAD:PAD + gn.n].view(torch.float32).reshape(B, slots, cout, 2)
    assert gn_t.data_ptr() == gn.ptr
    kw = dict(bias=bias.to(dev), precision=_lib.PREC_H3, w_exp=w_exp)
    y = ops.conv3d(x.to(dev), wpk, cout, 3, gn_stats=gn_t, **kw)
    if must_split:
        assert not torch.equal(y, ops.conv3d(x.to(dev), wpk, cout, 3, split=False, **kw)), "the launch did not split"
    torch.cuda.synchronize()
    stored = y.cpu().numpy().reshape(B, vox, cout)
    _hold(entry, r, "output", stored, (y0 + bias.double()).numpy().reshape(B, vox, cout), 2e-5, final=False)
    part = gn.get()
    want = nc.rk.moments_acc(nc._t64(stored)).numpy()                            # float64 sums over the stored output
    got = part.astype(np.float64).sum(1)
    _hold(entry, r, "sums", got[..., 0], want[..., 0], LAYER_TOL, final=False)
    _hold(entry, r, "sums of squares", got[..., 1], want[..., 1], LAYER_TOL, final=False)
    rng = np.random.default_rng(r + cout)
    gamma, beta = (rng.random(cout) + 0.5).astype(np.float32), rng.standard_normal(cout).astype(np.float32)
    ref = nc.gn_reference(stored, groups, gamma, beta)
    bar, model = nc.slot_bar(stored, cout, groups, gamma, beta)
    bg, bb = Guarded(gamma, dev, IN), Guarded(beta, dev, IN)
    scale, shift = _zeros(dev, B, cout), _zeros(dev, B, cout)
    _call("dm3d_groupnorm_finalize2", gn.ptr, cout, None, 0, B, vox, groups, EPS, bg.ptr, bb.ptr, scale.ptr, shift.ptr)
    _hold(entry, r, "scale", scale.get(), ref[0], bar, model)
    _hold(entry, r, "shift", shift.get(), ref[1], bar, model)
    assert np.array_equal(gn.get().view(np.int32), part.view(np.int32))            # finalize2 only reads the partials


# ---- the row kernels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", R_VALUES)
@pytest.mark.parametrize("h2", [False, True], ids=["f32", "h2"])
@pytest.mark.parametrize("rows,c", nc.LN_SHAPES)
def test_layernorm3_rows_with_an_offset(dev, rows, c, h2, r):
    entry = "layernorm3_h2" if h2 else "layernorm3"
    x, _, params = nc.row_input(rows, c, r)
    model = nc.ln_forward_model_error(rows, c, r, "h2" if h2 else "f4")
    bar = nc.bar(ROW_TOL, model)
    bx = Guarded(x, dev, IN)
    pb = [(Guarded(g, dev, IN), Guarded(b, dev, IN)) for g, b in params]
    outs = [_zeros(dev, rows, c) for _ in params]
    args = []
    for (g, b), o in zip(pb, outs):
        args += [g.ptr, b.ptr, o.ptr]
    _call("dm3d_layernorm3_h2" if h2 else "dm3d_layernorm3", bx.ptr, rows, c, EPS, *args)
    for i, ((g, b), o) in enumerate(zip(params, outs)):
        got = h2_decode(o.get()) if h2 else o.get()
        _hold(entry, r, f"output {i}", got, nc.ln_reference(x, g, b), bar, model)
    bx.unchanged()
    for g, b in pb:
        g.unchanged(), b.unchanged()


@pytest.mark.parametrize("r", R_VALUES)
@pytest.mark.parametrize("rows,c", nc.LN_SHAPES)
def test_layernorm_bwd_rows_with_an_offset(dev, rows, c, r):
    x, dy, params = nc.row_input(rows, c, r)
    gamma = params[0][0]
    ref = nc.ln_bwd_reference(rows, c, r)
    models = nc.ln_bwd_model_errors(rows, c, r)
    bx, bdy, bg = Guarded(x, dev, IN), Guarded(dy, dev, IN), Guarded(gamma, dev, IN)
    dx, dg, db = _zeros(dev, rows, c), _zeros(dev, c), _zeros(dev, c)
    _call("dm3d_layernorm_bwd", bx.ptr, rows, c, EPS, bg.ptr, bdy.ptr, dx.ptr, dg.ptr, db.ptr)
    for what, o, f, m in zip(("dx", "dgamma", "dbeta"), (dx, dg, db), ref, models):
        _hold("layernorm_bwd", r, what, o.get(), f, nc.bar(ROW_TOL, m), m)
    bx.unchanged(), bdy.unchanged(), bg.unchanged()


# ---- dm3d_bn_act_bwd on the statistics of the chain ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", nc.BN_BWD_R)
def test_bn_act_bwd_on_the_statistics_of_an_offset_tensor(dev, r):
    entry = "groupnorm_stats -> batchnorm_finalize -> bn_act_bwd"
    rows, c1, c2 = nc.BN_BWD_SHAPE
    c = c1 + c2
    x, g, gamma, beta = nc.bn_bwd_input(r)
    bg, bb, bgo = Guarded(gamma, dev, IN), Guarded(beta, dev, IN), Guarded(g, dev, IN)
    acc = _zeros(dev, 1, c, 2, dtype=np.float64)
    b1, b2 = _stats(dev, x, c1, acc)
    st = [_zeros(dev, c) for _ in range(4)]                                        # scale, shift, mean, rstd
    _call("dm3d_batchnorm_finalize", acc.ptr, 1, rows, c, EPS, bg.ptr, bb.ptr, *(o.ptr for o in st), None, None, MOMENTUM, 1)
    for o, f, what in zip(st, nc.bn_reference(x, gamma, beta, None, 1), nc.BN_OUTPUTS):
        _hold(entry, r, what, o.get(), f, LAYER_TOL)
    red = _zeros(dev, c, 2, dtype=np.float64)
    dx1, dx2, dgam, dbet = _zeros(dev, rows, c1), _zeros(dev, rows, c2), _zeros(dev, c), _zeros(dev, c)
    _call("dm3d_bn_act_bwd", bgo.ptr, b1.ptr, c1, b2.ptr, c2, rows, *(o.ptr for o in st), nc.SILU, red.ptr, dx1.ptr, dx2.ptr, dgam.ptr, dbet.ptr)
    dx_ref, dgamma_ref, dbeta_ref, red_ref = nc.bn_bwd_reference(r)
    m_dx, m_dg, m_db, m_red = nc.bn_bwd_model_errors(r)
    _hold(entry, r, "dx", np.concatenate([dx1.get(), dx2.get()], 1), dx_ref, nc.bar(LAYER_TOL, m_dx), m_dx)
    _hold(entry, r, "dgamma", dgam.get(), dgamma_ref, nc.bar(LAYER_TOL, m_dg), m_dg)
    _hold(entry, r, "dbeta", dbet.get(), dbeta_ref, nc.bar(LAYER_TOL, m_db), m_db)
    _hold(entry, r, "red", red.get(), red_ref, nc.bar(LAYER_TOL, m_red), m_red)
    for b in (b1, b2, bg, bb, bgo):
        b.unchanged()


# ---- one layer of the training path ------------------------------------------------------------------------------------------------------------------
def test_trainer_bn_act_layer_on_offset_channels(dev):
    """Trainer.bn_act forward and backward on a two-input tensor whose channels sit at +-30 standard deviations, against float64 autograd
    and the moving-average rule of oracle/ref_train.py; built as tests/test_gpu_train.py::test_bn_act_gradients builds its layer, at its bars."""
    import dm3d_amd
    from dm3d_amd import _lib
    from dm3d_amd.train import Param, Trainer, Var
    from oracle import ref_train
    entry, r = "Trainer.bn_act", 30
    cfg = dm3d_amd.UNetConfig(img_size=4, img_channels=4, widths=(16,), has_attention=(False, False), num_res_blocks=1, first_conv_channels=16)
    tr = Trainer(cfg, dm3d_amd.synthetic_weights(cfg, seed=0), dev)
    tr.tape, tr._cache, tr.update_moving = [], {}, True

    def param(name, arr):
        w = torch.from_numpy(np.array(arr, np.float32)).to(dev)                     # a copy: the cached inputs are read-only
        tr.params[name] = Param(name, arr.shape, w.reshape(-1), torch.zeros(w.numel(), device=dev))

    B, S, c1, c2 = 3, 4, 8, 12
    c = c1 + c2
    x, gamma, beta = nc.stats_input(B, S ** 3, c, r)
    gout = torch.from_numpy(np.random.default_rng(31).standard_normal((B, S, S, S, c)).astype(np.float32))
    xt = torch.from_numpy(x.copy()).reshape(B, S, S, S, c)
    x1, x2 = xt[..., :c1].contiguous(), xt[..., c1:].contiguous()
    mm0, mv0 = torch.zeros(c), torch.ones(c)
    a, b2, ga, be = (t.clone().double().requires_grad_(True) for t in (x1, x2, torch.from_numpy(gamma.copy()), torch.from_numpy(beta.copy())))
    cat = torch.cat([a, b2], -1)
    mean, var = cat.mean((0, 1, 2, 3)), cat.var((0, 1, 2, 3), unbiased=False)
    y = torch.nn.functional.silu((cat - mean) / torch.sqrt(var + ref_train.rt.BN_EPS) * ga + be)
    y.backward(gout.double())
    moved = ref_train.moving_update({"n.mean": mm0.double(), "n.var": mv0.double()}, {"n": (mean.detach(), var.detach(), B * S ** 3)})
    param("n.gamma", gamma)
    param("n.beta", beta)
    tr.moving["n.mean"], tr.moving["n.var"] = mm0.to(dev), mv0.to(dev)
    v1, v2 = Var(x1.to(dev)), Var(x2.to(dev))
    out = tr.bn_act(v1, v2, "n", _lib.ACT_SILU)
    out.g = gout.to(dev)
    tr.backward()
    torch.cuda.synchronize()
    _hold(entry, r, "forward", out.v.cpu().numpy(), y.detach().numpy(), 1e-5)
    _hold(entry, r, "dx1", v1.g.cpu().numpy(), a.grad.numpy(), LAYER_TOL)
    _hold(entry, r, "dx2", v2.g.cpu().numpy(), b2.grad.numpy(), LAYER_TOL)
    _hold(entry, r, "dgamma", tr.params["n.gamma"].g.cpu().numpy(), ga.grad.numpy(), LAYER_TOL)
    _hold(entry, r, "dbeta", tr.params["n.beta"].g.cpu().numpy(), be.grad.numpy(), LAYER_TOL)
    _hold(entry, r, "moving mean", tr.moving["n.mean"].cpu().numpy(), moved["n.mean"].numpy(), 1e-5)
    _hold(entry, r, "moving var", tr.moving["n.var"].cpu().numpy(), moved["n.var"].numpy(), 1e-6)
