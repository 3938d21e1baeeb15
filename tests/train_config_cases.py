"""What the tests of the training path across build_model arguments share (plain helper, no test in it): the cases, their inputs,
the float64 / float32 oracle pair of each case (computed once per process, never modified) and the gradient metric.
tests/test_train_configs_host.py pins the inputs on the CPU; tests/test_gpu_train_configs.py holds the HIP path to them.

The cases.  Trainer walks weights.walk(cfg) generically, so every build_model argument changes the graph it differentiates: how many
skip tensors are pushed and popped, which tensors have two consumers, where the concat / alias / upsample / stride-2 / attention
backward closures sit and which dm3d_wgrad / dm3d_colsum shapes are launched.  Each case is
(id, img_size, img_channels, B, ctx ids or None, UNetConfig kwargs, weights seed); all use T = 50, global_bs = B, lc = img_channels.
Widths within a case are distinct (equal widths break the reference's own skip bookkeeping, see _random_unet_configs in
tests/test_gpu_unet.py).

The metric.  In training mode every bias that feeds a BatchNormalization has gradient exactly zero (conv1.bias, temb.bias, a key bias
under softmax, with B = 1 the whole time_mlp): the float64 oracle gives ~1e-17 for them, float32 arithmetic gives rounding noise, and a
relative comparison of noise with noise says nothing.  So grad_errors() splits the tensors by the float64 reference alone: *zero* where
max|ref_k| < 1e-9 of the largest gradient entry overall, *live* otherwise.  A live tensor's error is max|got_k - ref_k| / max|ref_k|,
relative to its own largest entry with no floor borrowed from other tensors; a zero tensor's error is max|got_k| relative to the
largest gradient entry overall.

The bars.  COND_CAP and ZCOND_CAP are conditions on the chosen inputs (the float32 oracle's own error under this metric; the six
cases were measured at 4e-6 ... 1.2e-5 and <= 4.5e-7): random weights can make a draw ill-conditioned (NEGATIVE_CONTROL: 9.5e-3), and
no fixed bar survives such a case.  The device bars are live_bar() / zero_bar(): the project's whole-network gradient bar 1e-4, or 8
times the float32 oracle's own error (the margin of test_unet_random_build_model_arguments) where that is larger; with the caps never
above 1.6e-4 / 8e-6."""
import functools
import os

import numpy as np
import torch

T_STEPS = 50
DATA_SEED = 11
ZERO_REL = 1e-9          # a tensor is zero when its largest reference entry is below this share of the largest entry overall
COND_CAP = 2e-5          # float32 oracle vs float64 oracle, live tensors: a condition on the inputs
ZCOND_CAP = 1e-6         # float32 oracle's zero tensors against the largest gradient entry: likewise

CASES = [
    ("narrow", 8, 4, 2, (1, 0), dict(widths=(32, 64), has_attention=(False, True), num_res_blocks=1, first_conv_channels=16), 3),
    ("odd_widths", 8, 4, 3, (1, 0, 1), dict(widths=(48, 80, 112), has_attention=(True, False, True), num_res_blocks=1), 3),
    ("single_level", 4, 8, 2, (1, 0), dict(widths=(64,), has_attention=(True,), num_res_blocks=3), 3),
    ("uncond_noattn_b1", 8, 1, 1, None, dict(widths=(64, 128), has_attention=(False, False), num_res_blocks=2, conditional=False,
                                             first_conv_channels=64), 3),
    ("uncond_attn", 8, 4, 2, None, dict(widths=(32, 48), has_attention=(True, True), num_res_blocks=1, conditional=False,
                                        first_conv_channels=32), 3),
    ("dup_ctx", 4, 4, 3, (1, 0, 1), dict(widths=(16, 32), has_attention=(False, True), num_res_blocks=2, first_conv_channels=16), 3),
]
CASE_IDS = [c[0] for c in CASES]
# the ill-conditioned draw the caps exist for: single_level's network at 8^3 x 8 (512 tokens).  Host only, never run on the device.
NEGATIVE_CONTROL = ("single_level_8cube", 8, 8, 2, (1, 0), dict(widths=(64,), has_attention=(True,), num_res_blocks=3), 3)

for _c in CASES + [NEGATIVE_CONTROL]:
    assert len(set(_c[5]["widths"])) == len(_c[5]["widths"]), _c[0]


def case_inputs(case):
    """The case's weights (float32 NumPy, as synthetic_weights draws them) and data: latents, noise, t drawn in that order from one
    seeded generator; ctx as the oracle takes it ([B, 1, 1] int64) or None."""
    import dm3d_amd
    _, size, ch, B, ids, kw, seed = case
    cfg = dm3d_amd.UNetConfig(img_size=size, img_channels=ch, **kw)
    g = torch.Generator().manual_seed(DATA_SEED)
    lat = torch.randn(B, size, size, size, ch, generator=g)
    noise = torch.randn(B, size, size, size, ch, generator=g)
    t = torch.randint(0, T_STEPS, (B,), generator=g)
    ctx = None if ids is None else torch.tensor(ids, dtype=torch.int64).reshape(B, 1, 1)
    assert (ctx is not None) == cfg.conditional, case[0]
    return dict(cfg=cfg, W=dm3d_amd.synthetic_weights(cfg, seed=seed), lat=lat, noise=noise, t=t, ctx=ctx, B=B, lc=ch)


@functools.lru_cache(maxsize=None)
def _oracle(case_id):
    from oracle import ref_torch as rt, ref_train as ot
    case = next(c for c in CASES + [NEGATIVE_CONTROL] if c[0] == case_id)
    inp = case_inputs(case)
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    ocfg = rt.UNetConfig(img_size=case[1], img_channels=case[2], **case[5])
    ob = rt.Betas(T_STEPS)
    out = dict(inp)
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        W = {k: torch.from_numpy(v).to(dt) for k, v in inp["W"].items()}
        stats = {}
        loss, grads, pred = ot.loss_and_grads(W, ocfg, ob, inp["lat"].to(dt), inp["t"], inp["noise"].to(dt), inp["ctx"], inp["B"], inp["lc"],
                                              stats=stats)
        out[f"loss{tag}"], out[f"grads{tag}"], out[f"pred{tag}"] = loss, grads, pred
        if tag == "64":
            out["W64"], out["moving64"] = W, ot.moving_update(W, stats)
    live, zero, zset = grad_errors(out["grads32"], out["grads64"])
    out["cond"], out["cond_name"], out["zcond"], out["zcond_name"], out["zero_names"] = live[1], live[0], zero[1], zero[0], zset
    return out


def oracle(case):
    """The inputs of case_inputs() plus, from oracle/ref_train.py: loss64 / grads64 / pred64 / W64 / moving64 (float64 weights and data),
    loss32 / grads32 / pred32 (float32), and the float32 oracle's own error under grad_errors(): cond, zcond (with cond_name,
    zcond_name) and zero_names.  One evaluation per process, shared by every test that asks: treat it as read-only."""
    return _oracle(case[0])


def grad_errors(got, ref64):
    """((worst live name, error), (worst zero name, error), frozenset of the zero names); see the module docstring."""
    ref = {k: torch.as_tensor(v).double() for k, v in ref64.items()}
    gmax = max(float(r.abs().max()) for r in ref.values())
    live, zero, zset = ("", 0.0), ("", 0.0), set()
    for name, r in ref.items():
        g = torch.as_tensor(got[name]).double().cpu().reshape(r.shape)
        rmax = float(r.abs().max())
        if rmax < ZERO_REL * gmax:
            zset.add(name)
            e = float(g.abs().max()) / gmax
            if e > zero[1] or not zero[0]:
                zero = (name, e)
        else:
            e = float((g - r).abs().max()) / rmax
            if e > live[1] or not live[0]:
                live = (name, e)
    return live, zero, frozenset(zset)


def live_bar(cond):
    return max(1e-4, 8 * cond)


def zero_bar(zcond):
    """1e-7 is what tests/test_gpu_train.py's _compare_grads allows such a tensor in effect: 1e-4 of its 1e-3 * gmax floor."""
    return max(1e-7, 8 * zcond)


def required_zero_names(case, names):
    """What the analysis says must be zero: conv1.bias (norm2 follows conv1 + temb) and temb.bias of every res block; with B = 1
    the per-sample time vector is one constant per channel over the whole batch, so all of time_mlp as well."""
    need = {n for n in names if n.endswith((".conv1.bias", ".temb.bias"))}
    if case[3] == 1:
        need |= {n for n in names if n.startswith("time_mlp.")}
    return need


def conv_kernel_names(cfg):
    """Every Conv3D kernel of the network (rank 5 in the Keras layout): none of them may be classified zero."""
    from dm3d_amd.weights import param_spec
    return {n for n, shape in param_spec(cfg).items() if n.endswith(".kernel") and len(shape) == 5}
