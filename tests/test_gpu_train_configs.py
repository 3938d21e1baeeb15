"""GPU parity of the training path (train.py, class Trainer: tape autograd over the HIP kernels) across build_model arguments:
loss, prediction, every gradient, BatchNormalization moving statistics, one Adam step and a second pass over the same batch, for each
case of tests/train_config_cases.py, against oracle/ref_train.py in float64.  tests/test_gpu_train.py checks the default network; the
graph Trainer differentiates changes with every argument (skip pushes and pops, tensors with two consumers, concat / alias /
upsample / stride-2 / attention closures, dm3d_wgrad and dm3d_colsum shapes), and this file walks those.

The metric and the bars are train_config_cases.grad_errors / live_bar / zero_bar: live tensors purely relative to their own largest
entry at max(1e-4, 8 cond), analytically zero tensors against the largest gradient entry overall at max(1e-7, 8 zcond), cond and zcond
being the float32 oracle's own errors, which tests/test_train_configs_host.py caps."""
import numpy as np
import pytest
import torch

import train_config_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _rel(a, ref):
    a, ref = torch.as_tensor(a).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("case", tc.CASES, ids=tc.CASE_IDS)
def test_training_parity_across_build_model_arguments(dev, case):
    import dm3d_amd
    from dm3d_amd.betas import BETAS_FIELDS
    from dm3d_amd.train import Trainer
    from oracle import ref_train as ot
    o = tc.oracle(case)
    cfg, W, B, lc = o["cfg"], o["W"], o["B"], o["lc"]
    lat, noise, t = o["lat"].to(dev), o["noise"].to(dev), o["t"]
    ids = None if o["ctx"] is None else o["ctx"].reshape(-1).numpy()
    grads_ref, loss_ref = o["grads64"], float(o["loss64"])
    tr = Trainer(cfg, W, dev)
    tab = dm3d_amd.Betas(tc.T_STEPS).device_tables(dev)
    betas = (tab[BETAS_FIELDS.index("sqrt_alpha_bar")], tab[BETAS_FIELDS.index("sqrt_one_minus_alpha_bar")])
    loss, pred = tr.loss_and_grad(lat, t, noise, ids, betas, tc.T_STEPS, B, lc)
    torch.cuda.synchronize()
    # loss and prediction: the bars of test_training_forward_loss_and_all_gradients
    lerr = abs(float(loss.item()) - loss_ref) / loss_ref
    perr = _rel(pred, o["pred64"])
    print(f"{case[0]}: loss {float(loss.item()):.8f} vs oracle {loss_ref:.8f} (rel {lerr:.2e}); pred rel err {perr:.2e}")
    assert tuple(pred.shape) == tuple(o["pred64"].shape)
    assert lerr < 1e-5 and perr < 1e-4
    # every gradient
    got = tr.grads()
    assert set(got) == set(grads_ref)
    live, zero, zset = tc.grad_errors(got, grads_ref)
    assert zset == o["zero_names"]
    print(f"{case[0]}: cond {o['cond']:.3e} ({o['cond_name']}) zcond {o['zcond']:.3e} ({o['zcond_name']}) | "
          f"device worst live {live[1]:.3e} at {live[0]}, worst zero {zero[1]:.3e} at {zero[0]}")
    assert live[1] <= tc.live_bar(o["cond"]), live
    assert zero[1] <= tc.zero_bar(o["zcond"]), zero
    # BatchNormalization moving statistics as Keras updates them
    st = tr.state_dict()
    assert o["moving64"]
    for name, ref in o["moving64"].items():
        assert _rel(st[name], ref) < 1e-5, name
    # a second pass over the same batch: zero_grad and the per-step cache leak nothing between steps, and the atomic order of
    # dm3d_wgrad's K split moves a gradient by rounding only (the bar of test_wgrad_and_dgrad_in_the_atomic_ksplit_regime).  The
    # analytically zero tensors are rounding noise in both passes: relative to themselves they need not agree, so they are held to
    # their own bar again instead.
    loss2, _ = tr.loss_and_grad(lat, t, noise, ids, betas, tc.T_STEPS, B, lc, update_moving=False)
    torch.cuda.synchronize()
    got2 = tr.grads()
    assert abs(float(loss2.item()) - loss_ref) / loss_ref < 1e-5
    again = max(((_rel(got2[k], got[k]), k) for k in got if k not in zset))
    live2, zero2, _ = tc.grad_errors(got2, grads_ref)
    print(f"{case[0]}: second pass differs from the first by {again[0]:.3e} at {again[1]}; worst live {live2[1]:.3e}, worst zero {zero2[1]:.3e}")
    assert again[0] < 1e-5, again
    assert live2[1] <= tc.live_bar(o["cond"]) and zero2[1] <= tc.zero_bar(o["zcond"]), (live2, zero2)
    # one Adam step (Keras defaults) from zero moments.  Live tensors: compared with the oracle's step where the gradient matters
    # (|g| > 1e-3 of the tensor's largest), 1e-5 absolute at lr 1e-4, as the default-config test does.  Zero tensors: the first step
    # is lr * g / (|g| + 1e-7), the oracle's g is ~1e-17 and the device's is float32 rounding noise of free sign and of a size that
    # can exceed Adam's epsilon (uncond_noattn_b1: time_mlp.0.kernel moves by 4.6e-5 where the oracle's stays), so against the oracle
    # they may differ by a whole step and by no more; what the kernel did with them is held instead to the float64 step of the
    # device's own gradient, at the same 1e-5.
    zeros = {k: torch.zeros_like(v) for k, v in grads_ref.items()}
    Wn, _, _ = ot.adam_step(o["W64"], grads_ref, zeros, zeros, 1, 1e-4)
    own = {k: torch.from_numpy(got2[k]).double() for k in zset}
    Wz, _, _ = ot.adam_step(o["W64"], own, zeros, zeros, 1, 1e-4)
    tr.adam_step()
    st = tr.state_dict()
    worst, worst_own = ("", 0.0), ("", 0.0)
    for k in Wn:
        new = torch.from_numpy(st[k]).double()
        if k in zset:
            d = float((new - Wz[k]).abs().max())
            worst_own = max(worst_own, (k, d), key=lambda p: p[1])
            assert d < 1e-5, (k, d)
            continue
        sel = grads_ref[k].abs() > 1e-3 * grads_ref[k].abs().max()
        assert sel.any()
        d = float((new - Wn[k]).abs()[sel].max())
        worst = max(worst, (k, d), key=lambda p: p[1])
        assert d < 1e-5, (k, d)
    moved = max((float(np.abs(st[k].astype(np.float64) - W[k].astype(np.float64)).max()), k) for k in zset)
    print(f"{case[0]}: after one Adam step max |w - w_ref| = {worst[1]:.3e} at {worst[0]}; zero tensors: moved by at most {moved[0]:.3e} "
          f"({moved[1]}), within {worst_own[1]:.3e} of the float64 step of their own gradient ({worst_own[0]})")
    assert moved[0] <= 1.01e-4, moved


def test_add_hands_each_input_a_gradient_of_its_own(dev):
    """Trainer.add's backward: "the first takes it, the second gets a copy".  In build_model's graph both inputs of every add have
    finished reading before anything accumulates into the shared buffer, so handing one buffer to both is invisible to every
    whole-network case above; the contract (Var.add_grad may accumulate into what it was given) is held here on the smallest tape
    where it matters: both inputs have a consumer recorded before the add, whose backward therefore runs after it and accumulates.
    Against the closed form in float64, at the per-layer bar of tests/test_gpu_train.py (2e-5)."""
    import dm3d_amd
    from dm3d_amd.train import Trainer, Var
    cfg = dm3d_amd.UNetConfig(img_size=4, img_channels=4, widths=(16,), has_attention=(False, False), num_res_blocks=1, first_conv_channels=16)
    tr = Trainer(cfg, dm3d_amd.synthetic_weights(cfg, seed=0), dev)
    tr.tape, tr._cache = [], {}
    g = torch.Generator().manual_seed(4)
    a, b, gu, gv, gs = (torch.randn(3, 4, 4, 4, 12, generator=g) for _ in range(5))
    ar, br = (x.clone().double().requires_grad_(True) for x in (a, b))
    (torch.nn.functional.silu(ar) * gu.double() + torch.nn.functional.silu(br) * gv.double() + (ar + br) * gs.double()).sum().backward()
    av, bv = Var(a.to(dev)), Var(b.to(dev))
    u, v = tr.silu(av), tr.silu(bv)
    s = tr.add(av, bv)
    assert _rel(s.v, a.double() + b.double()) < 1e-6
    u.g, v.g, s.g = gu.to(dev), gv.to(dev), gs.to(dev)
    tr.backward()
    torch.cuda.synchronize()
    errs = dict(da=_rel(av.g, ar.grad), db=_rel(bv.g, br.grad))
    print(errs)
    assert max(errs.values()) < 2e-5, errs
    assert av.g.data_ptr() != bv.g.data_ptr()


def test_trainer_refuses_attention_token_counts_the_gemm_cannot_take(dev):
    """12^3 with three levels has 3^3 = 27 tokens at the deepest level; the attention contractions of the training path run on the
    MFMA GEMM and dm3d_wgrad with rows of L floats read as float4, so L must be a multiple of 4, as on the sampling path
    (test_unet_other_latent_sizes).  Trainer says so when it is built: nothing is allocated and nothing is launched."""
    import dm3d_amd
    from dm3d_amd.train import Trainer
    bad = dm3d_amd.UNetConfig(img_size=12, img_channels=4, widths=(16, 32, 48), num_res_blocks=1, first_conv_channels=16)
    with pytest.raises(ValueError, match="tokens"):
        Trainer(bad, {}, dev)                       # (an empty state: the refusal comes before the weights are read)
