"""CPU tier: the inputs of tests/test_gpu_train_configs.py are pinned here, not the kernels.  For every case of
tests/train_config_cases.py the float32 oracle must sit within COND_CAP of the float64 one on the live gradient tensors and within
ZCOND_CAP (of the largest gradient entry) on the analytically zero ones: the device bars are max(1e-4, 8 cond) / max(1e-7, 8 zcond),
and these caps keep them from going loose on an ill-conditioned draw.  The zero / live classification is pinned from both sides:
it must contain what the analysis says is zero, and it must contain no conv kernel."""
import pytest

import train_config_cases as tc


@pytest.mark.parametrize("case", tc.CASES, ids=tc.CASE_IDS)
def test_case_is_well_conditioned_and_classified(case):
    o = tc.oracle(case)
    print(f"{case[0]}: cond {o['cond']:.3e} at {o['cond_name']}; zcond {o['zcond']:.3e} at {o['zcond_name']}; "
          f"{len(o['zero_names'])} zero tensors of {len(o['grads64'])}")
    assert set(o["grads32"]) == set(o["grads64"])
    assert o["cond"] <= tc.COND_CAP, (o["cond_name"], o["cond"])
    assert o["zcond"] <= tc.ZCOND_CAP, (o["zcond_name"], o["zcond"])
    need = tc.required_zero_names(case, o["grads64"])
    blocks = {n.rsplit(".", 2)[0] for n in o["grads64"] if n.endswith(".conv1.kernel")}
    assert len(need) >= 2 * len(blocks) and blocks, "every res block has a conv1.bias and a temb.bias"
    if case[0] == "uncond_noattn_b1":
        assert {"time_mlp.0.kernel", "time_mlp.0.bias", "time_mlp.1.kernel", "time_mlp.1.bias"} <= need
    assert need <= o["zero_names"], sorted(need - o["zero_names"])
    kernels = tc.conv_kernel_names(o["cfg"])
    assert kernels and kernels <= set(o["grads64"])
    assert not (kernels & o["zero_names"]), sorted(kernels & o["zero_names"])


def test_the_cap_rejects_an_ill_conditioned_draw():
    """Negative control: single_level's network at 8^3 x 8 with the same weights seed has 512-token attention whose softmax
    saturates; the float32 and float64 oracles differ by 9.5e-3 on up0.attn0.proj_in.kernel.  Such a case must not pass the cap."""
    o = tc.oracle(tc.NEGATIVE_CONTROL)
    print(f"negative control: cond {o['cond']:.3e} at {o['cond_name']}; zcond {o['zcond']:.3e} at {o['zcond_name']}")
    assert o["cond"] > tc.COND_CAP


def test_trainer_refuses_27_tokens_before_it_touches_a_device():
    """The refusal of tests/test_gpu_train_configs.py comes before the device is even asked for: it holds on a machine without one."""
    import dm3d_amd
    from dm3d_amd.train import Trainer
    bad = dm3d_amd.UNetConfig(img_size=12, img_channels=4, widths=(16, 32, 48), num_res_blocks=1, first_conv_channels=16)
    with pytest.raises(ValueError, match="27 tokens"):
        Trainer(bad, {}, "cuda:0")


def test_grad_errors_metric():
    """The metric on hand-made tensors: a live tensor is judged against its own largest entry (no floor from the others), a zero
    tensor against the largest entry overall, and the classification follows the reference alone."""
    import torch
    ref = {"big": torch.tensor([100.0, -50.0]), "small": torch.tensor([1e-4, 2e-4]), "zero": torch.tensor([1e-15, 0.0])}
    got = {"big": torch.tensor([100.0, -50.01]), "small": torch.tensor([1e-4, 2.2e-4]), "zero": torch.tensor([0.0, 3e-6])}
    live, zero, zset = tc.grad_errors(got, ref)
    assert zset == {"zero"}
    assert live[0] == "small" and live[1] == pytest.approx(0.1, rel=1e-6)
    assert zero[0] == "zero" and zero[1] == pytest.approx(3e-8, rel=1e-6)
    assert tc.live_bar(0.0) == 1e-4 and tc.live_bar(tc.COND_CAP) == pytest.approx(1.6e-4)
    assert tc.zero_bar(0.0) == 1e-7 and tc.zero_bar(tc.ZCOND_CAP) == pytest.approx(8e-6)
