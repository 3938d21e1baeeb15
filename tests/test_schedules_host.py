"""schedules.py: the host arithmetic diffusion.py re-exports, and the per-volume helper its two table builders share."""
import numpy as np
import pytest
import torch


def test_diffusion_reexports_every_public_name():
    from dm3d_amd import diffusion, schedules
    public = [n for n, v in vars(schedules).items()                      # what the module defines: its functions and FLOAT32_MAX
              if not n.startswith("_") and (getattr(v, "__module__", None) == schedules.__name__ or isinstance(v, float))]
    assert set(public) >= {"ddim_timesteps", "ddim_coefficients", "dpm_coefficients", "threshold_rank", "FLOAT32_MAX", "threshold_tables",
                           "edit_steps", "edit_levels", "latent_mask", "context_dropout", "guide_tables"}
    for name in public + ["_indices"]:
        assert getattr(diffusion, name) is getattr(schedules, name), name
    assert diffusion.DiffusionModel._guide_tables is schedules.guide_tables


def test_per_volume_helper_keeps_both_messages_under_both_callers():
    from dm3d_amd.schedules import _per_volume, guide_tables, threshold_tables
    calls = {"dynamic_threshold": lambda v: threshold_tables(2, 64, v), "threshold_max": lambda v: threshold_tables(2, 64, 0.9, v),
             "guidance_scale": lambda v: guide_tables(2, v, 0.0), "guidance_rescale": lambda v: guide_tables(2, 2.0, v)}
    for name, call in calls.items():
        with pytest.raises(ValueError) as e:
            call([0.5, 0.5, 0.5])
        assert str(e.value) == f"{name} must hold one value or one per volume (2), got 3"
        for bad in (float("nan"), [0.5, float("inf")], torch.tensor([float("nan"), 0.5])):
            with pytest.raises(ValueError) as e:
                call(bad)
            assert str(e.value) == f"{name} must be finite"
    a = _per_volume("x", torch.tensor([0.25]), 3)
    assert a.dtype == np.float64 and a.tolist() == [0.25] * 3
    assert _per_volume("x", [1, 2, 3], 3).tolist() == [1.0, 2.0, 3.0]
