"""CPU tier of the offset-tensor cases (tests/norm_offset_cases.py): the float32 models of the statistics and row kernels against the
float64 references, with no kernel in the loop.  The errors measured here are what the bars of tests/test_gpu_norm_offsets.py are built
from; tests/golden/norm_offset_model_errors.json pins them, so a changed model cannot quietly loosen a bar
(`PYTHONPATH=. python tests/norm_offset_cases.py` rewrites the file; the diff is then there to be reviewed).  Every figure is printed."""
import numpy as np
import pytest

import norm_offset_cases as nc
from norm_offset_cases import LAYER_TOL, ROW_TOL, R_VALUES


@pytest.fixture(scope="module")
def errors():
    e = nc.model_errors()
    for k in sorted(e):
        print(f"{k}: {e[k]:.2e}")
    return e


def test_model_errors_are_the_recorded_ones(errors):
    """Each model's error per (kernel, shape, r) equals the committed record: to 2 % where it is a float32 effect, and below 1e-8 where the
    record is below 1e-8 (float64-ordered models: their last digits depend on the summation order of the reference)."""
    rec = nc.recorded_model_errors()
    assert sorted(rec) == sorted(errors)
    for k, v in errors.items():
        if rec[k] < 1e-8:
            assert v < 1e-8, (k, v, rec[k])
        else:
            assert abs(v - rec[k]) <= 0.02 * rec[k], (k, v, rec[k])


def test_float64_ordered_statistics_model_holds_at_every_offset(errors):
    """groupnorm_stats_kernel as it stands (float64 per-thread sums): under LAYER_TOL / 2 up to r = 1000 for every statistics shape, into
    dm3d_batchnorm_finalize and into dm3d_groupnorm_finalize.  Its bar is therefore LAYER_TOL at every offset."""
    for k, v in errors.items():
        if k.startswith(("bn_chain64/", "gn_chain64/")):
            assert v < LAYER_TOL / 2, (k, v)
            assert nc.bar(LAYER_TOL, v) == LAYER_TOL


def test_float32_slot_model_leaves_the_bar_at_ratio_100(errors):
    """The negative control: 64-voxel float32 slots (dm3d_groupnorm_partials, gn_stats) do not stay under LAYER_TOL at r = 100 at any shape:
    the reason the slot path's bar is a curve in r and not a constant."""
    for shape in nc.GN_SHAPES:
        v = errors[f"gn_slot32/{nc.shape_id(shape)}/r100"]
        assert v > LAYER_TOL, (shape, v)
        assert errors[f"gn_slot32/{nc.shape_id(shape)}/r0"] < LAYER_TOL / 2


def test_lattice_case_tells_a_float32_finalize2_from_a_float64_one(errors):
    """Integer noise on an offset of 150: the float32 slots are exact (model error 0, bar LAYER_TOL), and adding the slots and channels in
    float32 instead of float64 leaves the bar wherever the total needs more than 24 bits (47 slots x 25 channels; 2 slots x 32 channels)."""
    for shape in nc.GN_SHAPES:
        tag = f"{nc.shape_id(shape)}/r100lattice"
        assert errors[f"gn_slot32/{tag}"] == 0.0 and errors[f"gn_chain64/{tag}"] < 1e-12
        if shape[1] * (shape[2] + shape[3]) // shape[4] > 2000:
            assert errors[f"gn_slot32_sum32/{tag}"] > 10 * LAYER_TOL, (tag, errors[f"gn_slot32_sum32/{tag}"])


def test_float32_chain_model_is_what_the_float64_sums_replaced(errors):
    """The per-thread float32 sums groupnorm_stats_kernel kept before: inside the bar at r <= 10, outside it at r = 1000 at every shape (and at
    r = 100 for every BatchNormalization shape)."""
    for shape in nc.BN_SHAPES:
        sid = nc.shape_id(shape)
        assert errors[f"bn_chain32/{sid}/r10"] < LAYER_TOL and errors[f"bn_chain32/{sid}/r100"] > LAYER_TOL and errors[f"bn_chain32/{sid}/r1000"] > LAYER_TOL
    for shape in nc.GN_SHAPES:
        sid = nc.shape_id(shape)
        assert errors[f"gn_chain32/{sid}/r10"] < LAYER_TOL and errors[f"gn_chain32/{sid}/r1000"] > LAYER_TOL


def test_one_channel_offset_is_spread_not_offset(errors):
    """One channel of a group carrying the offset raises the group's variance with it: no cancellation, every model stays inside the bar."""
    for k, v in errors.items():
        if k.endswith("one") and "sum32" not in k:
            assert v < LAYER_TOL / 2, (k, v)


def test_one_pass_layernorm_is_told_apart_from_two_pass(errors):
    """E[x^2] - m^2 in float32 exceeds the bar built from the two-pass model at every r >= 30 and every shape, for both lane layouts; at r = 0
    it does not (which is why the suite could not see such a rewrite before)."""
    for rows, c in nc.LN_SHAPES:
        for r in R_VALUES:
            tag = f"{rows}x{c}/r{r}"
            one = errors[f"ln_one_pass/{tag}"]
            for form in ("f4", "h2"):
                b = nc.bar(ROW_TOL, errors[f"ln_two_pass_{form}/{tag}"])
                print(f"layernorm {tag} {form}: one-pass {one:.2e}, two-pass bar {b:.2e}")
                assert one > b if r >= 30 else (one < b or r == 10), (tag, form, one, b)      # r = 10: already over at some shapes


def test_two_pass_model_at_zero_offset_is_inside_the_existing_bar(errors):
    """At r = 0 every row model is inside ROW_TOL / 4: the bars of the offset cases start from the existing ones."""
    for k, v in errors.items():
        if k.startswith(("ln_two_pass", "ln_bwd")) and k.endswith("/r0"):
            assert 4 * v < ROW_TOL, (k, v)


def test_stats_launch_arithmetic():
    """The slab and voxel-lane arithmetic of dm3d_groupnorm_stats the chain model restates, at the shapes the cases were chosen for."""
    assert nc.stats_launch(37, 20) == (1, 37, 51)
    assert nc.stats_launch(321, 12) == (1, 321, 85)                  # 85 * 3 = 255 threads: one idle
    assert nc.stats_launch(3000, 36) == (6, 500, 28)
    assert nc.stats_launch(4096, 1028) == (64, 64, 1)                # c/4 = 257 > 256: the quad loop runs twice
    assert nc.stats_launch(32 ** 3, 32) == (64, 512, 32)             # the training shapes: 16 ... 128 voxels per thread
    assert nc.stats_launch(8 ** 3, 512) == (16, 32, 2)


def test_models_agree_with_float64_on_exactly_representable_input():
    """Small integers: every sum is exact in float32, so each model must return the float64 sums bit for bit (a model that skipped or
    repeated a voxel, a slab or a lane would not)."""
    rng = np.random.default_rng(0)
    for B, V, c in nc.BN_SHAPES[:3] + [(1, 200, 1028)]:
        x = rng.integers(-3, 4, (B, V, c)).astype(np.float32)
        ref = nc.rk.moments_acc(nc._t64(x)).numpy()
        for dtype in (np.float32, np.float64):
            assert np.array_equal(nc.stats_chain(x, dtype), ref)
        assert np.array_equal(nc.partials_to_acc(nc.slot_partials(x, "f32"), None), ref)
        assert np.array_equal(nc.slot_partials(x, "f32").astype(np.float64), nc.slot_partials(x, "f64"))
    for rows, c in nc.LN_SHAPES:
        x = rng.integers(-3, 4, (rows, c)).astype(np.float32)
        x[:, 0] -= x.sum(1)                                           # integer rows of mean 0: mean and squared deviations are exact
        var = (x.astype(np.float64) ** 2).mean(1)
        for form in ("f4", "h2"):
            mean, rstd = nc.ln_stats(x, form)
            assert not mean.any()
            assert np.allclose(rstd, 1 / np.sqrt(var + nc.EPS), rtol=3e-7, atol=0)
