"""The training entries with a bitwise contract against bits recorded on the GPU from the build before their kernels were merged
(tests/golden/train_bits.npz, written by tests/golden/make_train_bits.py, which also holds the cases and runs them): dm3d_adam_ema,
dm3d_adam_scaled, dm3d_grad_scale, dm3d_objective_loss_grad and dm3d_guide_update with a rescale.  The cross-form tests of
test_gpu_clip.py and test_gpu_ema.py compare instantiations of one kernel with each other; this file says that none of them moved.
Every buffer sits between the sentinel pads of tests/guarded_buffers.py.  The CPU test at the end holds the recording itself against
the float64 references, so that a recording made from a broken build cannot become the standard."""
import importlib.util
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_train_bits", os.path.join(HERE, "golden", "make_train_bits.py"))
mtb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mtb)

ELEM_TOL = 1e-6                          # test_adam_three_steps' bar
ULP2 = 2.0 ** -22                        # test_norm_and_factor's bar


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(HERE, "golden", "train_bits.npz")) as f:
        return {k: f[k] for k in f.files}


def _of(recorded, case_id):
    return {k.split("/", 1)[1]: v for k, v in recorded.items() if k.split("/", 1)[0] == case_id}


def test_the_recording_holds_every_case_and_nothing_else(recorded):
    assert {k.split("/", 1)[0] for k in recorded} == set(mtb.CASES)
    for case_id in mtb.CASES:
        assert int(recorded[f"{case_id}/seed"]) == mtb.seed_of(case_id), case_id


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", list(mtb.CASES))
def test_recorded_bits_replay(recorded, case_id):
    """Equal words, or equal digests where the case stores those; run_case asserts that pads and inputs are untouched."""
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    want = _of(recorded, case_id)
    got = mtb.run_case(torch.device("cuda:0"), case_id, int(want.pop("seed")))
    assert set(got) == set(want), case_id
    for k, v in got.items():
        assert v.dtype == want[k].dtype and v.shape == want[k].shape, (case_id, k, v.dtype, v.shape)
        assert np.array_equal(v, want[k]), f"{case_id}: {k} differs from the recording in {int((v != want[k]).sum())} of {v.size} words"


def _err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all()
    return float(np.abs(got - ref).max() / max(float(np.abs(ref).max()), 1e-30))


@pytest.mark.parametrize("case_id", [c for c, s in mtb.CASES.items() if s["kind"] == "adam" and not s["digest"]])
def test_recorded_adam_agrees_with_the_reference(recorded, case_id):
    """w, m, v of every Adam case stored in full against oracle/ref_kernels.py's float64 adam on the regenerated inputs fed
    float32(state[1]) * g, at test_adam_three_steps' bar; a skipped step left every buffer bitwise as it was."""
    from oracle import ref_kernels as rk
    spec, rec = mtb.CASES[case_id], _of(recorded, case_id)
    start, grads, lr_ts = mtb.adam_inputs(spec["n"], int(rec["seed"]))
    if spec["variant"] == "scaled_skip":
        for k in ("w", "m", "v", "ema"):
            assert np.array_equal(rec[k], mtb.pack(start[k])), k
        return
    s = np.float32(1.0) if spec["variant"] == "ema" else mtb.adam_state(spec["variant"])[1]
    w, m, v = (torch.from_numpy(start[k].astype(np.float64)) for k in ("w", "m", "v"))
    b1, b2, eps = (float(np.float32(c)) for c in (mtb.B1, mtb.B2, mtb.EPS))     # the float32 values the entry receives, as there
    for g, lr_t in zip(grads, lr_ts):
        w, m, v = rk.adam(w, torch.from_numpy((s * g).astype(np.float64)), m, v, lr_t, b1, b2, eps)
    errs = dict(m=_err(rec["m"].view(np.float32), m.numpy()), v=_err(rec["v"].view(np.float32), v.numpy()),
                step=_err(rec["w"].view(np.float32).astype(np.float64) - start["w"], w.numpy() - start["w"]))
    print(f"{case_id}: {errs}")
    assert max(errs.values()) < ELEM_TOL, errs
    assert ("ema" in rec) == (spec["variant"] != "scaled_plain")
    if "ema" in rec:                                         # the last rate is 0 and the one before 0.25: the average is neither start nor w
        assert np.isfinite(rec["ema"].view(np.float32)).all() and not np.array_equal(rec["ema"], mtb.pack(start["ema"]))


@pytest.mark.parametrize("case_id", [c for c, s in mtb.CASES.items() if s["kind"] == "grad_scale"])
def test_recorded_norm_agrees_with_float64(recorded, case_id):
    """state[0] = pre_scale * sqrt(sum g^2) in float64 numpy within two float32 ulps (state is stored in full in every case)."""
    spec, rec = mtb.CASES[case_id], _of(recorded, case_id)
    g = mtb.norm_inputs(spec["n"], int(rec["seed"])).astype(np.float64)
    want = spec["pre"] * float(np.sqrt(np.sum(g * g)))
    st = rec["state"].view(np.float32)
    err = abs(float(st[0]) - want) / want
    print(f"{case_id}: norm error {err:.2e} (bound {ULP2:.2e})")
    assert err <= ULP2 and float(st[2]) == 0.0 and float(st[3]) == 0.0
