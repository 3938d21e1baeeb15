"""CPU tier of v- / x0-prediction and min-SNR loss weighting: the dm3d_pred_to_eps and dm3d_objective_loss_grad ABI and their host
checks, the prediction and objective tables against an independent float64 restatement, the identities that tie them together, the
argument rules of the constructor and compile(), and the meta/prediction entry of checkpoints (no kernel is launched)."""
import ctypes
import inspect
import math
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRED_FIELDS = ("pred", "x", "out", "table", "t_idx", "batch", "per_sample", "timesteps")
LOSS_FIELDS = ("pred", "noise", "x0", "coef", "dpred", "partials", "loss_rows", "loss", "batch", "per_sample", "inv_divisor")


def _model(conditional=True, seed=0, **kw):
    from dm3d_amd.networks import conditional_dm3d, dm3d
    args = SimpleNamespace(timesteps=20, num_gpus=1, kernel_resize=False, bs=2)
    mod = conditional_dm3d if conditional else dm3d
    return mod.DiffusionModel(8, 1024, 4, None, args, device="cpu", seed=seed, **kw)


def test_entries_are_declared_exported_and_bound(built_library):
    from dm3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dm3d.h")).read()
    assert re.search(r"\bint\s+dm3d_pred_to_eps\s*\(const dm3d_pred_desc\* d, void\* stream\);", header)
    assert re.search(r"\bint\s+dm3d_objective_loss_grad\s*\(const dm3d_loss_desc\* d, void\* stream\);", header)
    handle = ctypes.CDLL(built_library)
    for name, desc in (("dm3d_pred_to_eps", _lib.PredDesc), ("dm3d_objective_loss_grad", _lib.LossDesc)):
        assert hasattr(handle, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == 2 and args[0]._type_ is desc and args[1] is ctypes.c_void_p
    assert _lib.lib().dm3d_version() == _lib.ABI_VERSION == 111                         # additive: the version stays


def test_struct_layouts_agree_with_a_c99_translation_unit(built_library, tmp_path):
    from dm3d_amd import _lib
    assert PRED_FIELDS == tuple(n for n, _ in _lib.PredDesc._fields_) and LOSS_FIELDS == tuple(n for n, _ in _lib.LossDesc._fields_)
    offs = [f"offsetof(dm3d_pred_desc, {f})" for f in PRED_FIELDS] + [f"offsetof(dm3d_loss_desc, {f})" for f in LOSS_FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dm3d.h"\nint main(void){printf("%d %zu %zu' + " %zu" * len(offs)
                   + '\\n", DM3D_LOSS_PARTIAL_BLOCKS, sizeof(dm3d_pred_desc), sizeof(dm3d_loss_desc), ' + ", ".join(offs) + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == _lib.LOSS_PARTIAL_BLOCKS == 64
    assert vals[1:3] == [ctypes.sizeof(_lib.PredDesc), ctypes.sizeof(_lib.LossDesc)]
    assert vals[3:] == [getattr(_lib.PredDesc, f).offset for f in PRED_FIELDS] + [getattr(_lib.LossDesc, f).offset for f in LOSS_FIELDS]


def _refusals(call, make, ok, bad, tag):
    """Every override of ``bad`` makes ``call`` return DM3D_EINVAL with a fresh message that names the entry (the pointers are made-up
    addresses nothing may dereference: a launch would fail differently, with DM3D_EHIP, on a machine without a device)."""
    from dm3d_amd import _lib
    L = _lib.lib()
    failures = []
    for override, what in bad:
        d = make()
        for k, v in {**ok, **override}.items():
            setattr(d, k, v)
        L.dm3d_fill(None, 0, 0.0, None)                             # leaves a known message behind
        stale = L.dm3d_last_error()
        rc = call(ctypes.byref(d), None)
        msg = L.dm3d_last_error()
        if rc != -1 or not msg or msg == stale or tag not in msg:
            failures.append(f"{tag.decode()}({what}): rc {rc}, message {msg!r}")
    assert not failures, "\n".join(failures)


def test_pred_to_eps_refuses_bad_arguments(built_library):
    from dm3d_amd import _lib
    L = _lib.lib()
    assert L.dm3d_pred_to_eps(None, None) == -1 and b"null descriptor" in L.dm3d_last_error()
    n = 3 * 1004 * 4                                                # bytes of one tensor of the descriptor below
    ok = dict(pred=0x100000, x=0x200000, out=None, table=0x300000, t_idx=0x400000, batch=3, per_sample=1004, timesteps=1000)
    bad = [({k: None}, f"{k} null") for k in ("pred", "x", "table", "t_idx")]
    bad += [({k: ok[k] + 4}, f"{k} misaligned") for k in ("pred", "x")] + [(dict(out=0x500004), "out misaligned")]
    bad += [(dict(table=ok["table"] + 2), "table misaligned"), (dict(t_idx=ok["t_idx"] + 1), "t_idx misaligned")]
    bad += [(dict(per_sample=v), f"per_sample {v}") for v in (6, 1002, 0, -4)]
    bad += [(dict(batch=v), f"batch {v}") for v in (0, -1, 65536)]
    bad += [(dict(timesteps=v), f"timesteps {v}") for v in (0, -5)]
    bad += [(dict(out=ok["pred"] + 16), "out inside pred"), (dict(out=ok["pred"] - 16), "out ends inside pred"),
            (dict(out=ok["x"] + n - 16), "out begins in x's last float4"), (dict(out=ok["x"] - n + 16), "out ends in x's first float4"),
            (dict(x=ok["pred"] + 16), "in place with x inside pred")]
    _refusals(L.dm3d_pred_to_eps, _lib.PredDesc, ok, bad, b"pred_to_eps")


def test_objective_loss_grad_refuses_bad_arguments(built_library):
    from dm3d_amd import _lib
    L = _lib.lib()
    assert L.dm3d_objective_loss_grad(None, None) == -1 and b"null descriptor" in L.dm3d_last_error()
    ok = dict(pred=0x100000, noise=0x200000, x0=0x300000, coef=0x400000, dpred=0x500000, partials=0x600000, loss_rows=0x700000,
              loss=0x800000, batch=3, per_sample=1004, inv_divisor=1.0 / 2048)
    ptrs = ("pred", "noise", "x0", "coef", "partials", "loss_rows", "loss")
    bad = [({k: None}, f"{k} null") for k in ptrs] + [({k: ok[k] + 4}, f"{k} misaligned") for k in ptrs + ("dpred",)]
    bad += [(dict(per_sample=v), f"per_sample {v}") for v in (6, 1002, 0, -4)]
    bad += [(dict(batch=v), f"batch {v}") for v in (0, -1, 65536)]
    bad += [(dict(inv_divisor=v), f"inv_divisor {v}") for v in (float("nan"), float("inf"))]
    bad += [(dict(dpred=ok[k]), f"dpred == {k}") for k in ("pred", "noise", "x0")] + [(dict(dpred=ok["noise"] + 16), "dpred inside noise")]
    _refusals(L.dm3d_objective_loss_grad, _lib.LossDesc, ok, bad, b"objective_loss_grad")


# ---- the host arithmetic -------------------------------------------------------------------------------------------------------
def _alpha_bar(T):
    from dm3d_amd.betas import Betas
    return np.asarray(Betas(T).alpha_bar, dtype=np.float32)


def _within_one_ulp(got, want64):
    """``got`` (float32) against a float64 value: at most one float32 ulp of the value apart."""
    got = np.asarray(got)
    assert got.dtype == np.float32
    want32 = np.asarray(want64, dtype=np.float64).astype(np.float32)
    return bool(np.all(np.abs(got.astype(np.float64) - np.asarray(want64, dtype=np.float64)) <= np.spacing(np.abs(want32)).astype(np.float64)))


@pytest.mark.parametrize("T", [50, 1000])
def test_tables_match_an_independent_float64_restatement(T):
    """Restated with math.sqrt, element by element, from the same float32 alpha_bar."""
    from dm3d_amd.diffusion import objective_rows, prediction_table
    ab = _alpha_bar(T)
    a = np.array([math.sqrt(float(v)) for v in ab])
    s = np.array([math.sqrt(1.0 - float(v)) for v in ab])
    want = {"v": np.stack([a, s], 1), "x0": np.stack([-a / s, 1.0 / s], 1), "eps": np.stack([np.ones(T), np.zeros(T)], 1)}
    for kind, ref in want.items():
        tab = prediction_table(ab, kind)
        assert tab.shape == (T, 2) and _within_one_ulp(tab, ref), kind
    assert np.array_equal(prediction_table(ab, "eps"), want["eps"].astype(np.float32))
    t = np.array([0, 1, T // 3, T // 2, T - 2, T - 1])
    snr = np.array([float(ab[i]) / (1.0 - float(ab[i])) for i in t])
    targets = {"eps": (np.ones(6), np.zeros(6)), "v": (a[t], -s[t]), "x0": (np.zeros(6), np.ones(6))}
    for kind, (az, a0) in targets.items():
        for gamma in (None, 5.0, 0.5, 20.0):
            rows = objective_rows(ab, t, kind) if gamma is None else objective_rows(ab, t, kind, "min_snr", gamma)
            w = np.ones(6)
            if gamma is not None:
                clipped = np.minimum(snr, gamma)
                w = {"eps": clipped / snr, "v": clipped / (snr + 1.0), "x0": clipped}[kind]
            assert rows.shape == (6, 4) and np.all(rows[:, 3] == 0)
            assert _within_one_ulp(rows[:, :3], np.stack([az, a0, w], 1)), (kind, gamma)
    for bad in (dict(prediction="noise"), dict(prediction="v", loss_weighting="snr"), dict(prediction="v", loss_weighting="min_snr", snr_gamma=0.0),
                dict(prediction="v", loss_weighting="min_snr", snr_gamma=float("nan"))):
        with pytest.raises(ValueError):
            objective_rows(ab, t, **bad)
    with pytest.raises(ValueError):
        prediction_table(ab, "V")


@pytest.mark.parametrize("T", [50, 1000])
def test_identities_in_float64(T):
    """Converting the exact v (or x0) built from random (x0, z, t) gives z back; the min-SNR weight of the eps target is 1 exactly
    wherever SNR <= gamma.  The table entries are formed here in float64, as prediction_table forms them before it rounds."""
    from dm3d_amd.diffusion import objective_rows
    ab = _alpha_bar(T).astype(np.float64)
    rng = np.random.default_rng(T)
    x0, z = rng.standard_normal((64, 32)), rng.standard_normal((64, 32))
    t = rng.integers(0, T, size=64)
    a, s = np.sqrt(ab[t])[:, None], np.sqrt(1 - ab[t])[:, None]
    x = a * x0 + s * z
    v = a * z - s * x0
    assert np.abs(a * v + s * x - z).max() < 1e-12
    assert np.abs((-a / s) * x0 + (1 / s) * x - z).max() < 1e-12     # (operands up to |x| / s = 400 at t = 0 of T = 1000: 1e-13)
    # the targets of objective_rows are v and x0 themselves
    rows = objective_rows(ab, t, "v").astype(np.float64)
    assert np.abs(rows[:, :1] * z + rows[:, 1:2] * x0 - v).max() < 1e-6              # (float32 rows)
    every = np.arange(T)
    snr = ab / (1 - ab)
    for gamma in (5.0, 20.0):
        w = objective_rows(ab, every, "eps", "min_snr", gamma)[:, 2]
        assert np.any(snr <= gamma) and np.any(snr > gamma)
        assert np.all(w[snr <= gamma] == 1.0) and np.all(w[snr > gamma] < 1.0)


def test_constructor_and_compile_argument_rules():
    from dm3d_amd.networks import conditional_dm3d, dm3d
    for DM in (conditional_dm3d.DiffusionModel, dm3d.DiffusionModel):
        p = inspect.signature(DM.__init__).parameters["prediction"]
        assert p.kind == inspect.Parameter.KEYWORD_ONLY and p.default == "eps"
        c = inspect.signature(DM.compile).parameters
        assert c["loss_weighting"].kind == inspect.Parameter.KEYWORD_ONLY and c["loss_weighting"].default is None
        assert c["snr_gamma"].kind == inspect.Parameter.KEYWORD_ONLY and c["snr_gamma"].default == 5.0
    assert _model().prediction == "eps"
    for cond in (True, False):
        for kind in ("eps", "v", "x0"):
            assert _model(cond, prediction=kind).prediction == kind
        for bad in ("V", "noise", None, 0):
            with pytest.raises(ValueError):
                _model(cond, prediction=bad)
    m = _model(prediction="v")
    for kw in (dict(loss_weighting="snr"), dict(loss_weighting=True), dict(loss_weighting="min_snr", snr_gamma=0.0),
               dict(loss_weighting="min_snr", snr_gamma=-1.0), dict(loss_weighting="min_snr", snr_gamma=float("nan")),
               dict(snr_gamma=3.0), dict(snr_gamma=float("nan"))):
        with pytest.raises(ValueError):
            m.compile(optimizer=1e-3, **kw)
    assert (m.loss_weighting, m.snr_gamma) == (None, 5.0) and not hasattr(m, "optimizer")     # a refused compile() changes nothing
    m.compile(optimizer=1e-3, loss_weighting="min_snr")
    assert (m.loss_weighting, m.snr_gamma) == ("min_snr", 5.0)
    m.compile(optimizer=1e-3, loss_weighting="min_snr", snr_gamma=1.5)
    assert (m.loss_weighting, m.snr_gamma) == ("min_snr", 1.5)
    m.compile()                                                                              # the defaults switch it off again
    assert (m.loss_weighting, m.snr_gamma) == (None, 5.0)
    # the chains' argument rules are those of an eps model, checked before any plan exists
    with pytest.raises(ValueError):
        m.generate((2, 8, 8, 8, 4), context_value=1, sampler="ddim", num_steps=5, eta=-1.0)
    with pytest.raises(ValueError):
        m.predict_eps(np.zeros((2, 8, 8, 8, 4), np.float32), np.zeros((2, 8, 8, 8, 4), np.float32), 20)
    with pytest.raises(ValueError):
        m.predict_eps(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32), 1)
    assert not m.network._plans


def test_graph_kinds_of_a_converting_chain_are_their_own():
    from dm3d_amd import diffusion as d
    kinds = set()
    for c in d._CHAINS.values():
        for thr in (None, ()):
            for pred in (None, object()):
                s = object.__new__(c)
                s.threshold, s._pred_d = thr, pred
                kinds.add(s.graph_kind)
                assert s.graph_kind.endswith("+pred") == (pred is not None)
    assert len(kinds) == 4 * len(d._CHAINS)


def test_checkpoints_carry_the_prediction(tmp_path):
    path = str(tmp_path / "ckpt.npz")
    eps, v = _model(seed=0), _model(seed=1, prediction="v")
    eps.save_weights(path)
    plain = dict(np.load(path))
    assert set(plain) == set(eps.network.state_dict())                                      # an eps model writes no new entry
    v.save_weights(path)
    saved = dict(np.load(path))
    assert set(saved) == set(plain) | {"meta/prediction"} and str(saved["meta/prediction"]) == "v"
    for other in (_model(seed=2), _model(seed=2, prediction="x0")):                         # a mismatch fails with the model as it was
        before = other.network.state_dict()
        with pytest.raises(ValueError, match="prediction"):
            other.load_weights(path)
        now = other.network.state_dict()
        assert all(np.array_equal(now[k], before[k]) for k in before)
    back = _model(seed=3, prediction="v")
    back.load_weights(path)
    st, want = back.network.state_dict(), v.network.state_dict()
    assert all(np.array_equal(st[k], want[k]) for k in want)
    back.save_weights(path)
    assert set(np.load(path)) == set(saved)
    # a checkpoint without the entry loads into any model
    x0 = _model(seed=4, prediction="x0")
    x0.load_state_dict(plain)
    st = x0.network.state_dict()
    assert all(np.array_equal(st[k], plain[k]) for k in plain)
    # the TF format has no place for it: the weights load into a model of any prediction
    prefix = str(tmp_path / "v.ckpt")
    v.save_weights(prefix)
    other = _model(seed=5)
    other.load_weights(prefix)
    st = other.network.state_dict()
    assert all(np.array_equal(st[k], want[k]) for k in want)
