"""CPU tier of the training extensions: the dm3d_adam_ema ABI and its host checks, the decay schedule of the weight average, the
argument rules of compile() / use_ema() / null_context, the context-dropout helper and the ema/ entries of checkpoints (no kernel is
launched)."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(context_dim=1, conditional=True, seed=0):
    from dm3d_amd.networks import conditional_dm3d, dm3d
    args = SimpleNamespace(timesteps=20, num_gpus=1, kernel_resize=False, bs=2)
    if not conditional:
        return dm3d.DiffusionModel(8, 1024, 4, None, args, device="cpu", seed=seed)
    return conditional_dm3d.DiffusionModel(8, 1024, 4, None, args, device="cpu", context_dim=context_dim, seed=seed)


def test_adam_ema_is_declared_exported_and_bound(built_library):
    from dm3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dm3d.h")).read()
    assert re.search(r"\bint\s+dm3d_adam_ema\s*\(float\* w, const float\* g, float\* m, float\* v, float\* ema, int64_t n,", header)
    assert hasattr(ctypes.CDLL(built_library), "dm3d_adam_ema")
    res, args = _lib.SIGNATURES["dm3d_adam_ema"]
    assert res is ctypes.c_int and len(args) == 12 and args[5] is ctypes.c_int64 and args[6:11] == [ctypes.c_float] * 5
    assert _lib.lib().dm3d_version() == _lib.ABI_VERSION == 111


def test_adam_ema_refuses_bad_arguments(built_library):
    """Every documented precondition is checked before anything is launched: DM3D_EINVAL and a fresh message, with no GPU in the
    machine (the pointers are made-up addresses nothing may dereference)."""
    from dm3d_amd import _lib
    lib = _lib.lib()
    ptrs = dict(w=0x10000, g=0x20000, m=0x30000, v=0x40000, ema=0x50000)
    ok = dict(**ptrs, n=1024, lr_t=1e-4, beta1=0.9, beta2=0.999, eps=1e-7, ema_rate=0.1)
    bad = [({k: None}, f"{k} null") for k in ptrs] + [({k: ptrs[k] + 4}, f"{k} misaligned") for k in ptrs]
    bad += [(dict(n=0), "n = 0"), (dict(n=6), "n = 6"), (dict(n=-4), "n < 0")]
    bad += [(dict(ema_rate=r), f"ema_rate {r}") for r in (-0.1, 1.5, float("nan"), float("inf"))]
    bad += [(dict(ema=ptrs["w"]), "ema == w"), (dict(ema=ptrs["g"]), "ema == g"), (dict(ema=ptrs["m"]), "ema == m"),
            (dict(ema=ptrs["v"]), "ema == v"), (dict(ema=ptrs["w"] + 16), "ema inside w"), (dict(ema=ptrs["v"] - 16, n=8), "ema ends inside v")]
    failures = []
    for override, what in bad:
        a = {**ok, **override}
        lib.dm3d_fill(None, 0, 0.0, None)                           # leaves a known message behind
        stale = lib.dm3d_last_error()
        rc = lib.dm3d_adam_ema(a["w"], a["g"], a["m"], a["v"], a["ema"], a["n"], a["lr_t"], a["beta1"], a["beta2"], a["eps"], a["ema_rate"], None)
        msg = lib.dm3d_last_error()
        if rc != -1 or not msg or msg == stale or b"adam_ema" not in msg:
            failures.append(f"dm3d_adam_ema({what}): rc {rc}, message {msg!r}")
    assert not failures, "\n".join(failures)


def test_decay_schedule():
    from dm3d_amd.train import ema_decay_at
    for n, want in ((0, 0.1), (1, 2 / 11), (9, 10 / 19), (10 ** 4, 0.999)):
        assert ema_decay_at(0.999, n, True) == pytest.approx(want, rel=1e-15, abs=0), n
    assert ema_decay_at(0.999, 8000, True) == 8001 / 8010 < 0.999 == ema_decay_at(0.999, 9000, True)     # (1 + n) / (10 + n) reaches 0.999 at n = 8990
    assert all(ema_decay_at(0.999, n, False) == 0.999 for n in (0, 1, 9, 10 ** 4))
    assert ema_decay_at(0.05, 0, True) == 0.05                                                # a decay under the warm-up's is kept


def test_compile_and_use_ema_argument_rules():
    m = _model(context_dim=2)
    for kw in (dict(context_dropout=0.1), dict(context_dropout=1.0),                          # dropout without a null id
               dict(null_context=3), dict(null_context=-1), dict(null_context=1.5),          # outside [0, context_dim]
               dict(context_dropout=-0.1, null_context=2), dict(context_dropout=1.1, null_context=2),
               dict(context_dropout=float("nan"), null_context=2),
               dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=float("nan"))):
        with pytest.raises(ValueError):
            m.compile(optimizer=1e-3, **kw)
    assert (m._ema_decay, m.context_dropout, m.null_context) == (None, 0.0, None)            # a refused compile() changes nothing
    assert not hasattr(m, "optimizer")
    m.compile(optimizer=1e-3, ema_decay=0.0, context_dropout=0.0, null_context=0)
    m.compile(optimizer=1e-3, ema_decay=0.999, ema_warmup=False, context_dropout=0.25, null_context=2)
    assert (m._ema_decay, m._ema_warmup, m.context_dropout, m.null_context) == (0.999, False, 0.25, 2)
    with pytest.raises(ValueError, match="no averaged weights"):
        m.use_ema(True)                                                                       # compiled for an average, but none exists yet
    assert m.use_ema(False) is False
    with pytest.raises(ValueError):
        m.save_weights("unused.npz", weights="ema")
    with pytest.raises(ValueError):
        m.save_weights("unused.npz", weights="both")
    m.compile()                                                                               # the defaults switch everything off again
    assert (m._ema_decay, m.context_dropout, m.null_context) == (None, 0.0, None)
    with pytest.raises(ValueError):
        _model(context_dim=1).compile(null_context=2)
    u = _model(conditional=False)
    for kw in (dict(null_context=0), dict(context_dropout=0.5, null_context=0)):
        with pytest.raises(ValueError):
            u.compile(**kw)
    u.compile(ema_decay=0.99)


def test_guidance_defaults_to_the_null_context():
    """negative_context=None stands for compile()'s null_context; without one the old refusal and its wording stay."""
    m = _model(context_dim=2)
    with pytest.raises(ValueError, match=r"guidance_scale needs negative_context \(the model has no reserved null context\)"):
        m._guidance(2, 2.0, None, 0.0)
    m.compile(null_context=2)
    w, phi, neg = m._guidance(2, 2.0, None, 0.0)
    assert neg.tolist() == [2, 2] and w.tolist() == [2.0, 2.0]
    assert m._guidance(2, 2.0, [0, 1], 0.0)[2].tolist() == [0, 1]                              # an explicit one still wins
    assert m._guidance(2, None, None, 0.0) is None


def test_context_dropout_helper():
    from dm3d_amd.diffusion import context_dropout
    ids = np.array([1, 0, 1, 1, 0], dtype=np.int32)
    keep = ids.copy()
    assert np.array_equal(context_dropout(ids, 0.0, 2, seed=3), keep)
    assert np.array_equal(context_dropout(ids, 1.0, 2, seed=3), np.full(5, 2))
    assert np.array_equal(ids, keep)                                                          # the caller's ids are left alone
    assert np.array_equal(context_dropout(ids, 0.5, 2, drop=[True, False, False, True, False]), [2, 0, 1, 2, 0])
    big = np.zeros(100_000, dtype=np.int32)
    a, b = context_dropout(big, 0.1, 7, seed=1234), context_dropout(big, 0.1, 7, seed=1234)
    assert np.array_equal(a, b) and a.dtype == np.int32
    assert not np.array_equal(a, context_dropout(big, 0.1, 7, seed=1235))
    share = float((a == 7).mean())
    print(f"dropped share at p = 0.1 over 100 000 draws: {share:.5f}")
    assert abs(share - 0.1) < 0.005                                                           # five sigma, sigma = sqrt(0.1 * 0.9 / 1e5) = 9.5e-4
    for bad in (dict(drop=[True, False]), dict(drop=[1, 0, 0, 1, 0])):
        with pytest.raises(ValueError):
            context_dropout(ids, 0.5, 2, **bad)
    with pytest.raises(ValueError):
        context_dropout(ids, 1.5, 2, seed=0)


def _with_average(m, seed=5):
    """A checkpoint of ``m``: its weights and a made-up average of them."""
    rng = np.random.default_rng(seed)
    sd = m.network.state_dict()
    ema = {f"ema/{n}": (sd[n] + rng.standard_normal(sd[n].shape).astype(np.float32) * 0.01).astype(np.float32) for n in m._trainable_names()}
    return {**sd, "ema/num_updates": np.asarray(17, dtype=np.int64), **ema}


def test_load_state_dict_validates_and_round_trips_the_average(tmp_path):
    m = _model(seed=0)
    before = m.network.state_dict()
    full = _with_average(_model(seed=1))
    some = sorted(k for k in full if k.startswith("ema/") and k != "ema/num_updates")
    wrong_shape = dict(full)
    wrong_shape[some[0]] = np.zeros(np.asarray(full[some[0]]).size + 1, np.float32)
    for bad in ({k: v for k, v in full.items() if k != some[3]},                               # a partial set
                {k: v for k, v in full.items() if k != "ema/num_updates"},
                {**full, "ema/no.such.weight": np.zeros(4, np.float32)},
                wrong_shape):
        with pytest.raises(ValueError, match="ema/"):
            m.load_state_dict(bad)
        now = m.network.state_dict()
        assert all(np.array_equal(now[k], before[k]) for k in before) and m.weights.pending_ema is None and not m._has_ema()
    m.load_state_dict(full)
    assert m.weights.trainer is None and m._has_ema()
    path = str(tmp_path / "ckpt.npz")
    m.save_weights(path)
    back = dict(np.load(path))
    assert set(back) == set(full)
    for k in full:
        assert back[k].dtype == np.asarray(full[k]).dtype and np.array_equal(back[k], full[k]), k
    # the switch, on the host: the network takes the averaged weights, save_weights still writes the live ones, and back again
    assert m.use_ema(True) is False
    st = m.network.state_dict()
    assert all(np.array_equal(st[n], full[f"ema/{n}"]) for n in m._trainable_names())
    assert all(np.array_equal(st[k], full[k]) for k in st if k.endswith((".mean", ".var")))
    m.save_weights(path)
    back = dict(np.load(path))
    assert all(np.array_equal(back[k], full[k]) for k in full) and m.weights.trainer is None
    m.save_weights(path, weights="ema")
    exported = dict(np.load(path))
    assert set(exported) == set(st) and all(np.array_equal(exported[k], st[k]) for k in st)
    assert m.use_ema(False) is True
    st = m.network.state_dict()
    assert all(np.array_equal(st[k], full[k]) for k in st)
    # a checkpoint without an average takes the average away, and the switch with it
    m.use_ema(True)
    m.load_state_dict(before)
    assert not m._has_ema() and m.weights.want == "live"
    assert all(np.array_equal(m.network.state_dict()[k], before[k]) for k in before)


def test_tf_format_export_of_the_average(tmp_path):
    """weights="ema" writes the averaged model under the ordinary names into a reference-format checkpoint; a live TF save beside an
    average warns once that the average is not in the file."""
    m = _model(seed=0)
    full = _with_average(m)
    m.load_state_dict(full)
    prefix = str(tmp_path / "avg.ckpt")
    m.save_weights(prefix, weights="ema")
    other = _model(seed=2)
    other.load_weights(prefix)
    st = other.network.state_dict()
    assert all(np.array_equal(st[n], full[f"ema/{n}"]) for n in m._trainable_names()) and not other._has_ema()
    with pytest.warns(UserWarning, match="average is not in this file"):
        m.save_weights(str(tmp_path / "live.ckpt"))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m.save_weights(str(tmp_path / "live2.ckpt"))                                           # said once
    other.load_weights(str(tmp_path / "live.ckpt"))
    st = other.network.state_dict()
    assert all(np.array_equal(st[k], full[k]) for k in st)
