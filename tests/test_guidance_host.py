"""CPU tier of classifier-free guidance: the argument rules of generate() / edit() / sampler(), the public signatures, the
dm3d_guide_update ABI and its host checks, and the per-rank slicing of generate_sharded (no kernel is launched)."""
import ctypes
import inspect
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 8, 8, 8, 4)
GUIDE_KW = {"guidance_scale": None, "negative_context": None, "guidance_rescale": 0.0}


def _model(T=20, B=2, conditional=True):
    from dm3d_amd.networks import conditional_dm3d, dm3d
    mod = conditional_dm3d if conditional else dm3d
    return mod.DiffusionModel(8, 1024, 4, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B), device="cpu")


def _no_plan(m):
    """The rules are checked before any plan or device buffer is made (the model lives on the CPU, where a launch would fail)."""
    return not m.network._plans


BAD = [
    dict(negative_context=0),                                                   # without guidance_scale
    dict(guidance_rescale=0.5),
    dict(guidance_rescale=[0.0, 0.3]),
    dict(guidance_scale=3.0),                                                   # without negative_context
    dict(guidance_scale=float("nan"), negative_context=0),
    dict(guidance_scale=float("inf"), negative_context=0),
    dict(guidance_scale=[1.0, float("-inf")], negative_context=0),
    dict(guidance_scale=[1.0, 2.0, 3.0], negative_context=0),                   # one value or one per volume
    dict(guidance_scale=3.0, negative_context=0, guidance_rescale=-0.1),
    dict(guidance_scale=3.0, negative_context=0, guidance_rescale=1.5),
    dict(guidance_scale=3.0, negative_context=0, guidance_rescale=[0.2, 1.01]),
    dict(guidance_scale=3.0, negative_context=0, guidance_rescale=float("nan")),
    dict(guidance_scale=3.0, negative_context=2),                               # validated as context_value is
    dict(guidance_scale=3.0, negative_context=-1),
    dict(guidance_scale=3.0, negative_context=[0, 1, 1]),
]


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_argument_rules(kind):
    m = _model()
    x0 = np.zeros(SHAPE, np.float32)
    ddim = dict(num_steps=5) if kind == "ddim" else {}
    for kw in BAD:
        with pytest.raises(ValueError):
            m.generate(SHAPE, context_value=1, sampler=kind, **ddim, **kw)
        with pytest.raises(ValueError):
            m.edit(x0, 1, sampler=kind, **ddim, **kw)
        with pytest.raises(ValueError):
            m.sampler(SHAPE, 1, kind=kind, **ddim, **kw)
    assert _no_plan(m)


def test_unconditional_model_rejects_the_keywords():
    m = _model(conditional=False)
    x0 = np.zeros(SHAPE, np.float32)
    for kw in (dict(guidance_scale=3.0), dict(negative_context=0), dict(guidance_rescale=0.5),
               dict(guidance_scale=3.0, negative_context=0), dict(guidance_scale=3.0, negative_context=0, guidance_rescale=0.5)):
        with pytest.raises(ValueError):
            m.generate(SHAPE, **kw)
        with pytest.raises(ValueError):
            m.generate(SHAPE, sampler="ddim", num_steps=5, **kw)
        with pytest.raises(ValueError):
            m.edit(x0, **kw)
        with pytest.raises(ValueError):
            m.sampler(SHAPE, **kw)
    assert _no_plan(m)


def test_guide_eps_argument_rules():
    m = _model()
    e = np.zeros(SHAPE, np.float32)
    for args in ((e, e[:1], 3.0), (e, e, float("nan")), (e, e, [1.0, 2.0, 3.0]), (e, e, 3.0, 1.5), (e, e, 3.0, -0.5),
                 (e, e, 3.0, [0.1, 0.2, 0.3]), (np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32), 3.0)):
        with pytest.raises(ValueError):
            m.guide_eps(*args)


def test_signatures_carry_the_keywords():
    from dm3d_amd.networks import conditional_dm3d
    DM = conditional_dm3d.DiffusionModel
    for fn in (DM.generate, DM.edit, DM.sampler):
        p = inspect.signature(fn).parameters
        for name, default in GUIDE_KW.items():
            assert p[name].kind == inspect.Parameter.KEYWORD_ONLY and p[name].default == default, (fn.__name__, name)
    g = inspect.signature(DM.guide_eps).parameters
    assert list(g)[1:] == ["eps_pos", "eps_neg", "guidance_scale", "guidance_rescale"]
    assert g["guidance_scale"].default is inspect.Parameter.empty and g["guidance_rescale"].default == 0.0
    # the earlier keywords keep their defaults
    p = inspect.signature(DM.generate).parameters
    assert p["sampler"].default == "ddpm" and p["eta"].default == 0.0 and p["seed"].default is None


def test_guided_kinds_are_their_own():
    """A guided graph never replays as the plain step of the same 2 B-row plan: the cache key holds the kind."""
    from dm3d_amd import diffusion as d
    plain = {d.Sampler.KIND, d.DdimSampler.KIND, d.EditSampler.KIND, d.DdimEditSampler.KIND}
    guided = {d.GuidedSampler.KIND, d.GuidedDdimSampler.KIND, d.GuidedEditSampler.KIND, d.GuidedDdimEditSampler.KIND}
    assert len(plain) == 4 and len(guided) == 4 and not plain & guided
    assert d.Sampler.COPIES == 1 and d.GuidedSampler.COPIES == 2 and d.GuidedDdimEditSampler.COPIES == 2


def test_abi_entry_exported_and_struct_layout(built_library, tmp_path):
    from dm3d_amd import _lib
    assert hasattr(ctypes.CDLL(built_library), "dm3d_guide_update") and "dm3d_guide_update" in _lib.SIGNATURES
    assert _lib.lib().dm3d_version() == _lib.ABI_VERSION == 111                         # additive: the version stays
    src = tmp_path / "sz.c"
    fields = ("eps_pos", "eps_neg", "out", "batch", "per_sample", "scale", "rescale", "partials", "x", "t_idx", "mode")
    assert fields == tuple(n for n, _ in _lib.GuideDesc._fields_)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dm3d.h"\nint main(){printf("%d %zu'
                   + " %zu" * len(fields) + '\\n", DM3D_GUIDE_PARTIAL_BLOCKS, sizeof(dm3d_guide_desc)'
                   + "".join(f", offsetof(dm3d_guide_desc, {f})" for f in fields) + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == _lib.GUIDE_PARTIAL_BLOCKS
    assert vals[1] == ctypes.sizeof(_lib.GuideDesc)
    assert vals[2:] == [getattr(_lib.GuideDesc, f).offset for f in fields]


def test_guide_update_argument_validation_needs_no_gpu(built_library):
    from dm3d_amd import _lib
    L = _lib.lib()

    def refused(d, word):
        return L.dm3d_guide_update(ctypes.byref(d), None) != 0 and word in L.dm3d_last_error()

    assert L.dm3d_guide_update(None, None) != 0 and b"null descriptor" in L.dm3d_last_error()
    d = _lib.GuideDesc()
    d.eps_pos, d.eps_neg, d.out, d.scale = 4096, 8192, 4096, 4096                 # in place: out aliases eps_pos
    d.batch, d.per_sample, d.mode = 2, 6, 0                                       # per_sample not a multiple of 4
    assert refused(d, b"per_sample")
    d.per_sample, d.batch = 8, 65536
    assert refused(d, b"batch")
    d.batch, d.eps_neg = 2, 8196                                                  # unaligned
    assert refused(d, b"aligned")
    d.eps_neg, d.out = 8192, 8192                                                 # out aliasing eps_neg
    assert refused(d, b"never eps_neg")
    d.out, d.scale = 4096, None
    assert refused(d, b"non-null")
    d.scale, d.partials = 4096, 4096                                              # statistics without the rescale table
    assert refused(d, b"partials")
    d.partials, d.mode = None, 1                                                  # the rescale needs its tables
    assert refused(d, b"mode 1")
    d.mode = 2
    assert refused(d, b"mode 2")                                                  # the mirror needs x
    d.x = 4100
    assert refused(d, b"aligned")
    d.mode = 3
    assert refused(d, b"mode")


class _Stub:
    """Records what generate_sharded asks of DiffusionModel.generate."""
    device = torch.device("cpu")

    def generate(self, shape, last_step=0, context_value=None, **kw):
        self.shape, self.ctx, self.kw = tuple(shape), context_value, kw
        return torch.zeros(shape)


def test_generate_sharded_slices_per_volume_guidance(monkeypatch):
    """A single process and no process group: rank 0 of 1 takes the whole batch; the slicing itself is checked with a rank of a
    larger world by patching the shard range."""
    from dm3d_amd import parallel
    m, shape = _Stub(), (5, 2, 2, 2, 4)
    w, n, phi = [1.0, 2.0, 3.0, 4.0, 5.0], [0, 1, 0, 1, 1], [0.0, 0.1, 0.2, 0.3, 0.4]
    parallel.generate_sharded(m, shape, 0, [1, 0, 1, 0, 0], seed=7, guidance_scale=w, negative_context=n, guidance_rescale=phi,
                              sampler="ddim", num_steps=5)
    assert m.shape == shape and m.kw["sampler"] == "ddim" and m.kw["num_steps"] == 5 and m.kw["seed"] == 7
    assert np.asarray(m.kw["guidance_scale"]).tolist() == w and np.asarray(m.kw["negative_context"]).tolist() == n
    assert np.asarray(m.kw["guidance_rescale"]).tolist() == phi
    # scalars pass as given; an unguided call forwards none of the keywords
    parallel.generate_sharded(m, shape, 0, 1, guidance_scale=2.5, negative_context=0)
    assert m.kw["guidance_scale"] == 2.5 and m.kw["negative_context"] == 0 and "guidance_rescale" not in m.kw
    parallel.generate_sharded(m, shape, 0, 1)
    assert not set(GUIDE_KW) & set(m.kw)
    # rank 1 of 2 takes volumes 3..4 of every per-volume argument
    monkeypatch.setattr(parallel, "shard_range", lambda total, rank, world: (3, 5))
    parallel.generate_sharded(m, shape, 0, [1, 0, 1, 0, 0], guidance_scale=w, negative_context=n, guidance_rescale=0.25, gather=False)
    assert m.shape == (2, 2, 2, 2, 4) and np.asarray(m.ctx).tolist() == [0, 0]
    assert np.asarray(m.kw["guidance_scale"]).tolist() == [4.0, 5.0] and np.asarray(m.kw["negative_context"]).tolist() == [1, 1]
    assert m.kw["guidance_rescale"] == 0.25
    monkeypatch.undo()
    for kw in (dict(guidance_scale=[1.0, 2.0]), dict(negative_context=[0, 1, 1]), dict(guidance_rescale=[0.1] * 4)):
        with pytest.raises(ValueError):
            parallel.generate_sharded(m, shape, 0, 1, **kw)
