"""CPU tier of latent editing (inpainting / image-to-image): the level table against a float64 restatement, the strength rule, mask
pooling, edit()'s argument rules, the dm3d_edit_update ABI and the public signatures (no kernel is launched)."""
import ctypes
import inspect
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 8, 8, 8, 4)


def _model(T=20, B=2, conditional=True):
    from dm3d_amd.networks import conditional_dm3d, dm3d
    mod = conditional_dm3d if conditional else dm3d
    return mod.DiffusionModel(8, 1024, 4, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B), device="cpu")


def _levels64(ab, levels):
    """float64 restatement: (sqrt(a'), sqrt(1-a')) with a' = alpha_bar[level], 1 for level -1."""
    rows = []
    for lv in levels:
        ap = 1.0 if lv < 0 else float(ab[lv])
        rows.append([math.sqrt(ap), math.sqrt(1.0 - ap)])
    return np.array(rows)


@pytest.mark.parametrize("T,kind,S,strength", [(1000, "ddpm", None, 1.0), (1000, "ddpm", None, 0.37), (20, "ddpm", None, 0.5),
                                               (1000, "ddim", 50, 1.0), (1000, "ddim", 50, 0.6), (20, "ddim", 5, 0.5)])
def test_level_table_against_float64_restatement(T, kind, S, strength):
    from dm3d_amd.betas import Betas
    from dm3d_amd.diffusion import ddim_timesteps, edit_levels, edit_steps
    sched = np.arange(T) if kind == "ddpm" else ddim_timesteps(T, S)
    n = edit_steps(strength, len(sched))
    levels = np.concatenate([[-1], sched[:n]])              # row j: L_j of (clean, sched_0, ..., sched_{n-1})
    ab32 = Betas(T).alpha_bar
    want = _levels64(ab32.astype(np.float64), levels)
    np.testing.assert_allclose(edit_levels(ab32, levels), want, rtol=1e-14, atol=1e-15)
    tab = _model(T)._edit_table(levels).numpy()
    assert tab.dtype == np.float32 and tab.shape == (n + 1, 4)
    np.testing.assert_array_equal(tab[:, :2], want.astype(np.float32))         # rounded once from float64
    np.testing.assert_array_equal(tab[:, 2], levels.astype(np.float32))        # the Philox counter of each row
    assert np.all(tab[:, 3] == 0)
    # the row of the chain's last step (row 0) is exactly clean: known_t = x0
    assert tab[0, 0] == 1.0 and tab[0, 1] == 0.0
    if kind == "ddpm":                                       # row t holds level t-1
        assert np.all(tab[1:, 2] == np.arange(n))
    assert np.all(tab[1:, 1] > 0)


@pytest.mark.parametrize("strength,n,want", [(1.0, 1000, 1000), (0.5, 1000, 500), (0.37, 50, 19), (0.5, 3, 2), (0.3, 5, 2),
                                             (0.25, 2, 1), (1e-3, 1000, 1), (0.0005, 1000, 1), (0.7, 1, 1)])
def test_strength_rule(strength, n, want):
    from dm3d_amd.diffusion import edit_steps
    assert edit_steps(strength, n) == want == int(math.floor(strength * n + 0.5))


@pytest.mark.parametrize("strength", [0.0, -0.5, 1.0001, 2.0, float("nan"), 0.0004])
def test_strength_rejects(strength):
    from dm3d_amd.diffusion import edit_steps
    with pytest.raises(ValueError):
        edit_steps(strength, 1000)
    m = _model(20)
    with pytest.raises(ValueError):                           # before any plan or device buffer is made
        m.edit(np.zeros(SHAPE, np.float32), 1, strength=strength if strength != 0.0004 else 0.02)


def test_latent_mask_pooling():
    from dm3d_amd.diffusion import latent_mask
    g = torch.Generator().manual_seed(0)
    lat = (2, 4, 4, 4, 8)
    m1 = torch.rand((2, 4, 4, 4), generator=g)
    assert torch.equal(latent_mask(m1, lat), m1)                                      # k = 1: as given
    for k in (2, 4):
        m = (torch.rand((2, 4 * k, 4 * k, 4 * k), generator=g) > 0.97).float() * torch.rand((2, 4 * k, 4 * k, 4 * k), generator=g)
        got = latent_mask(m, lat)
        want = np.zeros((2, 4, 4, 4), np.float32)
        mn = m.numpy()
        for b in range(2):
            for d in range(4):
                for h in range(4):
                    for w in range(4):
                        want[b, d, h, w] = mn[b, d * k:(d + 1) * k, h * k:(h + 1) * k, w * k:(w + 1) * k].max()
        assert got.dtype == torch.float32 and got.shape == (2, 4, 4, 4)
        np.testing.assert_array_equal(got.numpy(), want)
    # one voxel of a 128^3 mask marks the one latent voxel of its 4^3 block
    big = torch.zeros((1, 128, 128, 128))
    big[0, 70, 3, 127] = 1.0
    p = latent_mask(big, (3, 32, 32, 32, 8))
    assert p.shape == (3, 32, 32, 32) and float(p.sum()) == 3.0 and torch.all(p[:, 17, 0, 31] == 1.0)
    # batch broadcast and a trailing channel axis
    one = torch.rand((1, 8, 8, 8, 1), generator=g)
    p = latent_mask(one, lat)
    assert p.shape == (2, 4, 4, 4) and torch.equal(p[0], p[1]) and torch.equal(p[0], latent_mask(one[..., 0], (1, 4, 4, 4, 8))[0])
    assert torch.equal(latent_mask(np.ones((2, 4, 4, 4), np.float64), lat), torch.ones(2, 4, 4, 4))
    assert torch.equal(latent_mask(torch.zeros((2, 4, 4, 4), dtype=torch.bool), lat), torch.zeros(2, 4, 4, 4))


@pytest.mark.parametrize("shape", [(2, 6, 6, 6), (2, 4, 8, 8), (2, 12, 12, 13), (2, 3, 3, 3), (3, 4, 4, 4), (2, 4, 4, 4, 2),
                                   (2, 4, 4), (2, 1, 4, 4, 4)])
def test_latent_mask_rejects_shapes(shape):
    from dm3d_amd.diffusion import latent_mask
    with pytest.raises(ValueError):
        latent_mask(torch.zeros(shape), (2, 4, 4, 4, 8))


@pytest.mark.parametrize("bad", [-0.01, 1.01, float("nan"), float("inf")])
def test_latent_mask_rejects_values(bad):
    from dm3d_amd.diffusion import latent_mask
    m = torch.zeros((2, 8, 8, 8))
    m[1, 2, 3, 4] = bad
    with pytest.raises(ValueError):
        latent_mask(m, (2, 4, 4, 4, 8))


def test_edit_argument_rules():
    """Every rule is checked before any device work (the model here lives on the CPU, where a kernel launch would fail)."""
    m = _model(20)
    x0 = np.zeros(SHAPE, np.float32)
    bad = [
        dict(sampler="plms"),
        dict(sampler="ddpm", num_steps=5),
        dict(sampler="ddpm", eta=0.5),
        dict(sampler="ddpm", clip_x0=False),
        dict(sampler="ddim", num_steps=0),
        dict(sampler="ddim", num_steps=5, eta=-1.0),
        dict(sampler="ddim", timesteps=[3, 1]),
        dict(mask=np.zeros((2, 6, 6, 6), np.float32)),
        dict(mask=np.full((2, 8, 8, 8), 2.0, np.float32)),
        dict(strength=0.0),
        dict(noise=np.zeros((19,) + SHAPE, np.float32)),                           # DDPM at strength 1: [T, *shape]
        dict(strength=0.5, noise=np.zeros((20,) + SHAPE, np.float32)),             # strength 0.5 of T = 20: [10, *shape]
        dict(known_noise=np.zeros((20,) + SHAPE, np.float32)),                     # [n + 1, *shape]
        dict(sampler="ddim", num_steps=5, strength=0.6, known_noise=np.zeros((5,) + SHAPE, np.float32)),
        dict(steps=-1),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            m.edit(x0, 1, **kw)
    with pytest.raises(ValueError):
        m.edit(np.zeros((2, 8, 8, 8, 3), np.float32), 1)                           # not the latent shape
    with pytest.raises(ValueError):
        m.edit(x0, None)                                                           # the conditional model needs a context
    with pytest.raises(ValueError):
        m.edit(x0, [0, 1, 1])                                                      # one id or one per volume
    with pytest.raises(ValueError):
        m.q_sample(x0, 20)
    with pytest.raises(ValueError):
        m.q_sample(x0, -2)
    with pytest.raises(ValueError):
        _model(20, conditional=False).edit(x0, strength=1.5)


def test_abi_entry_exported_and_struct_layout(built_library, tmp_path):
    from dm3d_amd import _lib
    assert hasattr(ctypes.CDLL(built_library), "dm3d_edit_update") and "dm3d_edit_update" in _lib.SIGNATURES
    assert _lib.lib().dm3d_version() == _lib.ABI_VERSION == 111                         # additive: the version stays
    src = tmp_path / "sz.c"
    fields = ("x0", "w", "noise", "out", "batch", "per_sample", "channels", "levels", "rows", "pos", "seed", "seed_dev", "mode")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dm3d.h"\nint main(){printf("%zu'
                   + " %zu" * len(fields) + '\\n", sizeof(dm3d_edit_desc)'
                   + "".join(f", offsetof(dm3d_edit_desc, {f})" for f in fields) + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(_lib.EditDesc)
    assert vals[1:] == [getattr(_lib.EditDesc, f).offset for f in fields]


def test_plain_c_program_calls_the_edit_entry(built_library, tmp_path):
    """A C99 translation unit including only dm3d.h links; a null or empty descriptor is refused before any device call."""
    src = tmp_path / "edit.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "dm3d.h"
int main(void) {
    dm3d_edit_desc d;
    memset(&d, 0, sizeof d);
    int rc0 = dm3d_edit_update(NULL, NULL);
    printf("%d|%s\n", rc0, dm3d_last_error());
    int rc1 = dm3d_edit_update(&d, NULL);
    printf("%d|%s\n", rc1, dm3d_last_error());
    return 0;
}
''')
    exe = tmp_path / "edit"
    libdir = os.path.dirname(built_library)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-ldm3d_hip", f"-Wl,-rpath,{libdir}"], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == 2
    for line in lines:
        rc, text = line.split("|", 1)
        assert int(rc) != 0 and "edit" in text
    assert "null descriptor" in lines[0]


def test_edit_update_argument_validation_needs_no_gpu(built_library):
    from dm3d_amd import _lib
    L = _lib.lib()

    def refused(d, word):
        return L.dm3d_edit_update(ctypes.byref(d), None) != 0 and word in L.dm3d_last_error()

    d = _lib.EditDesc()
    d.x = d.x0 = d.w = d.levels = d.pos = 4096
    d.batch, d.per_sample, d.channels, d.rows, d.mode = 2, 6, 2, 4, 1             # per_sample not a multiple of 4
    assert refused(d, b"per_sample")
    d.per_sample, d.channels = 8, 3                                               # channels does not divide per_sample
    assert refused(d, b"channels")
    d.channels, d.batch = 4, 65536                                                # more than 65535 samples
    assert refused(d, b"batch")
    d.batch, d.rows = 2, 0
    assert refused(d, b"rows")
    d.rows, d.x0 = 4, 4100                                                        # unaligned
    assert refused(d, b"aligned")
    d.x0, d.w = 4096, None                                                        # mode 1 without weights
    assert refused(d, b"mode 1")
    d.w, d.mode = 4096, 0                                                         # mode 0 without out
    assert refused(d, b"out")
    d.mode = 2
    assert refused(d, b"mode")
    d.mode, d.pos = 1, None
    assert refused(d, b"non-null")


def test_signatures_are_keyword_only_extensions():
    from dm3d_amd.networks import conditional_dm3d, dm3d
    e = inspect.signature(conditional_dm3d.DiffusionModel.edit).parameters
    assert list(e)[1:3] == ["x0", "context_value"] and e["context_value"].default is None
    new = {"mask": None, "strength": 1.0, "sampler": "ddpm", "num_steps": None, "timesteps": None, "eta": 0.0, "clip_x0": True,
           "seed": None, "use_graph": True, "noise": None, "known_noise": None, "steps": None}
    for name, default in new.items():
        assert e[name].kind == inspect.Parameter.KEYWORD_ONLY and e[name].default == default, name
    q = inspect.signature(conditional_dm3d.DiffusionModel.q_sample).parameters
    assert list(q)[1:4] == ["x0", "t", "noise"] and q["seed"].kind == inspect.Parameter.KEYWORD_ONLY
    u = inspect.signature(dm3d.DiffusionModel.edit).parameters
    assert list(u)[1] == "x0" and u["kw"].kind == inspect.Parameter.VAR_KEYWORD
    # the existing entries are unchanged
    g = inspect.signature(conditional_dm3d.DiffusionModel.generate).parameters
    assert "mask" not in g and "strength" not in g
