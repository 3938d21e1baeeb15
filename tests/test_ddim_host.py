"""CPU tier of the DDIM sampler: schedule rule, coefficient table against a float64 restatement, the dm3d_ddim_update ABI and
the public signatures (no kernel is launched)."""
import ctypes
import inspect
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _schedule(T, S):
    """tau_i = round(i (T-1) / (S-1)), halves up; [T-1] for S = 1."""
    if S == 1:
        return [T - 1]
    return [int(math.floor(i * (T - 1) / (S - 1) + 0.5)) for i in range(S)]


def _coefficients(ab, src, dst, eta):
    """float64 restatement of one DDIM row per step src -> dst (dst < 0: the x0 target, alpha_bar' = 1)."""
    rows = []
    for s, d in zip(src, dst):
        a = float(ab[s])
        ap = 1.0 if d < 0 else float(ab[d])
        sigma = eta * math.sqrt((1 - ap) / (1 - a)) * math.sqrt(1 - a / ap) if eta else 0.0
        rows.append([math.sqrt(a), math.sqrt(1 - a), math.sqrt(ap), math.sqrt(max(1 - ap - sigma * sigma, 0.0)), sigma])
    return np.array(rows)


def _alpha_bar64(T):
    beta = np.linspace(0.0001, 0.02, T)
    return beta, np.cumprod(1 - beta, 0)


def _model(T=20, B=2):
    from dm3d_amd.networks import conditional_dm3d
    return conditional_dm3d.DiffusionModel(8, 1024, 4, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B),
                                           device="cpu")


@pytest.mark.parametrize("T,S", [(1000, 50), (300, 50), (20, 5), (50, 10), (7, 7), (5, 1), (1000, 1)])
def test_schedule_rule(T, S):
    from dm3d_amd.diffusion import ddim_timesteps
    got = ddim_timesteps(T, num_steps=S)
    assert got.tolist() == _schedule(T, S)
    assert got[-1] == T - 1 and (S == 1 or got[0] == 0) and np.all(np.diff(got) > 0)


def test_schedule_exact_lists():
    from dm3d_amd.diffusion import ddim_timesteps
    assert ddim_timesteps(20, 5).tolist() == [0, 5, 10, 14, 19]
    assert ddim_timesteps(1000, 50).tolist()[:6] == [0, 20, 41, 61, 82, 102]
    assert ddim_timesteps(300, 50).tolist()[-4:] == [281, 287, 293, 299]
    assert ddim_timesteps(1000, 1000).tolist() == list(range(1000))
    assert ddim_timesteps(13).tolist() == list(range(13))                      # neither given: every timestep
    assert ddim_timesteps(10, 1).tolist() == [9]
    assert ddim_timesteps(10, timesteps=[0, 3, 9]).tolist() == [0, 3, 9]


@pytest.mark.parametrize("kw", [dict(num_steps=0), dict(num_steps=21), dict(num_steps=-3), dict(timesteps=[0, 5, 5]),
                                dict(timesteps=[4, 2]), dict(timesteps=[0, 20]), dict(timesteps=[-1, 3]), dict(timesteps=[]),
                                dict(timesteps=[0.5, 3]), dict(num_steps=5, timesteps=[0, 3])])
def test_schedule_rejects(kw):
    from dm3d_amd.diffusion import ddim_timesteps
    with pytest.raises(ValueError):
        ddim_timesteps(20, **kw)
    m = _model(20)
    with pytest.raises(ValueError):                               # refused before any plan or device buffer is made
        m.generate((2, 8, 8, 8, 4), context_value=1, sampler="ddim", **kw)


def test_generate_argument_rules():
    m = _model(20)
    with pytest.raises(ValueError, match="last_step"):
        m.generate((2, 8, 8, 8, 4), last_step=3, context_value=1, sampler="ddim", num_steps=5)
    with pytest.raises(ValueError):
        m.generate((2, 8, 8, 8, 4), context_value=1, sampler="ddpm", num_steps=5)        # DDIM-only arguments on the DDPM path
    with pytest.raises(ValueError):
        m.generate((2, 8, 8, 8, 4), context_value=1, sampler="ddpm", eta=0.5)
    with pytest.raises(ValueError):
        m.generate((2, 8, 8, 8, 4), context_value=1, sampler="plms")
    with pytest.raises(ValueError):
        m.generate((2, 8, 8, 8, 4), context_value=1, sampler="ddim", num_steps=5, eta=-1.0)
    with pytest.raises(ValueError):
        m.invert(np.zeros((2, 8, 8, 8, 4), np.float32), 1, num_steps=0)
    with pytest.raises(ValueError):
        m.ddim_step(np.zeros((2, 8, 8, 8, 4), np.float32), np.zeros((2, 8, 8, 8, 4), np.float32), 5, 5)      # t_prev must be < t


@pytest.mark.parametrize("T,S,eta", [(1000, 50, 0.0), (1000, 50, 0.5), (300, 50, 1.0), (20, 5, 0.3), (20, 20, 1.0)])
def test_coefficient_table_against_float64_restatement(T, S, eta):
    from dm3d_amd.betas import Betas
    from dm3d_amd.diffusion import DdimSampler, ddim_coefficients, ddim_timesteps
    taus = ddim_timesteps(T, S)
    ab32 = Betas(T).alpha_bar
    for invert in (False, True):
        src, dst = DdimSampler._rows(SimpleNamespace(taus=taus, invert=invert))
        if invert:
            assert src.tolist() == taus[:-1][::-1].tolist() and dst.tolist() == taus[1:][::-1].tolist()
        else:
            assert src.tolist() == taus.tolist() and dst.tolist() == [-1] + taus[:-1].tolist()
        e = 0.0 if invert else eta
        want = _coefficients(ab32.astype(np.float64), src, dst, e)
        np.testing.assert_allclose(ddim_coefficients(ab32, src, dst, e), want, rtol=1e-14, atol=1e-15)
        # the device table: the same rows rounded once to float32, the clip flag in column 5
        tab = _model(T)._ddim_table(src, dst, e, not invert).numpy()
        assert tab.dtype == np.float32 and tab.shape == (len(src), 8)
        np.testing.assert_array_equal(tab[:, :5], want.astype(np.float32))
        assert np.all(tab[:, 5] == (0.0 if invert else 1.0)) and np.all(tab[:, 6:] == 0)
    src, dst = taus, np.concatenate([[-1], taus[:-1]])
    c = ddim_coefficients(ab32, src, dst, eta)
    assert c[0, 2] == 1.0 and c[0, 3] == 0.0 and c[0, 4] == 0.0            # the tau_0 row lands on x0
    if eta == 0:
        assert np.all(c[:, 4] == 0)
    assert np.all(c[:, 4] >= 0) and np.all(np.isfinite(c))


def test_eta_one_full_schedule_is_the_ddpm_variance():
    """eta = 1, S = T: sigma^2 = (1 - alpha_bar_prev) beta / (1 - alpha_bar), the posterior variance of Betas, in float64."""
    from dm3d_amd.diffusion import ddim_coefficients
    for T in (1000, 300, 20):
        beta, ab = _alpha_bar64(T)
        abp = np.append(1.0, ab[:-1])
        t = np.arange(T)
        c = ddim_coefficients(ab, t, t - 1, 1.0)
        var = (1 - abp) * beta / (1 - ab)
        assert c[0, 4] == 0.0
        np.testing.assert_allclose(c[1:, 4] ** 2, var[1:], rtol=1e-12, atol=0)
    # inversion rows (a' < a) with eta = 0 stay finite: sigma = 0, a_eps = sqrt(1 - a')
    _, ab = _alpha_bar64(50)
    c = ddim_coefficients(ab, np.arange(49), np.arange(1, 50), 0.0)
    assert np.all(c[:, 4] == 0) and np.allclose(c[:, 3], np.sqrt(1 - ab[1:]))


def test_abi_entry_exported_and_struct_layout(built_library, tmp_path):
    from dm3d_amd import _lib
    assert hasattr(ctypes.CDLL(built_library), "dm3d_ddim_update") and "dm3d_ddim_update" in _lib.SIGNATURES
    assert _lib.lib().dm3d_version() == _lib.ABI_VERSION == 111                         # additive: the version stays
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dm3d.h"\n'
                   'int main(){printf("%zu %zu %zu\\n", sizeof(dm3d_ddim_desc), offsetof(dm3d_ddim_desc, seed), '
                   'offsetof(dm3d_ddim_desc, mode));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off_seed, off_mode = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert size == ctypes.sizeof(_lib.DdimDesc)
    assert off_seed == _lib.DdimDesc.seed.offset and off_mode == _lib.DdimDesc.mode.offset


def test_plain_c_program_calls_the_ddim_entry(built_library, tmp_path):
    """A C99 translation unit including only dm3d.h links; a null or empty descriptor is refused before any device call."""
    src = tmp_path / "ddim.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "dm3d.h"
int main(void) {
    dm3d_ddim_desc d;
    memset(&d, 0, sizeof d);
    int rc0 = dm3d_ddim_update(NULL, NULL);
    printf("%d|%s\n", rc0, dm3d_last_error());
    int rc1 = dm3d_ddim_update(&d, NULL);
    printf("%d|%s\n", rc1, dm3d_last_error());
    return 0;
}
''')
    exe = tmp_path / "ddim"
    libdir = os.path.dirname(built_library)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-ldm3d_hip", f"-Wl,-rpath,{libdir}"], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    for line in lines:
        rc, text = line.split("|", 1)
        assert int(rc) != 0 and "ddim" in text
    assert "null descriptor" in lines[0]


def test_ddim_update_argument_validation_needs_no_gpu(built_library):
    from dm3d_amd import _lib
    d = _lib.DdimDesc()
    d.x = d.eps = d.coef = d.tau = d.pos = 4096
    d.batch, d.per_sample, d.rows, d.mode = 2, 6, 4, 1                   # per_sample not a multiple of 4
    assert _lib.lib().dm3d_ddim_update(ctypes.byref(d), None) != 0 and b"per_sample" in _lib.lib().dm3d_last_error()
    d.per_sample, d.mode = 8, 0                                          # mode 0 without out
    assert _lib.lib().dm3d_ddim_update(ctypes.byref(d), None) != 0 and b"out" in _lib.lib().dm3d_last_error()
    d.mode, d.t_idx = 1, 8192                                            # t_idx without t_next
    assert _lib.lib().dm3d_ddim_update(ctypes.byref(d), None) != 0 and b"t_next" in _lib.lib().dm3d_last_error()
    d.t_idx, d.rows = None, 0
    assert _lib.lib().dm3d_ddim_update(ctypes.byref(d), None) != 0 and b"rows" in _lib.lib().dm3d_last_error()


def test_signatures_are_keyword_only_extensions():
    from dm3d_amd.networks import conditional_dm3d
    g = inspect.signature(conditional_dm3d.DiffusionModel.generate).parameters
    assert list(g)[1:4] == ["shape", "last_step", "context_value"] and g["shape"].default == (1, 16, 16, 16, 16)
    new = {"sampler": "ddpm", "num_steps": None, "timesteps": None, "eta": 0.0, "clip_x0": True}
    for name, default in new.items():
        assert g[name].kind == inspect.Parameter.KEYWORD_ONLY and g[name].default == default
    inv = inspect.signature(conditional_dm3d.DiffusionModel.invert).parameters
    assert list(inv)[1:3] == ["x0", "context_value"]
    assert all(inv[n].kind == inspect.Parameter.KEYWORD_ONLY for n in ("num_steps", "timesteps", "use_graph", "seed"))
    st = inspect.signature(conditional_dm3d.DiffusionModel.ddim_step).parameters
    assert list(st)[1:7] == ["x_t", "pred_noise", "t", "t_prev", "eta", "noise"] and st["eta"].default == 0.0
    smp = inspect.signature(conditional_dm3d.DiffusionModel.sampler).parameters
    assert smp["kind"].kind == inspect.Parameter.KEYWORD_ONLY and smp["kind"].default == "ddpm"
