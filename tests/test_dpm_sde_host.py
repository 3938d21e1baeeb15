"""CPU tier of the stochastic DPM-Solver++(2M) sampler (sampler="dpmpp_sde"): the coefficient rows' identities, the marginals the rows
give a chain on Gaussian data (moments pushed through, nothing sampled), the argument rules, the dm3d_dpm_sde_update ABI and the
kernels' build (no kernel is launched)."""
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
CSRC = os.path.join(ROOT, "3d-condtional-stable-diffusion_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SHAPE = (2, 8, 8, 8, 4)
F = np.float32


def _model(T=20, B=2, **kw):
    from dm3d_amd.networks import conditional_dm3d
    return conditional_dm3d.DiffusionModel(8, 1024, 4, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B),
                                           device="cpu", **kw)


def _chain_rows(taus, order=2, lower_order_final=True):
    """(src, dst, prev) of rows 0..n-1 of a chain over taus (row n-1 runs first): the order rule of generate(sampler="dpmpp")."""
    taus = [int(v) for v in taus]
    n = len(taus)
    prev = taus[1:] + [-1]
    if order == 1:
        prev = [-1] * n
    if lower_order_final and n > 1:
        prev[1] = -1
    return np.array(taus), np.array([-1] + taus[:-1]), np.array(prev)


def _alpha_bar(T, ztsnr):
    from dm3d_amd.betas import Betas
    return Betas(T, zero_terminal_snr=ztsnr).alpha_bar


# ---- 1. coefficient identities -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ztsnr", [False, True])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("T,S", [(1000, 5), (1000, 20), (1000, 1000), (20, 5), (20, 20)])
def test_eta_zero_rows_are_the_ode_rows_bitwise(T, S, order, ztsnr):
    from dm3d_amd.diffusion import ddim_timesteps, dpm_coefficients, dpm_sde_coefficients
    ab = _alpha_bar(T, ztsnr)
    src, dst, prev = _chain_rows(ddim_timesteps(T, S), order)
    got = dpm_sde_coefficients(ab, src, dst, prev, order, eta=0.0)
    want = dpm_coefficients(ab, src, dst, prev, order)
    assert got.dtype == np.float64 and got.shape == (S, 4)
    assert np.array_equal(got[:, :3].view(np.int64), want.view(np.int64))
    assert np.all(got[:, 3] == 0) and np.all(np.isfinite(got))


@pytest.mark.parametrize("ztsnr", [False, True])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0, 2.0])
def test_rows_keep_the_mean_and_the_noise_level(eta, order, ztsnr):
    """With x = alpha_s x0 + sigma_s e and a perfect x0 (history included), x' must be alpha_t x0 + sigma_t e': the x0 weights sum to
    alpha_t - c_x alpha_s and c_x^2 sigma_s^2 + c_z^2 = sigma_t^2, at every row: clean, first order, second order, from a = 0."""
    from dm3d_amd.diffusion import ddim_timesteps, dpm_sde_coefficients
    for T, S in ((1000, 20), (1000, 7), (20, 5), (1000, 1000)):
        ab = _alpha_bar(T, ztsnr)
        ab64 = ab.astype(np.float64)
        src, dst, prev = _chain_rows(ddim_timesteps(T, S), order)
        c = dpm_sde_coefficients(ab, src, dst, prev, order, eta)
        a_s, a_t = ab64[src], np.where(dst < 0, 1.0, ab64[np.maximum(dst, 0)])
        assert np.all(np.isfinite(c))
        assert np.abs(c[:, 0] * np.sqrt(a_s) + c[:, 1] + c[:, 2] - np.sqrt(a_t)).max() < 1e-12
        assert np.abs(c[:, 0] ** 2 * (1 - a_s) + c[:, 3] ** 2 - (1 - a_t)).max() < 1e-12
        assert c[0].tolist() == [0.0, 1.0, 0.0, 0.0]                                       # the row to clean, exactly
        second = (prev >= 0) & (dst >= 0) & (order == 2) & (a_s > 0) & (ab64[np.maximum(prev, 0)] > 0)
        assert np.all((c[:, 2] != 0) == second) and np.all(c[:, 2] <= 0) and np.all(c[:, 3] >= 0)
        if eta > 0:
            assert np.all(c[1:, 3] > 0)                                                    # every step but the one to clean draws


def test_rows_against_a_scalar_restatement():
    """One second-order row and one first-order row, written out with math.* from the formulas of the header."""
    from dm3d_amd.diffusion import dpm_sde_coefficients
    ab = _alpha_bar(1000, False)
    al, sg = (lambda i: math.sqrt(float(ab[i]))), (lambda i: math.sqrt(1.0 - float(ab[i])))
    lam = lambda i: math.log(al(i) / sg(i))
    for eta in (0.3, 1.0):
        for s, t, p in ((500, 450, 560), (999, 900, -1), (3, 0, 50)):
            h = lam(t) - lam(s)
            A = al(t) * (1 - math.exp(-(1 + eta) * h))
            g = 0.0 if p < 0 else h / (2 * (lam(s) - lam(p)))
            want = [sg(t) / sg(s) * math.exp(-eta * h), A * (1 + g), -A * g, sg(t) * math.sqrt(1 - math.exp(-2 * eta * h))]
            got = dpm_sde_coefficients(ab, [s], [t], [p], 2, eta)[0]
            np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-14)
    with pytest.raises(ValueError):
        dpm_sde_coefficients(ab, [5], [3], [7], order=3)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sde_eta"):
            dpm_sde_coefficients(ab, [5], [3], [7], eta=bad)


@pytest.mark.parametrize("T,S", [(1000, 20), (20, 5), (1000, 1000)])
def test_zero_terminal_snr_rows(T, S):
    from dm3d_amd.diffusion import ddim_timesteps, dpm_sde_coefficients
    ab = _alpha_bar(T, True)
    assert ab[-1] == 0.0
    src, dst, prev = _chain_rows(ddim_timesteps(T, S), 2, lower_order_final=False)
    a_t = float(ab[dst[-1]])
    for eta in (0.0, 0.5, 1.0):
        c = dpm_sde_coefficients(ab, src, dst, prev, 2, eta)
        assert np.all(np.isfinite(c)), eta
        first = [math.sqrt(1 - a_t), math.sqrt(a_t), 0.0, 0.0] if eta == 0 else [0.0, math.sqrt(a_t), 0.0, math.sqrt(1 - a_t)]
        assert c[-1].tolist() == first
        assert c[-2, 2] == 0.0 and prev[-2] == src[-1]                  # the row after it: its history level has lambda = -inf, g = 0
        assert np.all(c[1:-2, 2] < 0)                                   # the rows after that are second order again


# ---- 2. what the rows do to Gaussian data -------------------------------------------------------------------------------------------
MU, S2 = 0.3, 0.25


def _gaussian_marginal(ab, taus, order, eta):
    """Mean and variance of a chain's result on data N(MU, S2) per element under the exact predictor E[x0 | x_t] = MU + k (x_t - alpha MU),
    k = alpha S2 / (alpha^2 S2 + sigma^2): the mean and the 2x2 covariance of (x, hist) pushed through the rows, z independent of
    both, from the true marginal at the chain's first level.  Nothing is sampled."""
    from dm3d_amd.diffusion import dpm_sde_coefficients
    ab = np.asarray(ab, dtype=np.float64)
    src, dst, prev = _chain_rows(taus, order, True)
    c = dpm_sde_coefficients(ab, src, dst, prev, order, eta)
    a = ab[src[-1]]
    mean = np.array([math.sqrt(a) * MU, 0.0])
    cov = np.array([[a * S2 + 1 - a, 0.0], [0.0, 0.0]])                 # the first row's c_1 is 0: the history's moments are not read
    for r in range(len(src) - 1, -1, -1):
        a = ab[src[r]]
        al = math.sqrt(a)
        k = al * S2 / (a * S2 + 1 - a)
        d = MU - k * al * MU                                           # x0 = k x + d
        c_x, c_0, c_1, c_z = c[r]
        M = np.array([[c_x + c_0 * k, c_1], [k, 0.0]])
        mean = M @ mean + np.array([c_0 * d, d])
        cov = M @ cov @ M.T + np.diag([c_z ** 2, 0.0])
    return mean[0], cov[0, 0]


@pytest.mark.parametrize("ztsnr", [False, True])
@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_gaussian_marginals(eta, ztsnr):
    """The final mean is MU for both orders; first order's variance error falls with every doubling of S and second order's lies
    below it at every S (it is not monotone itself: it changes sign).  At eta = 1 on the plain schedule the first-order errors are
    0.146, 0.0995, 0.0629, 0.0372 and the second-order ones 0.115, 0.0205, 0.0125, 0.0091 at S = 10, 20, 40, 80."""
    from dm3d_amd.diffusion import ddim_timesteps
    T = 1000
    ab = _alpha_bar(T, ztsnr)
    err = {}
    for S in (10, 20, 40, 80):
        for order in (1, 2):
            mean, var = _gaussian_marginal(ab, ddim_timesteps(T, S), order, eta)
            err[order, S] = abs(var - S2)
            print(f"eta={eta} ztsnr={ztsnr} S={S} order={order}: mean - mu {mean - MU:+.2e}, |var - s2| {err[order, S]:.4f}")
            assert abs(mean - MU) < 1e-12
    for lo, hi in ((10, 20), (20, 40), (40, 80)):
        assert err[1, hi] < err[1, lo]
    for S in (10, 20, 40, 80):
        assert err[2, S] < err[1, S]
    if eta == 1.0 and not ztsnr:
        got = [err[o, S] for o in (1, 2) for S in (10, 20, 40, 80)]
        np.testing.assert_allclose(got, [0.146, 0.0995, 0.0629, 0.0372, 0.115, 0.0205, 0.0125, 0.0091], rtol=0.02)


# ---- 3. argument rules, before any device buffer exists ------------------------------------------------------------------------------
def test_argument_rules():
    from dm3d_amd import diffusion
    m = _model(20)
    x0 = np.zeros(SHAPE, F)
    calls = {"generate": lambda **kw: m.generate(SHAPE, context_value=1, **kw),
             "edit": lambda **kw: m.edit(x0, 1, **kw),
             "sampler": lambda sampler=None, **kw: m.sampler(SHAPE, 1, **({} if sampler is None else dict(kind=sampler)), **kw)}
    for name, call in calls.items():
        for sampler in ("ddpm", "ddim", "dpmpp"):
            with pytest.raises(ValueError, match="sde_eta"):
                call(sampler=sampler, sde_eta=1.0)
            with pytest.raises(ValueError, match="sde_eta"):
                call(sampler=sampler, sde_eta=0.0)
        with pytest.raises(ValueError, match="sde_eta"):
            call(sde_eta=0.5)                                                       # the default sampler
        with pytest.raises(ValueError, match="eta"):
            call(sampler="dpmpp_sde", num_steps=5, eta=0.5)
        for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match="sde_eta"):
                call(sampler="dpmpp_sde", num_steps=5, sde_eta=bad)
        for order in (0, 3):
            with pytest.raises(ValueError, match="solver_order"):
                call(sampler="dpmpp_sde", num_steps=5, solver_order=order)
        with pytest.raises(ValueError, match="negative_context"):
            call(sampler="dpmpp_sde", num_steps=5, guidance_scale=2.0)
        with pytest.raises(ValueError, match="clip_x0"):
            call(sampler="dpmpp_sde", num_steps=5, dynamic_threshold=0.9, clip_x0=False)
        with pytest.raises(ValueError):
            call(sampler="dpmpp_sde", num_steps=21)
        with pytest.raises(ValueError):
            call(sampler="dpm_sde")
        # the refusals of the deterministic solver hold, and name its stochastic form
        with pytest.raises(ValueError, match=r"eta.*dpmpp_sde"):
            call(sampler="dpmpp", num_steps=5, eta=0.5)
    for call in (calls["generate"], calls["edit"]):
        with pytest.raises(ValueError, match="noise"):
            call(sampler="dpmpp", num_steps=5, noise=np.zeros((5,) + SHAPE, F))
        with pytest.raises(ValueError, match="noise"):
            call(sampler="dpmpp_sde", num_steps=5, noise=np.zeros((4,) + SHAPE, F))      # the wrong leading size
    with pytest.raises(ValueError, match="noise"):
        m.edit(x0, 1, sampler="dpmpp_sde", num_steps=5, strength=0.6, noise=np.zeros((5,) + SHAPE, F))     # n = 3 rows
    with pytest.raises(ValueError, match="known_noise"):
        m.edit(x0, 1, sampler="dpmpp_sde", num_steps=5, strength=0.6, known_noise=np.zeros((5,) + SHAPE, F))
    with pytest.raises(ValueError, match="last_step"):
        m.generate(SHAPE, last_step=3, context_value=1, sampler="dpmpp_sde", num_steps=5)
    assert len(diffusion._CHAINS) == 12 and all(len(k) == 3 for k in diffusion._CHAINS)
    assert diffusion.dpm_sde_coefficients is __import__("dm3d_amd.schedules", fromlist=["x"]).dpm_sde_coefficients


def test_dpm_step_argument_rules():
    m = _model(20)
    x = np.zeros(SHAPE, F)
    with pytest.raises(ValueError, match="sde_eta"):
        m.dpm_step(x, x, 5, 3, noise=x)
    with pytest.raises(ValueError, match="sde_eta"):
        m.dpm_step(x, x, 5, 3, seed=4)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sde_eta"):
            m.dpm_step(x, x, 5, 3, sde_eta=bad)
    with pytest.raises(ValueError, match="noise"):
        m.dpm_step(x, x, 5, 3, sde_eta=1.0, noise=x[:1])
    with pytest.raises(ValueError, match="together"):
        m.dpm_step(x, x, 5, 3, x0_prev=x, sde_eta=1.0)


def test_zero_terminal_snr_refusals_name_the_stochastic_solver():
    m = _model(zero_terminal_snr=True, prediction="v")
    x = np.zeros(SHAPE, F)
    for call in (lambda: m.generate(SHAPE, context_value=1), lambda: m.edit(x, 1, sampler="ddpm"), lambda: m.sampler(SHAPE, 1),
                 lambda: m.sample(x, x, [3, 3], SHAPE)):
        with pytest.raises(ValueError, match="sampler='dpmpp_sde'"):
            call()


def test_signatures_are_keyword_only_extensions():
    from dm3d_amd import diffusion
    M = diffusion.DiffusionModel
    for fn in (M.generate, M.edit, M.sampler):
        p = inspect.signature(fn).parameters
        assert p["sde_eta"].kind == inspect.Parameter.KEYWORD_ONLY and p["sde_eta"].default is None
        assert p["eta"].default == 0.0
    st = inspect.signature(M.dpm_step).parameters
    for name in ("sde_eta", "noise", "seed"):
        assert st[name].kind == inspect.Parameter.KEYWORD_ONLY and st[name].default is None
    p = inspect.signature(diffusion.DpmSampler.__init__).parameters
    assert p["sde_eta"].default is None
    assert diffusion.DpmSampler.UPDATE == "dpm_update" and diffusion.DpmSampler.DRAWS is False        # the class stays the ODE solver


def test_graph_kinds():
    """The SDE mode's kind differs from every other kind of its plan and combines with the thresholded, converting and native ones."""
    from dm3d_amd import diffusion
    kind = diffusion.Sampler.graph_kind.fget
    classes = [c for c in diffusion._CHAINS.values()]
    plain = {kind(SimpleNamespace(KIND=c.KIND, threshold=thr, _pred_d=pred, native=nat, sde_eta=None))
             for c in classes for thr in (None, ()) for pred, nat in ((None, False), (object(), False), (None, True))}
    assert len(plain) == 12 * 6
    dpm = [c for c in classes if issubclass(c, diffusion.DpmSampler)]
    assert len(dpm) == 4
    sde = set()
    for c in dpm:
        for eta in (0.0, 1.0):                                              # eta is table contents: eta = 0 is an SDE chain too
            for thr in (None, ()):
                for pred, nat in ((None, False), (object(), False), (None, True)):
                    k = kind(SimpleNamespace(KIND=c.KIND, threshold=thr, _pred_d=pred, native=nat, sde_eta=eta))
                    assert k.startswith(c.KIND + "+sde") and ("+thr" in k) == (thr is not None)
                    assert ("+pred" in k) == (pred is not None) and ("+frame" in k) == nat
                    sde.add(k)
    assert len(sde) == 4 * 6 and not sde & plain
    assert kind(SimpleNamespace(KIND="dpmpp", threshold=None, _pred_d=None, native=False)) == "dpmpp"      # a stand-in without the mode


class _Stub:
    """Records what generate_sharded asks of DiffusionModel.generate."""

    def __init__(self):
        import torch
        self.device = torch.device("cpu")

    def generate(self, shape, last_step=0, context_value=None, **kw):
        import torch
        self.shape, self.kw = tuple(shape), kw
        return torch.zeros(shape)


def test_generate_sharded_forwards_sde_eta():
    from dm3d_amd import parallel
    m = _Stub()
    parallel.generate_sharded(m, (5, 2, 2, 2, 4), 0, 1, seed=7, sampler="dpmpp_sde", num_steps=8, sde_eta=0.5)
    assert m.kw == dict(seed=7, sampler="dpmpp_sde", num_steps=8, sde_eta=0.5)
    assert "sde_eta" in parallel.generate_sharded.__doc__


def test_device_table_layout():
    """_dpm_sde_table: _dpm_table's rows with c_z in column 6, rounded once to float32; at eta = 0 the two tables are bitwise equal."""
    from dm3d_amd.diffusion import ddim_timesteps, dpm_sde_coefficients
    m = _model(20)
    src, dst, prev = _chain_rows(ddim_timesteps(20, 5))
    tab = m._dpm_sde_table(src, dst, prev, 2, True, 1.0).numpy()
    rows = dpm_sde_coefficients(m.b.alpha_bar, src, dst, prev, 2, 1.0).astype(F)
    assert tab.dtype == F and tab.shape == (5, 8)
    assert np.array_equal(tab[:, 2:5], rows[:, :3]) and np.array_equal(tab[:, 6], rows[:, 3])
    assert np.all(tab[:, 5] == 1) and np.all(tab[:, 7] == 0)
    ode = m._dpm_table(src, dst, prev, 2, True).numpy()
    assert np.array_equal(tab[:, :2], ode[:, :2])
    assert np.array_equal(m._dpm_sde_table(src, dst, prev, 2, True, 0.0).numpy().view(np.int32), ode.view(np.int32))


# ---- 4. the ABI -------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("dm3d_dpm_sde_update", "dm3d_dpm_sde_update_frame")


def test_abi_entries_and_struct_layout(built_library, tmp_path):
    from dm3d_amd import _lib
    handle = ctypes.CDLL(built_library)
    header = open(os.path.join(ROOT, "include", "dm3d.h")).read()
    for name in ENTRIES:
        assert hasattr(handle, name) and name in _lib.SIGNATURES and re.search(r"\bint " + name + r"\(", header)
    assert len(_lib.SIGNATURES[ENTRIES[0]][1]) == 2 and len(_lib.SIGNATURES[ENTRIES[1]][1]) == 3
    assert _lib.lib().dm3d_version() == _lib.ABI_VERSION == 111                         # additive: the version stays
    fields = [name for name, _ in _lib.DpmSdeDesc._fields_]
    old = [name for name, _ in _lib.DpmDesc._fields_]
    assert fields == old + ["noise", "tau", "seed", "seed_dev"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dm3d.h"\nint main(){printf("%zu %zu", sizeof(dm3d_dpm_desc), sizeof(dm3d_dpm_sde_desc));\n'
                   + "".join(f'printf(" %zu", offsetof(dm3d_dpm_sde_desc, {f}));\n' for f in fields)
                   + "".join(f'printf(" %zu", offsetof(dm3d_dpm_desc, {f}));\n' for f in old) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size_old, size, *offs = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert size == ctypes.sizeof(_lib.DpmSdeDesc)
    assert offs[:len(fields)] == [getattr(_lib.DpmSdeDesc, f).offset for f in fields]
    assert size_old == ctypes.sizeof(_lib.DpmDesc) == 112                               # dm3d_dpm_desc is as it was
    assert offs[len(fields):] == [getattr(_lib.DpmDesc, f).offset for f in old] == offs[:len(old)]


def test_plain_c_program_calls_the_entries(built_library, tmp_path):
    """A C99 translation unit including only dm3d.h links; a null or empty descriptor is refused before any device call."""
    src = tmp_path / "sde.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "dm3d.h"
int main(void) {
    dm3d_dpm_sde_desc d;
    memset(&d, 0, sizeof d);
    printf("%d|%s\n", dm3d_dpm_sde_update(NULL, NULL), dm3d_last_error());
    printf("%d|%s\n", dm3d_dpm_sde_update(&d, NULL), dm3d_last_error());
    printf("%d|%s\n", dm3d_dpm_sde_update_frame(NULL, NULL, NULL), dm3d_last_error());
    printf("%d|%s\n", dm3d_dpm_sde_update_frame(&d, NULL, NULL), dm3d_last_error());
    return 0;
}
''')
    exe = tmp_path / "sde"
    libdir = os.path.dirname(built_library)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-ldm3d_hip", f"-Wl,-rpath,{libdir}"], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == 4
    for line in lines:
        rc, text = line.split("|", 1)
        assert int(rc) != 0 and "dpm_sde" in text
    assert "null descriptor" in lines[0] and "non-null" in lines[1] and "null descriptor" in lines[2] and "non-null" in lines[3]


def test_argument_validation_needs_no_gpu(built_library):
    from dm3d_amd import _lib
    lib = _lib.lib()

    def refused(d, word, frame=None):
        plain = lib.dm3d_dpm_sde_update(ctypes.byref(d), None) != 0 and word in lib.dm3d_last_error()
        lib.dm3d_fill(None, 0, 0.0, None)                                    # leaves another message behind
        framed = lib.dm3d_dpm_sde_update_frame(ctypes.byref(d), frame, None) != 0 and word in lib.dm3d_last_error()
        return plain and framed and b"dpm_sde" in lib.dm3d_last_error()

    assert lib.dm3d_dpm_sde_update(None, None) != 0 and b"null descriptor" in lib.dm3d_last_error()
    d = _lib.DpmSdeDesc()
    d.x = d.eps = d.coef = d.pos = d.hist = d.tau = 4096
    d.batch, d.per_sample, d.rows, d.mode = 2, 6, 4, 1                   # per_sample not a multiple of 4
    assert refused(d, b"per_sample")
    d.per_sample, d.batch = 8, 65536
    assert refused(d, b"batch")
    d.batch, d.mode = 2, 0                                               # mode 0 without out
    assert refused(d, b"out")
    d.mode, d.hist = 1, None                                             # mode 1 without the history
    assert refused(d, b"hist")
    d.hist, d.t_idx = 4096, 8192                                         # t_idx without t_next
    assert refused(d, b"t_next")
    d.t_idx, d.rows = None, 0
    assert refused(d, b"rows")
    d.rows, d.mode = 4, 2
    assert refused(d, b"mode")
    d.mode, d.hist = 1, 4100
    assert refused(d, b"aligned")
    d.hist, d.noise = 4096, 4104                                         # the injected z is read 16 bytes at a time too
    assert refused(d, b"aligned")
    d.noise, d.mode, d.out, d.x0_out = None, 0, 4096, 4104
    assert refused(d, b"aligned")
    d.x0_out, d.tau = None, None                                         # tau is required: the Philox counter
    assert refused(d, b"non-null")
    d.tau, d.pos = 4096, None
    assert refused(d, b"non-null")
    d.pos = 4096
    assert lib.dm3d_dpm_sde_update_frame(ctypes.byref(d), 4100, None) != 0 and b"aligned" in lib.dm3d_last_error()     # the frame rows


# ---- 5. compile quality ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_build_without_scratch_and_stream_16_bytes_per_lane(tmp_path):
    """dpm_sde_kernel and dpm_sde_frame_kernel for gfx950: no scratch, no spill, no LDS, few registers (a stream kernel must not limit
    its own occupancy), and the loop moves float4s only: every vector load from global memory is 16 bytes wide (x, eps, hist, noise;
    the tables arrive through the scalar cache), and so is every store but the one lane's 4 bytes of t_idx ahead of the loop."""
    out = str(tmp_path / "dm3d_dpm_sde.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function",
                    "-ffp-contract=off", "-S", "--cuda-device-only", os.path.join(CSRC, "dm3d_dpm_sde.hip"), "-o", out], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    for kernel in ("dpm_sde_kernel", "dpm_sde_frame_kernel"):
        meta = re.search(r"\.name:\s+\S*" + kernel + r"\S*\n[\s\S]*?\.vgpr_spill_count:\s+(\d+)", text)
        assert meta and int(meta.group(1)) == 0, kernel
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", meta.group(0)).group(1)) == 0
        block = re.search(r"\.amdhsa_kernel \S*" + kernel + r"\S*\n[\s\S]*?\.end_amdhsa_kernel", text).group(0)
        field = lambda name: int(re.search(r"\.amdhsa_" + name + r"\s+(\d+)", block).group(1))
        assert field("private_segment_fixed_size") == 0 and field("group_segment_fixed_size") == 0, kernel
        assert field("next_free_vgpr") <= 64, kernel
    assert len(re.findall(r"\.amdhsa_kernel ", text)) == 2
    body = [l.strip() for l in text.splitlines()]
    assert not [l for l in body if l.startswith(("scratch_", "ds_", "buffer_", "flat_"))]
    loads = [l for l in body if l.startswith("global_load_")]
    stores = [l for l in body if l.startswith("global_store_")]
    assert len(loads) >= 2 * 4 and all(l.startswith("global_load_dwordx4") for l in loads)              # x, eps, hist, noise per kernel
    narrow = [l for l in stores if not l.startswith("global_store_dwordx4")]
    assert len(stores) - len(narrow) >= 2 * 2                                                           # x and the x0 estimate per kernel
    assert len(narrow) == 2 and all(l.startswith("global_store_dword ") for l in narrow)                # t_idx[b], once per kernel
    assert not [l for l in body if l.startswith("global_atomic")]
