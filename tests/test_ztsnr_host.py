"""CPU tier of the zero-terminal-SNR schedule (Lin et al. 2023, Algorithm 1) and of the update kernels' ``frame`` path: why the feature
exists (the eps frame's x0 estimate is 0/0 at alpha_bar = 0, the frame form is not), the schedule's tables, the frame table, the
coefficient rows at alpha_bar = 0, the grown threshold descriptor and the new update entries, every refusal, the checkpoint entry and the kernels' build (nothing is launched)."""
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


def _model(T=20, B=2, cls=None, **kw):
    from dm3d_amd.networks import conditional_dm3d
    cls = conditional_dm3d.DiffusionModel if cls is None else cls
    return cls(8, 1024, 4, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B), device="cpu", **kw)


def _linear64(T):
    """Today's schedule, written out: float64 alpha_bar of the linear 1e-4 .. 0.02 betas."""
    return np.cumprod(1 - np.linspace(0.0001, 0.02, T), 0)


def _ztsnr64(T):
    """Algorithm 1 of Lin et al. on the linear schedule, in float64, written independently of betas.py."""
    r = np.sqrt(_linear64(T))
    r0, rT = r[0], r[-1]
    r = (r - rT) * (r0 / (r0 - rT))
    return r ** 2


# ---- the reason ------------------------------------------------------------------------------------------------------------------------
def test_eps_frame_has_no_x0_at_zero_alpha_bar_and_the_frame_form_has():
    """dm3d_pred_to_eps followed by dm3d_x0_estimate, restated in float32: (x - s*eps) / a with eps = c_p*v + c_x*x.  At the rescaled
    schedule's last timestep a = 0 and s = 1: eps is x and the estimate 0/0, for any finite x and v.  The frame rows give -v and x."""
    from dm3d_amd.betas import Betas
    from dm3d_amd.diffusion import frame_table, prediction_table
    T = 1000
    b = Betas(T, zero_terminal_snr=True)
    rng = np.random.default_rng(0)
    x, v = (rng.standard_normal(4096).astype(F) * F(3) for _ in range(2))
    c_p, c_x = prediction_table(b.alpha_bar, "v")[T - 1]
    eps = c_p * v + c_x * x
    sqab, sq1ab = b.sqrt_alpha_bar[T - 1], b.sqrt_one_minus_alpha_bar[T - 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        x0 = (x - sq1ab * eps) / sqab                                        # dm3d_x0_estimate: mul, sub, div
    assert x0.dtype == F and np.all(np.isnan(x0))
    k0x, k0p, kex, kep = frame_table(b.alpha_bar, "v")[T - 1]
    x0_f, eps_f = k0x * x + k0p * v, kex * x + kep * v                       # the frame form: mul, mul, add
    assert x0_f.dtype == F
    assert np.array_equal(x0_f.view(np.int32), (-v).view(np.int32)) and np.array_equal(eps_f.view(np.int32), x.view(np.int32))
    # the plain schedule never gets there: its last alpha_bar is about 4e-5
    assert 3e-5 < Betas(T).alpha_bar[T - 1] < 5e-5


# ---- the schedule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 20, 50, 300, 1000])
def test_betas_zero_terminal_snr_tables(T):
    from dm3d_amd.betas import BETAS_FIELDS, Betas
    b, plain = Betas(T, zero_terminal_snr=True), Betas(T)
    assert b.zero_terminal_snr is True and plain.zero_terminal_snr is False
    for f in BETAS_FIELDS:
        assert getattr(b, f).dtype == F and getattr(b, f).shape == (T,) and np.all(np.isfinite(getattr(b, f)))
    assert b.alpha_bar[T - 1] == 0.0 and b.sqrt_alpha_bar[T - 1] == 0.0 and b.sqrt_one_minus_alpha_bar[T - 1] == 1.0
    assert b.alpha_bar[0] == plain.alpha_bar[0]
    assert np.all(np.diff(b.alpha_bar.astype(np.float64)) < 0)
    ab = _ztsnr64(T)
    np.testing.assert_allclose(b.alpha_bar, ab.astype(F), rtol=2e-7, atol=0)           # one float32 ulp of the restatement
    alpha = np.append(ab[0], ab[1:] / ab[:-1])
    np.testing.assert_allclose(b.alpha, alpha.astype(F), rtol=2e-7, atol=1e-12)
    np.testing.assert_allclose(b.beta, (1 - alpha).astype(F), rtol=1e-5, atol=1e-9)
    assert b.alpha[T - 1] == 0.0 and b.beta[T - 1] == 1.0
    np.testing.assert_array_equal(b.alpha_bar_prev[1:], b.alpha_bar[:-1])
    assert b.alpha_bar_prev[0] == 1.0


@pytest.mark.parametrize("T", [1, 20, 1000])
def test_default_tables_are_bitwise_the_linear_schedule(T):
    from dm3d_amd.betas import Betas
    beta = np.linspace(0.0001, 0.02, T)
    alpha = 1 - beta
    ab = np.cumprod(alpha, 0)
    prev = np.append(1.0, ab[:-1])
    want = dict(beta=beta, alpha=alpha, sqrt_alpha=np.sqrt(alpha), alpha_bar=ab, alpha_bar_prev=prev, sqrt_alpha_bar=np.sqrt(ab),
                sqrt_alpha_bar_prev=np.sqrt(prev), sqrt_one_minus_alpha_bar=np.sqrt(1 - ab))
    for b in (Betas(T), Betas(T, zero_terminal_snr=False), Betas(T, False)):
        for name, v in want.items():
            assert np.array_equal(getattr(b, name).view(np.int32), v.astype(F).view(np.int32)), name
    with pytest.raises(ValueError):
        Betas(1, zero_terminal_snr=True)


# ---- the frame table -------------------------------------------------------------------------------------------------------------------
def _frame64(ab, kind):
    rows = []
    for v in ab:
        a, s = math.sqrt(v), math.sqrt(1.0 - v)
        rows.append({"v": (a, -s, s, a), "x0": (0.0, 1.0, 1.0 / s, -a / s), "eps": (1.0 / a if a else 0.0, -s / a if a else 0.0, 0.0, 1.0)}[kind])
    return np.array(rows)


@pytest.mark.parametrize("T", [50, 1000])
@pytest.mark.parametrize("ztsnr", [False, True])
@pytest.mark.parametrize("kind", ["v", "x0", "eps"])
def test_frame_table_against_float64_restatement(T, ztsnr, kind):
    from dm3d_amd import diffusion, schedules
    from dm3d_amd.betas import Betas
    assert diffusion.frame_table is schedules.frame_table                    # re-exported
    ab32 = Betas(T, zero_terminal_snr=ztsnr).alpha_bar
    if kind == "eps" and ztsnr:
        with pytest.raises(ValueError, match="alpha_bar"):
            schedules.frame_table(ab32, kind)
        return
    got = schedules.frame_table(ab32, kind)
    assert got.dtype == F and got.shape == (T, 4)
    want = _frame64(ab32.astype(np.float64), kind)
    ulp = np.spacing(np.abs(want).astype(F)).astype(np.float64)
    assert np.all(np.abs(got.astype(np.float64) - want) <= ulp)
    if ztsnr:
        assert got[T - 1].tolist() == {"v": [0.0, -1.0, 1.0, 0.0], "x0": [0.0, 1.0, 1.0, 0.0]}[kind]


@pytest.mark.parametrize("ztsnr", [False, True])
@pytest.mark.parametrize("kind", ["v", "x0"])
def test_frame_rows_invert_the_forward_process_in_float64(ztsnr, kind):
    """x_t = a x0 + s z and the exact v or x0: the float64 rows give x0 and z back within 1e-12 at every t, T-1 included."""
    T = 1000
    ab = _ztsnr64(T) if ztsnr else _linear64(T)
    rows = _frame64(ab, kind)
    rng = np.random.default_rng(1)
    x0, z = rng.standard_normal((2, T, 16))
    a, s = np.sqrt(ab)[:, None], np.sqrt(1 - ab)[:, None]
    x = a * x0 + s * z
    pred = a * z - s * x0 if kind == "v" else x0
    back0 = rows[:, 0:1] * x + rows[:, 1:2] * pred
    backz = rows[:, 2:3] * x + rows[:, 3:4] * pred
    assert np.abs(back0 - x0).max() < 1e-12
    assert np.abs(backz - z).max() < 1e-12                                   # (x0 rows: through 1/s <= 100, 1e-14 at the worst)


# ---- coefficient rows ------------------------------------------------------------------------------------------------------------------
def _dpm_parent(alpha_bar, src, dst, prev, order=2):
    """dpm_coefficients as it stood before alpha_bar = 0 was legal, copied: the rows of a schedule without a zero stay bitwise these."""
    ab = np.asarray(alpha_bar, dtype=np.float64)
    src, dst, prev = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (src, dst, prev))
    lam = lambda a: 0.5 * (np.log(a) - np.log1p(-a))
    a_s, a_t, a_p = ab[src], ab[np.maximum(dst, 0)], ab[np.maximum(prev, 0)]
    h = lam(a_t) - lam(a_s)
    c_x = np.sqrt((1 - a_t) / (1 - a_s))
    A = -np.sqrt(a_t) * np.expm1(-h)
    second = (prev >= 0) & (dst >= 0) & (order == 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(second, h / (2 * (lam(a_s) - lam(a_p))), 0.0)
    out = np.stack([c_x, A * (1 + g), -A * g], axis=1)
    out[dst < 0] = (0.0, 1.0, 0.0)
    return out


def _ddim_parent(alpha_bar, src, dst, eta=0.0):
    ab = np.asarray(alpha_bar, dtype=np.float64)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    a = ab[src]
    ap = np.where(dst < 0, 1.0, ab[np.maximum(dst, 0)])
    sigma = np.zeros_like(a)
    if eta != 0:
        sigma = float(eta) * np.sqrt((1 - ap) / (1 - a)) * np.sqrt(1 - a / ap)
    a_eps = np.sqrt(np.maximum(1 - ap - sigma ** 2, 0.0))
    return np.stack([np.sqrt(a), np.sqrt(1 - a), np.sqrt(ap), a_eps, sigma], axis=1)


def _rows(taus, order=2, lof=True):
    taus = [int(v) for v in taus]
    prev = taus[1:] + [-1]
    if order == 1:
        prev = [-1] * len(taus)
    if lof and len(taus) > 1:
        prev[1] = -1
    return taus, [-1] + taus[:-1], prev


@pytest.mark.parametrize("S", [1, 2, 10, 20])
@pytest.mark.parametrize("lof", [True, False])
def test_dpm_rows_at_zero_alpha_bar(S, lof):
    from dm3d_amd.betas import Betas
    from dm3d_amd.diffusion import ddim_coefficients, ddim_timesteps, dpm_coefficients
    T = 1000
    ab = Betas(T, zero_terminal_snr=True).alpha_bar
    src, dst, prev = _rows(ddim_timesteps(T, S), 2, lof)
    with np.errstate(all="raise"):                                           # the limits are taken quietly
        c = dpm_coefficients(ab, src, dst, prev)
    assert c.shape == (S, 3) and not np.isnan(c).any() and np.all(np.isfinite(c))
    assert src[-1] == T - 1 and ab[src[-1]] == 0.0
    if S > 1:
        a_t = float(ab[dst[-1]])
        np.testing.assert_allclose(c[-1], [math.sqrt(1 - a_t), math.sqrt(a_t), 0.0], rtol=1e-15, atol=0)      # (sigma_t, alpha_t, 0)
        assert c[-1, 2] == 0.0
    else:
        assert c[0].tolist() == [0.0, 1.0, 0.0]
    if S > 2:
        # the row after it: prev is the level at -inf, 1/(2r) = 0: first order, c_1 exactly 0, the first-order c_0
        first = dpm_coefficients(ab, src, dst, [-1] * S)
        assert c[-2, 2] == 0.0 and c[-2].tolist()[:2] == first[-2].tolist()[:2]
        if not lof and S > 3:
            assert c[-3, 2] != 0.0                                           # and the one after that is second order again
    # a history level given for the first row changes nothing: the row from alpha_bar = 0 is first order whatever prev says
    if S > 1:
        forced = dpm_coefficients(ab, [src[-1]], [dst[-1]], [src[-1]])
        assert np.isfinite(forced).all() and forced[0, 2] == 0.0
    for eta in (0.0, 0.5, 1.0):
        d = ddim_coefficients(ab, src, dst, eta)
        assert np.all(np.isfinite(d))
        assert d[-1, 0] == 0.0 and d[-1, 1] == 1.0


@pytest.mark.parametrize("T,S", [(1000, 20), (1000, 7), (300, 50), (20, 5), (50, 50)])
def test_rows_of_the_linear_schedule_are_bitwise_what_they_were(T, S):
    from dm3d_amd.betas import Betas
    from dm3d_amd.diffusion import ddim_coefficients, ddim_timesteps, dpm_coefficients
    ab = Betas(T).alpha_bar
    for order, lof in ((2, True), (2, False), (1, True)):
        src, dst, prev = _rows(ddim_timesteps(T, S), order, lof)
        got, want = dpm_coefficients(ab, src, dst, prev, order), _dpm_parent(ab, src, dst, prev, order)
        assert np.array_equal(got.view(np.int64), want.view(np.int64))
    for eta in (0.0, 0.3, 1.0):
        got, want = ddim_coefficients(ab, src, dst, eta), _ddim_parent(ab, src, dst, eta)
        assert np.array_equal(got.view(np.int64), want.view(np.int64))
    inv = ddim_coefficients(ab, src[:-1], src[1:])                          # inversion rows
    assert np.array_equal(inv.view(np.int64), _ddim_parent(ab, src[:-1], src[1:]).view(np.int64))


# ---- training tables -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["v", "x0"])
def test_objective_rows_are_finite_at_zero_alpha_bar(kind):
    from dm3d_amd.betas import Betas
    from dm3d_amd.diffusion import objective_rows
    T = 1000
    b = Betas(T, zero_terminal_snr=True)
    t = [T - 1, T - 2, 0]
    with np.errstate(all="raise"):
        plain, snr = objective_rows(b.alpha_bar, t, kind), objective_rows(b.alpha_bar, t, kind, "min_snr", 5.0)
    assert np.all(np.isfinite(plain)) and np.all(np.isfinite(snr))
    assert plain[0].tolist() == ([0.0, -1.0, 1.0, 0.0] if kind == "v" else [0.0, 1.0, 1.0, 0.0])
    assert snr[0, 2] == 0.0 and snr[1, 2] > 0.0                              # min-SNR weighs the pure-noise timestep 0
    # q_sample's level row there: x_t = z
    assert b.sqrt_alpha_bar[T - 1] == 0.0 and b.sqrt_one_minus_alpha_bar[T - 1] == 1.0


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_thresh_descriptor_grew_by_one_trailing_pointer(built_library, tmp_path):
    from dm3d_amd import _lib
    S, cname = _lib.ThreshDesc, "dm3d_thresh_desc"
    fields = [name for name, _ in S._fields_]
    assert fields[-1] == "frame"
    assert _lib.lib().dm3d_version() == _lib.ABI_VERSION == 111
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <string.h>\n#include "dm3d.h"\n'
                   f'int main(void){{{cname} d; memset(&d, 0, sizeof d); printf("%d %zu", d.frame == NULL, sizeof({cname}));\n'
                   + "".join(f'printf(" %zu", offsetof({cname}, {f}));\n' for f in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    null, size, *offs = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert null == 1
    assert size == ctypes.sizeof(S) and offs == [getattr(S, f).offset for f in fields]
    assert offs[-1] == size - 8 and S.frame.offset == offs[-1]              # the last member, behind everything there was
    assert not S().frame


def test_update_descriptors_are_unchanged_and_the_frame_entries_take_the_table(built_library, tmp_path):
    """dm3d_ddim_desc and dm3d_dpm_desc keep x0_bound as their last member (their layouts are what they were): the frame table is an
    argument of the new entries.  A C99 translation unit calls them; a null descriptor is refused before any device call."""
    from dm3d_amd import _lib
    for S, size in ((_lib.DdimDesc, 128), (_lib.DpmDesc, 112)):
        assert [n for n, _ in S._fields_][-1] == "x0_bound" and ctypes.sizeof(S) == size
    handle = ctypes.CDLL(built_library)
    for name in ("dm3d_ddim_update_frame", "dm3d_dpm_update_frame"):
        assert hasattr(handle, name) and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 3
    src = tmp_path / "fr.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "dm3d.h"
int main(void) {
    dm3d_ddim_desc d; dm3d_dpm_desc p;
    memset(&d, 0, sizeof d); memset(&p, 0, sizeof p);
    printf("%d|%s\n", dm3d_ddim_update_frame(NULL, NULL, NULL), dm3d_last_error());
    printf("%d|%s\n", dm3d_ddim_update_frame(&d, NULL, NULL), dm3d_last_error());
    printf("%d|%s\n", dm3d_dpm_update_frame(NULL, NULL, NULL), dm3d_last_error());
    printf("%d|%s\n", dm3d_dpm_update_frame(&p, NULL, NULL), dm3d_last_error());
    printf("%zu %zu\n", sizeof d, sizeof p);
    return 0;
}
''')
    exe = tmp_path / "fr"
    libdir = os.path.dirname(built_library)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-ldm3d_hip", f"-Wl,-rpath,{libdir}"], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, word in zip(lines[:4], ("null descriptor", "non-null", "null descriptor", "non-null")):
        rc, text = line.split("|", 1)
        assert int(rc) != 0 and word in text
    assert lines[4].split() == ["128", "112"]


def test_frame_must_be_16_byte_aligned(built_library):
    from dm3d_amd import _lib
    lib = _lib.lib()
    d = _lib.DdimDesc()
    d.x = d.eps = d.coef = d.tau = d.pos = 4096
    d.batch, d.per_sample, d.rows, d.mode = 2, 8, 4, 1
    assert lib.dm3d_ddim_update_frame(ctypes.byref(d), 4100, None) != 0 and b"aligned" in lib.dm3d_last_error()
    p = _lib.DpmDesc()
    p.x = p.eps = p.coef = p.pos = p.hist = 4096
    p.batch, p.per_sample, p.rows, p.mode = 2, 8, 4, 1
    assert lib.dm3d_dpm_update_frame(ctypes.byref(p), 4104, None) != 0 and b"aligned" in lib.dm3d_last_error()
    t = _lib.ThreshDesc()
    t.x = t.eps = t.coef = t.pos = t.rank = t.frac = t.smax = t.bound = t.scratch = 4096
    t.batch, t.per_sample, t.rows, t.frame = 2, 8, 4, 4108
    assert lib.dm3d_x0_threshold(ctypes.byref(t), None) != 0 and b"aligned" in lib.dm3d_last_error()


# ---- the public interface --------------------------------------------------------------------------------------------------------------
def test_constructor_keyword_on_both_model_classes():
    from dm3d_amd import diffusion
    for cls in (diffusion.DiffusionModel, diffusion.UnconditionalDiffusionModel):
        p = inspect.signature(cls.__init__).parameters
        assert p["zero_terminal_snr"].kind == inspect.Parameter.KEYWORD_ONLY and p["zero_terminal_snr"].default is False
        assert list(p).index("zero_terminal_snr") == list(p).index("prediction") + 1
        with pytest.raises(ValueError, match="eps"):
            _model(cls=cls, zero_terminal_snr=True)
        with pytest.raises(ValueError, match="eps"):
            _model(cls=cls, zero_terminal_snr=True, prediction="eps")
        for kind in ("v", "x0"):
            m = _model(cls=cls, zero_terminal_snr=True, prediction=kind)
            assert m.zero_terminal_snr is True and m.b.alpha_bar[-1] == 0.0
        plain = _model(cls=cls, prediction="v")
        assert plain.zero_terminal_snr is False and plain.b.alpha_bar[-1] > 0.0
    M = diffusion.DiffusionModel
    for fn in (M.ddim_step, M.dpm_step, M.x0_threshold):
        p = inspect.signature(fn).parameters["prediction"]
        assert p.kind == inspect.Parameter.KEYWORD_ONLY and p.default is None


def test_refusals_name_the_alternative():
    m = _model(zero_terminal_snr=True, prediction="v")
    x = np.zeros(SHAPE, F)
    for call in (lambda: m.generate(SHAPE, context_value=1), lambda: m.generate(SHAPE, context_value=1, sampler="ddpm"),
                 lambda: m.edit(x, 1), lambda: m.edit(x, 1, sampler="ddpm", strength=0.5), lambda: m.sampler(SHAPE, 1),
                 lambda: m.sampler(SHAPE, 1, kind="ddpm")):
        with pytest.raises(ValueError, match=r"sampler='ddim', eta=1\.0"):
            call()
    with pytest.raises(ValueError, match="ddim_step"):
        m.sample(x, x, [3, 3], SHAPE)
    with pytest.raises(ValueError, match="invert"):
        m.invert(x, 1, num_steps=5)
    for call in (lambda: m.ddim_step(x, x, 5, 3, prediction="eps"), lambda: m.dpm_step(x, x, 5, 3, prediction="w"),
                 lambda: m.x0_threshold(x, x, 5, 0.9, prediction="eps")):
        with pytest.raises(ValueError, match="prediction"):
            call()
    u = _model(cls=__import__("dm3d_amd.diffusion", fromlist=["x"]).UnconditionalDiffusionModel, zero_terminal_snr=True, prediction="x0")
    with pytest.raises(ValueError, match=r"sampler='ddim', eta=1\.0"):
        u.generate(SHAPE)
    with pytest.raises(ValueError, match="invert"):
        u.invert(x, num_steps=5)
    # a model on the plain schedule refuses none of this at the rule stage (it fails later, for want of a device)
    plain = _model(prediction="v")
    taus, opts = plain._solver_rules("ddpm", None, None, 0.0, True, 2, True)
    assert len(taus) == 20 and opts == {}
    taus, opts = m._solver_rules("ddim", 5, None, 1.0, True, 2, True)
    assert len(taus) == 5 and opts == dict(eta=1.0, clip_x0=True)


def test_native_chain_kinds_have_their_own_suffix():
    from dm3d_amd import diffusion
    for cls in (diffusion.DdimSampler, diffusion.DpmSampler, diffusion.GuidedDdimSampler, diffusion.DpmEditSampler):
        base = SimpleNamespace(KIND=cls.KIND, threshold=None, _pred_d=None, native=False)
        assert diffusion.Sampler.graph_kind.fget(base) == cls.KIND
        kinds = {diffusion.Sampler.graph_kind.fget(SimpleNamespace(KIND=cls.KIND, threshold=thr, _pred_d=pred, native=nat))
                 for thr in (None, ()) for pred, nat in ((None, False), (object(), False), (None, True))}
        assert len(kinds) == 6
        native = diffusion.Sampler.graph_kind.fget(SimpleNamespace(KIND=cls.KIND, threshold=None, _pred_d=None, native=True))
        assert native.startswith(cls.KIND) and "+pred" not in native and native != cls.KIND


def test_checkpoint_round_trip_and_mismatch(tmp_path):
    m = _model(zero_terminal_snr=True, prediction="v")
    path = str(tmp_path / "z.npz")
    m.save_weights(path)
    sd = dict(np.load(path))
    assert bool(sd["meta/zero_terminal_snr"]) is True and str(sd["meta/prediction"]) == "v"
    _model(zero_terminal_snr=True, prediction="v").load_weights(path)
    plain = _model(prediction="v")
    before = {k: v.copy() for k, v in plain.network.state_dict().items()}
    with pytest.raises(ValueError, match="zero_terminal_snr"):
        plain.load_weights(path)
    after = plain.network.state_dict()
    assert all(np.array_equal(before[k], after[k]) for k in before)           # refused before anything was touched
    # a checkpoint without the entry loads anywhere, and a plain model writes none
    ppath = str(tmp_path / "p.npz")
    plain.save_weights(ppath)
    assert "meta/zero_terminal_snr" not in dict(np.load(ppath))
    m.load_weights(ppath)


# ---- the kernels' build ----------------------------------------------------------------------------------------------------------------
def _asm(name, tmp_path):
    """(assembly, {kernel name: (VGPRs, SGPRs, waves per SIMD)} from the compiler's resource report) of one translation unit."""
    out = str(tmp_path / (name + ".s"))
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function",
                          "-ffp-contract=off", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(CSRC, name + ".hip"), "-o", out], check=True, capture_output=True, text=True)
    report = {}
    for m in re.finditer(r"Function Name: (\S+)[\s\S]*?TotalSGPRs: (\d+)[\s\S]*?VGPRs: (\d+)[\s\S]*?Occupancy \[waves/SIMD\]: (\d+)", res.stderr):
        report[m.group(1)] = (int(m.group(3)), int(m.group(2)), int(m.group(4)))
    return open(out).read(), report


def _kernel(text, report, kernel):
    """(instructions from the kernel's label to its descriptor, its .amdhsa block, its resource row): ``kernel`` is the whole source
    name, so "ddim_kernel" does not match ddim_frame_kernel."""
    lines = [l.strip() for l in text.splitlines()]
    label = re.compile(r"^(_Z\S*\d+" + kernel + r"E\S*):")
    k0 = next(i for i, l in enumerate(lines) if label.match(l))
    name = label.match(lines[k0]).group(1)
    k1 = next(i for i in range(k0, len(lines)) if lines[i].startswith(".amdhsa_kernel"))
    k2 = next(i for i in range(k1, len(lines)) if lines[i].startswith(".end_amdhsa_kernel"))
    return lines[k0:k1], "\n".join(lines[k1:k2]), report[name]


def _count(body, prefix):
    return sum(l.startswith(prefix) for l in body)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("name,eps_kernel,frame_kernel,loads,stores", [("dm3d_ddim", "ddim_kernel", "ddim_frame_kernel", 3, 1),
                                                                       ("dm3d_dpm", "dpm_kernel", "dpm_frame_kernel", 3, 2)])
def test_update_kernels_of_both_frames(tmp_path, name, eps_kernel, frame_kernel, loads, stores):
    """The update has one kernel per frame, chosen by the host.  Both move float4s (``loads`` / ``stores`` 16-byte accesses a lane: x, the
    prediction, z or the history; the result, the estimate), without scratch, spill or LDS, and both keep 8 waves per SIMD (the
    compiler's own report: a register count that costs the stream its occupancy fails here).  The frame kernel has fewer divisions than
    the eps kernel: the estimate's are gone, the dynamic bound's stay."""
    text, report = _asm(name, tmp_path)
    divs = {}
    for kernel in (eps_kernel, frame_kernel):
        body, block, (vgprs, sgprs, waves) = _kernel(text, report, kernel)
        field = lambda f: int(re.search(r"\.amdhsa_" + f + r"\s+(\d+)", block).group(1))
        print(f"{kernel}: {vgprs} VGPRs, {sgprs} SGPRs, {waves} waves/SIMD")
        assert field("private_segment_fixed_size") == 0 and field("group_segment_fixed_size") == 0
        assert vgprs <= 64 and waves == 8
        assert not [l for l in body if l.startswith(("scratch_", "ds_"))]
        assert _count(body, "global_load_dwordx4") >= loads and _count(body, "global_store_dwordx4") >= stores
        divs[kernel] = _count(body, "v_div_fmas_f32")
    assert 0 < divs[frame_kernel] < divs[eps_kernel]
    assert not re.search(r"\.vgpr_spill_count:\s+[1-9]", text) and not re.search(r"\.sgpr_spill_count:\s+[1-9]", text)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_threshold_pass1_holds_both_streams(tmp_path):
    """thresh_pass1_kernel holds its stream once per frame (the branch is uniform and outside the loop): two 16-byte loads and the
    16-byte stash store of either, no scratch, no spill, the histogram's LDS, 8 waves per SIMD; its only divisions are the eps stream's
    estimate (the other kernels of the file divide nothing)."""
    text, report = _asm("dm3d_thresh", tmp_path)
    body, block, (vgprs, sgprs, waves) = _kernel(text, report, "thresh_pass1_kernel")
    field = lambda f: int(re.search(r"\.amdhsa_" + f + r"\s+(\d+)", block).group(1))
    print(f"thresh_pass1_kernel: {vgprs} VGPRs, {sgprs} SGPRs, {waves} waves/SIMD")
    assert field("private_segment_fixed_size") == 0 and 0 < field("group_segment_fixed_size") <= 16384
    assert vgprs <= 64 and waves == 8
    assert not [l for l in body if l.startswith("scratch_")]
    assert _count(body, "global_load_dwordx4") >= 4 and _count(body, "global_store_dwordx4") >= 2
    whole = [l.strip() for l in text.splitlines()]
    assert 0 < _count(body, "v_div_fmas_f32") == _count(whole, "v_div_fmas_f32")
    assert not re.search(r"\.vgpr_spill_count:\s+[1-9]", text)
