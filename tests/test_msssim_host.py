"""CPU tier of the 3-D multi-scale SSIM (no kernel is launched): dm3d_ms_ssim is declared, exported and bound and refuses every documented
bad argument; csrc/dm3d_msssim.hip compiles for gfx950 without spill, scratch, MFMA or atomics; the numpy restatement the GPU tests
compare against (tests/msssim_reference.py) checks itself against closed forms; its bar is what it measures; its inputs keep every
per-scale term away from the clamp; the Python wrappers refuse what they document."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import msssim_reference as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 0x10000                                   # an aligned non-null "pointer": nothing is launched, so nothing dereferences it

OK = dict(x=A, y=A, x_index=0, y_index=0, pairs=2, nx=2, ny=2, d=24, h=26, w=44, cx=1, cy=2, x0c=0, y0c=0, nc=1, filter_size=11,
          filter_sigma=1.5, scales=2, power_factors=(0.0448, 0.2856, 0.3001, 0.2363, 0.1333), max_val=A, out=A, partials=A,
          partials_elems=1 << 20, scratch=A, scratch_elems=1 << 24)
# (override, words the message must hold).  24 x 26 x 44 with 11 taps: scale 0 has 14 x 16 x 34 outputs, 1 x 1 x 2 tiles; scale 1 is
# 12 x 13 x 22 with 2 x 3 x 12 outputs, one tile: 3 tiles, 2 * 2 * 1 * 3 = 12 doubles; (2 + 2) * 1 * 12 * 13 * 22 = 13728 pooled floats.
BAD = [
    (dict(x=0), "non-null"), (dict(y=0), "non-null"), (dict(max_val=0), "non-null"), (dict(out=0), "non-null"), (dict(partials=0), "non-null"),
    (dict(scratch=0), "scratch must be non-null"),
    (dict(d=21), "at most 1 scales fit"), (dict(h=21), "smaller than filter_size=11"), (dict(w=10, scales=1), "at most 0 scales fit"),
    (dict(d=128, h=128, w=128, scales=5), "at most 4 scales fit"),
    (dict(filter_size=10), "filter_size=10"), (dict(filter_size=13), "filter_size=13"), (dict(filter_size=1), "filter_size=1"),
    (dict(filter_sigma=0.0), "filter_sigma=0"),
    (dict(scales=0), "scales=0"), (dict(scales=6), "scales=6"),
    (dict(power_factors=(0.5, 0.0, 1, 1, 1)), "power_factors[1]=0"), (dict(power_factors=(-0.25, 0.5, 1, 1, 1)), "power_factors[0]=-0.25"),
    (dict(nc=2), "outside x's cx=1"), (dict(x0c=1), "outside x's cx=1"), (dict(x0c=-1), "outside x"),
    (dict(y0c=2), "outside y's cy=2"), (dict(cx=2, nc=2, y0c=1), "outside y's cy=2"), (dict(y0c=-1), "outside y"), (dict(nc=0), "nc=0"),
    (dict(x_index=A, y_index=A, pairs=0), "pairs=0"), (dict(pairs=0), "pairs=0"), (dict(pairs=65536, x_index=A, y_index=A), "pairs=65536"),
    (dict(pairs=3), "exceeds nx=2"), (dict(pairs=3, x_index=A), "exceeds ny=2"), (dict(nx=0), "nx=0"), (dict(d=0), "d=0"),
    (dict(partials_elems=11), "partials holds 11 doubles, 12 are needed"),
    (dict(x_index=A, y_index=A, pairs=45, nx=10, ny=10, d=128, h=128, w=128, scales=4, partials_elems=2 * 45 * (128 + 16 + 2 + 1) - 1),
     "partials holds 13229 doubles, 13230 are needed"),
    (dict(scratch_elems=13727), "scratch holds 13727 floats, 13728 are needed"),
    (dict(partials=A + 4), "8-byte aligned"),
]


def _desc(_lib, **override):
    d = _lib.MsSsimDesc()
    for k, v in {**OK, **override}.items():
        if k == "power_factors":
            for j, w in enumerate(v):
                d.power_factors[j] = w
        else:
            setattr(d, k, v)
    return d


def test_entry_is_declared_exported_and_bound(built_library):
    from dm3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dm3d.h")).read()
    assert re.search(r"\bint dm3d_ms_ssim\(const dm3d_ms_ssim_desc\* d, void\* stream\);", header)
    assert hasattr(C.CDLL(built_library), "dm3d_ms_ssim")
    assert _lib.SIGNATURES["dm3d_ms_ssim"] == (C.c_int, [C.POINTER(_lib.MsSsimDesc), C.c_void_p])
    assert _lib.lib().dm3d_version() == _lib.ABI_VERSION == 111 and "#define DM3D_VERSION 111 " in header
    # the ctypes mirror has the header's fields, in its order
    body = re.search(r"typedef struct dm3d_ms_ssim_desc \{(.*?)\} dm3d_ms_ssim_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n).strip(" *") for decl in body.split(";") if decl.strip()
             for n in decl.strip().split(" ", 1 + decl.strip().startswith("const"))[-1].split(",")]
    assert names == [f[0] for f in _lib.MsSsimDesc._fields_]
    assert dict(_lib.MsSsimDesc._fields_)["power_factors"] is C.c_float * 5 and "float power_factors[5];" in header
    assert _lib.MSSSIM_TILE == ms.TILE
    for k, v in zip(("TD", "TH", "TW"), ms.TILE):
        assert f"#define DM3D_MSSSIM_{k} {v}\n" in header
    # the documented element counts are the ones the entry asks for (the two "holds .. are needed" rows of BAD) and ops computes
    assert "partials_elems  >= 2 * pairs * nc * sum_{j < scales} tiles_j" in header
    assert "scratch_elems   >= (nx + ny) * nc * sum_{1 <= j < scales} (d >> j)(h >> j)(w >> j)" in header


def test_entry_refuses_bad_arguments(built_library):
    """Every documented precondition is checked before anything is launched: DM3D_EINVAL and a message that starts "ms_ssim:" and names
    the fault, with no GPU in the machine."""
    from dm3d_amd import _lib
    lib = _lib.lib()
    failures = []
    for override, words in BAD:
        lib.dm3d_fill(None, 0, 0.0, None)                           # leaves a known message behind
        rc = lib.dm3d_ms_ssim(C.byref(_desc(_lib, **override)), None)
        msg = (lib.dm3d_last_error() or b"").decode()
        if rc != -1 or not msg.startswith("ms_ssim:") or words not in msg:
            failures.append(f"dm3d_ms_ssim({override}): rc {rc}, message {msg!r}, wanted {words!r}")
    if lib.dm3d_ms_ssim(None, None) != -1 or b"ms_ssim: null descriptor" not in lib.dm3d_last_error():
        failures.append("dm3d_ms_ssim(NULL)")
    assert not failures, "\n".join(failures)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_msssim_kernels_compile_without_spill_or_scratch(tmp_path):
    """The gfx950 listing of csrc/dm3d_msssim.hip (the library's flags): the tile kernel at each of its five window sizes, the pooling and
    the sum kernel, none with a spilled register or scratch."""
    import subprocess
    out = str(tmp_path / "dm3d_msssim.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function",
                    "-ffp-contract=off", "-S", "--cuda-device-only", os.path.join(ROOT, "3d-condtional-stable-diffusion_amd", "csrc", "dm3d_msssim.hip"),
                    "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    rows = re.findall(r"\.name:\s+(\S+)[\s\S]*?\.private_segment_fixed_size:\s+(\d+)[\s\S]*?\.sgpr_spill_count:\s+(\d+)[\s\S]*?\.vgpr_spill_count:\s+(\d+)", text)
    names = [r[0] for r in rows]
    for k in ["msssim_pool_kernel", "msssim_sum_kernel"] + [f"msssim_tile_kernelILi{f}E" for f in (3, 5, 7, 9, 11)]:
        assert any(k in n for n in names), (k, names)
    assert all(int(a) == 0 and int(b) == 0 and int(c) == 0 for _, a, b, c in rows), rows
    assert not re.search(r"^\s*(v_mfma|scratch_|global_atomic|flat_atomic|ds_add)", text, re.M)


def test_python_wrappers_refuse_what_they_document():
    from dm3d_amd import metrics, ops
    assert metrics.ms_ssim is ops.ms_ssim and {"ms_ssim", "pairwise_ms_ssim", "sample_diversity"} <= set(metrics.__all__)
    x = torch.zeros(2, 12, 12, 12, 1)
    kw = dict(power_factors=(0.5, 0.5), filter_size=3)
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        ops.ms_ssim(x, x, 1.0, **kw)
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        metrics.pairwise_ms_ssim(x, 1.0, **kw)
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        metrics.sample_diversity(x, 1.0, **kw)
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(0, 2, dtype=torch.int64),
                torch.zeros(2, 2), [[0, 1]]):
        with pytest.raises(ValueError, match=r"pairs must be an int32 or int64 tensor \[P, 2\]"):
            ops.ms_ssim(x, x, 1.0, pairs=bad, **kw)
    with pytest.raises(ValueError, match="max_val=None .* pair table"):
        ops.ms_ssim(x, x, None, pairs=torch.zeros(1, 2, dtype=torch.int64), **kw)
    with pytest.raises(ValueError, match="needs max_val"):
        metrics.pairwise_ms_ssim(x, None, **kw)
    with pytest.raises(ValueError, match="B >= 2"):
        metrics.pairwise_ms_ssim(x[:1], 1.0, **kw)
    with pytest.raises(ValueError, match="filter_size must be odd"):
        ops.ms_ssim(x, x, 1.0, filter_size=4)
    with pytest.raises(ValueError, match="1 to 5 positive"):
        ops.ms_ssim(x, x, 1.0, power_factors=(0.5, 0.0))
    assert ops.ms_ssim_max_scales((128, 128, 128), 11) == 4 and ops.ms_ssim_max_scales((12, 12, 12), 3) == 3
    assert ops.MS_SSIM_POWER_FACTORS == ms.POWER_FACTORS


# ---- the restatement against closed forms ------------------------------------------------------------------------------------------------
def test_window_follows_the_existing_table():
    import metrics_reference as mr
    assert np.array_equal(ms.window(11, 1.5), mr.window())                     # the rule of dm3d_ssim's G[] table
    for f in (3, 5, 7, 9, 11):
        g = ms.window(f, 1.5)
        assert g.shape == (f,) and abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == f // 2
        assert abs(g[f // 2 - 1] / g[f // 2] - math.exp(-1 / 4.5)) < 1e-15


def test_identical_volumes_score_exactly_one():
    x, _ = ms.make_pair((2, 13, 12, 14), ms.CHANNELS[1])
    for kw in (dict(power_factors=ms.POWER_FACTORS[:3], filter_size=3), dict(power_factors=(1.0,), filter_size=11),
               dict(max_val=0.37, power_factors=ms.POWER_FACTORS[:2], filter_size=5)):
        assert np.array_equal(ms.ms_ssim(x, x, **kw), np.ones(2))              # numerators and denominators are the same numbers


@pytest.mark.parametrize("a,b,L", [(0.3, 0.7, 1.0), (0.5, 0.5, 0.25), (0.9, 0.1, 2.0)])
def test_constant_pair_is_the_luminance_closed_form(a, b, L):
    x = np.full((1, 12, 13, 12, 1), a, np.float32)
    y = np.full((1, 12, 13, 12, 1), b, np.float32)
    a, b = float(np.float32(a)), float(np.float32(b))
    c1 = (0.01 * float(np.float32(L))) ** 2
    lum = (2 * a * b + c1) / (a * a + b * b + c1)                               # every cs = c2 / c2 = 1: only the last scale's lum is left
    w = ms.POWER_FACTORS[:3]
    got, per = ms.ms_ssim(x, y, L, w, 3, terms=True)
    assert all(np.abs(cs - 1).max() < 1e-9 for cs, _ in per)
    assert got.shape == (1,) and abs(got[0] - lum ** float(np.float32(w[2]))) < 1e-9, (got, lum)


def test_single_scale_is_the_direct_triple_loop():
    """M = 1, power factor 1, D = filter_size: the 3-D windowed SSIM by a direct loop over the window, on a tiny input."""
    f = 3
    x, y = ms.make_pair((1, f, 5, 6), (1, 0, 1, 0, 1), seed=3)
    L = 0.8
    g = ms.window(f)
    w3 = g[:, None, None] * g[None, :, None] * g[None, None, :]
    c1, c2 = (0.01 * float(np.float32(L))) ** 2, (0.03 * float(np.float32(L))) ** 2
    xv, yv = x[0, ..., 0].astype(np.float64), y[0, ..., 0].astype(np.float64)
    vals = []
    for i in range(5 - f + 1):
        for j in range(6 - f + 1):
            mx = my = sxx = syy = sxy = 0.0
            for dz in range(f):
                for dy in range(f):
                    for dx in range(f):
                        wt, p, q = w3[dz, dy, dx], xv[dz, i + dy, j + dx], yv[dz, i + dy, j + dx]
                        mx, my, sxx, syy, sxy = mx + wt * p, my + wt * q, sxx + wt * p * p, syy + wt * q * q, sxy + wt * p * q
            vals.append((2 * mx * my + c1) / (mx * mx + my * my + c1) * (2 * (sxy - mx * my) + c2) / (sxx - mx * mx + syy - my * my + c2))
    got = ms.ms_ssim(x, y, L, (1.0,), f)
    assert got.shape == (1,) and abs(got[0] - np.mean(vals)) < 1e-12, (got, np.mean(vals))


def test_symmetry_channels_and_pooling():
    x, y = ms.make_pair((2, 13, 9, 22), ms.CHANNELS[1])
    kw = dict(max_val=0.8, power_factors=ms.POWER_FACTORS[:2], filter_size=3)
    s = ms.ms_ssim(x, y, **kw)
    assert np.array_equal(s, ms.ms_ssim(y, x, **kw))                           # every term is symmetric in x and y, operation by operation
    assert (s > 0.2).all() and (s < 0.9999).all(), s
    per = [ms.ms_ssim(x[..., c:c + 1], y[..., c:c + 1], **kw) for c in range(2)]
    assert np.abs(s - (per[0] + per[1]) / 2).max() < 1e-15                     # the mean over channels
    # pooling of an odd edge drops the last plane: what lies there changes nothing past scale 0
    p = ms.pool(x.astype(np.float64))
    assert p.shape == (2, 6, 4, 11, 2)
    assert p[1, 2, 3, 4, 1] == x[1, 4:6, 6:8, 8:10, 1].astype(np.float64).mean()
    x2 = x.copy()
    x2[:, 12], x2[:, :, 8] = 0.25, 0.75                                         # the dropped planes of D = 13 and H = 9
    assert np.array_equal(ms.pool(x2.astype(np.float64)), p) and np.array_equal(ms.pool(x2), ms.pool(x))
    xt = torch.from_numpy(x.astype(np.float64)).permute(0, 4, 1, 2, 3)
    assert np.abs(torch.nn.functional.avg_pool3d(xt, 2).permute(0, 2, 3, 4, 1).numpy() - p).max() < 1e-15
    assert not np.array_equal(ms.ms_ssim(x2, y, **kw), s)                       # ... while scale 0 still sees them


def test_too_many_scales_are_refused_with_the_usable_count():
    z = np.zeros((1, 128, 128, 128, 1), np.float32)
    with pytest.raises(ValueError, match="at most 4 scales fit"):
        ms.ms_ssim(z, z, 1.0)                                                  # 128 >> 4 = 8 < 11
    assert ms.max_scales((128, 128, 128), 11) == 4 and ms.max_scales((12, 40, 40), 3) == 3 and ms.max_scales((10, 40, 40), 11) == 0


# ---- the bar and the inputs ----------------------------------------------------------------------------------------------------------
def test_the_bar_is_what_the_restatement_measures():
    """MSSSIM_TOL is four times the worst |f32 - f64| of the restatement over the inputs of the GPU cases."""
    worst, per = ms.measured_worst()
    for k, e in per.items():
        print(f"{k}: {e:.3e}")
    print(f"worst |f32 - f64|: {worst:.4e}")
    assert worst <= ms.MSSSIM_F32_WORST <= 1.01 * worst
    assert ms.MSSSIM_TOL == 4 * ms.MSSSIM_F32_WORST
    ids = [ms.case_id(c) for c in ms.CASES]
    assert len(set(ids)) == len(ids)
    # the shapes the issue names, and on each axis one tile exactly and one point past it
    shapes = {(c[0][1:], c[2], c[3]) for c in ms.CASES}
    assert {((12, 12, 12), 3, 3), ((13, 9, 22), 3, 2), ((16, 16, 16), 7, 2), ((22, 23, 44), 11, 2)} <= shapes
    for axis, edge in enumerate(ms.TILE):
        for extra in (0, 1):
            assert any(c[0][1 + axis] == edge + c[2] - 1 + extra for c in ms.CASES), (axis, extra)
    assert {c[1] for c in ms.CASES} == set(ms.CHANNELS)


def test_inputs_keep_every_term_away_from_the_clamp():
    """On every GPU case the reference's per-scale cs and ssim are at least 0.05: max(., 0) and the powers never hide an error."""
    for case in ms.CASES:
        out, per = ms.reference(case)
        assert len(per) == case[3]
        low = min(float(min(cs.min(), s.min())) for cs, s in per)
        assert low >= 0.05 and np.isfinite(out).all() and (out < 0.9999).all(), (ms.case_id(case), low, out)
    for name, (xr, yr, mv, power, f) in ms.extra_inputs().items():
        out, per = ms.ms_ssim(xr, yr, mv, power, f, terms=True)
        low = min(float(min(cs.min(), s.min())) for cs, s in per)
        assert low >= 0.05 and (out < 0.9999).all() and len(set(out.tolist())) == len(out), (name, low, out)
