"""CPU tier of the reconstruction metrics (no kernel is launched): the three entries of the C ABI are declared, exported and bound and
refuse every documented bad argument; the numpy restatement the GPU tests compare against (tests/metrics_reference.py) checks itself
against closed forms; the bars it carries are what it measures; the Mean tracker counts like keras.metrics.Mean; the autoencoders
carry test_step / evaluate."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import metrics_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dm3d_pair_stats", "dm3d_ssim", "dm3d_psnr_finalize")
A = 0x10000                                   # an aligned non-null "pointer": nothing is launched, so nothing dereferences it

OK = dict(x=A, y=A, batch=2, d=3, h=16, w=20, cx=1, cy=2, x0c=0, y0c=0, nc=1, partials=A, partials_elems=1 << 20, y_min=A, y_max=A, y_range=A,
          sse=A, max_val=A, out=A)
# (entries, override, words the message must hold)
BAD = [
    (ENTRIES[:2], dict(x=0), "non-null"), (ENTRIES[:2], dict(y=0), "non-null"), (ENTRIES[:2], dict(partials=0), "non-null"),
    (ENTRIES[:1], dict(y_min=0), "non-null"), (ENTRIES[:1], dict(y_max=0), "non-null"), (ENTRIES[:1], dict(sse=0), "non-null"),
    (ENTRIES[1:], dict(max_val=0), "non-null"), (ENTRIES[1:], dict(out=0), "non-null"), (ENTRIES[2:], dict(sse=0), "non-null"),
    (ENTRIES[1:2], dict(h=10), "h=10"), (ENTRIES[1:2], dict(w=10), "w=10"), (ENTRIES, dict(h=0), "h=0"), (ENTRIES, dict(w=0), "w=0"),
    (ENTRIES, dict(nc=0), "nc=0"), (ENTRIES, dict(batch=0), "batch=0"), (ENTRIES, dict(d=65536), "d=65536"),
    (ENTRIES[:2], dict(nc=2), "outside x's cx=1"), (ENTRIES[:2], dict(x0c=1), "outside x's cx=1"), (ENTRIES[:2], dict(x0c=-1), "outside x"),
    (ENTRIES[:2], dict(y0c=2), "outside y's cy=2"), (ENTRIES[:2], dict(cx=2, nc=2, y0c=1), "outside y's cy=2"), (ENTRIES[:2], dict(y0c=-1), "outside y"),
    (ENTRIES[:1], dict(partials_elems=3 * 2 * 3 * 1 - 1), "17 doubles, 18 are needed"),
    (ENTRIES[:1], dict(h=128, w=128, partials_elems=3 * 2 * 3 * 4 - 1), "71 doubles, 72 are needed"),
    (ENTRIES[1:2], dict(partials_elems=2 * 3 * 1 * 1 - 1), "5 doubles, 6 are needed"),
    (ENTRIES[1:2], dict(h=43, w=75, cx=2, nc=2, partials_elems=2 * 3 * 2 * 2 * 3 - 1), "71 doubles, 72 are needed"),
    (ENTRIES[:2], dict(partials=A + 4), "8-byte aligned"), (ENTRIES[:1], dict(sse=A + 4), "8-byte aligned"), (ENTRIES[2:], dict(sse=A + 4), "8-byte aligned"),
]


def _desc(_lib, **override):
    d = _lib.MetricDesc()
    for k, v in {**OK, **override}.items():
        setattr(d, k, v)
    return d


def test_entries_are_declared_exported_and_bound(built_library):
    from dm3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dm3d.h")).read()
    handle = C.CDLL(built_library)
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(const dm3d_metric_desc\* d, void\* stream\);", header), name
        assert hasattr(handle, name), name
        assert _lib.SIGNATURES[name] == (C.c_int, [C.POINTER(_lib.MetricDesc), C.c_void_p])
    assert _lib.lib().dm3d_version() == _lib.ABI_VERSION == 111
    # the ctypes mirror has the header's fields, in its order
    body = re.search(r"typedef struct dm3d_metric_desc \{(.*?)\} dm3d_metric_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.strip().split(" ", 1 + decl.strip().startswith("const"))[-1].split(",")]
    assert names == [f[0] for f in _lib.MetricDesc._fields_]
    assert (_lib.PAIR_PARTIAL_BLOCKS, _lib.SSIM_TILE) == (64, mr.TILE)
    assert "#define DM3D_PAIR_PARTIAL_BLOCKS 64" in header and f"#define DM3D_SSIM_TILE {mr.TILE}" in header


def test_entries_refuse_bad_arguments(built_library):
    """Every documented precondition is checked before anything is launched: DM3D_EINVAL and a message that names the entry and the
    fault, with no GPU in the machine."""
    from dm3d_amd import _lib
    lib = _lib.lib()
    failures = []
    for entries, override, words in BAD:
        for entry in entries:
            lib.dm3d_fill(None, 0, 0.0, None)                       # leaves a known message behind
            rc = getattr(lib, entry)(C.byref(_desc(_lib, **override)), None)
            msg = (lib.dm3d_last_error() or b"").decode()
            if rc != -1 or not msg.startswith(entry[5:] + ":") or words not in msg:
                failures.append(f"{entry}({override}): rc {rc}, message {msg!r}, wanted {words!r}")
    for entry in ENTRIES:
        if getattr(lib, entry)(None, None) != -1 or b"null descriptor" not in lib.dm3d_last_error():
            failures.append(f"{entry}(NULL)")
    assert not failures, "\n".join(failures)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_metric_kernels_compile_without_spill_or_scratch(tmp_path):
    """The gfx950 listing of csrc/dm3d_metrics.hip (the library's flags): five kernels, none with a spilled register or scratch."""
    import subprocess
    out = str(tmp_path / "dm3d_metrics.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function",
                    "-ffp-contract=off", "-S", "--cuda-device-only", os.path.join(ROOT, "3d-condtional-stable-diffusion_amd", "csrc", "dm3d_metrics.hip"),
                    "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    rows = re.findall(r"\.name:\s+(\S+)[\s\S]*?\.private_segment_fixed_size:\s+(\d+)[\s\S]*?\.sgpr_spill_count:\s+(\d+)[\s\S]*?\.vgpr_spill_count:\s+(\d+)", text)
    names = [r[0] for r in rows]
    for k in ("pair_stats_kernel", "pair_stats_sum_kernel", "ssim_tile_kernel", "ssim_sum_kernel", "psnr_kernel"):
        assert any(k in n for n in names), (k, names)
    assert all(int(a) == 0 and int(b) == 0 and int(c) == 0 for _, a, b, c in rows), rows
    assert not re.search(r"^\s*(v_mfma|scratch_|global_atomic|flat_atomic|ds_add)", text, re.M)


def test_python_wrappers_refuse_bad_shapes():
    from dm3d_amd import ops
    x = torch.zeros(1, 2, 12, 12, 1)
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        ops.pair_stats(x, x)


# ---- the restatement against closed forms ------------------------------------------------------------------------------------------------
def test_window_and_identity():
    g = mr.window()
    assert g.shape == (11,) and abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert abs(g[4] / g[5] - math.exp(-1 / 4.5)) < 1e-15
    x, _ = mr.make_pair((2, 3, 17, 23), mr.CHANNELS[1])
    assert np.array_equal(mr.ssim(x, x), np.ones((2, 3)))          # exactly 1 in float64: numerators and denominators are the same numbers
    assert np.array_equal(mr.ssim(x, x, 0.37), np.ones((2, 3)))
    assert np.isposinf(mr.psnr(x, x)).all()


@pytest.mark.parametrize("a,b,L", [(0.3, 0.7, 1.0), (0.5, 0.5, 0.25), (0.9, 0.1, 2.0)])
def test_constant_pair_is_the_closed_form(a, b, L):
    x = np.full((1, 2, 11, 11, 1), a, np.float32)
    y = np.full((1, 2, 11, 11, 1), b, np.float32)
    a, b = float(np.float32(a)), float(np.float32(b))
    c1 = (0.01 * float(np.float32(L))) ** 2
    want = (2 * a * b + c1) / (a * a + b * b + c1)                  # cs = c2 / c2 = 1: the filtered second moments cancel
    got = mr.ssim(x, y, L)
    assert got.shape == (1, 2) and np.abs(got - want).max() < 1e-9, (got, want)   # c2 = 9e-4 L^2 against a cancellation residue of 1e-16
    assert np.abs(mr.ssim(x, y, L, "f32") - want).max() < 1e-2      # a few float32 ulps of a^2 + b^2 against c2 >= 5.6e-5
    # max_val = 0 (max_val = None on a constant y) leaves what the formula leaves: on an all-zero pair 0/0, NaN, as TensorFlow gives
    z = np.zeros_like(x)
    assert np.isnan(mr.ssim(z, z)).all() and np.isnan(mr.ssim(z, z, order="f32")).all()


def test_ssim_is_symmetric_and_bounded():
    x, y = mr.make_pair((2, 2, 37, 50), mr.CHANNELS[1])
    s = mr.ssim(x, y, 0.8)
    assert np.array_equal(s, mr.ssim(y, x, 0.8))                   # every term is symmetric in x and y, operation by operation
    assert (s > 0.2).all() and (s < 0.999).all(), s
    two = mr.ssim(x, y, 0.8)
    per = [mr.ssim(x[..., c:c + 1], y[..., c:c + 1], 0.8) for c in range(2)]
    assert np.abs(two - (per[0] + per[1]) / 2).max() < 1e-15       # the mean over channels


def test_psnr_on_a_hand_made_slice():
    x = np.zeros((1, 1, 2, 2, 1), np.float32)
    y = np.array([0.5, 0.0, -0.5, 0.0], np.float32).reshape(1, 1, 2, 2, 1)
    # mse = (0.25 + 0.25) / 4 = 0.125; max - min = 1
    assert abs(mr.psnr(x, y)[0, 0] - (-10 * math.log10(0.125))) < 1e-12
    assert abs(mr.psnr(x, y, 2.0)[0, 0] - (20 * math.log10(2.0) - 10 * math.log10(0.125))) < 1e-12
    assert abs(mr.psnr(x, y, 2.0, "f32")[0, 0] - mr.psnr(x, y, 2.0)[0, 0]) < 2e-6
    assert mr.sse(x, y)[0, 0] == 0.5


def test_the_bars_are_what_the_restatement_measures():
    """SSIM_TOL / PSNR_TOL are four times the worst |f32 - f64| of the restatement over the inputs of the GPU cases; no input is too
    flat for float32 (1e-4)."""
    ws, wp, per = mr.measured_worst()
    for k, (es, ep) in per.items():
        print(f"{k}: ssim {es:.3e}  psnr {ep:.3e} dB")
    print(f"worst |f32 - f64|: ssim {ws:.4e}, psnr {wp:.4e} dB")
    assert all(es <= 1e-4 for es, _ in per.values())
    assert ws <= mr.SSIM_F32_WORST <= 1.01 * ws and wp <= mr.PSNR_F32_WORST <= 1.01 * wp
    assert mr.SSIM_TOL == 4 * mr.SSIM_F32_WORST and mr.PSNR_TOL == 4 * mr.PSNR_F32_WORST
    ids = [mr.case_id(c) for c in mr.cases()]
    assert len(set(ids)) == len(ids)
    for t in (mr.TILE + 10, mr.TILE + 11):
        assert any(s[2] == t for s in mr.SHAPES) and any(s[3] == t for s in mr.SHAPES)


# ---- the tracker ---------------------------------------------------------------------------------------------------------------------
def test_mean_tracker_counts_elements():
    from dm3d_amd.metrics import Mean
    import dm3d_amd
    assert dm3d_amd.metrics.Mean is Mean
    m = Mean("psnr")
    assert m.name == "psnr"
    r = m.result()
    assert r.dim() == 0 and r.dtype == torch.float64 and float(r) == 0.0          # before any update
    m.update_state(torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]))            # six values
    m.update_state(torch.tensor(10.0))                                           # one
    assert int(m.count) == 7 and float(m.result()) == 31.0 / 7.0
    assert m.result().dim() == 0
    m.reset_state()
    assert float(m.result()) == 0.0
    m.update_state(torch.tensor([2.0], dtype=torch.float32))
    assert float(m.result()) == 2.0
    # float64 accumulation: a float32 sum would lose the small terms
    m.reset_state()
    m.update_state(torch.tensor([1e8], dtype=torch.float32))
    m.update_state(torch.ones(100, dtype=torch.float32))
    assert float(m.result()) == (1e8 + 100) / 101


# ---- the autoencoders' interface -----------------------------------------------------------------------------------------------------
def test_autoencoders_carry_test_step_and_evaluate():
    from dm3d_amd.networks.vqgan import VQGAN
    from dm3d_amd.networks.vqvae3d_monai import VQVAE
    for cls in (VQVAE, VQGAN):
        assert list(inspect.signature(cls.test_step).parameters) == ["self", "data"]
        assert list(inspect.signature(cls.evaluate).parameters) == ["self", "batches"]
        assert isinstance(cls.metrics, property) and callable(cls.reset_metrics)
        assert isinstance(cls.last_loss, property)
    assert VQVAE.METRIC_KEYS == ("loss", "reconst_loss", "quantize_loss", "ssim", "psnr")
    assert VQGAN.METRIC_KEYS == ("reconst_loss", "quantize_loss", "ssim", "psnr")
    assert VQGAN.test_step is not VQVAE.test_step
    doc = VQGAN.test_step.__doc__
    for key in ("loss", "gen_loss", "gen_feat_loss", "disc_loss", "perceptual_loss"):
        assert f"``{key}``" in doc, key
    assert "discriminators" in doc and "LPIPS" in doc
    vq = VQVAE(2, 2, (8, 8), 1, (8, 8), downsample_parameters=((2, 4, 1, "same"),) * 2, upsample_parameters=((2, 4, 1, "same", 0),) * 2,
               num_embeddings=16, embedding_dim=8, input_size=16, device="cpu")
    assert [m.name for m in vq.metrics] == list(VQVAE.METRIC_KEYS)
    assert all(float(m.result()) == 0.0 for m in vq.metrics)
    with pytest.raises(RuntimeError, match="has not been called"):
        vq.last_loss
    assert vq.evaluate([]) == {k: 0.0 for k in VQVAE.METRIC_KEYS}
