"""CPU tier of the mask-channel scores (no kernel is launched): dm3d_mask_overlap, dm3d_edt and dm3d_surface_distance are declared,
exported and bound and refuse every documented bad argument; csrc/dm3d_mask.hip compiles for gfx950 without spill or scratch; the numpy
restatement the GPU tests compare against (tests/mask_reference.py) checks itself against closed forms and, where scipy is installed,
against scipy.ndimage on the inputs of the GPU tests; the Python wrappers refuse what they document."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import mask_reference as mk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 0x10000                                   # an aligned non-null "pointer": nothing is launched, so nothing dereferences it
ENTRIES = {"mask_overlap": "dm3d_mask_overlap", "edt": "dm3d_edt", "surface_distance": "dm3d_surface_distance"}

# 2 x 5 x 7 x 9 x 2 compared channels: 1260 voxels; bins = 16 + 36 + 64 + 1 = 117; work = 1260 + 2 * 4 * 118 = 2204 int32
OK = dict(x=A, y=A, batch=2, d=5, h=7, w=9, cx=3, cy=2, x0c=1, y0c=0, nc=2, threshold=0.5, of=0, percentile=95.0, counts=A, surf_x=0, surf_y=0,
          map=A, out=A, masks=A, masks_elems=1 << 20, work=A, work_elems=1 << 20)
ALL = tuple(ENTRIES)
# (entries, override, words the message must hold)
BAD = [
    (ALL, dict(x=0), "x must be non-null"),
    (("mask_overlap", "surface_distance"), dict(y=0), "y must be non-null"),
    (("mask_overlap",), dict(counts=0), "counts must be non-null"),
    (("mask_overlap",), dict(surf_x=A), "both given or both null"),
    (("mask_overlap",), dict(counts=A + 4), "8-byte aligned"),
    (("edt",), dict(map=0), "map and masks must be non-null"), (("edt",), dict(masks=0), "map and masks must be non-null"),
    (("surface_distance",), dict(out=0), "out, masks and work must be non-null"),
    (("surface_distance",), dict(masks=0), "out, masks and work must be non-null"),
    (("surface_distance",), dict(work=0), "out, masks and work must be non-null"),
    (("surface_distance",), dict(out=A + 4), "8-byte aligned"), (("surface_distance",), dict(work=A + 2), "4-byte aligned"),
    (ALL, dict(nc=3), "outside x's cx=3"), (ALL, dict(x0c=2), "outside x's cx=3"), (ALL, dict(x0c=-1), "outside x"),
    (("mask_overlap", "surface_distance"), dict(y0c=1), "outside y's cy=2"), (("mask_overlap", "surface_distance"), dict(y0c=-1), "outside y"),
    (("mask_overlap", "surface_distance"), dict(cx=4, nc=3), "outside y's cy=2"),
    (ALL, dict(d=0), "d=0"), (ALL, dict(h=0), "h=0"), (ALL, dict(w=0), "w=0"), (ALL, dict(batch=0), "batch=0"), (ALL, dict(nc=0), "nc=0"),
    (ALL, dict(d=513), "d=513 h=7 w=9 exceeds DM3D_EDT_MAX_EXTENT=512"), (ALL, dict(h=513), "exceeds DM3D_EDT_MAX_EXTENT=512"),
    (ALL, dict(w=513), "exceeds DM3D_EDT_MAX_EXTENT=512"),
    (ALL, dict(batch=32768), "batch * nc = 65536"),
    (ALL, dict(threshold=float("nan")), "threshold=nan"), (ALL, dict(threshold=float("inf")), "threshold=inf"),
    (("edt",), dict(of=2), "of=2"), (("edt",), dict(of=-1), "of=-1"),
    (("surface_distance",), dict(percentile=0.0), "percentile=0"), (("surface_distance",), dict(percentile=100.5), "percentile=100.5"),
    (("surface_distance",), dict(percentile=-5.0), "percentile=-5"), (("surface_distance",), dict(percentile=float("nan")), "percentile=nan"),
    (("edt",), dict(masks_elems=1259), "masks holds 1259 bytes, 1260 are needed"),
    (("surface_distance",), dict(masks_elems=2519), "masks holds 2519 bytes, 2520 are needed"),
    (("surface_distance",), dict(work_elems=2203), "work holds 2203 int32, 2204 are needed"),
    (("surface_distance",), dict(batch=8, d=128, h=128, w=128, cx=1, cy=1, x0c=0, nc=1, masks_elems=1 << 30,
                                 work_elems=8 * (128 ** 3 + 2 * (3 * 127 ** 2 + 2)) - 1), "work holds 17551439 int32, 17551440 are needed"),
]


def _desc(_lib, **override):
    d = _lib.MaskDesc()
    for k, v in {**OK, **override}.items():
        setattr(d, k, v)
    return d


def test_entries_are_declared_exported_and_bound(built_library):
    from dm3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dm3d.h")).read()
    handle = C.CDLL(built_library)
    for name in ENTRIES.values():
        assert re.search(r"\bint %s\(const dm3d_mask_desc\* d, void\* stream\);" % name, header), name
        assert hasattr(handle, name), name
        assert _lib.SIGNATURES[name] == (C.c_int, [C.POINTER(_lib.MaskDesc), C.c_void_p]), name
    assert _lib.lib().dm3d_version() == _lib.ABI_VERSION == 111 and "#define DM3D_VERSION 111 " in header
    # the ctypes mirror has the header's fields, in its order, with its types
    body = re.search(r"typedef struct dm3d_mask_desc \{(.*?)\} dm3d_mask_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in (s.strip() for s in body.split(";")):
        if decl:
            ctype, names = decl.removeprefix("const ").split(" ", 1)
            fields += [(n.strip(" *"), ctype + ("*" if "*" in ctype + names else "")) for n in names.split(",")]
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
    assert [f[0] for f in fields] == [f[0] for f in _lib.MaskDesc._fields_]
    for (name, ctype), (_, mirror) in zip(fields, _lib.MaskDesc._fields_):
        assert mirror is (C.c_void_p if ctype.endswith("*") else kinds[ctype]), (name, ctype, mirror)
    assert f"#define DM3D_EDT_MAX_EXTENT {_lib.EDT_MAX_EXTENT}\n" in header and _lib.EDT_MAX_EXTENT == 512
    assert f"#define DM3D_EDT_SURFACE {_lib.EDT_SURFACE}\n" in header and f"#define DM3D_EDT_FOREGROUND {_lib.EDT_FOREGROUND}\n" in header
    # the documented element counts are the ones the entries ask for (the "holds .. are needed" rows of BAD) and ops computes
    assert "masks_elems >= batch * nc * d * h * w " in header and "masks_elems >= 2 * batch * nc * d * h * w " in header
    assert "work_elems  >= batch * nc * (d * h * w + 2 * (bins + 1))" in header and "bins         = (d-1)^2 + (h-1)^2 + (w-1)^2 + 1" in header


def test_entries_refuse_bad_arguments(built_library):
    """Every documented precondition is checked before anything is launched: DM3D_EINVAL and a message that starts with the entry's short
    name and names the fault, with no GPU in the machine."""
    from dm3d_amd import _lib
    lib = _lib.lib()
    failures = []
    for entries, override, words in BAD:
        for short in entries:
            lib.dm3d_fill(None, 0, 0.0, None)                       # leaves a known message behind
            rc = getattr(lib, ENTRIES[short])(C.byref(_desc(_lib, **override)), None)
            msg = (lib.dm3d_last_error() or b"").decode()
            if rc != -1 or not msg.startswith(short + ":") or words not in msg:
                failures.append(f"{ENTRIES[short]}({override}): rc {rc}, message {msg!r}, wanted {words!r}")
    for short, name in ENTRIES.items():
        if getattr(lib, name)(None, None) != -1 or f"{short}: null descriptor".encode() not in lib.dm3d_last_error():
            failures.append(f"{name}(NULL)")
    assert not failures, "\n".join(failures)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_mask_kernels_compile_without_spill_or_scratch(tmp_path):
    """The gfx950 listing of csrc/dm3d_mask.hip (the library's flags): every kernel is there, none with a spilled register or a private
    segment."""
    import subprocess
    out = str(tmp_path / "dm3d_mask.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function",
                    "-ffp-contract=off", "-S", "--cuda-device-only", os.path.join(ROOT, "3d-condtional-stable-diffusion_amd", "csrc", "dm3d_mask.hip"),
                    "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    rows = re.findall(r"\.name:\s+(\S+)[\s\S]*?\.private_segment_fixed_size:\s+(\d+)[\s\S]*?\.sgpr_spill_count:\s+(\d+)[\s\S]*?\.vgpr_spill_count:\s+(\d+)", text)
    names = [r[0] for r in rows]
    for k in ("mask_zero_kernel", "mask_feature_kernel", "edt_pass_kernelILb0E", "edt_pass_kernelILb1E", "mask_hist_kernel", "mask_stat_kernel"):
        assert any(k in n for n in names), (k, names)
    assert all(int(a) == 0 and int(b) == 0 and int(c) == 0 for _, a, b, c in rows), rows


def test_python_wrappers_refuse_what_they_document():
    from dm3d_amd import metrics, ops
    from dm3d_amd.networks.vqvae3d_monai import VQVAE
    assert metrics.mask_overlap is ops.mask_overlap and metrics.surface_distances is ops.surface_distances
    assert {"NanMean", "dice", "iou", "hausdorff", "mask_metrics", "distance_transform"} <= set(metrics.__all__)
    x = torch.zeros(2, 4, 4, 4, 1)
    for fn in (ops.mask_overlap, ops.surface_distances, metrics.dice, metrics.iou, metrics.hausdorff, metrics.mask_metrics):
        with pytest.raises(ValueError, match="contiguous float32 device tensor"):
            fn(x, x)
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        ops.distance_transform(x)
    with pytest.raises(ValueError, match='of must be "surface" or "foreground"'):
        ops.distance_transform(x, of="edge")
    for p in (0.0, 100.5, -1.0, float("nan")):
        with pytest.raises(ValueError, match=r"percentile must be in \(0, 100\]"):
            ops.surface_distances(x, x, percentile=p)
        with pytest.raises(ValueError, match=r"percentile must be in \(0, 100\]"):
            metrics.mask_metrics(x, x, percentile=p)
    for name in ("distance_transform", "surface_distances", "hausdorff"):
        assert "anisotropic spacing is not offered" in " ".join(getattr(metrics, name).__doc__.split())
    # a reconstruction without mask channels is refused by name, before anything is launched
    with pytest.raises(ValueError, match="no mask channels to score"):
        VQVAE._mask_values(None, torch.zeros(1, 4, 4, 4, 1), torch.zeros(1, 4, 4, 4, 1), 1)
    assert VQVAE.MASK_METRIC_KEYS == ("mask_dice", "mask_iou", "mask_hd95", "mask_assd")
    # the running mean that skips NaN
    m, plain = metrics.NanMean("dice"), metrics.Mean("dice")
    assert float(m.result()) == 0.0
    for v in (torch.tensor([[0.5, float("nan")], [1.0, 0.75]], dtype=torch.float64), torch.tensor([float("nan")]), torch.tensor(0.25)):
        m.update_state(v), plain.update_state(v)
    assert float(m.result()) == (0.5 + 1.0 + 0.75 + 0.25) / 4 and int(m.count) == 4 and math.isnan(float(plain.result()))
    m.reset_state()
    m.update_state(torch.tensor([float("nan")]))
    assert float(m.result()) == 0.0


# ---- the restatement against closed forms ------------------------------------------------------------------------------------------------
def _volume(shape, *voxels):
    m = np.zeros(shape, bool)
    for v in voxels:
        m[v] = True
    return m


def test_single_voxel_against_single_voxel():
    a, b = _volume((6, 7, 8), (1, 2, 3)), _volume((6, 7, 8), (4, 6, 1))
    want = math.sqrt(9 + 16 + 4)
    for p in (95.0, 50.0, 100.0):
        s = mk.surface_stats(a, b, p)
        assert s["hd"] == s["hd_percentile"] == s["assd"] == want and s["n"] == 2 and not s["split"]
    assert mk.sq_distance_map(a)[4, 6, 1] == 29 and mk.sq_distance_map(a)[1, 2, 3] == 0 and mk.sq_distance_map(a).max() == 16 + 16 + 16
    c = mk.overlap_counts(a[None, None], b[None, None])
    assert c.tolist() == [[[1, 1, 0]]] and [float(v[0, 0]) for v in mk.dice_iou(c)] == [0.0, 0.0]


@pytest.mark.parametrize("k", [1, 3, 6])
def test_two_parallel_planes_are_k_apart(k):
    a, b = np.zeros((9, 5, 6), bool), np.zeros((9, 5, 6), bool)
    a[1], b[1 + k] = True, True
    assert np.array_equal(mk.surface(a), a)                                     # a plane one voxel thick is all surface
    s = mk.surface_stats(a, b, 95.0)
    assert s["hd"] == s["hd_percentile"] == s["assd"] == float(k) and s["n"] == 60
    assert np.array_equal(mk.sq_distance_map(a), np.broadcast_to(((np.arange(9) - 1) ** 2)[:, None, None], (9, 5, 6)))


def test_cube_against_itself_and_an_empty_truth():
    cube = np.zeros((8, 9, 10), bool)
    cube[2:6, 3:8, 1:7] = True
    surf = mk.surface(cube)
    assert int(surf.sum()) == 4 * 5 * 6 - 2 * 3 * 4 and not surf[3:5, 4:7, 2:6].any()
    s = mk.surface_stats(cube, cube, 95.0)
    assert s["hd"] == s["hd_percentile"] == s["assd"] == 0.0
    c = mk.overlap_counts(cube[None, None], cube[None, None])
    assert [float(v[0, 0]) for v in mk.dice_iou(c)] == [1.0, 1.0]
    empty = np.zeros_like(cube)
    for a, b in ((empty, cube), (cube, empty), (empty, empty)):
        s = mk.surface_stats(a, b, 95.0)
        assert math.isnan(s["hd"]) and math.isnan(s["hd_percentile"]) and math.isnan(s["assd"])
    assert (mk.sq_distance_map(empty) == mk.INT32_MAX).all()
    dice, iou = mk.dice_iou(mk.overlap_counts(empty[None, None], cube[None, None]))         # MONAI's ignore_empty: an empty truth has no score
    assert math.isnan(dice[0, 0]) and math.isnan(iou[0, 0])
    dice, iou = mk.dice_iou(mk.overlap_counts(cube[None, None], empty[None, None]))
    assert dice[0, 0] == 0.0 and iou[0, 0] == 0.0
    # a volume-filling mask has its surface on the border only; NaN and the threshold itself are background
    full = np.ones((4, 5, 6), bool)
    assert np.array_equal(mk.surface(full), ~np.pad(np.ones((2, 3, 4), bool), 1))
    t = np.array([0.5, np.nan, 0.5000001, 1.0, -np.inf, np.inf], np.float32).reshape(1, 1, 1, 6, 1)
    assert mk.masks(t, 0, 1).reshape(-1).tolist() == [False, False, True, True, False, True]


def test_percentile_is_numpys_linear_rule_and_the_bound_is_relative():
    d = np.array([0, 1, 1, 2, 4, 5, 8, 9, 9, 13], np.int64)
    lo, hi, t = mk.interpolation_ranks(len(d), 95.0)
    assert (lo, hi) == (8, 9) and abs(t - 0.55) < 1e-12
    f = np.sqrt(d.astype(np.float64))
    assert np.percentile(f, 95.0, method="linear") == f[9] - (f[9] - f[8]) * (1 - t)         # numpy's form for t >= 0.5
    lo, hi, t = mk.interpolation_ranks(len(d), 25.0)
    assert np.percentile(f, 25.0, method="linear") == f[lo] + (f[hi] - f[lo]) * t
    assert mk.interpolation_ranks(7, 100.0) == (6, 6, 0.0)
    assert mk.bound(100) == 104 * 2.0 ** -52 and mk.within(1.0 + 2.0 ** -46, 1.0, 100) and not mk.within(1.0 + 2.0 ** -45, 1.0, 100)
    assert mk.within(math.nan, math.nan, 0) and not mk.within(0.0, math.nan, 0) and not mk.within(math.nan, 1.0, 5) and not mk.within(1e-300, 0.0, 9)


def test_the_inputs_are_what_the_issue_lists():
    assert set(mk.SHAPES) >= {(1, 1, 1), (1, 9, 1), (5, 7, 9), (17, 33, 65), (3, 130, 6), (130, 3, 5)}
    assert (mk.CX, mk.X0C, mk.CY, mk.Y0C, mk.NC) == (3, 1, 2, 0, 2)
    kinds = {k for g in mk.GROUPS.values() for pair in g for k in pair}
    assert kinds >= {"balls", "speckle", "blob", "full", "single", "empty"}
    assert ("empty", "empty") in mk.GROUPS["edges"] and any(a == "empty" != b for a, b in mk.GROUPS["edges"]) and any(
        b == "empty" != a for a, b in mk.GROUPS["edges"])
    shape = (17, 33, 65)
    blob = mk.mask_of("blob", shape)
    assert blob[0, 0, 0] and blob[0].any() and blob[:, 0].any() and blob[:, :, 0].any() and not blob[-1, -1, -1]
    assert abs(mk.mask_of("speckle", shape).mean() - 0.5) < 0.02 and mk.mask_of("full", shape).all() and mk.mask_of("single", shape).sum() == 1
    # at least one case has its two interpolation ranks on different squared distances, at both percentiles
    for p in mk.PERCENTILES:
        assert any(s["split"] for case in mk.CASES for row in mk.reference(case)["stats"][p] for s in row), p
    # the inputs hold NaN and the threshold itself in the background, and junk outside the window
    x, _ = mk.make_case(((5, 7, 9), "shapes"))
    assert np.isnan(x[..., 1:]).any() and (x[..., 1:] == 0.5).any() and (x[..., 0] > 0.5).any() and (x[..., 0] < 0.5).any()


def test_restatement_equals_scipy_on_the_gpu_inputs():
    ndi = pytest.importorskip("scipy.ndimage")
    for case in mk.CASES:
        ref = mk.reference(case)
        for m, surf, smap in ((ref["mx"], ref["surf_x"], ref["map_x"]), (ref["my"], ref["surf_y"], ref["map_y"])):
            for b in range(mk.BATCH):
                for c in range(mk.NC):
                    er = ndi.binary_erosion(m[b, c], border_value=0) if m[b, c].any() else m[b, c]
                    assert np.array_equal(surf[b, c], m[b, c] ^ er), (mk.case_id(case), b, c)
                    if surf[b, c].any():
                        edt = ndi.distance_transform_edt(~surf[b, c])
                        assert np.array_equal(np.rint(edt * edt).astype(np.int64), smap[b, c]), (mk.case_id(case), b, c)
                    else:
                        assert (smap[b, c] == mk.INT32_MAX).all()
