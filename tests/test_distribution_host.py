"""CPU tier of the distribution-metric entries (no kernel is launched): dm3d_feature_moments, dm3d_knn_radius, dm3d_prdc_counts and
dm3d_poly_mmd are declared, exported and bound and refuse every documented bad argument; csrc/dm3d_dist.hip compiles for gfx950 without
spill or scratch; the numpy restatement the GPU tests compare against (tests/distribution_reference.py) checks itself against closed
forms; the inputs of the GPU tests give scores that are neither 0 nor 1; the Python wrappers refuse what they document."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import distribution_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 0x10000                                   # an aligned non-null "pointer": nothing is launched, so nothing dereferences it
ENTRIES = {"feature_moments": "dm3d_feature_moments", "knn_radius": "dm3d_knn_radius", "prdc_counts": "dm3d_prdc_counts",
           "poly_mmd": "dm3d_poly_mmd"}
ALL = tuple(ENTRIES)
TWO = ("prdc_counts", "poly_mmd")

OK = dict(x=A, y=A + 0x100000, rows_x=0, rows_y=0, n=10, m=12, nx=10, ny=12, dim=8, k=3, subsets=1, radius_x=A + 0x200000,
          radius_y=A + 0x210000, mean=A + 0x300000, cov=A + 0x310000, radius=A + 0x400000, count_y=A + 0x500000, near_x=A + 0x510000,
          cover_x=A + 0x520000, sums=A + 0x600000, work=A + 0x700000, work_elems=1 << 20)
BAD = [
    (ALL, dict(x=0), "x must be non-null"), (ALL, dict(x=A + 4), "x must be 8-byte aligned"), (ALL, dict(rows_x=A + 2), "rows_x must be 4-byte aligned"),
    (ALL, dict(dim=0), "dim=0"), (ALL, dict(dim=4097), "dim=4097 exceeds DM3D_DIST_MAX_DIM=4096"),
    (ALL, dict(n=1), "n=1 (at least 2 rows)"), (ALL, dict(n=0), "n=0"), (ALL, dict(nx=0, rows_x=A), "nx=0"),
    (ALL, dict(n=65537, nx=65537), "n=65537 nx=65537 exceeds DM3D_DIST_MAX_ROWS=65536"), (ALL, dict(nx=65537), "exceeds DM3D_DIST_MAX_ROWS=65536"),
    (ALL, dict(n=11), "n=11 rows are read without a table, x holds nx=10"),
    (TWO, dict(y=0), "y must be non-null"), (TWO, dict(y=A + 0x100004), "y must be 8-byte aligned"),
    (TWO, dict(rows_y=A + 1), "rows_y must be 4-byte aligned"), (TWO, dict(ny=0, rows_y=A), "ny=0"),
    (TWO, dict(m=65537, ny=65537), "m=65537 ny=65537 exceeds DM3D_DIST_MAX_ROWS=65536"),
    (TWO, dict(m=13), "m=13 rows are read without a table, y holds ny=12"),
    (("prdc_counts",), dict(m=0), "m=0 (at least 1)"), (("poly_mmd",), dict(m=1), "m=1 (at least 2)"),
    (("feature_moments",), dict(mean=0), "mean and cov must be non-null"), (("feature_moments",), dict(cov=0), "mean and cov must be non-null"),
    (("feature_moments",), dict(mean=A + 0x300004), "mean and cov must be 8-byte aligned"),
    (("feature_moments",), dict(mean=A + 8), "mean overlaps x"), (("feature_moments",), dict(cov=A + 10 * 8 * 8 - 8), "cov overlaps x"),
    (("feature_moments",), dict(mean=A + 0x310000 + 8), "mean overlaps cov"),
    (("knn_radius",), dict(k=0), "k=0 (at least 1)"), (("knn_radius",), dict(k=17, n=30, nx=30), "k=17 exceeds DM3D_DIST_MAX_K=16"),
    (("knn_radius",), dict(k=10), "k=10 needs more than k rows, n=10"), (("knn_radius",), dict(k=12, rows_x=A + 0x800000, n=11), "k=12 needs more than k rows, n=11"),
    (("knn_radius",), dict(radius=0), "radius must be non-null"), (("knn_radius",), dict(radius=A + 0x400004), "radius must be 8-byte aligned"),
    (("knn_radius",), dict(radius=A + 16), "radius overlaps x"),
    (("prdc_counts",), dict(radius_x=0), "radius_x and radius_y must be non-null"), (("prdc_counts",), dict(radius_y=0), "radius_x and radius_y must be non-null"),
    (("prdc_counts",), dict(radius_y=A + 0x210004), "radius_x and radius_y must be 8-byte aligned"),
    (("prdc_counts",), dict(count_y=0), "count_y, near_x and cover_x must be non-null"), (("prdc_counts",), dict(near_x=0), "count_y, near_x and cover_x must be non-null"),
    (("prdc_counts",), dict(cover_x=0), "count_y, near_x and cover_x must be non-null"),
    (("prdc_counts",), dict(near_x=A + 0x510002), "count_y, near_x and cover_x must be 4-byte aligned"),
    (("prdc_counts",), dict(count_y=A + 0x100000 + 12 * 8 * 8 - 4), "count_y overlaps x or y"), (("prdc_counts",), dict(cover_x=A), "cover_x overlaps x or y"),
    (("prdc_counts",), dict(near_x=A + 0x200000 + 10 * 8 - 4), "near_x overlaps a radius vector"),
    (("poly_mmd",), dict(subsets=0), "subsets=0 (at least 1)"), (("poly_mmd",), dict(subsets=16385), "subsets=16385 exceeds DM3D_DIST_MAX_SUBSETS=16384"),
    (("poly_mmd",), dict(sums=0), "sums must be non-null"), (("poly_mmd",), dict(sums=A + 0x600004), "sums must be 8-byte aligned"),
    (("poly_mmd",), dict(work=0), "work must be non-null"), (("poly_mmd",), dict(work=A + 0x700004), "work must be 8-byte aligned"),
    (("poly_mmd",), dict(work_elems=2 * 10 + 12 - 1), "work holds 31 float64, 32 are needed (subsets * (2 * n + m))"),
    (("poly_mmd",), dict(subsets=3, rows_x=A + 0x800000, rows_y=A + 0x900000, work_elems=95), "work holds 95 float64, 96 are needed"),
    (("poly_mmd",), dict(sums=A + 0x100000), "sums overlaps x or y"), (("poly_mmd",), dict(work=A + 8), "work overlaps x or y"),
    (("poly_mmd",), dict(sums=A + 0x700000 + 8), "sums overlaps work"),
]


def _desc(_lib, **override):
    d = _lib.DistDesc()
    for k, v in {**OK, **override}.items():
        setattr(d, k, v)
    return d


def test_entries_are_declared_exported_and_bound(built_library, tmp_path):
    from dm3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dm3d.h")).read()
    handle = C.CDLL(built_library)
    for name in ENTRIES.values():
        assert re.search(r"\bint %s\(const dm3d_dist_desc\* d, void\* stream\);" % name, header), name
        assert hasattr(handle, name), name
        assert _lib.SIGNATURES[name] == (C.c_int, [C.POINTER(_lib.DistDesc), C.c_void_p]), name
    assert _lib.lib().dm3d_version() == _lib.ABI_VERSION == 111 and "#define DM3D_VERSION 111 " in header
    # the ctypes mirror has the header's fields, in its order, with its types
    body = re.search(r"typedef struct dm3d_dist_desc \{(.*?)\} dm3d_dist_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in (s.strip() for s in body.split(";")):
        if decl:
            ctype, names = decl.removeprefix("const ").split(" ", 1)
            fields += [(n.strip(" *"), ctype + ("*" if "*" in ctype + names else "")) for n in names.split(",")]
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    assert [f[0] for f in fields] == [f[0] for f in _lib.DistDesc._fields_]
    for (name, ctype), (_, mirror) in zip(fields, _lib.DistDesc._fields_):
        assert mirror is (C.c_void_p if ctype.endswith("*") else kinds[ctype]), (name, ctype, mirror)
    for name, value in (("MAX_ROWS", 65536), ("MAX_DIM", 4096), ("MAX_K", 16), ("MAX_SUBSETS", 16384), ("TILE", dr.TILE), ("CHUNK", dr.CHUNK)):
        assert f"#define DM3D_DIST_{name} {value}\n" in header and getattr(_lib, "DIST_" + name) == value, name
    assert dr.MAX_K == _lib.DIST_MAX_K
    assert "work_elems >= subsets * (2 * n + m) " in header
    # the mirror's size is the compiler's
    cc = next((p for p in ("/usr/bin/cc", "/usr/bin/gcc", "/usr/bin/clang", "/opt/rocm/llvm/bin/clang") if os.path.exists(p)), None)
    if cc is not None:
        import subprocess
        src, exe = tmp_path / "size.c", tmp_path / "size"
        src.write_text('#include <stdio.h>\n#include "dm3d.h"\nint main(void) { printf("%zu\\n", sizeof(dm3d_dist_desc)); return 0; }\n')
        subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        assert int(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout) == C.sizeof(_lib.DistDesc)
    assert C.sizeof(_lib.DistDesc) == 152


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
def test_dist_kernels_compile_without_spill_or_scratch(tmp_path):
    """The gfx950 listing of csrc/dm3d_dist.hip (the library's flags), read by its metadata alone: every kernel is there, none with a
    spilled register or a private segment, and the tile kernels fit three workgroups' LDS into a compute unit."""
    import subprocess
    out = str(tmp_path / "dm3d_dist.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function",
                    "-ffp-contract=off", "-S", "--cuda-device-only", os.path.join(ROOT, "3d-condtional-stable-diffusion_amd", "csrc", "dm3d_dist.hip"),
                    "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    rows = re.findall(r"\.group_segment_fixed_size:\s+(\d+)[\s\S]*?\.name:\s+(\S+)[\s\S]*?\.private_segment_fixed_size:\s+(\d+)[\s\S]*?"
                      r"\.sgpr_spill_count:\s+(\d+)[\s\S]*?\.vgpr_spill_count:\s+(\d+)", text)
    names = [r[1] for r in rows]
    kernels = [f"dist_tile_kernelILi{op}E" for op in range(4)] + ["dist_mean_kernel", "dist_total_kernel"]
    for k in kernels:
        assert any(k in n for n in names), (k, names)
    assert len(rows) == len(kernels), names
    assert all(int(a) == 0 and int(b) == 0 and int(c) == 0 for _, _, a, b, c in rows), rows
    assert all(int(lds) <= 160 * 1024 // 3 for lds, *_ in rows), rows


# ---- the restatement against closed forms ------------------------------------------------------------------------------------------------
def test_frechet_of_diagonal_moments():
    rng = np.random.default_rng(0)
    a, b = rng.uniform(0.5, 2.0, 9), rng.uniform(0.5, 2.0, 9)
    mu1, mu2 = rng.standard_normal(9), rng.standard_normal(9)
    want = ((mu1 - mu2) ** 2).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    for how in ("symmetric", "product"):
        got = dr.frechet_from_moments(mu1, np.diag(a), mu2, np.diag(b), how=how)
        assert abs(got - want) <= 1e-13 * want, (how, got, want)
    from dm3d_amd import metrics
    got = metrics.frechet_distance_from_moments(mu1, np.diag(a), mu2, np.diag(b))
    assert got.dtype == torch.float64 and got.dim() == 0 and abs(float(got) - want) <= 1e-13 * want


def test_identical_sets():
    x = dr.clouds(dr.SMALL_CASE)[0][:23]
    p = dr.prdc(x, x, 3)
    assert p["precision"] == p["recall"] == p["coverage"] == 1.0                 # every row lies in its own ball: 0 < r^2
    assert 0.9 < p["density"] <= 1.0                # a ball holds k rows under the strict <, fewer where the duplicate ties at its edge
    # the cross sum is the within sum plus the diagonal, so mmd2 is what the formula gives for it: the terms cancel up to the diagonal
    n, s = x.shape[0], dr.poly_mmd(x, x)
    t = dr.dots(x, x).diagonal() / x.shape[1] + 1.0
    diag = (t * t * t).sum()
    assert s[0] == s[1] and abs(s[2] - (s[0] + diag)) <= 1e-12 * s[2]
    want = 2.0 * s[0] / (n * (n - 1)) - 2.0 * (s[0] + diag) / (n * n)
    assert abs(dr.mmd2(x, x) - want) <= 1e-12 * abs(want) + 1e-12
    mean, cov = dr.feature_moments(x)
    assert np.array_equal(cov, cov.T) and np.allclose(mean, x.mean(0), rtol=1e-13, atol=1e-15) and np.allclose(cov, np.cov(x.T), rtol=1e-12, atol=1e-14)
    assert abs(dr.frechet(x, x)) <= 1e-9 and abs(dr.frechet(x, x, "product")) <= 1e-9


def test_separated_sets_score_zero():
    x, y = dr.clouds(dr.SMALL_CASE)
    x, y = x[:23], y[:40] + 1000.0
    assert all(v == 0.0 for v in dr.prdc(x, y, 5).values())


def test_lattice_radii_and_duplicates():
    x = np.arange(40, dtype=np.float64)[:, None] * 0.5                          # spacing 1/2: every distance is exact
    for k in (1, 2, 3, 8):
        r = dr.knn_radius(x, k)
        inner = r[k:-k]
        assert np.array_equal(inner, np.full(inner.shape, (((k + 1) // 2) * 0.5) ** 2))         # k-th neighbour ceil(k / 2) spacings away
        assert r[0] == (k * 0.5) ** 2 == r[-1]                                  # at the ends k spacings: k^2 spacings^2
    y = np.random.default_rng(1).standard_normal((12, 4))
    y[7] = y[2]
    r = dr.knn_radius(y, 1)
    assert r[2] == 0.0 and r[7] == 0.0 and (np.delete(r, (2, 7)) > 0.0).all()
    assert (dr.knn_radius(y, 2)[[2, 7]] > 0.0).all()


def test_the_gpu_inputs_show_something():
    """On the inputs of the GPU tests the restatement's precision, recall and coverage are strictly between 0.1 and 0.9 and some
    generated row counts at least 2 real balls: for every case at k = 1, and for the cases of more than one feature chunk's worth of
    D around the chunk size also at k = 5."""
    assert dr.MAIN_CASES == ((65, 127, 1), (65, 127, 31), (65, 127, 33), (65, 127, 70)) and dr.SMALL_CASE == (23, 40, 7)
    assert dr.KS == (1, 5, 16) and dr.TABLES == (None, "permute", "repeat")
    for case in dr.CASES:
        n, m, dim = case
        real, fake = dr.clouds(case)
        assert real.shape == (n + dr.SPARE, dim) and fake.shape == (m + dr.SPARE, dim)
        assert np.array_equal(real[3], real[10]) and np.array_equal(fake[5], fake[6]) and np.array_equal(fake[0], real[7])
        for k in (1, 5) if dim > 1 and case != dr.SMALL_CASE else (1,):
            x, y = real[:n], fake[:m]
            p = dr.prdc(x, y, k)
            count = dr.prdc_counts(x, y, dr.knn_radius(x, k), dr.knn_radius(y, k))[0]
            assert all(0.1 < p[key] < 0.9 for key in ("precision", "recall", "coverage")), (case, k, p)
            assert count.max() >= 2, (case, k)
        assert dr.sqdist(real[:n], fake[:m])[7, 0] == 0.0
        for kind in dr.TABLES[1:]:
            t = dr.table(kind, n, n + dr.SPARE, 3)
            assert t.dtype == np.int32 and t.shape == (n,) and t.min() >= 0 and t.max() < n + dr.SPARE
            assert (len(set(t.tolist())) == n) == (kind == "permute") and t.max() >= n


def test_python_wrappers_refuse_what_they_document():
    from dm3d_amd import metrics, ops
    public = {"distribution_metrics", "encoder_features", "frechet_distance", "frechet_distance_from_moments", "kid", "mmd2", "prdc"}
    assert public <= set(metrics.__all__) and all(callable(getattr(ops, n)) for n in ("feature_moments", "knn_radius", "prdc_counts", "poly_mmd"))
    a, b = torch.zeros(10, 4), torch.zeros(12, 4)
    pair = (metrics.frechet_distance, metrics.kid, metrics.mmd2, metrics.prdc, metrics.distribution_metrics, ops.poly_mmd,
            lambda x, y: ops.prdc_counts(x, y, None, None))
    for fn in pair:
        with pytest.raises(ValueError, match=r"must be a 2-D feature tensor \[rows, D\].*flatten or pool"):
            fn(torch.zeros(10, 2, 2), b)
        with pytest.raises(ValueError, match=r"must be a 2-D feature tensor"):
            fn(a, torch.zeros(4))
        with pytest.raises(ValueError, match="fake has D=5 features, the other set has D=4: both sets must come from one feature extractor"):
            fn(a, torch.zeros(12, 5))
        with pytest.raises(ValueError, match="real has 1 rows, at least 2 are needed"):
            fn(torch.zeros(1, 4), b)
        with pytest.raises(ValueError, match=r"must be float32 or float64, got torch.int64: cast with"):
            fn(a.long(), b)
        with pytest.raises(ValueError, match="real must be a device tensor: the distribution kernels have no CPU path"):
            fn(a, b)
    for fn in (metrics.prdc, metrics.distribution_metrics):
        with pytest.raises(ValueError, match="nearest_k=10 needs more than nearest_k rows in each set, got 10 and 12: lower nearest_k or add samples"):
            fn(a, b, nearest_k=10)
        with pytest.raises(ValueError, match="nearest_k must be an integer from 1 to 16"):
            fn(a, b, nearest_k=0)
        with pytest.raises(ValueError, match="nearest_k must be an integer from 1 to 16"):
            fn(torch.zeros(40, 4), torch.zeros(40, 4), nearest_k=17)
    for fn in (ops.feature_moments, ops.knn_radius):
        with pytest.raises(ValueError, match="x must be a 2-D feature tensor"):
            fn(torch.zeros(3))
        with pytest.raises(ValueError, match="x must be a device tensor"):
            fn(a)
    with pytest.raises(ValueError, match=r"x has D=4097 features; 1 to 4096 are taken"):
        ops.feature_moments(torch.zeros(2, 4097))
    with pytest.raises(ValueError, match=r"x has 65537 rows, at most 65536 are taken"):
        ops.knn_radius(torch.zeros(65537, 1))
    # the checks that follow the tensor's own: a stand-in that passes for a device tensor, so they are reached without a GPU
    from unittest import mock
    with mock.patch.object(ops, "_features", lambda t, name, other=None, min_rows=2: t.double()):
        with pytest.raises(ValueError, match="x has 1 rows, at least 2 are needed for a covariance"):
            ops.feature_moments(torch.zeros(1, 4))
        with pytest.raises(ValueError, match="k must be an integer from 1 to 16, got 17"):
            ops.knn_radius(torch.zeros(40, 4), 17)
        with pytest.raises(ValueError, match="k=10 needs more than k rows, the set has 10: lower k or add samples"):
            ops.knn_radius(a, 10)
        with pytest.raises(ValueError, match="rows must be an int32 or int64 tensor"):
            ops.knn_radius(a, 3, rows=torch.zeros(4))
        with pytest.raises(ValueError, match=r"radius_real must be a contiguous float64 device tensor \[10\], what knn_radius returns"):
            ops.prdc_counts(a, b, torch.zeros(10), torch.zeros(12))
        with pytest.raises(ValueError, match="must list the same number of subsets, got 2 and 3"):
            ops.poly_mmd(a, b, torch.zeros(2, 5, dtype=torch.int32), torch.zeros(3, 5, dtype=torch.int32))
        with pytest.raises(ValueError, match=r"rows_real must be an int32 or int64 tensor \[subsets, rows\] or None"):
            ops.poly_mmd(a, b, torch.zeros(5, dtype=torch.int32))
        with pytest.raises(ValueError, match="a subset needs at least 2 rows of each set, got 1 and 1"):
            ops.poly_mmd(a, b, torch.zeros(2, 1, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="num_subsets must be an integer of at least 1"):
        metrics.kid_subsets(10, 12, 0, 5, 0)
    with pytest.raises(ValueError, match="subset_size must be an integer of at least 2"):
        metrics.kid_subsets(10, 12, 3, 1, 0)
    with pytest.raises(ValueError, match='pool must be "mean" or "mean_std"'):
        metrics.encoder_features(None, torch.zeros(1, 8, 8, 8, 1), pool="max")
    with pytest.raises(ValueError, match="batch_size must be an integer of at least 1"):
        metrics.encoder_features(None, torch.zeros(1, 8, 8, 8, 1), batch_size=0)
    with pytest.raises(ValueError, match=r"volumes must be \[n, D, H, W, C\]"):
        metrics.encoder_features(None, torch.zeros(8, 8, 8, 1))
    with pytest.raises(ValueError, match=r"moments must be mu \[D\] and sigma \[D, D\] of one D"):
        metrics.frechet_distance_from_moments(torch.zeros(3), torch.zeros(3, 3), torch.zeros(3), torch.zeros(2, 2))


def test_kid_draws_the_restatements_subsets():
    from dm3d_amd import metrics
    for n, m, subsets, size, seed in ((65, 127, 3, 20, 0), (23, 40, 1, 1000, 7), (40, 23, 4, 23, 11)):
        ta, tb = metrics.kid_subsets(n, m, subsets, size, seed)
        ra, rb = dr.kid_subsets(n, m, subsets, size, seed)
        assert ta.dtype == tb.dtype == torch.int32 and tuple(ta.shape) == tuple(tb.shape) == (subsets, min(size, n, m))
        assert np.array_equal(ta.numpy(), ra) and np.array_equal(tb.numpy(), rb)
        assert all(len(set(r.tolist())) == r.numel() for r in ta) and int(ta.max()) < n and int(tb.max()) < m      # without replacement
    assert not np.array_equal(metrics.kid_subsets(65, 127, 3, 20, 1)[0].numpy(), dr.kid_subsets(65, 127, 3, 20, 0)[0])
