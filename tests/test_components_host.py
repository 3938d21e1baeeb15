"""CPU tier of the connected-component entries (no kernel is launched): dm3d_components and dm3d_component_filter are declared, exported
and bound and refuse every documented bad argument; csrc/dm3d_ccl.hip compiles for gfx950 without spill or scratch; the numpy
restatement the GPU tests compare against (tests/components_reference.py) checks itself against closed forms and, where scipy is
installed, against scipy.ndimage on the inputs of the GPU tests; the Python wrappers refuse what they document."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import components_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 0x10000                                   # an aligned non-null "pointer": nothing is launched, so nothing dereferences it
ENTRIES = {"components": "dm3d_components", "component_filter": "dm3d_component_filter"}

# 2 x 5 x 7 x 9 x 2 channels: 1260 voxels, one block of 1024 per volume: work = planes * 1260 + 1 + 4 * 5
OK = dict(x=A, batch=2, d=5, h=7, w=9, cx=3, x0c=1, nc=2, threshold=0.5, connectivity=6, mode=0, min_size=1, labels=A + 0x100000, count=A,
          largest=A, out=A + 0x100000, work=A, work_elems=1 << 20)
ALL = tuple(ENTRIES)
BAD = [
    (ALL, dict(x=0), "x must be non-null"), (ALL, dict(x=A + 2), "x must be 4-byte aligned"),
    (ALL, dict(work=0), "work must be non-null"), (ALL, dict(work=A + 4), "work must be 8-byte aligned"),
    (("components",), dict(labels=0), "labels, count and largest must be non-null"),
    (("components",), dict(count=0), "labels, count and largest must be non-null"),
    (("components",), dict(largest=0), "labels, count and largest must be non-null"),
    (("components",), dict(labels=A + 0x100002), "4-byte aligned"), (("components",), dict(count=A + 1), "4-byte aligned"),
    (("components",), dict(largest=A + 4), "largest must be 8-byte aligned"),
    (("component_filter",), dict(out=0), "out must be non-null"), (("component_filter",), dict(out=A + 0x100001), "out must be 4-byte aligned"),
    (ALL, dict(nc=3), "outside x's cx=3"), (ALL, dict(x0c=2), "outside x's cx=3"), (ALL, dict(x0c=-1), "outside x"),
    (ALL, dict(d=0), "d=0"), (ALL, dict(h=0), "h=0"), (ALL, dict(w=0), "w=0"), (ALL, dict(batch=0), "batch=0"), (ALL, dict(nc=0), "nc=0"),
    (ALL, dict(d=513), "d=513 h=7 w=9 exceeds DM3D_CCL_MAX_EXTENT=512"), (ALL, dict(h=513), "exceeds DM3D_CCL_MAX_EXTENT=512"),
    (ALL, dict(w=513), "exceeds DM3D_CCL_MAX_EXTENT=512"),
    (ALL, dict(batch=32768), "batch * nc = 65536"),
    (ALL, dict(threshold=float("nan")), "threshold=nan"), (ALL, dict(threshold=float("-inf")), "threshold=-inf"),
    (ALL, dict(connectivity=4), "connectivity=4"), (ALL, dict(connectivity=0), "connectivity=0"), (ALL, dict(connectivity=27), "connectivity=27"),
    (("component_filter",), dict(mode=3), "mode=3"), (("component_filter",), dict(mode=-1), "mode=-1"),
    (("component_filter",), dict(mode=1, min_size=0), "min_size=0"), (("component_filter",), dict(mode=1, min_size=-4), "min_size=-4"),
    (("components",), dict(work_elems=2 * 1260 + 1 + 20 - 1), "work holds 2540 int32, 2541 are needed"),
    (("component_filter",), dict(work_elems=3 * 1260 + 1 + 20 - 1), "work holds 3800 int32, 3801 are needed"),
    (("component_filter",), dict(batch=8, d=128, h=128, w=128, cx=1, x0c=0, nc=1, work_elems=3 * 8 * 128 ** 3 + 8 * (3 * 2048 + 2)),
     "work holds 50380816 int32, 50380817 are needed"),
    (("components",), dict(labels=A + 8), "labels overlaps x"), (("component_filter",), dict(out=A + 2 * 5 * 7 * 9 * 3 * 4 - 4), "out overlaps x"),
]


def _desc(_lib, **override):
    d = _lib.CclDesc()
    for k, v in {**OK, **override}.items():
        setattr(d, k, v)
    return d


def test_entries_are_declared_exported_and_bound(built_library, tmp_path):
    from dm3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dm3d.h")).read()
    handle = C.CDLL(built_library)
    for name in ENTRIES.values():
        assert re.search(r"\bint %s\(const dm3d_ccl_desc\* d, void\* stream\);" % name, header), name
        assert hasattr(handle, name), name
        assert _lib.SIGNATURES[name] == (C.c_int, [C.POINTER(_lib.CclDesc), C.c_void_p]), name
    assert _lib.lib().dm3d_version() == _lib.ABI_VERSION == 111 and "#define DM3D_VERSION 111 " in header
    # the ctypes mirror has the header's fields, in its order, with its types
    body = re.search(r"typedef struct dm3d_ccl_desc \{(.*?)\} dm3d_ccl_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in (s.strip() for s in body.split(";")):
        if decl:
            ctype, names = decl.removeprefix("const ").split(" ", 1)
            fields += [(n.strip(" *"), ctype + ("*" if "*" in ctype + names else "")) for n in names.split(",")]
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    assert [f[0] for f in fields] == [f[0] for f in _lib.CclDesc._fields_]
    for (name, ctype), (_, mirror) in zip(fields, _lib.CclDesc._fields_):
        assert mirror is (C.c_void_p if ctype.endswith("*") else kinds[ctype]), (name, ctype, mirror)
    assert f"#define DM3D_CCL_MAX_EXTENT {_lib.CCL_MAX_EXTENT}\n" in header and _lib.CCL_MAX_EXTENT == 512
    assert f"#define DM3D_CCL_BLOCK_VOXELS {_lib.CCL_BLOCK_VOXELS}\n" in header
    for name in ("LARGEST", "MIN_SIZE", "FILL_HOLES"):
        assert f"#define DM3D_CCL_{name} {getattr(_lib, 'CCL_' + name)}\n" in header, name
    assert "work_elems >= 2 * batch * nc * d * h * w + 1 + batch * nc * (3 * nblk + 2) " in header
    assert "work_elems >= 3 * batch * nc * d * h * w + 1 + batch * nc * (3 * nblk + 2) " in header
    assert "nblk        = ceil(d * h * w / DM3D_CCL_BLOCK_VOXELS)" in header
    # the mirror's size is the compiler's
    cc = next((p for p in ("/usr/bin/cc", "/usr/bin/gcc", "/usr/bin/clang", "/opt/rocm/llvm/bin/clang") if os.path.exists(p)), None)
    if cc is not None:
        import subprocess
        src, exe = tmp_path / "size.c", tmp_path / "size"
        src.write_text('#include <stdio.h>\n#include "dm3d.h"\nint main(void) { printf("%zu\\n", sizeof(dm3d_ccl_desc)); return 0; }\n')
        subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        assert int(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout) == C.sizeof(_lib.CclDesc)
    assert C.sizeof(_lib.CclDesc) == 104


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
def test_ccl_kernels_compile_without_spill_or_scratch(tmp_path):
    """The gfx950 listing of csrc/dm3d_ccl.hip (the library's flags), read by its metadata alone: every kernel is there, none with a
    spilled register or a private segment."""
    import subprocess
    out = str(tmp_path / "dm3d_ccl.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function",
                    "-ffp-contract=off", "-S", "--cuda-device-only", os.path.join(ROOT, "3d-condtional-stable-diffusion_amd", "csrc", "dm3d_ccl.hip"),
                    "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    rows = re.findall(r"\.name:\s+(\S+)[\s\S]*?\.private_segment_fixed_size:\s+(\d+)[\s\S]*?\.sgpr_spill_count:\s+(\d+)[\s\S]*?\.vgpr_spill_count:\s+(\d+)", text)
    names = [r[0] for r in rows]
    kernels = [f"ccl_{k}_kernelILi{n}E" for k in ("local", "seam") for n in (1, 2, 3)] + [
        "ccl_flatten_kernel", "ccl_count_kernel", "ccl_scan_kernel", "ccl_rank_kernel", "ccl_label_kernel", "ccl_filter_kernel"]
    for k in kernels:
        assert any(k in n for n in names), (k, names)
    assert len(rows) == len(kernels), names
    assert all(int(a) == 0 and int(b) == 0 and int(c) == 0 for _, a, b, c in rows), rows


def test_python_wrappers_refuse_what_they_document():
    from dm3d_amd import data, metrics, ops
    assert metrics.connected_components is ops.connected_components
    assert {"component_stats", "connected_components"} <= set(metrics.__all__) and callable(data.clean_mask)
    x = torch.zeros(2, 4, 4, 4, 1)
    calls = (ops.connected_components, metrics.component_stats, lambda t, **kw: ops.component_filter(t, keep="largest", **kw), data.clean_mask)
    for fn in calls:
        with pytest.raises(ValueError, match="contiguous float32 device tensor"):
            fn(x)
        with pytest.raises(ValueError, match="contiguous float32 device tensor"):
            fn(x.double())
    # the checks that follow the tensor's own: a stand-in that passes for a device tensor, so they are reached without a GPU
    from unittest import mock
    with mock.patch.object(ops, "_f32c", lambda t, name: t):
        for fn in calls:
            with pytest.raises(ValueError, match=r"x must be \[B,D,H,W,C\]"):
                fn(torch.zeros(4, 4, 4, 1))
            with pytest.raises(ValueError, match="exceeds 512 voxels per axis"):
                fn(torch.zeros(1, 1, 513, 1, 1))
            with pytest.raises(ValueError, match="connectivity must be 6, 18 or 26"):
                fn(x, connectivity=8)
        with pytest.raises(ValueError, match="threshold must be finite"):
            ops.connected_components(x, float("inf"))
    with pytest.raises(ValueError, match="needs at least one of"):
        ops.component_filter(x)
    with pytest.raises(ValueError, match="needs at least one of"):
        data.clean_mask(x, keep_largest=False, fill_holes=False)
    with pytest.raises(ValueError, match='keep must be "largest" or None'):
        ops.component_filter(x, keep="smallest")
    for n in (0, -3, 1.5):
        with pytest.raises(ValueError, match="min_size must be an integer of at least 1"):
            ops.component_filter(x, min_size=n)
        with pytest.raises(ValueError, match="min_size must be an integer of at least 1"):
            data.clean_mask(x, min_size=n)


# ---- the restatement against closed forms ------------------------------------------------------------------------------------------------
SHAPE = (17, 33, 65)


def test_checkerboard_counts():
    m = cr.mask_of("checker", SHAPE)
    labels, n = cr.label(m, 6)
    assert n == int(m.sum()) == (17 * 33 * 65 + 1) // 2
    assert np.array_equal(labels[m], np.arange(1, n + 1))                       # every voxel its own component, numbered in raster order
    assert cr.largest(labels) == (1, 1)                                         # the lowest label on a tie
    for conn in (18, 26):
        labels, n = cr.label(m, conn)
        assert n == 1 and np.array_equal(labels > 0, m) and cr.largest(labels) == (1, int(m.sum()))


def test_corner_and_edge_pairs_per_connectivity():
    assert cr.straddle(SHAPE) == cr.BRICK and cr.straddle((5, 7, 9)) == (2, 3, 4)
    for shape, voxels in ((SHAPE, (12, 24)), ((5, 7, 9), (16, 32))):             # 2 x 2 x 2 cubes, cut to one voxel along w past the brick of SHAPE
        corner, edge = cr.mask_of("corner_pair", shape), cr.mask_of("edge_pair", shape)
        assert (int(corner.sum()), int(edge.sum())) == voxels
        assert [cr.label(corner, c)[1] for c in cr.CONNECTIVITIES] == [2, 2, 1]
        assert [cr.label(edge, c)[1] for c in cr.CONNECTIVITIES] == [2, 1, 1]
    a, b, c = cr.BRICK                                                          # the touching voxels lie in different bricks on every axis
    corner = cr.mask_of("corner_pair", SHAPE)
    assert corner[a - 1, b - 1, c - 1] and corner[a, b, c] and not corner[a - 1, b, c] and not corner[a, b - 1, c - 1]


def test_serpentine_is_one_component_then_two():
    whole, cut = cr.mask_of("serpentine", SHAPE), cr.mask_of("serpentine_cut", SHAPE)
    assert int(whole.sum()) - int(cut.sum()) == 1
    assert whole[::2, ::2].all() and all(whole[z, y].any() for z in range(0, 17, 2) for y in range(33))   # it runs through every row of its planes
    for conn in cr.CONNECTIVITIES:
        assert cr.label(whole, conn)[1] == 1 and cr.label(cut, conn)[1] == 2, conn
    labels, _ = cr.label(cut, 6)
    sizes = np.bincount(labels.reshape(-1))[1:]
    assert sizes.min() > 1000                                                   # a cut in the middle, not a chipped end
    comb = cr.mask_of("comb", SHAPE)
    assert cr.label(comb, 6)[1] == 1 and cr.label(comb[:-1], 26)[1] == 17 * 33  # the teeth join only in the last plane


def test_tie_takes_the_lowest_label_and_sizes_filter():
    tie = cr.mask_of("tie", (5, 7, 9))
    labels, n = cr.label(tie, 26)
    assert n == 2 and cr.largest(labels) == (1, 8)
    assert np.array_equal(cr.keep_largest(tie, 26), labels == 1)
    m = tie.copy()
    m[2, 3, 4] = True                                                           # a speck
    assert cr.label(m, 6)[1] == 3 and np.array_equal(cr.keep_min_size(m, 6, 2), tie) and np.array_equal(cr.keep_min_size(m, 6, 1), m)
    assert not cr.keep_min_size(m, 6, 9).any()
    empty = np.zeros((5, 7, 9), bool)
    assert cr.label(empty, 6)[1] == 0 and cr.largest(cr.label(empty, 6)[0]) == (0, 0) and not cr.keep_largest(empty, 6).any()


def test_fill_holes_closed_forms():
    s, sh = cr.solid(SHAPE), cr.mask_of("shell", SHAPE)
    assert sh.sum() < s.sum() and np.array_equal(cr.fill_holes(sh), s)
    tunnel = cr.mask_of("shell_tunnel", SHAPE)
    assert tunnel.sum() < sh.sum() and np.array_equal(cr.fill_holes(tunnel), tunnel)           # the cavity is open: nothing is filled
    diag = cr.mask_of("shell_diagonal", SHAPE)
    want = np.ones(SHAPE, bool)
    want[0, 0, 0] = False
    assert not diag[1, 1, 1] and np.array_equal(cr.fill_holes(diag), want)                      # filled: a diagonal does not open a cavity
    full, empty = np.ones(SHAPE, bool), np.zeros(SHAPE, bool)
    assert np.array_equal(cr.fill_holes(full), full) and np.array_equal(cr.fill_holes(empty), empty)
    t = np.array([0.5, np.nan, 0.5000001, 1.0, -np.inf, np.inf], np.float32).reshape(1, 1, 1, 6, 1)
    assert cr.masks(t, 0, 1).reshape(-1).tolist() == [False, False, True, True, False, True]


def test_the_inputs_are_what_the_issue_lists():
    assert cr.SHAPES == ((1, 1, 1), (1, 9, 1), (5, 7, 9), (17, 33, 65), (3, 130, 6), (130, 3, 5))
    assert (cr.BATCH, cr.CX, cr.X0C, cr.NC) == (2, 3, 1, 2) and cr.CONNECTIVITIES == (6, 18, 26) and cr.MIN_SIZES == (1, 2, 5)
    kinds = {k for g in cr.GROUPS.values() for k in g}
    assert kinds >= {"ellipsoids", "speckle15", "speckle30", "speckle50", "checker", "serpentine", "serpentine_cut", "comb", "corner_pair",
                     "edge_pair", "tie", "shell", "shell_tunnel", "shell_diagonal", "full", "empty", "single", "nans"}
    assert all(len(g) == cr.BATCH * cr.NC for g in cr.GROUPS.values())
    assert all(n > b for n, b in zip(SHAPE, cr.BRICK))                          # a brick edge is crossed on every axis
    m = cr.mask_of("speckle15", SHAPE)
    assert [cr.label(m, c)[1] for c in cr.CONNECTIVITIES] == [3228, 745, 235]       # thousands of components at 6, a few hundred at 26 (this seed's)
    x = cr.make_case(((5, 7, 9), "holes"))
    assert np.isnan(x[..., 1:]).any() and (x[..., 1:] == 0.5).any() and (x[..., 0] > 0.5).any() and (x[..., 0] < 0.5).any()
    assert np.isnan(x[1, ..., 2][~cr.mask_of("nans", (5, 7, 9))]).all()


def test_restatement_equals_scipy_on_the_gpu_inputs():
    ndi = pytest.importorskip("scipy.ndimage")
    for case in cr.CASES:
        for conn, rank in zip(cr.CONNECTIVITIES, (1, 2, 3)):
            ref = cr.reference(case, conn)
            structure = ndi.generate_binary_structure(3, rank)
            for b in range(cr.BATCH):
                for c in range(cr.NC):
                    m, what = ref["m"][b, c], (cr.case_id(case), conn, b, c)
                    want, n = ndi.label(m, structure)
                    assert n == ref["count"][b, c] and np.array_equal(want, ref["labels"][b, c]), what
                    sizes = np.bincount(want.reshape(-1))
                    sizes[0] = 0
                    best = int(np.argmax(sizes)) if n else 0
                    assert ref["largest"][b, c].tolist() == [best, int(sizes[best])], what
                    assert np.array_equal(ref["filters"]["largest"][b, c], (want == best) & m), what
                    for k in cr.MIN_SIZES:
                        assert np.array_equal(ref["filters"][("min_size", k)][b, c], m & (sizes[want] >= k)), what
                    if conn == 6:
                        assert np.array_equal(ref["filters"]["fill_holes"][b, c], ndi.binary_fill_holes(m)), what
