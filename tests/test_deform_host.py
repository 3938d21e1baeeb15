"""CPU tier of the spatial augmentation (no kernel is launched): the numpy restatement the GPU tests compare against
(tests/deform_reference.py) equals scipy.ndimage — the Gaussian filter bit for bit, the warp exactly at orders 0 and 1 and within the
bound of tests/test_resample_host.py at order 3; the three entries are declared, exported and bound and refuse every documented bad
argument; the Python wrappers refuse what they document before the library is touched; random_affine's matrices are the stated ones;
the inputs of the GPU warp test meet the conditions that test relies on."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import deform_reference as dr
import resample_reference as rr
from dm3d_amd import data, ops          # every test here belongs to the feature: none runs without these

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 0x10000                                   # an aligned non-null "pointer": nothing is launched, so nothing dereferences it
SCIPY_BOUND = 1e-12                           # tests/test_resample_host.py's bound on the affine restatement
DESCS = {"gaussian_filter": "GaussDesc", "uniform_field": "FieldDesc", "warp": "WarpDesc"}
ENTRY = {"gaussian_filter": "dm3d_gaussian_filter", "uniform_field": "dm3d_uniform_field", "warp": "dm3d_warp"}
STRUCT = {"gaussian_filter": "dm3d_gauss_desc", "uniform_field": "dm3d_field_desc", "warp": "dm3d_warp_desc"}
WEIGHTS = np.zeros((3, dr.GAUSS_MAX_RADIUS + 1))
WEIGHTS[:, 0] = 1.0
OK = {
    "gaussian_filter": dict(x=A, out=A, weights=WEIGHTS.ctypes.data, volumes=2, d=5, h=6, w=7, rd=1, rh=-1, rw=0, mode=0, cval=0.0, gains=0),
    "uniform_field": dict(out=A, n=100, seed=1, draw=0),
    "warp": dict(src=A, table=A, field=A, out=A + (1 << 20), in_f64=0, field_f64=0, volumes=4, vols_per_field=2, id=5, ih=6, iw=7, od=3, oh=4, ow=5,
                 order=1, cval=0.0),
}
BAD = [
    ("gaussian_filter", dict(x=0), "x and out must be non-null"), ("gaussian_filter", dict(out=0), "x and out must be non-null"),
    ("gaussian_filter", dict(out=A + 2), "4-byte aligned"), ("gaussian_filter", dict(volumes=0), "volumes=0"),
    ("gaussian_filter", dict(d=0), "d=0"), ("gaussian_filter", dict(w=0), "w=0"),
    ("gaussian_filter", dict(h=513), "d=5 h=513 w=7 exceeds DM3D_SPLINE_MAX_EXTENT=512"),
    ("gaussian_filter", dict(rd=65), "rd=65 rh=-1 rw=0 (-1, an axis left out, to DM3D_GAUSS_MAX_RADIUS=64)"), ("gaussian_filter", dict(rw=-2), "rw=-2"),
    ("gaussian_filter", dict(weights=0), "weights must be non-null"), ("gaussian_filter", dict(mode=4), "mode=4"), ("gaussian_filter", dict(mode=-1), "mode=-1"),
    ("gaussian_filter", dict(cval=float("nan")), "cval=nan"), ("gaussian_filter", dict(cval=float("inf")), "cval=inf"),
    ("gaussian_filter", dict(gains=2), "gains=2"), ("gaussian_filter", dict(gains=3, gain1=float("inf")), "gain (0, inf, 0)"),
    ("gaussian_filter", dict(out=A + 8), "out must be x itself or share no byte with it"),
    ("uniform_field", dict(out=0), "out must be non-null"), ("uniform_field", dict(out=A + 1), "4-byte aligned"), ("uniform_field", dict(n=0), "n=0"),
    ("uniform_field", dict(draw=-1), "draw=-1"), ("uniform_field", dict(n=1 << 42), "exceeds the grid"),
    ("warp", dict(src=0), "src, table and out must be non-null"), ("warp", dict(table=0), "src, table and out must be non-null"),
    ("warp", dict(out=0), "src, table and out must be non-null"), ("warp", dict(in_f64=2), "in_f64=2"), ("warp", dict(field_f64=-1), "field_f64=-1"),
    ("warp", dict(field_f64=1, field=A + 4), "aligned"), ("warp", dict(table=A + 4), "aligned"), ("warp", dict(order=2), "order=2 (0, 1 or 3"),
    ("warp", dict(volumes=0), "volumes=0"), ("warp", dict(volumes=65536), "volumes=65536"), ("warp", dict(vols_per_field=0), "vols_per_field=0"),
    ("warp", dict(vols_per_field=3), "vols_per_field=3 (at least 1, a divisor of volumes=4)"), ("warp", dict(id=0), "input d=0"),
    ("warp", dict(ow=0), "output d=3 h=4 w=0"), ("warp", dict(cval=float("nan")), "cval=nan"), ("warp", dict(id=2048, ih=2048, iw=512), "at most 2^31 - 1"),
    ("warp", dict(out=A + 16), "out must not overlap src"),
]


def _desc(_lib, short, **override):
    d = getattr(_lib, DESCS[short])()
    for k, v in {**OK[short], **override}.items():
        setattr(d, k, v)
    return d


def test_entries_are_declared_exported_and_bound(built_library):
    from dm3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dm3d.h")).read()
    handle = C.CDLL(built_library)
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
    for short, name in ENTRY.items():
        mirror = getattr(_lib, DESCS[short])
        assert re.search(r"\bint %s\(const %s\* d, void\* stream\);" % (name, STRUCT[short]), header), name
        assert hasattr(handle, name), name
        assert _lib.SIGNATURES[name] == (C.c_int, [C.POINTER(mirror), C.c_void_p]), name
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (STRUCT[short], STRUCT[short]), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in (s.strip() for s in body.split(";")):
            if decl:
                ctype, names = decl.removeprefix("const ").split(" ", 1)
                fields += [(n.strip(" *"), ctype + ("*" if "*" in ctype + names else "")) for n in names.split(",")]
        assert [f[0] for f in fields] == [f[0] for f in mirror._fields_], short
        for (fname, ctype), (_, m) in zip(fields, mirror._fields_):
            assert m is (C.c_void_p if ctype.endswith("*") else kinds[ctype]), (short, fname, ctype, m)
    assert _lib.lib().dm3d_version() == _lib.ABI_VERSION == 111 and "#define DM3D_VERSION 111 " in header
    assert f"#define DM3D_GAUSS_MAX_RADIUS {_lib.GAUSS_MAX_RADIUS}\n" in header and _lib.GAUSS_MAX_RADIUS == dr.GAUSS_MAX_RADIUS >= 64
    for i, mode in enumerate(dr.MODES):
        assert f"#define DM3D_GAUSS_{mode.upper()} {i}\n" in header and _lib.GAUSS_MODES[mode] == i
    assert "#define DM3D_STREAM_ELASTIC 0x%Xu\n" % _lib.STREAM_ELASTIC in header and _lib.STREAM_ELASTIC == dr.STREAM_ELASTIC
    from oracle import ref_philox as rp
    assert dr.STREAM_ELASTIC not in (rp.STREAM_RANDN, rp.STREAM_DDPM, rp.STREAM_DDIM, rp.STREAM_DPM_SDE, rp.STREAM_EDIT, _lib.STREAM_AUGMENT,
                                     _lib.STREAM_CODEBOOK, _lib.STREAM_CODEBOOK_SHUFFLE)
    csrc = os.path.join(ROOT, "3d-condtional-stable-diffusion_amd", "csrc")
    assert "dm3d_deform.hip" in open(os.path.join(csrc, "Makefile")).read()
    # the tap code has one home: both resampling files include it, neither defines it
    for f in ("dm3d_resample.hip", "dm3d_deform.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "dm3d_interp.h"' in text and "int mirror_tap(" not in text and "void axis_taps(" not in text, f


def test_entries_refuse_bad_arguments(built_library):
    """Every documented precondition is checked before anything is launched: DM3D_EINVAL and a message that starts with the entry's short
    name and names the fault, with no GPU in the machine."""
    from dm3d_amd import _lib
    lib = _lib.lib()
    failures = []
    for short, override, words in BAD:
        lib.dm3d_fill(None, 0, 0.0, None)                           # leaves a known message behind
        rc = getattr(lib, ENTRY[short])(C.byref(_desc(_lib, short, **override)), None)
        msg = (lib.dm3d_last_error() or b"").decode()
        if rc != -1 or not msg.startswith(short + ":") or words not in msg:
            failures.append(f"{ENTRY[short]}({override}): rc {rc}, message {msg!r}, wanted {words!r}")
    for short, name in ENTRY.items():
        if getattr(lib, name)(None, None) != -1 or f"{short}: null descriptor".encode() not in lib.dm3d_last_error():
            failures.append(f"{name}(NULL)")
    assert not failures, "\n".join(failures)


def test_python_wrappers_refuse_what_they_document():
    """ValueError with the argument named, on CPU tensors: the library is never reached."""
    x = torch.zeros(2, 4, 5, 6)
    im = torch.zeros(2, 4, 5, 6, 2)
    u = torch.zeros(2, 3, 4, 5, 6)
    # 1. the filter
    with pytest.raises(ValueError, match="order must be 0"):
        ops.gaussian_filter(x, 1.0, order=1)
    for mode in ("wrap", "grid-wrap", "grid-constant"):
        with pytest.raises(ValueError, match='mode must be "reflect", "mirror", "nearest" or "constant"'):
            ops.gaussian_filter(x, 1.0, mode=mode)
    for cval in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cval must be finite"):
            ops.gaussian_filter(x, 1.0, cval=cval)
    for sigma in (-1.0, float("nan"), [1.0, float("inf"), 1.0], [1.0, 2.0], "a"):
        with pytest.raises(ValueError, match="sigma must be a finite scalar or 3-vector of at least 0"):
            ops.gaussian_filter(x, sigma)
    with pytest.raises(ValueError, match="radius 68, above DM3D_GAUSS_MAX_RADIUS=64"):
        ops.gaussian_filter(x, 17.0)
    with pytest.raises(ValueError, match="truncate must be a positive finite number"):
        ops.gaussian_filter(x, 1.0, truncate=0.0)
    with pytest.raises(ValueError, match="exceeds 512 voxels per axis"):
        ops.gaussian_filter(torch.zeros(1, 1, 513, 1), 1.0)
    with pytest.raises(ValueError, match="must be a float32 tensor"):
        ops.gaussian_filter(x.double(), 1.0)
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        ops.gaussian_filter(x, 16.0)                                # radius 64, everything in order: only the device is missing
    # 2. the warp
    for order in (2, 4, 5, -1):
        with pytest.raises(ValueError, match="order must be 0, 1 or 3"):
            ops.warp(x, u, order=order)
        with pytest.raises(ValueError, match="order must be 0, 1 or 3"):
            ops.map_coordinates(x, u.double(), order=order)
    with pytest.raises(ValueError, match="cval must be finite"):
        ops.warp(x, u, cval=float("nan"))
    with pytest.raises(ValueError, match="displacement and coordinates must not both be given"):
        ops.warp(x, u, coordinates=u.double())
    with pytest.raises(ValueError, match="matrix must stay None with coordinates"):
        ops.warp(x, matrix=np.eye(3), coordinates=u.double())
    for bad in (torch.zeros(2, 3, 4, 5, 7), torch.zeros(3, 3, 4, 5, 6), torch.zeros(2, 2, 4, 5, 6), torch.zeros(3, 4, 5, 6)):
        with pytest.raises(ValueError, match=r"displacement must be \[B,3,od,oh,ow\] or \[1,3,od,oh,ow\] with B=2 and the output shape \(4, 5, 6\)"):
            ops.warp(x, bad, output_shape=(4, 5, 6))
    with pytest.raises(ValueError, match=r"coordinates must be \[B,3,od,oh,ow\]"):
        ops.map_coordinates(x, torch.zeros(3, 4, 5, 6, dtype=torch.float64))
    with pytest.raises(ValueError, match="displacement must be a float32 or float64 tensor"):
        ops.warp(x, u.half())
    with pytest.raises(ValueError, match="displacement must be a float32 or float64 tensor"):
        ops.warp(x, np.zeros((2, 3, 4, 5, 6), np.float32))
    with pytest.raises(ValueError, match="displacement must be a contiguous device tensor"):
        ops.warp(x, u)                                              # a host field
    with pytest.raises(ValueError, match="displacement must be a contiguous device tensor"):
        ops.warp(im, torch.zeros(2, 3, 4, 5, 12)[..., ::2])         # a non-contiguous one
    with pytest.raises(ValueError, match="coordinates must be a contiguous device tensor"):
        ops.map_coordinates(x, u.double())
    with pytest.raises(ValueError, match="coordinates must be given"):
        ops.map_coordinates(x, None)
    with pytest.raises(ValueError, match="output_shape must be three positive extents"):
        ops.warp(x, output_shape=(4, 0, 4))
    with pytest.raises(ValueError, match=r"matrix must be a 3-vector, \[3,3\], \[4,4\] homogeneous or \[B,3,3\]"):
        ops.warp(x, matrix=np.eye(2))
    with pytest.raises(ValueError, match="must be a float32 tensor"):
        ops.warp(x.double(), u)
    with pytest.raises(ValueError, match="exceeds 512 voxels per axis"):
        ops.warp(torch.zeros(1, 1, 1, 513), order=3)
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        ops.warp(x)                                                 # everything else in order: only the device is missing
    # 3. the field
    for shape in ((4, 5), (4, 0, 5), 7):
        with pytest.raises(ValueError, match="shape must be three positive extents"):
            ops.elastic_field(shape, 2, 1.0, 1.0, 1)
    with pytest.raises(ValueError, match="exceeds 512 voxels per axis"):
        ops.elastic_field((4, 513, 4), 2, 1.0, 1.0, 1)
    for batch in (0, -1, 1.5):
        with pytest.raises(ValueError, match="batch must be a positive integer"):
            ops.elastic_field((4, 5, 6), batch, 1.0, 1.0, 1)
    for alpha in (float("nan"), [1.0, 2.0], None):
        with pytest.raises(ValueError, match="alpha must be a finite scalar or 3-vector"):
            ops.elastic_field((4, 5, 6), 2, alpha, 1.0, 1)
    with pytest.raises(ValueError, match="sigma must be a finite scalar or 3-vector of at least 0"):
        ops.elastic_field((4, 5, 6), 2, 1.0, -1.0, 1)
    with pytest.raises(ValueError, match="above DM3D_GAUSS_MAX_RADIUS=64"):
        ops.elastic_field((4, 5, 6), 2, 1.0, 20.0, 1)
    with pytest.raises(ValueError, match="seed must be an integer"):
        ops.elastic_field((4, 5, 6), 2, 1.0, 1.0, 1.5)
    for draw in (-1, 2 ** 31, 0.5):
        with pytest.raises(ValueError, match="draw must be an integer in"):
            ops.elastic_field((4, 5, 6), 2, 1.0, 1.0, 1, draw=draw)
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        ops.elastic_field((4, 5, 6), 2, 1.0, 1.0, 1, device="cpu")
    # 4. data
    for fn, kw in ((data.elastic_deform, dict(alpha=1.0, sigma=1.0, seed=1)), (data.random_affine, dict(seed=1)),
                   (data.spatial_augment, dict(seed=1, elastic_alpha=1.0, elastic_sigma=1.0))):
        with pytest.raises(ValueError, match=r"images must be \[B,D,H,W,C\]"):
            fn(x, **kw)
        with pytest.raises(ValueError, match=r"masks must be \[B,D,H,W,C\] with the batch and spatial shape of images"):
            fn(im, torch.zeros(2, 4, 5, 7, 1), **kw)
        with pytest.raises(ValueError, match="masks must be a float32 tensor"):
            fn(im, im.bool(), **kw)
    for name in ("rotate_range", "scale_range", "translate_range"):
        for bad in (-0.1, float("nan"), [0.1, 0.2]):
            with pytest.raises(ValueError, match=f"{name} must be a non-negative finite scalar or 3-vector"):
                data.random_affine(im, seed=1, **{name: bad})
    with pytest.raises(ValueError, match="scale_range must stay below 1"):
        data.random_affine(im, seed=1, scale_range=1.0)
    for seed in (-1, 1.5, None):
        with pytest.raises(ValueError, match="seed must be a non-negative integer"):
            data.random_affine(im, seed=seed)
    with pytest.raises(ValueError, match="elastic_alpha and elastic_sigma must be given together"):
        data.spatial_augment(im, seed=1, elastic_alpha=1.0)
    with pytest.raises(ValueError, match="alpha must be a finite scalar or 3-vector"):
        data.elastic_deform(im, alpha=float("inf"), sigma=1.0, seed=1)
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        data.random_affine(im, seed=1)                              # everything else in order: only the device is missing
    assert all(callable(getattr(data, n)) for n in ("elastic_deform", "random_affine", "spatial_augment"))
    for doc, words in ((data.random_affine.__doc__, ("numpy.random.Philox(seed)", "rng.uniform", "R @ diag(scales)", "centre")),
                       (data.elastic_deform.__doc__, ("coarse-grid-then-upsample", "not offered")), (data.spatial_augment.__doc__, ("one", "dm3d_warp")),
                       (ops.gaussian_filter.__doc__, ('"wrap"', "derivatives")), (ops.elastic_field.__doc__, ("0xE1A5", "e & 3"))):
        assert all(w in doc for w in words), words


# ---- the restatement against scipy -------------------------------------------------------------------------------------------------------
def test_gaussian_restatement_equals_scipy_bit_for_bit():
    ndi = pytest.importorskip("scipy.ndimage")
    for shape in dr.TAIL_SHAPES:
        x = rr.volumes(shape, 1)[0]
        for mode in dr.MODES:
            for sigma in dr.SIGMAS + ((1.5, 0.0, 0.7),):
                for cval in (0.0, -0.375):
                    ours = dr.gaussian_filter(x, sigma, mode, cval)
                    theirs = ndi.gaussian_filter(x, sigma, order=0, mode=mode, cval=cval, truncate=4.0)
                    assert ours.dtype == theirs.dtype == np.float32 and ours.tobytes() == theirs.tobytes(), (shape, mode, sigma, cval)
    r, w = dr.gaussian_weights(3.0)
    assert r == 12 > max(dr.TAIL_SHAPES[2]) and abs(w[0] + 2 * w[1:].sum() - 1.0) < 1e-15
    assert np.array_equal(dr.gaussian_filter(x, 0.0), x)                        # every axis left out
    one = np.full((1, 1, 1), 0.75, np.float32)                                  # a line of 1 is filtered: its extended taps are summed
    assert dr.gaussian_filter(one, 1.0, "constant", 2.0).tobytes() == ndi.gaussian_filter(one, 1.0, mode="constant", cval=2.0).tobytes() != one.tobytes()
    # the host table of the wrapper is the restatement's
    radii, table = ops._gauss_table((0.7, 0.0, 3.0), 4.0)
    assert radii == [3, -1, 12] and np.array_equal(table[2, :13], w) and np.array_equal(table[0, :4], dr.gaussian_weights(0.7)[1]) and not table[1].any()


def _warp_case(dtype=np.float32):
    x = rr.volumes(dr.WARP_SHAPE, 1)[0]
    field = dr.elastic_field(dr.WARP_SHAPE, 1, dr.WARP_ALPHA, dr.WARP_SIGMA, dr.WARP_SEED)[0].astype(dtype)
    return x, field


def test_warp_restatement_equals_scipy_map_coordinates():
    ndi = pytest.importorskip("scipy.ndimage")
    x, field = _warp_case()
    for matrix in (None, dr.warp_matrix()):
        coords = dr.warp_coordinates(matrix, 0.0, field)
        for order in (0, 1, 3):
            for cval in (0.0, -0.375):
                ours = dr.warp(x, field, matrix, order=order, cval=cval)
                theirs = ndi.map_coordinates(x.astype(np.float64), coords, order=order, mode="constant", cval=cval)
                if order == 3:
                    err = float(np.abs(ours - theirs).max())
                    print(f"order 3 against scipy.ndimage.map_coordinates: worst {err:.3e}")
                    assert err <= SCIPY_BOUND
                else:
                    assert np.array_equal(ours, theirs), (order, cval)
    grid = np.stack(np.meshgrid(*(np.arange(s, dtype=np.float64) for s in dr.WARP_SHAPE), indexing="ij"))
    assert np.array_equal(dr.warp_coordinates(None, 0.0, field), grid + field.astype(np.float64))          # the identity adds the grid exactly


def test_warp_inputs_meet_the_gpu_tests_conditions():
    """Asserted from the reference alone: 50 % to 99 % of the coordinates are inside, at most 0.1 % lie within 1 ulp of a half-integer,
    and the field is no small perturbation (it moves voxels by more than one voxel)."""
    x, field = _warp_case()
    assert field.dtype == np.float32 and float(np.abs(field).max()) > 1.0
    for matrix in (None, dr.warp_matrix()):
        coords = dr.warp_coordinates(matrix, 0.0, field)
        inside = float(rr.inside_mask(coords, dr.WARP_SHAPE).mean())
        share = float(dr.near_half(coords).mean())
        print(f"matrix {'given' if matrix is not None else 'none'}: {100 * inside:.1f} % inside, {100 * share:.3f} % near a half-integer, "
              f"worst |u| {np.abs(field).max():.2f}")
        assert 0.5 <= inside <= 0.99 and share <= dr.HALF_ULP_SHARE


def test_uniform_field_is_the_philox_block():
    from oracle import ref_philox as rp
    seed = 0x0123456789ABCDEF
    u = dr.uniform_field(1001, seed, draw=3)
    words = rp.philox4x32_10(np.arange(251, dtype=np.uint64), 0, 3, 0xE1A5, 0x89ABCDEF, 0x01234567)
    want = 2.0 * (np.stack(words, 1).reshape(-1)[:1001].astype(np.float64) / 2.0 ** 32) - 1.0
    assert u.dtype == np.float32 and u.shape == (1001,) and np.abs(u - want).max() < 2e-7 and u.min() >= -1.0 and u.max() <= 1.0
    assert abs(float(u.mean())) < 0.1 and abs(float(u.std()) - 3 ** -0.5) < 0.05
    assert np.array_equal(dr.uniform_field(64, seed, 3), u[:64])                # an element's draw depends on its index alone
    assert not np.array_equal(dr.uniform_field(64, seed, 4), u[:64]) and not np.array_equal(dr.uniform_field(64, seed + 1, 3), u[:64])
    f = dr.elastic_field((3, 4, 5), 2, (1.0, 2.0, 0.0), 0.0, seed)
    raw = dr.uniform_field(2 * 3 * 60, seed).reshape(2, 3, 3, 4, 5)
    assert np.array_equal(f[:, 0], raw[:, 0]) and np.array_equal(f[:, 1], raw[:, 1] * np.float32(2.0)) and not f[:, 2].any()


# ---- random_affine's matrices ------------------------------------------------------------------------------------------------------------
def test_affine_matrices():
    shape = (5, 9, 37)
    eye = data.affine_matrices(shape, 3, seed=7)
    assert eye.shape == (3, 4, 4) and eye.dtype == np.float64 and np.array_equal(eye, np.broadcast_to(np.eye(4), (3, 4, 4)))
    kw = dict(rotate_range=0.3, scale_range=(0.1, 0.2, 0.0), translate_range=2.5)
    a, b = data.affine_matrices(shape, 3, seed=7, **kw), data.affine_matrices(shape, 3, seed=7, **kw)
    assert np.array_equal(a, b) and np.array_equal(a, dr.affine_matrices(shape, 3, 7, **kw))
    assert not np.array_equal(a, data.affine_matrices(shape, 3, seed=8, **kw)) and not np.allclose(a[0], a[1])
    assert np.array_equal(a[:, 3], np.broadcast_to([0.0, 0.0, 0.0, 1.0], (3, 4)))
    centre = (np.array(shape) - 1) / 2.0
    for m in a:                                                                 # c = M (o - centre) + centre + t: the centre moves by t alone
        t = m[:3, :3] @ centre + m[:3, 3] - centre
        assert np.abs(t).max() <= 2.5 + 1e-12
        s = np.linalg.norm(m[:3, :3], axis=0)                                   # R is orthogonal: the column norms are the scales
        assert np.all(np.abs(s - 1.0) <= np.array([0.1, 0.2, 0.0]) + 1e-12) and abs(np.linalg.det(m[:3, :3]) - s.prod()) < 1e-12
    only_shift = data.affine_matrices(shape, 2, seed=3, translate_range=1.0)
    assert np.array_equal(only_shift[:, :3, :3], np.broadcast_to(np.eye(3), (2, 3, 3))) and only_shift[:, :3, 3].any()
