"""CPU tier of the volume preprocessing (no kernel is launched): the four entries are declared, exported and bound and refuse every
documented bad argument; the numpy restatement the GPU tests compare against (tests/resample_reference.py) equals scipy.ndimage on the
inputs of the GPU tests and the closed forms; the inputs of the GPU tests keep every coordinate away from the decisions a last bit
could flip; the Python wrappers refuse what they document; the bar is what the restatement measures."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import resample_reference as rr
from dm3d_amd import data, ops          # every test here belongs to the feature: none runs without these

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 0x10000                                   # an aligned non-null "pointer": nothing is launched, so nothing dereferences it
DESCS = {"spline_filter": "SplineDesc", "affine_resample": "ResampleDesc", "volume_normalize": "NormalizeDesc", "augment": "AugmentDesc"}
ENTRY = {"spline_filter": "dm3d_spline_filter", "affine_resample": "dm3d_affine_resample", "volume_normalize": "dm3d_volume_normalize",
         "augment": "dm3d_augment"}
STRUCT = {"spline_filter": "dm3d_spline_desc", "affine_resample": "dm3d_resample_desc", "volume_normalize": "dm3d_normalize_desc",
          "augment": "dm3d_augment_desc"}
OK = {
    "spline_filter": dict(x=A, coeff=A, volumes=2, d=5, h=6, w=7),
    "affine_resample": dict(src=A, table=A, out=A, in_f64=0, volumes=2, id=5, ih=6, iw=7, od=3, oh=4, ow=5, order=3, cval=0.0),
    "volume_normalize": dict(x=A, out=A, volumes=2, n=100, partials=A, minmax=A, flag=A),
    "augment": dict(x=A, out=A + (1 << 20), mask=A + (2 << 20), mask_out=A + (3 << 20), batch=2, d=3, h=4, w=5, c=1, cm=2, flip=A, brightness=A, contrast=A, draw=7, seed=1,
                    flip_chance=0.6, brightness_lo=0.9, brightness_hi=1.1, contrast_lo=0.9, contrast_hi=1.1, partials=A),
}
BAD = [
    ("spline_filter", dict(x=0), "x and coeff must be non-null"), ("spline_filter", dict(coeff=0), "x and coeff must be non-null"),
    ("spline_filter", dict(coeff=A + 4), "8-byte aligned"), ("spline_filter", dict(volumes=0), "volumes=0"),
    ("spline_filter", dict(d=0), "d=0"), ("spline_filter", dict(h=0), "h=0"), ("spline_filter", dict(w=0), "w=0"),
    ("spline_filter", dict(d=513), "d=513 h=6 w=7 exceeds DM3D_SPLINE_MAX_EXTENT=512"),
    ("spline_filter", dict(h=513), "exceeds DM3D_SPLINE_MAX_EXTENT=512"), ("spline_filter", dict(w=513), "exceeds DM3D_SPLINE_MAX_EXTENT=512"),
    ("affine_resample", dict(src=0), "src, table and out must be non-null"), ("affine_resample", dict(table=0), "src, table and out must be non-null"),
    ("affine_resample", dict(out=0), "src, table and out must be non-null"), ("affine_resample", dict(in_f64=2), "in_f64=2"),
    ("affine_resample", dict(in_f64=1, src=A + 4), "aligned"), ("affine_resample", dict(table=A + 4), "aligned"),
    ("affine_resample", dict(order=2), "order=2 (0, 1 or 3; orders 2, 4 and 5 are not offered)"), ("affine_resample", dict(order=5), "order=5"),
    ("affine_resample", dict(order=-1), "order=-1"), ("affine_resample", dict(volumes=0), "volumes=0"), ("affine_resample", dict(volumes=65536), "volumes=65536"),
    ("affine_resample", dict(id=0), "input d=0"), ("affine_resample", dict(iw=0), "input d=5 h=6 w=0"), ("affine_resample", dict(oh=0), "output d=3 h=0"),
    ("affine_resample", dict(cval=float("nan")), "cval=nan"), ("affine_resample", dict(cval=float("inf")), "cval=inf"),
    ("affine_resample", dict(id=2048, ih=2048, iw=512), "at most 2^31 - 1"),
    ("volume_normalize", dict(x=0), "must be non-null"), ("volume_normalize", dict(flag=0), "must be non-null"), ("volume_normalize", dict(minmax=0), "must be non-null"),
    ("volume_normalize", dict(partials=A + 2), "4-byte aligned"), ("volume_normalize", dict(volumes=0), "volumes=0"), ("volume_normalize", dict(n=0), "n=0"),
    ("augment", dict(x=0), "must be non-null"), ("augment", dict(flip=0), "must be non-null"), ("augment", dict(partials=0), "must be non-null"),
    ("augment", dict(mask=0), "both given or both null"), ("augment", dict(mask_out=0), "both given or both null"),
    ("augment", dict(partials=A + 4), "8-byte"), ("augment", dict(batch=0), "batch=0"), ("augment", dict(d=0), "d=0"), ("augment", dict(c=0), "c=0"),
    ("augment", dict(cm=0), "cm=0"), ("augment", dict(draw=8), "draw=8"), ("augment", dict(out=A), "out must not overlap x"),
    ("augment", dict(out=A + 476), "out must not overlap x"), ("augment", dict(mask_out=A + (2 << 20)), "mask_out must not overlap mask"),
    ("augment", dict(mask_out=A + (2 << 20) + 956), "mask_out must not overlap mask"), ("augment", dict(out=A + (2 << 20)), "out must not overlap mask"),
    ("augment", dict(mask_out=A), "mask_out must not overlap x"), ("augment", dict(mask_out=A + (1 << 20)), "out and mask_out must not overlap"),
    ("augment", dict(flip_chance=1.5), "flip_chance=1.5"), ("augment", dict(brightness_lo=1.2), "brightness range"),
    ("augment", dict(contrast_hi=float("nan")), "contrast range"),
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
        # the ctypes mirror has the header's fields, in its order, with its types
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
    assert f"#define DM3D_SPLINE_MAX_EXTENT {_lib.SPLINE_MAX_EXTENT}\n" in header and _lib.SPLINE_MAX_EXTENT >= 256
    assert f"#define DM3D_SPLINE_LANES {rr.SPLINE_TILE}\n" in header
    assert f"#define DM3D_RESAMPLE_F32 {_lib.RESAMPLE_F32}\n" in header and f"#define DM3D_RESAMPLE_F64 {_lib.RESAMPLE_F64}\n" in header
    assert f"#define DM3D_NORM_PARTIAL_BLOCKS {_lib.NORM_PARTIAL_BLOCKS}\n" in header and f"#define DM3D_AUG_PARTIAL_BLOCKS {_lib.AUG_PARTIAL_BLOCKS}\n" in header
    assert "#define DM3D_STREAM_AUGMENT 0x%Xu\n" % _lib.STREAM_AUGMENT in header and _lib.STREAM_AUGMENT == rr.STREAM_AUGMENT
    from oracle import ref_philox as rp
    assert rr.STREAM_AUGMENT not in (rp.STREAM_RANDN, rp.STREAM_DDPM, rp.STREAM_DDIM, rp.STREAM_DPM_SDE, rp.STREAM_EDIT)
    assert "dm3d_resample.hip" in open(os.path.join(ROOT, "3d-condtional-stable-diffusion_amd", "csrc", "Makefile")).read()


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
    x = torch.zeros(2, 4, 5, 6)
    eye = [1.0, 1.0, 1.0]
    for order in (2, 4, 5, -1):
        with pytest.raises(ValueError, match="order must be 0, 1 or 3"):
            ops.affine_transform(x, eye, order=order)
    for mode in ("mirror", "nearest", "reflect", "wrap", "grid-constant"):
        with pytest.raises(ValueError, match='mode must be "constant"'):
            ops.affine_transform(x, eye, mode=mode)
    with pytest.raises(ValueError, match="exceeds 512 voxels per axis"):
        ops.spline_filter(torch.zeros(1, 513, 1, 1))
    with pytest.raises(ValueError, match="exceeds 512 voxels per axis"):
        ops.affine_transform(torch.zeros(1, 1, 1, 513), eye)
    for bad in (x.double(), x.half(), x.int(), np.zeros((2, 4, 5, 6), np.float32)):
        with pytest.raises(ValueError, match="must be a float32 tensor"):
            ops.affine_transform(bad, eye)
        with pytest.raises(ValueError, match="must be a float32 tensor"):
            ops.spline_filter(bad)
        with pytest.raises(ValueError, match="must be a float32 tensor"):
            data.normalize(bad)
    with pytest.raises(ValueError, match=r"\[B,D,H,W\] or \[B,D,H,W,C\]"):
        ops.spline_filter(torch.zeros(4, 5))
    for bad in ([1.0, 1.0], np.eye(2), np.eye(5), np.zeros((3, 3, 3)), np.zeros((2, 3, 4)), 1.0):
        with pytest.raises(ValueError, match=r"matrix must be a 3-vector, \[3,3\], \[4,4\] homogeneous or \[B,3,3\]"):
            ops.affine_transform(x, bad)
    bad_row = np.eye(4)
    bad_row[3, 0] = 1e-9
    for bad in (bad_row, np.stack([np.eye(4), 2.0 * np.eye(4)])):
        with pytest.raises(ValueError, match=r"last row of a homogeneous matrix must be \(0, 0, 0, 1\)"):
            ops.affine_transform(x, bad)
    with pytest.raises(ValueError, match="offset must be left at 0 with a homogeneous matrix"):
        ops.affine_transform(x, np.eye(4), offset=[1.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="offset must be a scalar, a 3-vector"):
        ops.affine_transform(x, eye, offset=[1.0, 2.0])
    with pytest.raises(ValueError, match="matrix and offset must be finite"):
        ops.affine_transform(x, [1.0, float("nan"), 1.0])
    with pytest.raises(ValueError, match="output_shape must be three positive extents"):
        ops.affine_transform(x, eye, output_shape=(4, 0, 4))
    with pytest.raises(ValueError, match="cval must be finite"):
        ops.affine_transform(x, eye, cval=float("inf"))
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        ops.affine_transform(x, eye)                                # everything else in order: only the device is missing
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        ops.spline_filter(x)
    with pytest.raises(ValueError, match="one channel per volume"):
        ops.volume_normalize(torch.zeros(1, 2, 2, 2, 2))
    with pytest.raises(ValueError, match="BraTS branch .* is not offered"):
        data.preprocess(x, np.eye(4), (1, 1, 1), branch="brats")
    with pytest.raises(ValueError, match="three positive finite voxel sizes"):
        data.reslice(x, np.eye(4), (1.0, 0.0, 1.0), (1, 1, 1))
    with pytest.raises(ValueError, match=r"affine must be \[4,4\] or \[B,4,4\]"):
        data.reslice(x, np.eye(3), (1, 1, 1), (1, 1, 1))
    with pytest.raises(ValueError, match=r"images must be \[B,D,H,W,C\]"):
        data.augment(x, seed=1)
    assert set(data.__all__) == {"reslice", "transform_image", "normalize", "augment", "preprocess"}
    for doc, words in ((data.augment.__doc__, ("(1 + factor)", "un-augmented", "0xA063")), (data.preprocess.__doc__, ("np.zeros_like", "fury")),
                       (data.normalize.__doc__, ("check=True", "at once"))):
        assert all(w in doc for w in words), words


# ---- the restatement against scipy, on the inputs of the GPU tests ------------------------------------------------------------------------
SCIPY_BOUND = 1e-12


def test_restatement_equals_scipy_on_the_gpu_inputs():
    ndi = pytest.importorskip("scipy.ndimage")
    mats, offs = rr.generic_matrices()
    x = rr.volumes(rr.IN_SHAPE, 3)
    worst = 0.0
    for b in range(3):
        for order in (0, 1, 3):
            for cval in rr.CVALS:
                ours = rr.affine_transform(x[b], mats[b], offs[b], rr.OUT_SHAPE, order, cval)
                theirs = ndi.affine_transform(x[b].astype(np.float64), mats[b], offs[b], rr.OUT_SHAPE, order=order, mode="constant", cval=cval)
                worst = max(worst, float(np.abs(ours - theirs).max()))
    shape, m, off, oshape = rr.thin_case()
    v = rr.volumes(shape, 1)[0]
    for order in (0, 1, 3):
        worst = max(worst, float(np.abs(rr.affine_transform(v, m, off, oshape, order) - ndi.affine_transform(v.astype(np.float64), m, off, oshape, order=order)).max()))
    for name, ishape, m, off, oshape in rr.exact_cases():
        v = rr.volumes(ishape, 1)[0]
        for order in (0, 1):
            theirs = ndi.affine_transform(v.astype(np.float64), np.diag(m), off, oshape, order=order, cval=rr.CVALS[1])
            assert np.array_equal(rr.affine_transform(v, m, off, oshape, order, rr.CVALS[1]), theirs), (name, order)
    for shape in rr.PREFILTER_SHAPES:
        v = rr.volumes(shape, 1)[0]
        worst = max(worst, float(np.abs(rr.spline_filter(v) - ndi.spline_filter(v.astype(np.float64), 3, mode="mirror")).max()))
    x2 = rr.volumes(rr.IN_SHAPE + (2,), 2, rr.SEED + 1)
    for b in range(2):
        for c in range(2):
            theirs = ndi.affine_transform(x2[b, ..., c].astype(np.float64), mats[b], offs[b], rr.OUT_SHAPE)
            worst = max(worst, float(np.abs(rr.affine_transform(x2[b, ..., c], mats[b], offs[b], rr.OUT_SHAPE, 3) - theirs).max()))
    print(f"restatement against scipy.ndimage: worst {worst:.3e}")
    assert worst <= SCIPY_BOUND


def test_prefilter_in_front_of_constant_mode_is_the_mirror_one():
    ndi = pytest.importorskip("scipy.ndimage")
    v = rr.volumes(rr.IN_SHAPE, 1)[0].astype(np.float64)
    m, off = rr.generic_matrices()
    a = ndi.affine_transform(v, m[0], off[0], rr.OUT_SHAPE, order=3, mode="constant")
    b = ndi.affine_transform(ndi.spline_filter(v, 3, mode="mirror"), m[0], off[0], rr.OUT_SHAPE, order=3, mode="constant", prefilter=False)
    assert np.array_equal(a, b)


def test_pipeline_equals_scipy_carrying_float64():
    """transform_image with nothing rounded between the stages is the reference's chain of scipy calls."""
    ndi = pytest.importorskip("scipy.ndimage")
    v = rr.volumes(rr.TI_SHAPE, 1)[0]

    def sp_reslice(x, aff, z, nz):
        z, nz = np.array(z, float), np.array(nz, float)
        Rx = np.eye(4)
        Rx[:3, :3] = np.diag(nz / z)
        return ndi.affine_transform(x, nz / z, output_shape=tuple(np.round(z / nz * np.array(x.shape)).astype(int)), order=1), aff @ Rx

    i2, a2 = sp_reslice(v.astype(np.float64), rr.ti_affine(), rr.TI_VOXSIZE, (1, 1, 1))
    a2[:3, 3] += np.array(rr.TI_INIT) // 2
    t, _ = sp_reslice(ndi.affine_transform(i2, np.linalg.inv(a2), output_shape=rr.TI_INIT), np.eye(4), (1, 1, 1), (rr.TI_SCALE,) * 3)
    ours, a2_ours = rr.transform_image(v, rr.ti_affine(), rr.TI_VOXSIZE, rr.TI_SCALE, rr.TI_INIT, between=lambda a: a)
    assert ours.shape == (8, 8, 8) and np.array_equal(a2_ours, a2)
    assert np.abs(ours - t).max() <= SCIPY_BOUND
    stored, _ = rr.transform_image(v, rr.ti_affine(), rr.TI_VOXSIZE, rr.TI_SCALE, rr.TI_INIT)
    print(f"float32 stores between the stages against float64 carried: {np.abs(stored - t).max():.3e}")
    assert np.abs(stored - t).max() <= rr.RESAMPLE_TOL                  # the stores between the stages stay inside the bar of one
    assert 0.2 <= (stored != 0).mean() <= 0.9


# ---- the restatement against closed forms ------------------------------------------------------------------------------------------------
def test_closed_forms():
    v = rr.volumes((9, 12, 7), 1)[0]
    v64 = v.astype(np.float64)
    for order in (0, 1):
        assert np.array_equal(rr.affine_transform(v, (1.0, 1.0, 1.0), 0.0, None, order), v64)
        shifted = rr.affine_transform(v, (1.0, 1.0, 1.0), (2.0, -1.0, 3.0), None, order, cval=-2.0)
        want = np.full(v.shape, -2.0)
        want[:7, 1:, :4] = v64[2:, :11, 3:]
        assert np.array_equal(shifted, want)
        assert np.array_equal(rr.affine_transform(v, (2.0, 2.0, 2.0), 0.0, (5, 6, 4), order), v64[::2, ::2, ::2])
    half = rr.affine_transform(v, (0.5, 0.5, 0.5), 0.0, (18, 24, 14), 1, cval=-2.0)
    assert np.array_equal(half[:17:2, :23:2, :13:2], v64) and (half[17] == -2.0).all() and (half[:, 23] == -2.0).all() and (half[:, :, 13] == -2.0).all()
    assert np.array_equal(half[1:16:2, 0, 0], (v64[:-1, 0, 0] * 0.5 + v64[1:, 0, 0] * 0.5))
    # order 3 through the prefilter interpolates: the identity returns the data, a constant stays a constant
    assert np.abs(rr.affine_transform(v, (1.0, 1.0, 1.0), 0.0, None, 3) - v64).max() < 1e-14
    m, off = rr.generic_matrices()
    const = rr.affine_transform(np.full(rr.IN_SHAPE, 0.625, np.float32), m[0], off[0], rr.OUT_SHAPE, 3, cval=-1.0)
    assert np.abs(const[const != -1.0] - 0.625).max() < 1e-14
    assert np.array_equal(rr.spline_filter(np.ones((1, 1, 1), np.float32)), np.ones((1, 1, 1)))          # lines of 1 are left alone
    assert np.array_equal(rr.mirror(np.arange(-4, 7), 3), [0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2]) and np.array_equal(rr.mirror(np.arange(-2, 4), 2), [0, 1, 0, 1, 0, 1])
    # normalize and augment
    x = np.array([[-3.0, 1.0], [0.5, 2.0]], np.float32).reshape(1, 2, 2)
    mn, mx, n = rr.normalize(x)
    assert (mn, mx) == (0.5, 3.0) and np.array_equal(n, np.array([1.0, 0.2, 0.0, 0.6]).reshape(1, 2, 2))
    img = np.array([0.0, 0.5, 1.0, 0.25], np.float32).reshape(2, 1, 2, 1)
    msk = np.arange(4, dtype=np.float32).reshape(2, 1, 2, 1)
    out, m2 = rr.augment(img, msk, 1, 1.0, 0.0)
    assert np.array_equal(out, img[::-1].astype(np.float64)) and np.array_equal(m2, msk[::-1])
    out, _ = rr.augment(img, None, 0, 2.0, 1.0)                                 # t = (0, 1, 1, .5), mean .625, gain 2: the literal (1 + factor)
    assert np.array_equal(out.reshape(-1), [0.0, 1.0, 1.0, 0.375])


def test_reslice_rule():
    v = rr.volumes((10, 12, 9), 1)[0]
    out, a2 = rr.reslice(v, np.diag([1.5, 1.0, 2.0, 1.0]), (1.5, 1.0, 2.0), (1.0, 1.0, 1.0))
    assert out.shape == (15, 12, 18) and np.array_equal(a2, np.eye(4))
    out, _ = rr.reslice(v, np.eye(4), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0))
    assert out.shape == (5, 6, 4) and np.array_equal(out, v.astype(np.float64)[::2, ::2, ::2][:5, :6, :4])       # round(4.5) = 4: half to even


# ---- the conditions on the inputs of the GPU tests ---------------------------------------------------------------------------------------
def test_generic_cases_stay_clear_of_every_decision():
    mats, offs = rr.generic_matrices()
    for b in range(3):
        c = rr.coordinates(mats[b], offs[b], rr.OUT_SHAPE)
        for h in range(3):
            assert np.abs(c[h] - np.round(c[h])).min() > 1e-6, (b, h)           # 0 and n - 1 are integers too
            assert np.abs(c[h] + 0.5 - np.round(c[h] + 0.5)).min() > 1e-6, (b, h)      # the rounding of order 0
        outside = 1.0 - rr.inside_mask(c, rr.IN_SHAPE).mean()
        print(f"volume {b}: {100 * outside:.0f} % of the outputs are outside")
        assert 0.2 <= outside <= 0.8, (b, outside)
        assert not np.allclose(mats[b], mats[(b + 1) % 3])
    shape, m, off, oshape = rr.thin_case()
    c = rr.coordinates(m, off, oshape)
    assert (c[0] == 0.0).all() and all(np.abs(c[h] - np.round(c[h])).min() > 1e-6 for h in (1, 2))
    assert 0.05 <= rr.inside_mask(c, shape).mean() <= 0.95
    a = rr.ti_affine()
    z, one = np.array(rr.TI_VOXSIZE), np.ones(3)
    stages = [(rr.TI_SHAPE, np.diag(one / z), np.zeros(3), (15, 12, 18))]
    a2 = a @ np.diag(list(one / z) + [1.0])
    a2[:3, 3] += 8
    inv = np.linalg.inv(a2)
    stages.append(((15, 12, 18), inv[:3, :3], inv[:3, 3], rr.TI_INIT))
    c = rr.coordinates(*stages[1][1:])
    assert all(np.abs(c[h] - np.round(c[h])).min() > 1e-6 for h in range(3))


def test_the_bar_is_what_the_restatement_measures():
    worst = max(rr.f32_gap(v) for v in rr.interpolating_values())
    print(f"worst |f32 - f64| over the interpolating GPU cases: {worst:.4e}")
    assert worst <= rr.RESAMPLE_F32_WORST <= 1.01 * worst
    assert rr.RESAMPLE_TOL == 4 * rr.RESAMPLE_F32_WORST and not hasattr(rr, "TRANSFORM_TOL")          # transform_image's stages are in the set
    stages = []
    rr.transform_image(rr.volumes(rr.TI_SHAPE, 1)[0], rr.ti_affine(), rr.TI_VOXSIZE, rr.TI_SCALE, rr.TI_INIT, stages=stages)
    assert len(stages) == 3 and any(np.array_equal(stages[1], v) for v in rr.interpolating_values())


def test_augment_draw_is_the_philox_block():
    from oracle import ref_philox as rp
    flip, b, c = rr.augment_draw(0x0123456789ABCDEF, 64)
    words = rp.philox4x32_10(np.arange(64, dtype=np.uint64), 0, 0, 0xA063, 0x89ABCDEF, 0x01234567)
    u = [w.astype(np.float64) / 2.0 ** 32 for w in words]
    assert np.array_equal(flip, (u[0].astype(np.float32) >= np.float32(0.6)).astype(np.int32)) and 0 < flip.sum() < 64
    assert b.dtype == c.dtype == np.float32 and np.abs(b - (0.9 + 0.2 * u[1])).max() < 1e-6 and np.abs(c - (0.9 + 0.2 * u[2])).max() < 1e-6
    assert b.min() >= 0.9 and b.max() <= np.float32(1.1) and c.min() >= 0.9 and c.max() <= np.float32(1.1)
    f2, b2, c2 = rr.augment_draw(0x0123456789ABCDEF, 8)
    assert np.array_equal(f2, flip[:8]) and np.array_equal(b2, b[:8]) and np.array_equal(c2, c[:8])          # a sample's draw depends on its index alone
    assert not np.array_equal(rr.augment_draw(1, 64)[1], b)
    small = rr.augment_draw(rr.SEED, 6)[0]
    assert 0 < small.sum() < 6                                                  # the GPU test's batch holds flipped and kept samples
