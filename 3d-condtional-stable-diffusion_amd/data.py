"""Device-side volume preprocessing: the reference's ``dataset_utils.py`` between a loaded MRI volume and ``train_step`` / ``test_step``.

Every voxel is touched by HIP kernels only (``ops.affine_transform``, ``ops.volume_normalize``, ``ops.augment``); the 4 x 4 affines, voxel
sizes and shapes are host values in float64, as they are in the reference.  Volumes are float32 device tensors [B,D,H,W] or NDHWC (a
single [D,H,W] volume is taken as a batch of one and returned as one).  NIfTI reading is not offered: callers pass arrays, affines and
voxel sizes.  Between two resamples a volume is rounded to float32, where the reference carries float64."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops

__all__ = ["reslice", "transform_image", "normalize", "augment", "preprocess"]    # the preprocessing set, pinned by its host test; clean_mask and the spatial augmentations are public beside it


def _batched(x):
    """[D,H,W] -> ([1,D,H,W], squeeze back); anything else as it is."""
    if isinstance(x, torch.Tensor) and x.dim() == 3:
        return x.unsqueeze(0), lambda t: t.squeeze(0)
    return x, lambda t: t


def _vec3(v, name):
    a = np.asarray(v, np.float64)
    if a.shape != (3,) or not np.isfinite(a).all() or (a <= 0).any():
        raise ValueError(f"{name} must be three positive finite voxel sizes, got {v!r}")
    return a


def _affine44(affine):
    a = np.asarray(affine.detach().cpu().numpy() if isinstance(affine, torch.Tensor) else affine, np.float64)
    if a.shape[-2:] != (4, 4) or a.ndim not in (2, 3):
        raise ValueError(f"affine must be [4,4] or [B,4,4], got {tuple(a.shape)}")
    return a


def reslice(x: torch.Tensor, affine, zooms, new_zooms, order: int = 1, cval: float = 0.0):
    """dipy's ``reslice`` restated: ``R = new_zooms / zooms``; ``new_shape = round(zooms / new_zooms * shape)`` (numpy's round, half to
    even); ``affine_transform(x, matrix=R, output_shape=new_shape, order=order, cval=cval)``; ``affine2 = affine @ diag(R, 1)``.
    Returns (volume, affine2); ``affine`` is [4,4] or [B,4,4]."""
    x, back = _batched(x)
    zooms, new_zooms, affine = _vec3(zooms, "zooms"), _vec3(new_zooms, "new_zooms"), _affine44(affine)
    ops._volume_check(x)
    R = new_zooms / zooms
    new_shape = tuple(int(s) for s in np.round(zooms / new_zooms * np.array(x.shape[1:4], np.float64)).astype(np.int64))
    if min(new_shape) < 1:
        raise ValueError(f"reslice of a {tuple(x.shape[1:4])} volume from {tuple(zooms)} to {tuple(new_zooms)} leaves an empty axis: {new_shape}")
    out = ops.affine_transform(x, R, output_shape=new_shape, order=order, cval=cval)
    Rx = np.eye(4)
    Rx[:3, :3] = np.diag(R)
    return back(out), affine @ Rx


def transform_image(x: torch.Tensor, affine, voxsize, scale=2, init_shape=(256, 256, 256)):
    """The reference's ``transform_image``: reslice to 1 mm (trilinear), add ``init_shape // 2`` to the translation of the resliced
    affine, resample through the inverse of that affine into ``init_shape`` with the cubic B-spline (``scipy.ndimage.affine_transform``'s
    default: order 3, prefiltered, zeros outside), then reslice by ``scale`` (trilinear).  The 4 x 4 inverse is taken on the host in
    float64.  Returns (volume of shape ``init_shape / scale``, affine2)."""
    x, back = _batched(x)
    init_shape = tuple(int(s) for s in init_shape)
    if len(init_shape) != 3 or min(init_shape) < 1:
        raise ValueError(f"init_shape must be three positive extents, got {init_shape!r}")
    image2, affine2 = reslice(x, affine, voxsize, (1.0, 1.0, 1.0))
    affine2 = affine2.copy()
    affine2[..., :3, 3] += np.array([s // 2 for s in init_shape], np.float64)
    inv = np.linalg.inv(affine2)
    centred = ops.affine_transform(image2, inv[..., :3, :3], inv[..., :3, 3], output_shape=init_shape, order=3)
    out, _ = reslice(centred, np.eye(4), (1.0, 1.0, 1.0), (float(scale),) * 3)
    return back(out), affine2


def normalize(x: torch.Tensor, *, check: bool = True) -> torch.Tensor:
    """Per volume: fold the negatives (``v[v < 0] *= -1``), then ``(v - min) / (max - min)``; min and max are exact, the quotient is
    evaluated in float64 and rounded once.  A constant volume (max = min, where the reference divides by zero) is refused on the device:
    it is written as zeros and a flag word is raised.  ``check=True`` reads the flags at once, one copy of B words that waits for the
    stream, and raises ``ValueError`` naming the constant volumes; ``check=False`` reads nothing back and returns the zeros
    (``ops.volume_normalize`` also returns the flags and the extrema, on the device)."""
    x, back = _batched(x)
    res = ops.volume_normalize(x)
    if check:
        bad = torch.nonzero(res.constant).flatten().tolist()
        if bad:
            raise ValueError(f"normalize: volume(s) {bad} are constant (max = min): there is no range to normalise by")
    return back(res.out)


def augment(images: torch.Tensor, masks: Optional[torch.Tensor] = None, *, seed: Optional[int] = None, flip_chance: float = 0.6,
            brightness_range=(0.9, 1.1), contrast_range=(0.9, 1.1), flip=None, brightness=None, contrast=None) -> ops.Augmented:
    """The reference's ``flip_axis_0``, ``adjust_brightness`` and ``adjust_contrast`` per sample of an NDHWC batch, the mask flipped with
    the image:

        t   = clip(x * b, 0, 1)
        out = clip((1 + c) * (t - mean(t)) + mean(t), 0, 1)         read at the position flipped along axis 0 (D) where the sample flips

    in float64 with a fixed-order sum behind the mean, stored as float32.  The gain is the reference's literal ``(1 + factor)``, so with
    c ~ U(0.9, 1.1) the contrast is about doubled, as it is there; it is kept, not corrected.  A sample flips with probability
    ``1 - flip_chance`` = 0.4 (the reference keeps the volume when ``random() < 0.6``), and b and c are uniform over their ranges.

    The stream.  The three uniforms of sample i are words 0, 1, 2 of the Philox4x32-10 block of counter (i, 0, 0, 0xA063) under the
    64-bit key ``seed``, each ``float32(word) * 2^-32``; flip = not (u0 < flip_chance), b = lo + (hi - lo) * u1, c = lo + (hi - lo) * u2 in
    float32.  They are drawn on the device, depend on (seed, sample index) alone and are returned.  Explicit ``flip`` (int32 [B]),
    ``brightness``, ``contrast`` (float32 [B]) device tensors override the draw; ``seed`` is needed unless all three are given.

    The reference's ``augmentDatasetHelperFunc`` computes the augmented volume and then returns the un-augmented one; this returns the
    augmented one.  Returns ``ops.Augmented(images, masks, flip, brightness, contrast)``."""
    return ops.augment(images, masks, seed=seed, flip_chance=flip_chance, brightness_range=brightness_range, contrast_range=contrast_range,
                       flip=flip, brightness=brightness, contrast=contrast)


def preprocess(x: torch.Tensor, affine, voxsize, mask: Optional[torch.Tensor] = None, *, branch: str = "default", scale=2,
               init_shape=(256, 256, 256)):
    """The reference's ``load_transform_img`` after loading, for its non-BraTS branch: multiply by ``mask`` (its CC359 / NFBS skull
    strip) when one is given, ``transform_image``, ``normalize``.  Returns ``(image[..., None], mask_out, context)`` in the layout
    ``train_step`` and ``test_step`` take: image float32 [B,d,h,w,1] in [0, 1], ``mask_out`` float32 zeros of the same shape, context int64
    zeros [B,1,1].  ``mask_out`` is all zeros because the reference overwrites the mask with ``np.zeros_like`` on this branch; the mask
    only strips the input.  ``branch="brats"`` is refused: the reference pads that branch through ``fury``'s slicer, which is not here."""
    if branch == "brats":
        raise ValueError('preprocess: the BraTS branch (transform_brats_image, padded through fury) is not offered')
    if branch != "default":
        raise ValueError(f'preprocess: branch must be "default", got {branch!r}')
    x, _ = _batched(x)
    ops._volume_check(x, one_channel=True)
    if x.dim() == 5:
        x = x.squeeze(-1)
    if mask is not None:
        mask, _ = _batched(mask)
        if mask.dim() == 5:
            mask = mask.squeeze(-1)
        if mask.shape != x.shape:
            raise ValueError(f"mask must have the volume's shape {tuple(x.shape)}, got {tuple(mask.shape)}")
        x = x * mask.to(x.dtype)
    vol, _ = transform_image(x, affine, voxsize, scale=scale, init_shape=init_shape)
    image = normalize(vol).unsqueeze(-1)
    context = torch.zeros(image.shape[0], 1, 1, dtype=torch.int64, device=image.device)
    return image, torch.zeros_like(image), context


class SpatialAugmented(NamedTuple):
    """What the spatial augmentations return: the warped ``images`` and ``masks`` (None without masks), the host ``matrices`` float64
    [B,4,4] that map an output voxel to its input coordinate (None where no affine was drawn) and the device displacement ``field``
    float32 [B,3,D,H,W] (None where none was drawn)."""
    images: torch.Tensor
    masks: Optional[torch.Tensor]
    matrices: Optional[np.ndarray]
    field: Optional[torch.Tensor]


def _image_mask_check(images, masks, host=None):
    """Dtype, rank and shape rules of both tensors, then ``host()`` (the caller's host arguments, whose value is returned), the devices last."""
    def masks_match():
        if masks.shape[:4] != images.shape[:4]:
            raise ValueError(f"masks must be [B,D,H,W,C] with the batch and spatial shape of images, got {tuple(masks.shape)} and {tuple(images.shape)}")

    def rest():
        checked = host() if host is not None else None
        if masks is not None:
            ops._volume_check(masks, "masks", ndhwc=True, host=masks_match)
        return checked

    return ops._volume_check(images, "images", ndhwc=True, host=rest)


def _range3(v, name):
    a = np.asarray(v, np.float64)
    if a.shape not in ((), (3,)) or not np.isfinite(a).all() or (a < 0).any():
        raise ValueError(f"{name} must be a non-negative finite scalar or 3-vector, got {v!r}")
    return np.broadcast_to(a, (3,))


def affine_matrices(shape, batch: int, seed: int, rotate_range=0.0, scale_range=0.0, translate_range=0.0) -> np.ndarray:
    """The float64 [batch,4,4] matrices of ``random_affine`` for volumes of the spatial ``shape`` (its docstring states the draw order
    and the composition).  Host work only."""
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"shape must be three positive extents, got {shape!r}")
    if not isinstance(seed, int) or seed < 0:
        raise ValueError(f"seed must be a non-negative integer, got {seed!r}")
    rot, sc, tr = _range3(rotate_range, "rotate_range"), _range3(scale_range, "scale_range"), _range3(translate_range, "translate_range")
    if (sc >= 1).any():
        raise ValueError(f"scale_range must stay below 1 (scales are drawn from U(1 - s, 1 + s)), got {scale_range!r}")
    rng = np.random.Generator(np.random.Philox(seed))
    angles = rng.uniform(-rot, rot, (batch, 3))
    scales = rng.uniform(1.0 - sc, 1.0 + sc, (batch, 3))
    shifts = rng.uniform(-tr, tr, (batch, 3))
    centre = (np.array(shape, np.float64) - 1.0) / 2.0
    out = np.zeros((batch, 4, 4))
    for b in range(batch):
        (cx, cy, cz), (sx, sy, sz) = np.cos(angles[b]), np.sin(angles[b])
        R = (np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]]) @ np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]]) @
             np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]]))
        M = R @ np.diag(scales[b])
        out[b, :3, :3], out[b, :3, 3], out[b, 3, 3] = M, (centre - M @ centre) + shifts[b], 1.0
    return out


def _spatial(images, masks, matrices, field, order, mask_order, cval):
    """One ``ops.warp`` launch per tensor under the same table and field; without a field it is ``ops.affine_transform``."""
    def one(t, o):
        if field is None:
            return ops.affine_transform(t, matrices, order=o, cval=cval)
        return ops.warp(t, field, matrices, order=o, cval=cval)
    return SpatialAugmented(one(images, order), None if masks is None else one(masks, mask_order), matrices, field)


def random_affine(images: torch.Tensor, masks: Optional[torch.Tensor] = None, *, seed: int, rotate_range=0.0, scale_range=0.0, translate_range=0.0,
                  order: int = 1, mask_order: int = 0, cval: float = 0.0) -> SpatialAugmented:
    """A random rotation, scale and translation per item of an NDHWC batch, the masks under the same matrix (``mask_order`` 0 keeps a
    binary mask binary), zeros (``cval``) outside.  Each range is a scalar or a 3-vector over the axes (d, h, w).

    The draw, on the host: ``rng = numpy.random.Generator(numpy.random.Philox(seed))``, then in this order
    ``angles = rng.uniform(-rotate_range, rotate_range, (B, 3))`` (radians, about the d, h and w axis),
    ``scales = rng.uniform(1 - scale_range, 1 + scale_range, (B, 3))`` and
    ``shifts = rng.uniform(-translate_range, translate_range, (B, 3))`` (voxels); all three are drawn whatever the ranges.

    The composition, in float64: ``R = Rd(a0) @ Rh(a1) @ Rw(a2)`` with Rd = [[1,0,0],[0,c,-s],[0,s,c]], Rh = [[c,0,s],[0,1,0],[-s,0,c]],
    Rw = [[c,-s,0],[s,c,0],[0,0,1]]; ``M = R @ diag(scales)``; the input coordinate of output voxel o is
    ``c = M (o - centre) + centre + shifts`` with centre = (n - 1) / 2 per axis, uploaded as the table (M, (centre - M centre) + shifts)
    of ``dm3d_affine_resample``.  Nothing is read back.  Returns ``SpatialAugmented(images, masks, matrices, None)``; all ranges 0 give
    identity matrices.  Per-item probabilities and anisotropic voxel spacing are not offered."""
    matrices = _image_mask_check(images, masks, lambda: affine_matrices(images.shape[1:4], images.shape[0], seed, rotate_range, scale_range, translate_range))
    return _spatial(images, masks, matrices, None, order, mask_order, cval)


def elastic_deform(images: torch.Tensor, masks: Optional[torch.Tensor] = None, *, alpha, sigma, seed: int, order: int = 1, mask_order: int = 0,
                   cval: float = 0.0) -> SpatialAugmented:
    """A random elastic deformation (Simard et al. 2003) per item of an NDHWC batch: one displacement field
    ``gaussian_filter(U(-1, 1), sigma, mode="constant") * alpha`` per item (``ops.elastic_field`` documents the Philox stream), images and
    masks resampled at ``o + field[:, o]`` by one ``ops.warp`` each.  ``alpha`` (voxels) and ``sigma`` are scalars or 3-vectors.  Returns
    ``SpatialAugmented(images, masks, None, field)``.  The field is drawn at full resolution: MONAI's coarse-grid-then-upsample field is
    not offered, nor are the other boundary modes of the warp."""
    _image_mask_check(images, masks, lambda: ops._field_arguments(alpha, sigma, seed))
    field = ops.elastic_field(images.shape[1:4], images.shape[0], alpha, sigma, seed, device=images.device)
    return _spatial(images, masks, None, field, order, mask_order, cval)


def spatial_augment(images: torch.Tensor, masks: Optional[torch.Tensor] = None, *, seed: int, rotate_range=0.0, scale_range=0.0, translate_range=0.0,
                    elastic_alpha=None, elastic_sigma=None, order: int = 1, mask_order: int = 0, cval: float = 0.0) -> SpatialAugmented:
    """``random_affine`` and ``elastic_deform`` composed: the input coordinate of output voxel o is ``(M o + offset) + field[:, o]``, the
    table of the one and the field of the other under the same ``seed``, in **one** ``dm3d_warp`` launch per tensor, so an image is
    interpolated once.  With ``elastic_alpha=None`` it is ``random_affine``; with all ranges 0 it is ``elastic_deform`` (the identity
    table adds nothing to a coordinate).  Returns ``SpatialAugmented(images, masks, matrices, field)``."""
    def host_arguments():
        if (elastic_alpha is None) != (elastic_sigma is None):
            raise ValueError("elastic_alpha and elastic_sigma must be given together or both left None")
        if elastic_alpha is not None:
            ops._field_arguments(elastic_alpha, elastic_sigma, seed)
        return affine_matrices(images.shape[1:4], images.shape[0], seed, rotate_range, scale_range, translate_range)

    matrices = _image_mask_check(images, masks, host_arguments)
    field = None if elastic_alpha is None else ops.elastic_field(images.shape[1:4], images.shape[0], elastic_alpha, elastic_sigma, seed, device=images.device)
    return _spatial(images, masks, matrices, field, order, mask_order, cval)


def clean_mask(mask: torch.Tensor, *, keep_largest: bool = True, fill_holes: bool = True, min_size: Optional[int] = None, connectivity: int = 6,
               threshold: float = 0.5) -> torch.Tensor:
    """A predicted or generated mask made fit for scoring, between a reconstruction and ``metrics.mask_metrics``: binarise the NDHWC
    float32 device tensor at ``threshold`` per volume and channel, drop the components below ``min_size`` voxels (when given), keep the
    largest component (``keep_largest``), fill the holes (``fill_holes``), in that order (``ops.component_filter``).  ``connectivity``
    (6, 18, 26) is the foreground's.  Returns float32 zeros and ones of the same shape; nothing is read back.  At least one step must
    be asked for."""
    return ops.component_filter(mask, threshold, connectivity=connectivity, keep="largest" if keep_largest else None, min_size=min_size,
                                fill_holes=fill_holes)
