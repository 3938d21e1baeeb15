"""Device-side volume preprocessing: the reference's ``dataset_utils.py`` between a loaded MRI volume and ``train_step`` / ``test_step``.

Every voxel is touched by HIP kernels only (``ops.affine_transform``, ``ops.volume_normalize``, ``ops.augment``); the 4 x 4 affines, voxel
sizes and shapes are host values in float64, as they are in the reference.  Volumes are float32 device tensors [B,D,H,W] or NDHWC (a
single [D,H,W] volume is taken as a batch of one and returned as one).  NIfTI reading is not offered: callers pass arrays, affines and
voxel sizes.  Between two resamples a volume is rounded to float32, where the reference carries float64."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops

__all__ = ["reslice", "transform_image", "normalize", "augment", "preprocess"]    # the preprocessing set, pinned by its host test; clean_mask is public beside it


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


def clean_mask(mask: torch.Tensor, *, keep_largest: bool = True, fill_holes: bool = True, min_size: Optional[int] = None, connectivity: int = 6,
               threshold: float = 0.5) -> torch.Tensor:
    """A predicted or generated mask made fit for scoring, between a reconstruction and ``metrics.mask_metrics``: binarise the NDHWC
    float32 device tensor at ``threshold`` per volume and channel, drop the components below ``min_size`` voxels (when given), keep the
    largest component (``keep_largest``), fill the holes (``fill_holes``), in that order (``ops.component_filter``).  ``connectivity``
    (6, 18, 26) is the foreground's.  Returns float32 zeros and ones of the same shape; nothing is read back.  At least one step must
    be asked for."""
    return ops.component_filter(mask, threshold, connectivity=connectivity, keep="largest" if keep_largest else None, min_size=min_size,
                                fill_holes=fill_holes)
