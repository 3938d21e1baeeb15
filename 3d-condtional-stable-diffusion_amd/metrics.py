"""Reconstruction metrics of the autoencoders (reference ``VQVAE.test_step``, vqvae3d_monai.py:504-544, and ``VQGAN.test_step``,
vqgan.py:821-919): SSIM and PSNR per depth slice as ``tf.image.ssim`` / ``tf.image.psnr`` compute them on a volume, the squared error
behind ``reconst_loss``, and the running mean Keras keeps of each.

Everything runs on the dm3d HIP kernels (``ops.pair_stats``, ``ops.ssim``, ``ops.psnr``; include/dm3d.h, dm3d_metric_desc) and stays on
the device: nothing here reads a value back, so a loop over batches synchronises once, when its caller asks for Python numbers.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import ops
from .ops import connected_components, distance_transform, mask_overlap, ms_ssim, pair_stats, psnr, ssim, surface_distances

__all__ = ["Mean", "NanMean", "component_stats", "connected_components", "dice", "distance_transform", "hausdorff", "iou", "mask_metrics", "mask_overlap", "ms_ssim", "pair_stats",
           "pairwise_ms_ssim", "psnr", "sample_diversity", "ssim", "surface_distances", "volume_metrics"]


def volume_metrics(x: torch.Tensor, y: torch.Tensor, max_val=None, *, x_channels=None, y_channels=None) -> Dict[str, torch.Tensor]:
    """Truth ``x`` against reconstruction ``y`` (NDHWC float32; ``*_channels = (first, count)`` reads a channel window in place) in three
    launches that share one pass over the pair.  Per volume ``y_min``, ``y_max``, ``max_val`` [B]; per depth slice ``sse`` (float64),
    ``mse``, ``ssim``, ``psnr`` [B, D]; ``max_val=None`` is the reference's max(y) - min(y) per volume."""
    stats = pair_stats(x, y, x_channels=x_channels, y_channels=y_channels)
    kw = dict(x_channels=x_channels, y_channels=y_channels, stats=stats)
    nc = x.shape[4] if x_channels is None else x_channels[1]
    mv = ops._max_val(max_val, stats, x, y, x_channels, y_channels)
    return {"y_min": stats.y_min, "y_max": stats.y_max, "max_val": mv,
            "sse": stats.sse, "mse": stats.sse / float(x.shape[2] * x.shape[3] * nc),
            "ssim": ssim(x, y, mv, **kw), "psnr": psnr(x, y, mv, **kw)}


def pairwise_ms_ssim(volumes: torch.Tensor, max_val, **kw) -> torch.Tensor:
    """3-D multi-scale SSIM (``ops.ms_ssim``; ``kw`` goes to it) of every pair i < j of ``volumes`` [B, D, H, W, C], B >= 2: float32
    [B (B - 1) / 2] in lexicographic order (0, 1), (0, 2), .., (B - 2, B - 1).  The volumes are read in place through a pair table, in
    one launch sequence.  ``max_val`` is a number or a tensor of one value per pair; there is no truth whose range could stand in."""
    if max_val is None:
        raise ValueError("pairwise_ms_ssim needs max_val: a generated batch has no truth whose range could stand in")
    if not isinstance(volumes, torch.Tensor) or volumes.dim() != 5 or volumes.shape[0] < 2:
        raise ValueError(f"volumes must be [B, D, H, W, C] with B >= 2, got {tuple(getattr(volumes, 'shape', ()))}")
    n = volumes.shape[0]
    pairs = torch.triu_indices(n, n, 1, device=volumes.device).t().contiguous()
    return ms_ssim(volumes, volumes, max_val, pairs=pairs, **kw)


def sample_diversity(volumes: torch.Tensor, max_val, **kw) -> torch.Tensor:
    """The diversity score of a generated batch: the mean of ``pairwise_ms_ssim`` as a 0-d float64 device tensor (lower is more diverse)."""
    return pairwise_ms_ssim(volumes, max_val, **kw).double().mean()


# ---- the mask channels: Dice, IoU, Hausdorff, ASSD of binarised masks (MONAI's definitions; include/dm3d.h, dm3d_mask_desc) ------------
def _dice_iou(counts: ops.MaskOverlap):
    """float64 Dice = 2 |X and Y| / (|X| + |Y|) and IoU = |X and Y| / |X or Y| from the exact counts; NaN where the truth mask is empty
    (MONAI's ``ignore_empty=True``)."""
    x, y, both = counts.x.double(), counts.y.double(), counts.both.double()
    nan = torch.full_like(x, float("nan"))
    return torch.where(counts.x > 0, 2.0 * both / (x + y), nan), torch.where(counts.x > 0, both / (x + y - both), nan)


def dice(x: torch.Tensor, y: torch.Tensor, threshold: float = 0.5, *, x_channels=None, y_channels=None) -> torch.Tensor:
    """Dice of the masks ``x > threshold`` (the truth) and ``y > threshold`` per volume and compared channel: float64 [B, nc], NaN where
    the truth mask is empty.  NDHWC float32 device tensors, ``*_channels = (first, count)`` read in place (``ops.mask_overlap``)."""
    return _dice_iou(mask_overlap(x, y, threshold, x_channels=x_channels, y_channels=y_channels))[0]


def iou(x: torch.Tensor, y: torch.Tensor, threshold: float = 0.5, *, x_channels=None, y_channels=None) -> torch.Tensor:
    """Intersection over union of the two masks, as ``dice``: float64 [B, nc], NaN where the truth mask is empty."""
    return _dice_iou(mask_overlap(x, y, threshold, x_channels=x_channels, y_channels=y_channels))[1]


def hausdorff(x: torch.Tensor, y: torch.Tensor, threshold: float = 0.5, percentile: Optional[float] = 95.0, *, x_channels=None,
              y_channels=None) -> torch.Tensor:
    """The Hausdorff distance of the two masks' surfaces per volume and compared channel, float64 [B, nc] in voxels (anisotropic spacing
    is not offered: the caller scales): the larger of the two directed ``percentile``-th percentiles (numpy's linear rule), or with
    ``percentile=None`` the plain maximum.  NaN where either mask is empty (``ops.surface_distances``)."""
    dist = surface_distances(x, y, threshold, 100.0 if percentile is None else percentile, x_channels=x_channels, y_channels=y_channels)
    return dist.hd if percentile is None else dist.hd_percentile


def mask_metrics(x: torch.Tensor, y: torch.Tensor, threshold: float = 0.5, percentile: float = 95.0, *, x_channels=None,
                 y_channels=None) -> Dict[str, torch.Tensor]:
    """Everything above from one launch sequence (the overlap pass of ``ops.surface_distances`` also leaves the counts): float64 [B, nc]
    ``dice``, ``iou``, ``hd``, ``hd_percentile``, ``assd``, ``surface_x``, ``surface_y`` and the int64 ``counts`` (``ops.MaskOverlap``).
    Distances are in voxels."""
    dist, counts = ops._surface_distances(x, y, threshold, percentile, x_channels, y_channels, True)
    d, i = _dice_iou(counts)
    return {"dice": d, "iou": i, **dist._asdict(), "counts": counts}


def component_stats(x: torch.Tensor, threshold: float = 0.5, *, channels=None, connectivity: int = 6) -> Dict[str, torch.Tensor]:
    """How many blobs the masks ``x > threshold`` fall into (``ops.connected_components``; ``connectivity`` 6, 18 or 26): ``components``
    int32 [B, nc] and ``largest_fraction`` float64 [B, nc], the share of the mask's voxels its largest component holds (1 for one blob,
    NaN for an empty mask).  Nothing is read back."""
    comp = connected_components(x, threshold, channels=channels, connectivity=connectivity)
    total = (comp.labels > 0).sum(dim=(1, 2, 3)).double()
    nan = torch.full_like(total, float("nan"))
    return {"components": comp.count, "largest_fraction": torch.where(total > 0, comp.largest[..., 1].double() / total.clamp(min=1.0), nan)}


class Mean:
    """``keras.metrics.Mean``: the mean of every element it was shown, so an update with a [B, D] tensor counts B*D values.  The float64
    sum and the count live on the device of the values: ``update_state`` enqueues two additions and never synchronises; ``result()`` is
    a 0-d float64 tensor there (0 before any update, as Keras' divide_no_nan gives)."""

    def __init__(self, name: str = "mean"):
        self.name = name
        self.reset_state()

    def reset_state(self) -> None:
        self.total: Optional[torch.Tensor] = None
        self.count: Optional[torch.Tensor] = None

    def update_state(self, values) -> None:
        v = torch.as_tensor(values)
        if self.total is None:
            self.total = torch.zeros((), dtype=torch.float64, device=v.device)
            self.count = torch.zeros((), dtype=torch.int64, device=v.device)
        self.total += v.to(device=self.total.device, dtype=torch.float64).sum()
        self.count += v.numel()

    def result(self) -> torch.Tensor:
        if self.total is None:
            return torch.zeros((), dtype=torch.float64)
        return torch.where(self.count > 0, self.total / self.count.clamp(min=1), torch.zeros_like(self.total))


class NanMean(Mean):
    """``Mean`` over the values that are not NaN (a Dice whose truth mask is empty, a Hausdorff distance of an empty surface): they add
    nothing to the sum or the count.  0 before any value that counts, as ``Mean``."""

    def update_state(self, values) -> None:
        v = torch.as_tensor(values)
        if self.total is None:
            self.total = torch.zeros((), dtype=torch.float64, device=v.device)
            self.count = torch.zeros((), dtype=torch.int64, device=v.device)
        v = v.to(device=self.total.device, dtype=torch.float64)
        keep = ~torch.isnan(v)
        self.total += torch.where(keep, v, torch.zeros_like(v)).sum()
        self.count += keep.sum()
