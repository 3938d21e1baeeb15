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
from .ops import ms_ssim, pair_stats, psnr, ssim

__all__ = ["Mean", "ms_ssim", "pair_stats", "pairwise_ms_ssim", "psnr", "sample_diversity", "ssim", "volume_metrics"]


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
