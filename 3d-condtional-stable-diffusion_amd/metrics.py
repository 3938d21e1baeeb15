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

__all__ = ["Mean", "NanMean", "component_stats", "connected_components", "dice", "distance_transform", "distribution_metrics", "encoder_features",
           "frechet_distance", "frechet_distance_from_moments", "hausdorff", "iou", "kid", "kid_subsets", "mask_metrics", "mask_overlap", "mmd2",
           "ms_ssim", "pair_stats", "pairwise_ms_ssim", "prdc", "psnr", "sample_diversity", "ssim", "surface_distances", "volume_metrics"]


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


# ---- does the generated set match the real set: Frechet distance, KID, precision / recall / density / coverage of feature vectors ------
# (include/dm3d.h, dm3d_dist_desc).  Features are [rows, D] float32 or float64 device tensors, one vector per sample; the default
# extractor is ``encoder_features``.  Not offered: Inception or Med3D features (no downloaded weights), MMD kernels other than KID's cubic
# one, anisotropic or non-Euclidean distances, and a device-side matrix square root (the Frechet tail runs on the host).
def frechet_distance_from_moments(mu1, sigma1, mu2, sigma2) -> torch.Tensor:
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2) of two Gaussians' moments, a 0-d float64 host tensor.  The trace term is the
    sum of the square roots of the eigenvalues of the symmetric form S1^(1/2) S2 S1^(1/2) (``torch.linalg.eigh`` / ``eigvalsh`` in
    float64 on the host; eigenvalues below 0, rounding of a rank-deficient covariance, are taken as 0).  Moments on a device are read
    back here: 2 D + 2 D^2 numbers, the one read-back of the distribution metrics.  Use it with a real set's cached moments."""
    mu1, sigma1, mu2, sigma2 = (torch.as_tensor(t).detach().to(device="cpu", dtype=torch.float64) for t in (mu1, sigma1, mu2, sigma2))
    dim = mu1.numel()
    if mu1.dim() != 1 or mu2.shape != mu1.shape or sigma1.shape != (dim, dim) or sigma2.shape != (dim, dim):
        raise ValueError(f"moments must be mu [D] and sigma [D, D] of one D, got {tuple(mu1.shape)}, {tuple(sigma1.shape)}, {tuple(mu2.shape)}, "
                         f"{tuple(sigma2.shape)}")
    w, v = torch.linalg.eigh(sigma1)
    root1 = (v * w.clamp(min=0.0).sqrt()) @ v.T
    form = root1 @ sigma2 @ root1
    ev = torch.linalg.eigvalsh((form + form.T) * 0.5)
    diff = mu1 - mu2
    return (diff * diff).sum() + torch.trace(sigma1) + torch.trace(sigma2) - 2.0 * ev.clamp(min=0.0).sqrt().sum()


def frechet_distance(real: torch.Tensor, fake: torch.Tensor) -> torch.Tensor:
    """The Frechet distance (the "F" of FID) between Gaussians fitted to the feature sets ``real`` [N, D] and ``fake`` [M, D]: a 0-d
    float64 host tensor.  Means and unbiased covariances come from the device (``ops.feature_moments``, bitwise repeatable); the tail is
    ``frechet_distance_from_moments``, which reads them back (2 D + 2 D^2 numbers): the one function here that synchronises."""
    real, fake = ops._feature_pair(real, fake)
    m1, m2 = ops.feature_moments(real), ops.feature_moments(fake)
    return frechet_distance_from_moments(m1.mean, m1.cov, m2.mean, m2.cov)


def _div(t: torch.Tensor, value) -> torch.Tensor:
    """``t / value`` as a correctly rounded float64 division: torch divides a device tensor by a Python number through the number's
    reciprocal, which moves the last bit, so the divisor goes to the device first."""
    return t / torch.full((), float(value), dtype=torch.float64, device=t.device)


def _mmd2(sums: torch.Tensor, n: int, m: int) -> torch.Tensor:
    """The unbiased MMD^2 of ``ops.poly_mmd``'s sums [S, 3]: (xx / (n (n - 1)) + yy / (m (m - 1))) - (2 xy) / (n m), float64 [S]."""
    return (_div(sums[:, 0], n * (n - 1)) + _div(sums[:, 1], m * (m - 1))) - _div(2.0 * sums[:, 2], n * m)


def mmd2(real: torch.Tensor, fake: torch.Tensor) -> torch.Tensor:
    """The unbiased squared maximum mean discrepancy of the whole sets under KID's kernel (a . b / D + 1)^3: a 0-d float64 device tensor
    (it can be slightly negative for matching sets).  Nothing is read back."""
    real, fake = ops._feature_pair(real, fake)
    return _mmd2(ops.poly_mmd(real, fake), real.shape[0], fake.shape[0])[0]


def kid_subsets(n_real: int, n_fake: int, num_subsets: int, subset_size: int, seed: int):
    """The row tables ``kid`` scores, int32 host tensors [num_subsets, m] each with m = min(subset_size, n_real, n_fake).  One
    ``torch.Generator().manual_seed(seed)`` on the host serves every draw; subset s takes the first m entries of
    ``torch.randperm(n_real, generator=g)`` and then of ``torch.randperm(n_fake, generator=g)``, s = 0, 1, .. in order."""
    if int(num_subsets) != num_subsets or num_subsets < 1:
        raise ValueError(f"num_subsets must be an integer of at least 1, got {num_subsets!r}")
    if int(subset_size) != subset_size or subset_size < 2:
        raise ValueError(f"subset_size must be an integer of at least 2, got {subset_size!r}")
    m = min(int(subset_size), n_real, n_fake)
    g = torch.Generator().manual_seed(int(seed))
    rows_real, rows_fake = [], []
    for _ in range(int(num_subsets)):
        rows_real.append(torch.randperm(n_real, generator=g)[:m])
        rows_fake.append(torch.randperm(n_fake, generator=g)[:m])
    return torch.stack(rows_real).to(torch.int32), torch.stack(rows_fake).to(torch.int32)


def kid(real: torch.Tensor, fake: torch.Tensor, num_subsets: int = 100, subset_size: int = 1000, seed: int = 0):
    """The kernel distance KID (Binkowski et al. 2018): ``(mean, std)`` of the unbiased MMD^2 over ``num_subsets`` subsets of
    ``min(subset_size, N, M)`` rows of each set, drawn without replacement as ``kid_subsets`` documents; two 0-d float64 device
    tensors.  All subsets go through one launch (``ops.poly_mmd``) and read the features in place.  Mean and variance over the subsets
    are sequential sums in subset order (``ops.feature_moments`` of the [S, 1] column); ``std`` is numpy's default, the population
    form sqrt(var * ((S - 1) / S)), and 0 for one subset.  Nothing is read back."""
    real, fake = ops._feature_pair(real, fake)
    rows_real, rows_fake = kid_subsets(real.shape[0], fake.shape[0], num_subsets, subset_size, seed)
    m = rows_real.shape[1]
    values = _mmd2(ops.poly_mmd(real, fake, rows_real, rows_fake), m, m)
    s = values.numel()
    if s == 1:
        return values[0], torch.zeros((), dtype=torch.float64, device=values.device)
    mom = ops.feature_moments(values.reshape(s, 1).contiguous())
    return mom.mean[0], (mom.cov[0, 0] * (float(s - 1) / float(s))).sqrt()


def _prdc(counts: ops.PrdcCounts, nearest_k: int) -> Dict[str, torch.Tensor]:
    n_fake, n_real = counts.count_fake.numel(), counts.near_real.numel()
    return {"precision": _div((counts.count_fake > 0).sum().double(), n_fake), "recall": _div(counts.near_real.sum().double(), n_real),
            "density": _div(counts.count_fake.sum().double(), nearest_k * n_fake), "coverage": _div(counts.cover_real.sum().double(), n_real)}


def _prdc_check(real, fake, nearest_k):
    ops._features_check(real, "real")
    ops._features_check(fake, "fake", real)
    if int(nearest_k) != nearest_k or not 1 <= nearest_k <= 16:
        raise ValueError(f"nearest_k must be an integer from 1 to 16, got {nearest_k!r}")
    if nearest_k >= min(real.shape[0], fake.shape[0]):
        raise ValueError(f"nearest_k={nearest_k} needs more than nearest_k rows in each set, got {real.shape[0]} and {fake.shape[0]}: lower "
                         "nearest_k or add samples")
    return ops._feature_pair(real, fake)


def prdc(real: torch.Tensor, fake: torch.Tensor, nearest_k: int = 5) -> Dict[str, torch.Tensor]:
    """Precision and recall (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020) of generated features ``fake`` [M, D]
    against real features ``real`` [N, D], as the ``prdc`` package defines them on squared Euclidean distances with each row's
    ``nearest_k``-th-neighbour ball: a dict of 0-d float64 device tensors, formed on the device from the integer outputs of
    ``ops.prdc_counts``.  Nothing is read back."""
    real, fake = _prdc_check(real, fake, nearest_k)
    counts = ops.prdc_counts(real, fake, ops.knn_radius(real, nearest_k), ops.knn_radius(fake, nearest_k))
    return _prdc(counts, int(nearest_k))


def distribution_metrics(real: torch.Tensor, fake: torch.Tensor, nearest_k: int = 5, num_subsets: int = 100, subset_size: int = 1000,
                         seed: int = 0) -> Dict[str, torch.Tensor]:
    """Every score above for one pair of feature sets: ``frechet_distance`` (0-d float64 on the host, the one value read back),
    ``kid_mean``, ``kid_std``, ``precision``, ``recall``, ``density``, ``coverage`` (0-d float64 on the device).  The features are
    widened once and each set's radii are computed once."""
    real, fake = _prdc_check(real, fake, nearest_k)
    out = prdc(real, fake, nearest_k)
    kid_mean, kid_std = kid(real, fake, num_subsets, subset_size, seed)
    return {"frechet_distance": frechet_distance(real, fake), "kid_mean": kid_mean, "kid_std": kid_std, **out}


def encoder_features(vqvae, volumes, pool: str = "mean", batch_size: int = 8) -> torch.Tensor:
    """The default features of the scores above: the autoencoder's pre-quantisation encoder output (``vqvae._encode``, a ``VQVAE`` or
    ``VQGAN`` bracket: the latents the diffusion model is trained on) pooled over D, H, W per channel, in float64.  ``volumes`` is
    float32 [n, S, S, S, C] (NDHWC, host or device), encoded ``batch_size`` at a time.  ``pool="mean"`` gives [n, C]; ``"mean_std"``
    gives [n, 2 C], the means followed by the population standard deviations.  A float64 device tensor; nothing is read back."""
    if pool not in ("mean", "mean_std"):
        raise ValueError(f'pool must be "mean" or "mean_std", got {pool!r}')
    if int(batch_size) != batch_size or batch_size < 1:
        raise ValueError(f"batch_size must be an integer of at least 1, got {batch_size!r}")
    volumes = torch.as_tensor(volumes)
    if volumes.dim() != 5 or volumes.shape[0] < 1:
        raise ValueError(f"volumes must be [n, D, H, W, C] with n >= 1, got {tuple(volumes.shape)}")
    rows = []
    for at in range(0, volumes.shape[0], int(batch_size)):
        z = vqvae._encode(volumes[at:at + int(batch_size)]).double()
        z = z.reshape(z.shape[0], -1, z.shape[-1])
        mean = z.mean(dim=1)
        rows.append(mean if pool == "mean" else torch.cat([mean, z.std(dim=1, unbiased=False)], dim=1))
    return torch.cat(rows).contiguous()


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
