"""Fitting a VQ codebook on the device: the reference's ``VectorQuantizerEMA`` (networks/emavqvae.py:170-232) with the usage counter
and the dead-code replacement of its ``NSVQ`` (networks/nsvqvae.py:140, 186, 193-230).

Every step is a dm3d HIP kernel (no fallback): nearest-code assignment and lookup through ``ops.vq_assign`` / ``ops.gather_rows`` (the
kernels inference uses, so the codes that are fitted are the codes inference picks), per-code counts and float64 member sums through
``ops.code_stats``, the moving-average update through ``ops.codebook_ema``, perplexity through ``ops.code_usage`` and replacement
through ``ops.codebook_replace``.  Nothing synchronises and nothing is read back; sums run in a fixed order with no floating-point
atomic, so a fit repeats bitwise.

Not offered: NSVQ's noise-substitution forward, gradient training of an encoder or decoder (``quantized`` is the forward value, there
is no straight-through graph), Laplace smoothing of the cluster sizes, k-means initialisation, more than 4096 codes.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import _lib, ops

USAGE_EPS = 1e-10       # inside the log of the perplexity, as VQVAE._quantize; VectorQuantizerEMA reads a self.eps it never defines
NOISE_SCALE = 1e-12     # NSVQ.eps (:123): the scale of the noise a replaced code gets


class EMACodebook:
    """``VectorQuantizerEMA(num_embeddings, embedding_dim, commitment_cost, decay, epsilon)`` on the device.  The codebook is held as
    [K, D] float32 (rows are codes); ``state_dict`` speaks the reference's shapes: ``embeddings`` [D, K], ``ema_cluster_size`` [K],
    ``ema_w`` [D, K].  Keras' 'uniform' initialiser draws embeddings and ema_w from U(-0.05, 0.05); here both come from ``seed``."""

    def __init__(self, num_embeddings=512, embedding_dim=128, commitment_cost=6, decay=0.99, epsilon=1e-5, *, discarding_threshold=0.01,
                 device="cuda", seed=0):
        if not 1 <= num_embeddings <= _lib.CODEBOOK_MAX_K:
            raise ValueError(f"num_embeddings={num_embeddings}; 1 to {_lib.CODEBOOK_MAX_K} are taken")
        if not 4 <= embedding_dim <= _lib.CODEBOOK_MAX_DIM or embedding_dim % 4:
            raise ValueError(f"embedding_dim={embedding_dim}; a multiple of 4 from 4 to {_lib.CODEBOOK_MAX_DIM} is taken")
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"decay must lie in [0, 1], got {decay!r}")
        if not epsilon >= 0:
            raise ValueError(f"epsilon must be at least 0, got {epsilon!r}")
        self.num_embeddings, self.embedding_dim, self.commitment_cost = int(num_embeddings), int(embedding_dim), commitment_cost
        self.decay, self.epsilon, self.discarding_threshold = float(decay), float(epsilon), float(discarding_threshold)
        self.device, self.seed = torch.device(device), int(seed)
        self._replacements = 0
        rng = np.random.default_rng(seed)
        shape = (self.embedding_dim, self.num_embeddings)
        self.load_state_dict({"embeddings": rng.uniform(-0.05, 0.05, shape).astype(np.float32),
                              "ema_cluster_size": np.zeros(self.num_embeddings, np.float32),
                              "ema_w": rng.uniform(-0.05, 0.05, shape).astype(np.float32)})

    # ---- state -------------------------------------------------------------------------------------------------------
    def load_state_dict(self, sd) -> None:
        k, dim = self.num_embeddings, self.embedding_dim
        host = {}
        for name, shape in (("embeddings", (dim, k)), ("ema_cluster_size", (k,)), ("ema_w", (dim, k))):
            if name not in sd:
                raise ValueError(f"missing {name}")
            arr = sd[name]
            if isinstance(arr, torch.Tensor):
                arr = arr.detach().cpu().numpy()
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            if arr.shape != shape:
                raise ValueError(f"{name}: expected shape {shape}, got {arr.shape}")
            host[name] = arr
        _lib.require_device()
        emb = host["embeddings"]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.codebook_t = up(emb.T)                                                # [K, D]
        self.esq = up((emb ** 2).sum(axis=0, dtype=np.float32))                    # what VQVAE.prepare computes
        self.cluster_size = up(host["ema_cluster_size"])
        self.ema_w_t = up(host["ema_w"].T)
        used = sd.get("codebooks_used")
        if isinstance(used, torch.Tensor):
            used = used.detach().cpu().numpy()
        self._used = torch.zeros(k, dtype=torch.int32, device=self.device) if used is None else up(np.asarray(used, np.int32).reshape(k))

    def state_dict(self) -> Dict[str, np.ndarray]:
        """The reference's variables as numpy arrays (one read-back): ``embeddings`` [D, K], ``ema_cluster_size`` [K], ``ema_w`` [D, K],
        and ``codebooks_used`` [K] int32.  ``np.savez`` / ``np.load`` round-trip them bitwise."""
        return {"embeddings": np.ascontiguousarray(self.codebook_t.cpu().numpy().T), "ema_cluster_size": self.cluster_size.cpu().numpy(),
                "ema_w": np.ascontiguousarray(self.ema_w_t.cpu().numpy().T), "codebooks_used": self._used.cpu().numpy()}

    @property
    def codebooks_used(self) -> torch.Tensor:
        """int32 [K] on the device: how many rows each code has taken since the last replacement (NSVQ.codebooks_used)."""
        return self._used

    # ---- forward -------------------------------------------------------------------------------------------------------
    def __call__(self, inputs, training=True):
        """``VectorQuantizerEMA.call``: ``(loss, quantized, encoding_indices, perplexity)`` for float32 device ``inputs`` [..., D].
        ``quantized`` has the shape of ``inputs`` and holds the codes as they were when the rows were assigned, ``encoding_indices``
        (int32) the shape without the last axis; ``loss`` = commitment_cost * mean((quantized - inputs)^2) and ``perplexity`` are 0-d
        float64 device tensors.  ``training=True`` then moves the codes (counts, sums, EMA update) and adds the counts to
        ``codebooks_used``; ``training=False`` changes no state."""
        k, dim = self.num_embeddings, self.embedding_dim
        if not isinstance(inputs, torch.Tensor) or inputs.dtype != torch.float32 or inputs.dim() < 2 or inputs.shape[-1] != dim:
            raise ValueError(f"inputs must be a float32 tensor [..., {dim}], got {getattr(inputs, 'dtype', type(inputs).__name__)} "
                             f"{list(getattr(inputs, 'shape', ()))}")
        if not inputs.is_cuda:
            raise ValueError("inputs must be a device tensor: the codebook kernels have no CPU path")
        z = inputs.contiguous()
        flat = z.reshape(-1, dim)
        rows = flat.shape[0]
        idx = ops.vq_assign(flat, self.codebook_t, self.esq)
        q = ops.gather_rows(self.codebook_t, idx)
        b = z.shape[0]
        sse = ops.pair_stats(q.reshape(b, 1, 1, -1, 1), z.reshape(b, 1, 1, -1, 1)).sse
        loss = self.commitment_cost * (sse.sum() / z.numel())
        stats = ops.code_stats(flat, idx, k)
        usage = ops.code_usage(stats.counts, rows, USAGE_EPS, used_accum=self._used if training else None)
        if training:
            ops.codebook_ema(self.codebook_t, self.esq, self.cluster_size, self.ema_w_t, stats.counts, stats.sums, self.decay, self.epsilon)
        self.last_stats, self.last_usage = stats, usage
        return loss, q.reshape(z.shape), idx.reshape(z.shape[:-1]), usage.perplexity

    def replace_unused_codebooks(self, num_batches, noise_scale=NOISE_SCALE) -> ops.Replaced:
        """``NSVQ.replace_unused_codebooks(num_batches)``: codes with ``codebooks_used / num_batches < discarding_threshold`` take a
        used code's row (and its EMA state) plus noise; ``codebooks_used`` is zeroed.  Returns the device counts of used and unused codes."""
        out = ops.codebook_replace(self.codebook_t, self.esq, self._used, num_batches, self.discarding_threshold, seed=self.seed,
                                   draw=self._replacements, noise_scale=noise_scale, cluster_size=self.cluster_size, ema_w=self.ema_w_t)
        self._replacements += 1
        return out
