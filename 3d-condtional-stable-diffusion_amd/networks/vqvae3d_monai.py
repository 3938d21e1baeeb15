"""Drop-in for the inference side of the reference's ``networks/vqvae3d_monai.py`` — the autoencoder that brackets the
diffusion sampler (``DiffusionModel.encoder / quantizer / decoder``, conditional_dm3d.py:425-460, 478, 42).

Same constructor signature as the reference ``VQVAE`` (:394-406) and the same three callables:
``vq.encoder(x) -> latents``, ``vq.quantizer(z) -> (quantized, perplexity)``, ``vq.decoder(z) -> image``, all NDHWC float32
device tensors.  Every layer runs on the dm3d HIP kernels (no fallback):

  Conv3D k4/s2 + ReLU (Encoder :266-285)            -> dm3d_conv3d_ndhwc(ksize 4, stride 2, relu)
  VQVAEResidualUnit (:218-234)                      -> conv k3 + ReLU ; conv k3 with the inference BatchNormalization folded
                                                       into its weights, PReLU slope, + x, ReLU — two launches
  Conv3D k3 + PReLU (:296-301, 346-350)             -> conv k3 with the PReLU epilogue
  Conv3DTranspose k4/s2 [+ ReLU] (:373-381)         -> 8 parity 2x2x2 convs on the input grid (dm3d_pack_weights_convt)
  VectorQuantizer.get_code_indices + lookup (:140-177) -> float32 GEMM z.E, dm3d_vq_assign, dm3d_gather_rows

Keras' ``PReLU()`` has a full-shape slope ``[D,H,W,C]``, which ties the reference model to 128^3 inputs; here the spatial size
is the keyword ``input_size`` (default 128).  Gradient training (``train_step``) is out of scope; the codebook of the frozen
autoencoder can be fitted and inspected on the device (``fit_codebook``, ``codebook_usage``; ``dm3d_amd.codebook``); evaluation is here:
``test_step`` / ``evaluate`` report ``reconst_loss``, ``quantize_loss``, ``ssim`` and ``psnr`` as the reference's ``test_step`` (:504-544)
does, through the fused metric kernels (``dm3d_amd.metrics``).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .. import _lib, ops
from ..metrics import Mean, NanMean
from ..metrics import mask_metrics as mask_metrics_of

BN_EPS = 1e-3
VQ_BETA = 0.25          # VectorQuantizer(beta=0.25) (:113): the weight of the commitment term in its loss


def vqvae_param_spec(in_channels, out_channels, num_channels, num_res_layers, num_res_channels, num_embeddings,
                     embedding_dim, input_size) -> Dict[str, tuple]:
    """Weight inventory in layer-creation order (Encoder, codebook, Decoder), Keras shapes."""
    spec: Dict[str, tuple] = {}

    def res_unit(name, ch, rc, e):
        spec[f"{name}.conv1.kernel"] = (3, 3, 3, ch, rc)
        spec[f"{name}.conv1.bias"] = (rc,)
        spec[f"{name}.conv2.kernel"] = (3, 3, 3, rc, ch)
        spec[f"{name}.conv2.bias"] = (ch,)
        for s in ("gamma", "beta", "mean", "var"):
            spec[f"{name}.bn.{s}"] = (ch,)
        spec[f"{name}.prelu.alpha"] = (e, e, e, ch)

    ch_in, edge = in_channels, input_size
    for i, ch in enumerate(num_channels):
        edge //= 2
        spec[f"enc.down{i}.kernel"] = (4, 4, 4, ch_in, ch)
        spec[f"enc.down{i}.bias"] = (ch,)
        for j in range(num_res_layers):
            res_unit(f"enc.l{i}.res{j}", ch, num_res_channels[i], edge)
        ch_in = ch
    spec["enc.out.kernel"] = (3, 3, 3, ch_in, embedding_dim)
    spec["enc.out.bias"] = (embedding_dim,)
    spec["enc.out_prelu.alpha"] = (edge, edge, edge, embedding_dim)
    spec["vq.embeddings"] = (embedding_dim, num_embeddings)
    rev, rrev = list(reversed(num_channels)), list(reversed(num_res_channels))
    spec["dec.in.kernel"] = (3, 3, 3, embedding_dim, rev[0])
    spec["dec.in.bias"] = (rev[0],)
    spec["dec.in_prelu.alpha"] = (edge, edge, edge, rev[0])
    for i, ch in enumerate(rev):
        for j in range(num_res_layers):
            res_unit(f"dec.l{i}.res{j}", ch, rrev[i], edge)
        out = out_channels if i == len(rev) - 1 else rev[i + 1]
        spec[f"dec.up{i}.kernel"] = (4, 4, 4, out, ch)
        spec[f"dec.up{i}.bias"] = (out,)
        edge *= 2
    return spec


def keras_init_vqvae_weights(spec: Dict[str, tuple], seed: int = 0) -> Dict[str, np.ndarray]:
    """What Keras creates: glorot-uniform kernels, zero biases, BN identity, PReLU slope 0, HeUniform codebook (:125-131)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in spec.items():
        if name.endswith(".kernel"):
            rf = int(np.prod(shape[:3]))
            lim = math.sqrt(6.0 / (shape[3] * rf + shape[4] * rf))
            out[name] = rng.uniform(-lim, lim, size=shape).astype(np.float32)
        elif name.endswith(".embeddings"):
            lim = math.sqrt(6.0 / shape[0])
            out[name] = rng.uniform(-lim, lim, size=shape).astype(np.float32)
        elif name.endswith((".gamma", ".var")):
            out[name] = np.ones(shape, np.float32)
        else:
            out[name] = np.zeros(shape, np.float32)
    return out


class _Layer:
    __slots__ = ("wpk", "w_exp", "bias", "cout", "alpha")


class VQVAE:
    METRIC_KEYS = ("loss", "reconst_loss", "quantize_loss", "ssim", "psnr")      # what test_step returns, in the reference's order
    MASK_METRIC_KEYS = ("mask_dice", "mask_iou", "mask_hd95", "mask_assd")       # what mask_test_step adds: the mask half, not in the reference

    def __init__(self, in_channels, out_channels, num_channels, num_res_layers, num_res_channels,
                 downsample_parameters=((2, 4, 1, 1), (2, 4, 1, 1), (2, 4, 1, 1)),
                 upsample_parameters=((2, 4, 1, 1, 0), (2, 4, 1, 1, 0), (2, 4, 1, 1, 0)),
                 num_embeddings=128, embedding_dim=64, dropout=0.1, act="relu", output_act=None, num_gpus=2,
                 kernel_resize=False, *, input_size=128, device="cuda", weights=None, seed=0, precision=None):
        import os
        for p in tuple(downsample_parameters)[:len(num_channels)]:
            if tuple(p[:3]) != (2, 4, 1) or p[3] not in ("same", 1):
                raise ValueError("only (stride 2, kernel 4, dilation 1, 'same') downsampling is implemented (the reference's setting)")
        for p in tuple(upsample_parameters)[:len(num_channels)]:
            if tuple(p[:3]) != (2, 4, 1) or p[3] not in ("same", 1):
                raise ValueError("only (stride 2, kernel 4, dilation 1, 'same') upsampling is implemented (the reference's setting)")
        if input_size % (1 << len(num_channels)):
            raise ValueError("input_size must be divisible by 2**levels")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.num_channels, self.num_res_channels = tuple(num_channels), tuple(num_res_channels)
        self.num_res_layers, self.num_embeddings, self.embedding_dim = num_res_layers, num_embeddings, embedding_dim
        self.output_act, self.num_gpus, self.input_size = output_act, num_gpus, input_size
        self.device = torch.device(device)
        self.precision = precision or os.environ.get("DM3D_PRECISION", "h3")
        if self.precision not in ("fp32", "h3"):
            raise ValueError("precision must be 'fp32' or 'h3'")
        self.spec = vqvae_param_spec(in_channels, out_channels, self.num_channels, num_res_layers, self.num_res_channels,
                                     num_embeddings, embedding_dim, input_size)
        self.state: Dict[str, np.ndarray] = {}
        self._prepared = False
        self.load_state_dict(weights if weights is not None else keras_init_vqvae_weights(self.spec, seed))
        self.encoder, self.quantizer, self.decoder = self._encode, self._quantize, self._decode
        self._last_pair = None
        self._trackers = {k: Mean(k) for k in self.METRIC_KEYS}
        self._mask_trackers = {k: NanMean(k) for k in self.MASK_METRIC_KEYS}

    # ---- weights ---------------------------------------------------------------------------------------------------
    def load_state_dict(self, sd, strict=True):
        new = {}
        for name, shape in self.spec.items():
            if name not in sd:
                if strict:
                    raise ValueError(f"missing weight {name}")
                new[name] = self.state[name]
                continue
            arr = sd[name]
            if isinstance(arr, torch.Tensor):
                arr = arr.detach().cpu().numpy()
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            if tuple(arr.shape) != tuple(shape):
                raise ValueError(f"weight {name}: expected shape {tuple(shape)}, got {tuple(arr.shape)}")
            new[name] = arr
        self.state, self._prepared = new, False

    def load_weights(self, path, root=()):
        """keras ``model.load_weights`` (conditional_dm3d.py:451-454): a TF2 checkpoint prefix written by the reference's
        ``save_weights`` (tf_checkpoint.load_vqvae_state; ``root`` = attribute path of the autoencoder inside the saved object),
        or an .npz of the state dict."""
        if str(path).endswith(".npz"):
            self.load_state_dict(dict(np.load(path)))
            return
        from ..tf_checkpoint import load_vqvae_state
        self.load_state_dict(load_vqvae_state(str(path), self.spec, root=tuple(root)))

    def save_weights(self, path, root=()):
        if str(path).endswith(".npz"):
            np.savez(path, **self.state)
            return
        from ..tf_checkpoint import save_vqvae_checkpoint
        save_vqvae_checkpoint(str(path), self.state, self.spec, root=tuple(root))

    def _dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)

    def _layer(self, kernel, bias, kind="conv", alpha=None) -> _Layer:
        L = _Layer()
        h3 = self.precision == "h3"
        k = self._dev(kernel)
        if kind == "convt":
            r = ops.pack_weights_convt(k, h3=h3)
            L.cout = kernel.shape[3]
        else:
            r = ops.pack_weights_h3(k) if h3 else ops.pack_weights(k)
            L.cout = kernel.shape[4]
        L.wpk, L.w_exp = (r if h3 else (r, 0))
        L.bias = self._dev(bias)
        L.alpha = self._dev(alpha) if alpha is not None else None
        return L

    def _res_unit(self, name):
        s = self.state
        c1 = self._layer(s[f"{name}.conv1.kernel"], s[f"{name}.conv1.bias"])
        # inference BatchNormalization after conv2 folds into its weights: W' = W*scale[co], b' = b*scale + shift
        scale = s[f"{name}.bn.gamma"].astype(np.float64) / np.sqrt(s[f"{name}.bn.var"].astype(np.float64) + BN_EPS)
        shift = s[f"{name}.bn.beta"].astype(np.float64) - s[f"{name}.bn.mean"].astype(np.float64) * scale
        w2 = (s[f"{name}.conv2.kernel"].astype(np.float64) * scale).astype(np.float32)
        b2 = (s[f"{name}.conv2.bias"].astype(np.float64) * scale + shift).astype(np.float32)
        c2 = self._layer(w2, b2, alpha=s[f"{name}.prelu.alpha"])
        return c1, c2

    def prepare(self):
        if self._prepared:
            return
        _lib.require_device()
        s, P = self.state, {}
        n = len(self.num_channels)
        for i in range(n):
            P[f"enc.down{i}"] = self._layer(s[f"enc.down{i}.kernel"], s[f"enc.down{i}.bias"])
            for j in range(self.num_res_layers):
                P[f"enc.l{i}.res{j}"] = self._res_unit(f"enc.l{i}.res{j}")
        P["enc.out"] = self._layer(s["enc.out.kernel"], s["enc.out.bias"], alpha=s["enc.out_prelu.alpha"])
        emb = s["vq.embeddings"]
        P["vq.codebook_t"] = self._dev(np.ascontiguousarray(emb.T))                    # [K, D]: rows = codes
        P["vq.esq"] = self._dev((emb.astype(np.float32) ** 2).sum(axis=0, dtype=np.float32))
        P["dec.in"] = self._layer(s["dec.in.kernel"], s["dec.in.bias"], alpha=s["dec.in_prelu.alpha"])
        for i in range(n):
            for j in range(self.num_res_layers):
                P[f"dec.l{i}.res{j}"] = self._res_unit(f"dec.l{i}.res{j}")
            P[f"dec.up{i}"] = self._layer(s[f"dec.up{i}.kernel"], s[f"dec.up{i}.bias"], kind="convt")
        self.P, self._prepared = P, True

    # ---- forward pieces --------------------------------------------------------------------------------------------
    def _conv(self, L: _Layer, x, ksize, **kw):
        prec = _lib.PREC_H3 if self.precision == "h3" else _lib.PREC_F32
        return ops.conv3d(x, L.wpk, L.cout, ksize, bias=L.bias, precision=prec, w_exp=L.w_exp, **kw)

    def _run_res_unit(self, name, x):
        c1, c2 = self.P[name]
        h = self._conv(c1, x, 3, relu=True)
        return self._conv(c2, h, 3, prelu_alpha=c2.alpha, res=x, relu_out=True)

    def _check(self, x, edge, ch, what):
        x = torch.as_tensor(x)
        if x.dim() != 5 or tuple(x.shape[1:]) != (edge, edge, edge, ch) or x.dtype != torch.float32:
            raise ValueError(f"{what} must be float32 [B,{edge},{edge},{edge},{ch}] (NDHWC), got {tuple(x.shape)} {x.dtype}")
        return x.to(self.device).contiguous()

    def _encode(self, x):
        """Encoder.call (:303-305)."""
        self.prepare()
        h = self._check(x, self.input_size, self.in_channels, "encoder input")
        if self.in_channels % 4:                     # the conv kernels read 4 channels per load: zero-pad the input channels
            pad = 4 - self.in_channels % 4
            h = torch.cat([h, torch.zeros(*h.shape[:4], pad, device=self.device)], dim=-1).contiguous()
        for i in range(len(self.num_channels)):
            L = self.P[f"enc.down{i}"]
            if i == 0 and self.in_channels % 4:
                L = self._padded_first_conv()
            h = self._conv(L, h, 4, stride=2, relu=True)
            for j in range(self.num_res_layers):
                h = self._run_res_unit(f"enc.l{i}.res{j}", h)
        L = self.P["enc.out"]
        return self._conv(L, h, 3, prelu_alpha=L.alpha)

    def _padded_first_conv(self):
        if "enc.down0.padded" not in self.P:
            k = self.state["enc.down0.kernel"]
            pad = 4 - self.in_channels % 4
            kp = np.concatenate([k, np.zeros(k.shape[:3] + (pad, k.shape[4]), np.float32)], axis=3)
            self.P["enc.down0.padded"] = self._layer(kp, self.state["enc.down0.bias"])
        return self.P["enc.down0.padded"]

    def get_code_indices(self, flattened_inputs):
        """VectorQuantizer.get_code_indices (:164-177)."""
        self.prepare()
        z = torch.as_tensor(flattened_inputs, dtype=torch.float32).to(self.device).contiguous()
        return ops.vq_assign(z, self.P["vq.codebook_t"], self.P["vq.esq"])

    def _quantize(self, x):
        """VectorQuantizer.call (:133-162), forward values: (quantized, perplexity)."""
        self.prepare()
        e = self.input_size >> len(self.num_channels)
        z = self._check(x, e, self.embedding_dim, "quantizer input")
        flat = z.reshape(-1, self.embedding_dim)
        idx = self.get_code_indices(flat)
        q = ops.gather_rows(self.P["vq.codebook_t"], idx).reshape(z.shape)
        probs = torch.bincount(idx.long(), minlength=self.num_embeddings).float() / idx.numel()
        perplexity = torch.exp(-(probs * torch.log(probs + 1e-10)).sum())
        self.last_indices = idx
        self._last_pair = (q, z)                     # what last_loss is computed from, when somebody asks
        return q, perplexity

    @property
    def last_loss(self):
        """The loss the reference's VectorQuantizer adds in ``call`` (:150-153), forward value, of the latest ``quantizer`` call:
        beta*mean((sg(q) - z)^2) + mean((q - sg(z))^2) = (1 + beta) * mean((q - z)^2), a 0-d float64 device tensor.  Computed when it
        is asked for (one pass of dm3d_pair_stats over the two latents), so a ``quantizer`` call costs what it did."""
        if self._last_pair is None:
            raise RuntimeError("last_loss: the quantizer has not been called yet")
        q, z = self._last_pair
        B, n = z.shape[0], z.numel() // z.shape[0]
        sse = ops.pair_stats(q.reshape(B, 1, 1, n, 1), z.reshape(B, 1, 1, n, 1)).sse
        return (1.0 + VQ_BETA) * sse.sum() / z.numel()

    # ---- the codebook of the frozen autoencoder ----------------------------------------------------------------------------
    def _latent_rows(self, batch):
        """The frozen encoder on one batch, an encoder input or ``(img, mask, _)`` as ``test_step`` takes it: latents [rows, D]."""
        if isinstance(batch, (tuple, list)):
            img = torch.as_tensor(batch[0], dtype=torch.float32).to(self.device)
            mask = torch.as_tensor(batch[1], dtype=torch.float32).to(self.device)
            batch = torch.cat([img, mask], dim=-1).contiguous()
        return self._encode(batch).reshape(-1, self.embedding_dim)

    def fit_codebook(self, batches, decay=0.99, epsilon=1e-5, replace_every=None, discarding_threshold=0.01, seed=0):
        """Fits the codebook to the latents of ``batches`` with the encoder frozen: per batch, encoder -> nearest code -> per-code
        counts and float64 sums -> the reference's moving-average update (VectorQuantizerEMA, emavqvae.py:213-222), and every
        ``replace_every`` batches NSVQ's dead-code replacement (nsvqvae.py:193-230) with ``discarding_threshold``.  All of it acts on
        the model's own device codebook and ``esq``; the moving averages start from the codebook with cluster sizes of 1.  Nothing
        synchronises in the loop; per-batch ``perplexity``, ``active_codes`` and ``quantize_loss`` (``last_loss``'s rule, before
        the batch's update) come back in one read at the end together with the codebook, which becomes ``state["vq.embeddings"]``:
        ``quantizer`` / ``test_step`` use it, and a model loaded from the state picks the same codes.  Sums run in a fixed order with
        no floating-point atomic, so a fit repeats bitwise."""
        if replace_every is not None and (int(replace_every) != replace_every or replace_every < 1):
            raise ValueError(f"replace_every must be None or an integer of at least 1, got {replace_every!r}")
        self.prepare()
        k, dim = self.num_embeddings, self.embedding_dim
        book, esq = self.P["vq.codebook_t"], self.P["vq.esq"]
        size, ema_w = torch.ones(k, dtype=torch.float32, device=self.device), book.clone()
        used = torch.zeros(k, dtype=torch.int32, device=self.device)
        kept, replacements = [], 0
        for i, batch in enumerate(batches):
            flat = self._latent_rows(batch)
            idx = ops.vq_assign(flat, book, esq)
            q = ops.gather_rows(book, idx)
            sse = ops.pair_stats(q.reshape(1, 1, 1, -1, 1), flat.reshape(1, 1, 1, -1, 1)).sse
            stats = ops.code_stats(flat, idx, k)
            usage = ops.code_usage(stats.counts, flat.shape[0], 1e-10, used_accum=used)
            ops.codebook_ema(book, esq, size, ema_w, stats.counts, stats.sums, decay, epsilon)
            kept.append(torch.stack([usage.perplexity, usage.active.double(), (1.0 + VQ_BETA) * sse.sum() / flat.numel()]))
            if replace_every is not None and (i + 1) % replace_every == 0:
                ops.codebook_replace(book, esq, used, int(replace_every), discarding_threshold, seed=seed, draw=replacements,
                                     cluster_size=size, ema_w=ema_w)
                replacements += 1
        host = torch.cat([book.double().reshape(-1)] + [v for v in kept]).cpu().numpy()      # the one read-back; float32 -> float64 is exact
        self.state["vq.embeddings"] = np.ascontiguousarray(host[:k * dim].reshape(k, dim).T.astype(np.float32))
        per = host[k * dim:].reshape(-1, 3)
        return {"batches": len(kept), "replacements": replacements, "perplexity": per[:, 0].tolist(),
                "active_codes": [int(v) for v in per[:, 1]], "quantize_loss": per[:, 2].tolist()}

    def codebook_usage(self, batches):
        """How the codebook is used on ``batches`` (encoder inputs or ``(img, mask, _)``), with one read-back: ``counts`` (numpy int64
        [K], rows per code), ``rows``, ``perplexity`` (over all rows), ``active_codes`` and ``dead_codes`` (the indices with no row)."""
        self.prepare()
        k = self.num_embeddings
        total = torch.zeros(k, dtype=torch.int32, device=self.device)
        rows = 0
        for batch in batches:
            flat = self._latent_rows(batch)
            idx = ops.vq_assign(flat, self.P["vq.codebook_t"], self.P["vq.esq"])
            ops.code_usage(ops.code_stats(flat, idx, k).counts, flat.shape[0], 1e-10, used_accum=total)
            rows += flat.shape[0]
        if rows == 0:
            raise ValueError("codebook_usage: no batch was given")
        usage = ops.code_usage(total, rows, 1e-10)
        host = torch.cat([total.double(), usage.perplexity.reshape(1), usage.active.double().reshape(1)]).cpu().numpy()
        counts = host[:k].astype(np.int64)
        return {"counts": counts, "rows": rows, "perplexity": float(host[k]), "active_codes": int(host[k + 1]),
                "dead_codes": np.flatnonzero(counts == 0).tolist()}

    def _decode(self, z):
        """Decoder.call (:388-391)."""
        self.prepare()
        n = len(self.num_channels)
        e = self.input_size >> n
        h = self._check(z, e, self.embedding_dim, "decoder input")
        L = self.P["dec.in"]
        h = self._conv(L, h, 3, prelu_alpha=L.alpha)
        for i in range(n):
            for j in range(self.num_res_layers):
                h = self._run_res_unit(f"dec.l{i}.res{j}", h)
            last = i == n - 1
            h = self._conv(self.P[f"dec.up{i}"], h, 4, stride=2, transpose=True, relu=(not last) or bool(self.output_act))
        return h

    def __call__(self, x):
        """VQVAE.call (:453-457): (decoder(quantizer(encoder(x))), perplexity)."""
        q, perplexity = self._quantize(self._encode(x))
        return self._decode(q), perplexity

    # ---- evaluation ------------------------------------------------------------------------------------------------
    @property
    def metrics(self):
        """The running means behind ``test_step``'s results (keras ``Model.metrics``), in ``METRIC_KEYS`` order."""
        return list(self._trackers.values())

    def reset_metrics(self):
        for m in list(self._trackers.values()) + list(self._mask_trackers.values()):
            m.reset_state()

    def _test_values(self, data, mask_metrics=False):
        """One batch through the model and the metric kernels: {key: device tensor} of everything ``test_step`` tracks (:504-536) and,
        with ``mask_metrics``, of what ``mask_test_step`` adds."""
        img, mask, _ = data
        img = torch.as_tensor(img, dtype=torch.float32).to(self.device).contiguous()
        mask = torch.as_tensor(mask, dtype=torch.float32).to(self.device)
        recon, _ = self(torch.cat([img, mask], dim=-1).contiguous())
        ci = img.shape[-1]
        if ci > recon.shape[-1]:
            raise ValueError(f"the image has {ci} channels, the reconstruction {recon.shape[-1]}")
        if mask_metrics:
            return {**self._image_values(img, recon, ci), **self._mask_values(mask.contiguous(), recon, ci)}
        return self._image_values(img, recon, ci)

    def _mask_values(self, mask, recon, ci):
        """The mask half of the reconstruction, channels [ci, ci + cm), against the mask at threshold 0.5: per (volume, channel) values."""
        cm = mask.shape[-1]
        if ci + cm > recon.shape[-1]:
            raise ValueError(f"the reconstruction has no mask channels to score: it has {recon.shape[-1]} channels, the image takes {ci} "
                             f"and the mask needs {cm} behind them")
        m = mask_metrics_of(mask, recon, x_channels=(0, cm), y_channels=(ci, cm))
        return {"mask_dice": m["dice"], "mask_iou": m["iou"], "mask_hd95": m["hd_percentile"], "mask_assd": m["assd"]}

    def _image_values(self, img, recon, ci):
        # tf.split(reconstructions, 2, axis=-1)[0]: the leading channels of the reconstruction, read in place
        ch = dict(x_channels=(0, ci), y_channels=(0, ci))
        stats = ops.pair_stats(img, recon, **ch)
        return {"reconst_loss": stats.sse.sum() / img.numel(), "quantize_loss": self.last_loss,
                "ssim": ops.ssim(img, recon, stats=stats, **ch).double().mean(), "psnr": ops.psnr(img, recon, stats=stats, **ch)}

    def _test_step(self, data):
        return self._track(self._test_values(data))

    def _track(self, values):
        if "loss" in self.METRIC_KEYS:               # :515-516; VQGAN's loss has terms this project does not carry
            values["loss"] = (values["reconst_loss"] + values["quantize_loss"]) / self.num_gpus
        for k in self.METRIC_KEYS:
            self._trackers[k].update_state(values[k])
        return {k: self._trackers[k].result() for k in self.METRIC_KEYS}

    def test_step(self, data):
        """VQVAE.test_step (:504-544) on ``data = (img, mask, _)``: ``x = concat([img, mask], -1)`` through the model, then
        reconst_loss = mean((img - img_recon)^2), quantize_loss = the quantizer's loss (``last_loss``), loss = their sum / num_gpus,
        ssim = the mean of tf.image.ssim over the [B, D] slices and psnr = tf.image.psnr per slice, both with the reference's
        max_val = max(img_recon) - min(img_recon) per volume.  Returns the running means since ``reset_metrics`` as 0-d device tensors
        (psnr weighted by its B*D values, the others one value a batch, as keras.metrics.Mean counts); nothing synchronises."""
        return self._test_step(data)

    def mask_test_step(self, data):
        """``test_step`` plus the scores of the mask half (not in the reference, whose test_step reads the image half only): the mask
        channels of the reconstruction, ``[ci, ci + cm)`` behind the image's, against ``mask``, both binarised at 0.5, per volume and
        channel: ``mask_dice``, ``mask_iou`` (NaN where the truth mask is empty), ``mask_hd95`` and ``mask_assd`` (in voxels; NaN where
        either mask is empty).  Their running means skip NaN.  One forward pass serves both halves; nothing synchronises.  A
        reconstruction without mask channels raises a ValueError."""
        values = self._test_values(data, mask_metrics=True)
        out = self._track(values)
        for k in self.MASK_METRIC_KEYS:
            self._mask_trackers[k].update_state(values[k])
            out[k] = self._mask_trackers[k].result()
        return out

    def evaluate(self, batches):
        """``reset_metrics``, ``test_step`` over an iterable of ``(img, mask, _)``, then the results as Python floats: the one
        synchronisation is the read-back at the end."""
        return self._evaluate(batches, self.test_step, self.METRIC_KEYS)

    def mask_evaluate(self, batches):
        """``evaluate`` with ``mask_test_step``: ``METRIC_KEYS`` and ``MASK_METRIC_KEYS``, one forward pass and one read-back."""
        return self._evaluate(batches, self.mask_test_step, self.METRIC_KEYS + self.MASK_METRIC_KEYS)

    def _evaluate(self, batches, step, keys):
        self.reset_metrics()
        out = None
        for data in batches:
            out = step(data)
        if out is None:
            return {k: 0.0 for k in keys}
        host = torch.stack([out[k] for k in keys]).cpu().tolist()
        return dict(zip(keys, host))
