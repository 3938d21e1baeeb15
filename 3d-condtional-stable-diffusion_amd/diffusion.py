"""``DiffusionModel`` — the reference's DDPM wrapper around the U-Net, on the dm3d HIP kernels.

reference: networks/conditional_dm3d.py:418-594 (conditional) and networks/dm3d.py:379-545 (unconditional).  Same
constructor, attributes and method signatures; tensors are PyTorch device tensors (NDHWC float32) instead of tf.Tensor.
Keyword-only extensions: ``x_T=`` / ``noise=`` inject the random draws (parity tests), ``seed=``
selects the in-kernel Philox stream, ``use_graph=`` toggles HIP-graph replay of the step; ``guidance_scale=`` /
``negative_context=`` / ``guidance_rescale=`` turn on classifier-free guidance (include/dm3d.h, dm3d_guide_desc);
``dynamic_threshold=`` / ``threshold_max=`` replace the static clamp of the x0 estimate by Imagen's dynamic thresholding in the DDIM
and DPM-Solver++ chains (include/dm3d.h, dm3d_thresh_desc); ``sampler="dpmpp_sde"`` / ``sde_eta=`` is the stochastic form of the
DPM-Solver++(2M) chain (include/dm3d.h, dm3d_dpm_sde_desc); ``sampler="unipc"`` / ``unipc_variant=`` is UniPC, a predictor-corrector of
order up to 3 with one fused update launch per step (include/dm3d.h, dm3d_unipc_desc).  Training extensions, off by default: ``compile(ema_decay=)`` keeps an
exponential moving average of the weights in the optimizer's launch (include/dm3d.h, dm3d_adam_ema) and ``use_ema()`` samples from it;
``compile(context_dropout=, null_context=)`` trains the unconditional branch that classifier-free guidance is defined against;
``compile(global_clipnorm=, grad_accum_steps=)`` clips the gradient by its global norm and applies the mean of k micro-batches, both as
device scalars the optimizer's launch reads (include/dm3d.h, dm3d_grad_scale / dm3d_adam_scaled).
``prediction="v"`` / ``"x0"`` (constructor) reads the network's output as v (Salimans & Ho 2022) or as x0 instead of eps: every chain
converts it to eps right after the U-Net (include/dm3d.h, dm3d_pred_desc) and train_step fits the matching target;
``compile(loss_weighting="min_snr", snr_gamma=)`` weighs each sample's loss by min-SNR-gamma (Hang et al. 2023; dm3d_loss_desc).
``zero_terminal_snr=True`` (constructor, with ``prediction="v"`` or ``"x0"``) rescales the schedule so that alpha_bar[T-1] = 0 (Lin et
al. 2023): the DDIM and DPM-Solver++ chains of such a model hand the network's raw output to update kernels that read it in its own
frame (include/dm3d.h, dm3d_ddim_update_frame), because x0 = (x - s eps) / a has no value at a = 0.

The sampling loop (:559-573) runs with no host synchronisation: the step index lives in device memory, one step
(U-Net forward + posterior update + index decrement) is captured once into a HIP graph and replayed T times.

Every chain (DDPM, DDIM, DPM-Solver++; plain, edit, guided) is a ``Sampler``: reset(), step() and the launch sequence of a step
exist once, in that class; a solver subclass names its update entry point and row counter and writes its tables, ``_EditChain``
and ``_GuidedChain`` mix the blend and the guidance in, and the table ``_CHAINS`` picks the class.  generate(), edit() and invert()
check their arguments through one rule function (``_solver_rules``) and drive the chain through one loop (``_run``).

Two halves live beside this file.  ``schedules.py``: the host arithmetic (schedules, coefficient rows, threshold and guidance tables,
mask pooling, context dropout), re-exported here.  ``weight_sets.py``: ``model.weights``, the one owner of the live weights, their
average, the Trainer and of which set the sampling network holds; compile()'s settings stay on the model and are handed to it.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import DdimDesc, DdpmDesc, DpmDesc, DpmSdeDesc, EditDesc, GuideDesc, PredDesc, ThreshDesc, UniPcDesc, check, lib
from .betas import BETAS_FIELDS, Betas
from .schedules import (FLOAT32_MAX, LOSS_WEIGHTINGS, PREDICTIONS, UNIPC_VARIANTS, _check_prediction, _check_unipc, _host, _indices,
                        context_dropout, ddim_coefficients, ddim_timesteps, dpm_coefficients, dpm_sde_coefficients, edit_levels, edit_steps,
                        frame_table, guide_tables, latent_mask, objective_rows, prediction_table, threshold_rank, threshold_tables,
                        unipc_coefficients, unipc_corrector, unipc_orders, unipc_predictor, unipc_system)
from .unet import UNet
from .weight_sets import WeightSets
from .weights import UNetConfig


def _fill(d, **tensors):
    """Points each named field of descriptor ``d`` at its tensor (None: a null pointer); the tensors live as long as ``d`` does."""
    for name, t in tensors.items():
        setattr(d, name, None if t is None else t.data_ptr())
    d._keep = tuple(tensors.values())
    return d


def _plan_buffer(plan, name, make):
    """The buffer ``name`` of a plan, made by ``make()`` on first use.  A chain's tables and state live with its plan and are
    rewritten by reset(), so the graph captured for (plan, kind) serves every later chain of that kind."""
    if getattr(plan, name, None) is None:
        setattr(plan, name, make())
    return getattr(plan, name)


class _LossTracker:
    """keras.metrics.Mean(name="loss") stand-in (conditional_dm3d.py:467, 507-515)."""

    def __init__(self, name="loss"):
        self.name, self.total, self.count = name, 0.0, 0

    def update_state(self, v):
        self.total += float(v)
        self.count += 1

    def result(self):
        return self.total / max(self.count, 1)

    def reset_state(self):
        self.total, self.count = 0.0, 0


class DiffusionModel:
    conditional = True

    def __init__(self, latent_size, num_embed, latent_channels, vqvae_load_ckpt, args, *, device="cuda", weights=None,
                 seed=0, precision=None, norm="batch", context_dim=1, prediction="eps", zero_terminal_snr=False):
        # conditional_dm3d.py:420-469.  ``args`` is any object with .timesteps .num_gpus .kernel_resize .bs
        # ``prediction``: what the network's output is: "eps" (the reference), "v" = sqrt(a) z - sqrt(1-a) x0 or "x0"
        # ``zero_terminal_snr``: the schedule rescaled to alpha_bar[T-1] = 0 (betas.py); the DDIM / DPM-Solver++ chains then run in the
        # network's own frame.  Not with "eps": at alpha_bar = 0 the noise says nothing about x0
        self.prediction = _check_prediction(prediction)
        self.zero_terminal_snr = bool(zero_terminal_snr)
        if self.zero_terminal_snr and self.prediction == "eps":
            raise ValueError("zero_terminal_snr needs prediction='v' or 'x0': eps carries no information at alpha_bar = 0")
        self._pred_table, self._frame_tables = None, {}
        self.loss_weighting, self.snr_gamma = None, 5.0
        self.timesteps = int(args.timesteps)
        self.b = Betas(self.timesteps, self.zero_terminal_snr)
        self.lc = latent_channels
        # The VQ-VAE bracket (networks/vqvae3d_monai.py; conditional_dm3d.py:425-460) is built lazily on first use of
        # .vqvae_trainer / .encoder / .quantizer / .decoder — Keras, too, creates its weights only on the first call.
        self.num_embed = num_embed
        self.vqvae_load_ckpt = vqvae_load_ckpt
        self._vqvae = None
        self._kernel_resize = getattr(args, "kernel_resize", False)
        self._precision = precision
        self.network = UNet(
            UNetConfig(img_size=latent_size, img_channels=latent_channels, widths=[64, 128, 256],
                       has_attention=[False, False, True, True], conditional=self.conditional, norm=norm,
                       context_dim=context_dim),
            device=device, weights=weights, seed=seed, precision=precision)
        self.loss_tracker = _LossTracker("loss")
        self.num_gpus = getattr(args, "num_gpus", 1)
        self.global_bs = getattr(args, "bs", 1)
        self.device = self.network.device
        self._graphs = {}
        self._stream = None
        self._ema_decay, self._ema_warmup = None, True
        self.context_dropout, self.null_context = 0.0, None
        self._global_clipnorm, self._grad_accum_steps, self._warned_skip = None, 1, False
        self.weights = WeightSets(self.network, self._make_trainer, self._drop_graphs)     # live / averaged weights and the Trainer
        self._warned_tf_ema = False
        self.network._before_use = self.weights.refresh
        self.network._training_engine = lambda: self.weights.engine_for_training_forward(*self._training_settings())

    # -- the autoencoder bracket --------------------------------------------------------------------------------------
    @property
    def vqvae_trainer(self):
        """VQVAE(in=1, out=1, channels (32,64,128,256), 5 residual layers, 4 x (stride 2, k4), num_embeddings=num_embed,
        embedding_dim=latent_channels) as in conditional_dm3d.py:425-449; input edge = 16 x latent_size (128 for the
        reference's latent_size 8)."""
        if self._vqvae is None:
            from .networks.vqvae3d_monai import VQVAE
            self._vqvae = VQVAE(
                in_channels=1, out_channels=1, num_channels=(32, 64, 128, 256), num_res_channels=(32, 64, 128, 256),
                num_res_layers=5, downsample_parameters=((2, 4, 1, "same"),) * 4,
                upsample_parameters=((2, 4, 1, "same", 0),) * 4, num_embeddings=self.num_embed, embedding_dim=self.lc,
                dropout=None, num_gpus=self.num_gpus, kernel_resize=self._kernel_resize,
                input_size=16 * self.network.cfg.img_size, device=self.device, precision=self._precision)
            if self.vqvae_load_ckpt is not None:
                print("Loading VQVAE weights")
                self._vqvae.load_weights(self.vqvae_load_ckpt)
        return self._vqvae

    @vqvae_trainer.setter
    def vqvae_trainer(self, v):
        self._vqvae = v

    @property
    def encoder(self):
        return self.vqvae_trainer.encoder

    @property
    def quantizer(self):
        return self.vqvae_trainer.quantizer

    @property
    def decoder(self):
        return self.vqvae_trainer.decoder

    # -- Keras-model conveniences the reference's drivers touch ----------------------------------------------------
    @property
    def metrics(self):
        return [self.loss_tracker]

    def compile(self, loss=None, optimizer=None, *, ema_decay=None, ema_warmup=True, context_dropout=0.0, null_context=None,
                loss_weighting=None, snr_gamma=5.0, global_clipnorm=None, grad_accum_steps=1):
        """keras ``model.compile``.  Keyword-only extensions, read again by every train_step like the learning rate (so a later compile()
        takes effect between steps):
        ``ema_decay`` in [0, 1) (None: off) keeps an exponential moving average of the trainable weights, updated in the optimizer's
        launch; ``ema_warmup`` holds the decay under (1 + n) / (10 + n) at update n (train.py, ema_decay_at).  use_ema() samples from it.
        ``null_context``: an id in [0, context_dim] reserved for "no context" (give the constructor ``context_dim`` one more than
        the classes to have a spare embedding row); guidance then defaults ``negative_context`` to it.  ``context_dropout`` in [0, 1]:
        train_step replaces each sample's id by ``null_context`` with this probability, which trains the unconditional branch
        classifier-free guidance is defined against.
        ``loss_weighting="min_snr"`` (None: every sample weighs 1) weighs each sample's loss by min-SNR-gamma (Hang et al. 2023) with
        gamma = ``snr_gamma`` > 0 (schedules.py, objective_rows): the weight that evens out the timesteps' pull on the shared weights,
        for whichever ``prediction`` the model was built with.  ``snr_gamma`` other than its default needs ``loss_weighting``.
        ``global_clipnorm`` (None: off; else finite and > 0) scales each applied gradient by min(1, global_clipnorm / |g|), |g| the L2
        norm over all trainable weights; a step whose gradient holds an inf or a NaN is skipped on the device (weights, Adam slots and
        the average stay as they are; ``trainer.skipped_steps`` counts them, ``trainer.grad_norm`` is the last norm).
        ``grad_accum_steps`` = k (an int >= 1): every k-th train_step applies the mean gradient of the last k calls, the others only add
        to the gradient buffer; a change in mid-cycle takes effect at the next cycle boundary."""
        from .train import _check_clipping, _check_ema_decay
        global_clipnorm, grad_accum_steps = _check_clipping(global_clipnorm, grad_accum_steps)
        if loss_weighting not in LOSS_WEIGHTINGS:
            raise ValueError(f"loss_weighting must be None or 'min_snr', got {loss_weighting!r}")
        if not float(snr_gamma) > 0:                         # (a NaN fails the comparison too)
            raise ValueError(f"snr_gamma must be > 0, got {snr_gamma}")
        if loss_weighting is None and float(snr_gamma) != 5.0:
            raise ValueError("snr_gamma needs loss_weighting='min_snr'")
        if ema_decay is not None:
            ema_decay = _check_ema_decay(ema_decay)
        context_dropout = float(context_dropout)
        if not 0 <= context_dropout <= 1:
            raise ValueError(f"context_dropout must lie in [0, 1], got {context_dropout}")
        if (null_context is not None or context_dropout > 0) and not self.conditional:
            raise ValueError("context_dropout / null_context need the conditional model: there is no context to drop")
        if null_context is not None:
            if int(null_context) != null_context or not 0 <= int(null_context) <= self.network.cfg.context_dim:
                raise ValueError(f"null_context must be an id in [0, {self.network.cfg.context_dim}], got {null_context!r}")
            null_context = int(null_context)
        if context_dropout > 0 and null_context is None:
            raise ValueError("context_dropout needs null_context: the id the dropped samples are trained under")
        self.loss, self.optimizer = loss, optimizer
        self._ema_decay, self._ema_warmup = ema_decay, bool(ema_warmup)
        self.context_dropout, self.null_context = context_dropout, null_context
        self.loss_weighting, self.snr_gamma = loss_weighting, float(snr_gamma)
        self._global_clipnorm, self._grad_accum_steps = global_clipnorm, grad_accum_steps

    # -- which weights the sampling network runs on -------------------------------------------------------------------------
    def _has_ema(self) -> bool:
        return self.weights.has_average()

    def use_ema(self, flag) -> bool:
        """Chooses the weights the SAMPLING network runs on (generate, edit, invert, network(...)): the exponential moving average
        (True) or the live Adam iterate (False, the default).  Returns the previous setting.  train_step and
        network(..., training=True) always use the live weights, and save_weights() writes them whatever this says.  After a change
        the other set is loaded before the network's next use, and the captured graphs are dropped."""
        return self.weights.select(bool(flag))

    def load_state_dict(self, sd, strict=True):
        """Weights by name; ``optimizer/...`` entries (save_weights of a trained model) restore the Adam slots and step count, so a
        resumed run continues the bias correction where it stopped; without them the optimizer starts afresh.  ``ema/...`` entries restore
        the weight average likewise (complete and of the weights' shapes, or the load fails); a checkpoint without them leaves the
        model without an average, and use_ema() back at False.  ``meta/prediction`` (save_weights of a v- or x0-model's .npz) must
        name this model's ``prediction``, or the load fails before anything is touched; a checkpoint without it loads into any model.
        ``meta/zero_terminal_snr`` (a zero-terminal-SNR model's .npz) follows the same rules against ``zero_terminal_snr``."""
        if "meta/prediction" in sd:
            theirs = str(np.asarray(sd["meta/prediction"]).reshape(-1)[0])
            if theirs != self.prediction:
                raise ValueError(f"the checkpoint holds a prediction={theirs!r} model, this model was built with "
                                 f"prediction={self.prediction!r}: its output would be read as the wrong quantity")
            sd = {k: v for k, v in sd.items() if k != "meta/prediction"}
        if "meta/zero_terminal_snr" in sd:
            theirs = bool(np.asarray(sd["meta/zero_terminal_snr"]).reshape(-1)[0])
            if theirs != self.zero_terminal_snr:
                raise ValueError(f"the checkpoint holds a zero_terminal_snr={theirs} model, this model was built with "
                                 f"zero_terminal_snr={self.zero_terminal_snr}: it was trained on another noise schedule")
            sd = {k: v for k, v in sd.items() if k != "meta/zero_terminal_snr"}
        self.weights.load(sd, strict)

    def _trainable_names(self):
        return self.weights.trainable_names()

    def load_weights(self, path, root=("network",)):
        """keras ``model.load_weights(ckpt)`` (main_conditional_dm.py:207-213): reads the U-Net from a TF2 checkpoint prefix
        saved by the reference (``root``: where the U-Net sits in the saved object, ("network",) for a DiffusionModel
        checkpoint, () for ``network.save_weights``), or from an .npz state dict.  If the checkpoint also holds the
        autoencoder under ``vqvae_trainer`` it is loaded too."""
        if str(path).endswith(".npz"):
            self.load_state_dict(dict(np.load(path)))
            return
        from . import tf_checkpoint as tc
        # (with the Adam slots and step count of a compiled model's checkpoint, if it carries them: the reference resumes training with
        # model.load_weights(<epoch>.ckpt), main_conditional_dm.py:174-183)
        self.load_state_dict(tc.load_unet_state(str(path), self.network.cfg, root=tuple(root), with_optimizer=True))
        rd = tc.BundleReader(str(path))
        if any(k.startswith("vqvae_trainer/") for k in rd.entries):
            self.vqvae_trainer.load_weights(path, root=("vqvae_trainer",))

    def save_weights(self, path, root=("network",), weights="live"):
        """Writes the LIVE weights under the ordinary names, whatever use_ema() says, with the Adam slots; an .npz file also carries
        the weight average as ``ema/...`` entries.  The TF-format writer holds no second copy of the weights (a warning says so once).
        ``weights="ema"`` exports the averaged model under the ordinary names instead, without optimizer or ema/ entries, in either
        format: how an averaged model reaches a reference-format TF checkpoint.  An .npz file of a v- or x0-model also carries
        ``meta/prediction`` (an eps model writes no such entry; the TF format has no place for it), and a zero-terminal-SNR model's
        ``meta/zero_terminal_snr``.  Checkpoints carry no half-filled accumulation cycle: under compile(grad_accum_steps=k) a save in
        mid-cycle writes the weights and slots as they are and the gradients gathered so far are not in the file, so save at cycle
        boundaries (after a train_step that applied an update)."""
        if weights not in ("live", "ema"):
            raise ValueError(f"weights must be 'live' or 'ema', got {weights!r}")
        if weights == "ema" and not self._has_ema():
            raise ValueError("save_weights(weights='ema'): the model has no averaged weights")
        state, opt, ema = self.weights.checkpoint(weights)
        if str(path).endswith(".npz"):
            meta = {} if self.prediction == "eps" else {"meta/prediction": np.asarray(self.prediction)}
            if self.zero_terminal_snr:
                meta["meta/zero_terminal_snr"] = np.asarray(True)
            np.savez(path, **state, **opt, **ema, **meta)
            return
        if ema and not self._warned_tf_ema:
            import warnings
            self._warned_tf_ema = True
            warnings.warn("the TF-format checkpoint holds the live weights only: the weight average is not in this file "
                          "(save an .npz beside it, or export the averaged model with weights='ema')")
        from . import tf_checkpoint as tc
        tc.save_unet_checkpoint(str(path), state, self.network.cfg, root=tuple(root), optimizer=opt or None)

    def _drop_graphs(self):
        for g in self._graphs.values():
            lib().dm3d_graph_destroy(g[0])
        self._graphs = {}

    def __del__(self):
        try:
            self._drop_graphs()
        except Exception:
            pass

    # -- a15: train_step --------------------------------------------------------------------------------------------------
    def _learning_rate(self) -> float:
        """``compile(optimizer=keras.optimizers.Adam(learning_rate=args.lr))`` (main_conditional_dm.py:153): a float, an object with
        ``learning_rate`` / ``lr``, or nothing (the reference's default --lr 1e-4, main_conditional_dm.py:228)."""
        opt = getattr(self, "optimizer", None)
        if isinstance(opt, (int, float)):
            return float(opt)
        for attr in ("learning_rate", "lr"):
            if opt is not None and hasattr(opt, attr):
                return float(getattr(opt, attr))
        return 1e-4

    def _make_trainer(self, live, lr):
        from .train import Trainer
        return Trainer(self.network.cfg, live, self.device, lr=lr)

    def _training_settings(self):
        """What compile() set for the Trainer, re-read whenever one is built or takes a step (so a later compile() takes effect between
        steps): the learning rate and the average's decay and warm-up."""
        return self._learning_rate(), self._ema_decay, self._ema_warmup

    @property
    def trainer(self):
        """The training engine (train.py), built on first use from the live weights."""
        return self.weights.ensure_trainer(*self._training_settings())

    def train_step(self, inputs, *, t=None, noise=None, latents=None, **extensions):
        """conditional_dm3d.py:471-510: ``inputs = (images, mask, context)`` ((images, _) for the unconditional model, dm3d.py:431-433).
        images [b, 16S, 16S, 16S, 1] go through the frozen encoder + quantizer (:478); t ~ U{0..T-1} (:474-476), noise ~ N(0,1) (:481),
        q_sample (:484-490), the network with training=True (:493), loss = MSE_SUM / (global_bs * lc^4) (:496-499), Adam (:501-504),
        loss tracker (:507-510).  Keyword-only extensions: ``t`` / ``noise`` inject the random draws (parity tests), ``latents`` skips the
        autoencoder (pre-encoded latents [b, S, S, S, lc]).  Under compile(context_dropout=p, null_context=k) each sample's context id
        becomes k with probability p, drawn on the host next to t; ``drop`` (bool [b]) injects that draw.  Under compile(ema_decay=)
        the optimizer's launch also advances the weight average.  The step runs on the live weights whatever use_ema() says.
        A ``prediction="v"`` / ``"x0"`` model is fitted to that target, and compile(loss_weighting="min_snr") weighs each sample's loss
        (dm3d_objective_loss_grad; the Trainer keeps the per-sample losses as ``sample_loss``); an eps model without weighting runs the
        reference's plain MSE launch.
        Under compile(grad_accum_steps=k) call j = 0..k-1 of a cycle adds its gradient to the buffer (the first zeroes it), and only call
        k-1 all-reduces, clips (compile(global_clipnorm=)), applies the mean of the k gradients and reads the norm and the skip flag
        back; the others leave the weights, the Adam slots, the average and their counters untouched.  The loss tracker takes every
        call's loss and the BatchNormalization moving statistics update on every call, as Keras would on every forward.  A step skipped
        for a non-finite gradient raises nothing and warns once per model.
        (``drop`` is the one name ``**extensions`` takes, by keyword only: the signature's named keywords stay t, noise and latents.)"""
        drop = extensions.pop("drop", None)
        if extensions:
            raise TypeError(f"train_step() got an unexpected keyword argument {next(iter(extensions))!r}")
        if self.conditional:
            images, _, context = inputs
        else:
            images, _ = inputs
            context = None
        dev, cfg, T = self.device, self.network.cfg, self.timesteps
        if latents is None and images is None:
            raise ValueError("train_step needs images (inputs[0]) or pre-encoded latents=")
        _lib.require_device()
        if torch.device(dev).type != "cuda":            # buffers of a CPU-built model would reach the kernels as host pointers
            raise _lib.Dm3dError(f"train_step: the model was built on {dev}; the dm3d kernels have no CPU path")
        if latents is None:
            latents = self.encode_latents(torch.as_tensor(images, dtype=torch.float32).to(dev))
        latents = torch.as_tensor(latents, dtype=torch.float32).to(dev).contiguous()
        B = latents.shape[0]
        want = (cfg.img_size,) * 3 + (cfg.img_channels,)
        if latents.dim() != 5 or tuple(latents.shape[1:]) != want:
            raise ValueError(f"latents must be [b,{','.join(map(str, want))}], got {tuple(latents.shape)}")
        if t is None:
            t = torch.from_numpy(np.random.default_rng(self.fresh_seed()).integers(0, T, size=B))
        t = torch.as_tensor(t).reshape(-1).to(torch.int64)
        if t.numel() != B or int(t.min()) < 0 or int(t.max()) >= T:
            raise ValueError("t must hold one index in [0, timesteps) per sample")
        if noise is None:
            noise = torch.empty_like(latents)
            check(lib().dm3d_randn(noise.data_ptr(), noise.numel(), self.fresh_seed(), 0x7ffffffe, torch.cuda.current_stream().cuda_stream), "randn")
        noise = torch.as_tensor(noise, dtype=torch.float32).to(dev).contiguous()
        if noise.shape != latents.shape:
            raise ValueError("noise must have the latents' shape")
        ids = None
        if self.conditional:
            ids = self._context_ids(context, B)
            if drop is not None or self.context_dropout > 0:
                if self.null_context is None:
                    raise ValueError("drop= needs compile(null_context=...): the id the dropped samples are trained under")
                ids = context_dropout(np.broadcast_to(ids, (B,)), self.context_dropout, self.null_context,
                                      seed=self.fresh_seed() if drop is None else None, drop=drop)
        elif drop is not None:
            raise ValueError("drop= needs the conditional model: there is no context to drop")
        tr = self.weights.ensure_trainer(*self._training_settings(), step=True)
        tab = self.b.device_tables(dev)
        betas = (tab[BETAS_FIELDS.index("sqrt_alpha_bar")], tab[BETAS_FIELDS.index("sqrt_one_minus_alpha_bar")])
        rows = None
        if self.prediction != "eps" or self.loss_weighting is not None:
            rows = objective_rows(self.b.alpha_bar, t, self.prediction, self.loss_weighting, self.snr_gamma)
        tr.set_clipping(self._global_clipnorm, self._grad_accum_steps)      # (re-read at every step, like the learning rate)
        accumulate, last = tr.micro_step()
        loss, _ = tr.loss_and_grad(latents, t, noise, ids, betas, T, self.global_bs, self.lc, objective=rows, accumulate=accumulate)
        tr.micro_step_done()                       # (only now: a call that raised has added nothing and is not counted)
        if last:
            tr.allreduce_grads(loss)               # data-parallel replicas (one process per GPU): flat RCCL all-reduces; no-op alone
            tr.adam_step()
        self.weights.trained()                     # (every call: the forward moved the moving statistics even where no step was applied)
        self.loss_tracker.update_state(float(loss.item()))
        if last and tr.finish_step() and not self._warned_skip:              # (after loss.item(): the stream has been waited for)
            import warnings
            self._warned_skip = True
            warnings.warn("train_step: the gradient was not finite, so the optimizer step was skipped (weights, Adam slots and the "
                          "average are unchanged); trainer.skipped_steps counts such steps")
        return {"loss": self.loss_tracker.result()}

    def encode_latents(self, images):
        """train_step's first half (conditional_dm3d.py:478): latents, _ = quantizer(encoder(images))."""
        return self.quantizer(self.encoder(images))[0]

    # -- a13: sample ------------------------------------------------------------------------------------------------
    def _ddpm_desc(self, x, eps, t_idx, mode, noise=None, seed=0, mean_out=None, var_out=None) -> DdpmDesc:
        tab = self.b.device_tables(self.device)
        d = _fill(DdpmDesc(), x=x, eps=eps, noise=noise, t=t_idx, mean_out=mean_out, var_out=var_out,
                  **{f: tab[i] for i, f in enumerate(BETAS_FIELDS) if f != "alpha"})
        d.batch, d.per_sample, d.timesteps = x.shape[0], x[0].numel(), self.timesteps
        d.seed, d.mode = int(seed) & (2 ** 64 - 1), mode
        return d

    def sample(self, x_t, pred_noise, curr_time_step, shape):
        """conditional_dm3d.py:517-548: returns (posterior_mean, posterior 'log_variance' [B,1,1,1,1]).  ``pred_noise`` is eps,
        whatever the model's ``prediction``: predict_eps() converts a v- or x0-model's output first.  A zero-terminal-SNR model has no
        DDPM posterior at its last timestep: use ddim_step(..., eta=1.0, prediction=...)."""
        if self.zero_terminal_snr:
            raise ValueError("sample() is the DDPM posterior, which a zero_terminal_snr model does not have at alpha_bar = 0: "
                             "use ddim_step(..., eta=1.0, prediction=model.prediction), or the chain sampler='dpmpp_sde'")
        x_t = torch.as_tensor(x_t, dtype=torch.float32).to(self.device).contiguous()
        eps = torch.as_tensor(pred_noise, dtype=torch.float32).to(self.device).contiguous()
        B = int(shape[0])
        if x_t.shape[0] != B or eps.shape != x_t.shape:
            raise ValueError("x_t / pred_noise / shape disagree")
        t = torch.as_tensor(curr_time_step).reshape(-1).to(torch.int32)
        if t.numel() != B or int(t.min()) < 0 or int(t.max()) >= self.timesteps:
            raise ValueError("curr_time_step must hold one index in [0, timesteps) per sample")
        t = t.to(self.device)
        mean = torch.empty_like(x_t)
        var = torch.empty(B, dtype=torch.float32, device=self.device)
        d = self._ddpm_desc(x_t, eps, t, 0, mean_out=mean, var_out=var)
        check(lib().dm3d_ddpm_update(C.byref(d), torch.cuda.current_stream().cuda_stream), "ddpm_update")
        return mean, var.reshape(B, 1, 1, 1, 1)

    def ddim_step(self, x_t, pred_noise, t, t_prev, eta=0.0, noise=None, *, clip_x0=True, seed=None, dynamic_threshold=None,
                  threshold_max=None, prediction=None):
        """One DDIM update (include/dm3d.h, dm3d_ddim_desc, mode 0): x_t at timestep ``t`` -> x at ``t_prev`` (-1: the x0
        estimate), the DDIM counterpart of sample().  ``t`` / ``t_prev``: one index or one per sample, -1 <= t_prev < t.
        ``noise`` (optional): z of the step (eta > 0); None draws it from Philox under ``seed`` (None: a fresh key).
        ``dynamic_threshold`` / ``threshold_max``: the x0 estimate is thresholded dynamically, as in generate().
        ``pred_noise`` is eps, whatever the model's ``prediction``: predict_eps() converts a v- or x0-model's output first.
        ``prediction="v"`` / ``"x0"`` (None: today's call): ``pred_noise`` is the network's raw output in that frame instead and the
        launch carries the frame rows (schedules.py, frame_table): the form a zero-terminal-SNR model's chain takes, and the only one
        with a value at alpha_bar[t] = 0."""
        if not eta >= 0:
            raise ValueError("eta must be >= 0")
        host, t, tp, thr = self._step_rules(x_t, pred_noise, t, t_prev, noise, prediction, clip_x0, dynamic_threshold, threshold_max)
        x_t, eps, noise, _ = self._staged(host)
        B = x_t.shape[0]
        coef = self._ddim_table(t, tp, eta, clip_x0).to(self.device)
        tau = torch.from_numpy(t.astype(np.int32)).to(self.device)
        pos = torch.arange(B, dtype=torch.int32, device=self.device)
        out = torch.empty_like(x_t)
        frame = self._frame_rows(prediction, t)
        bound = None if thr is None else self._x0_bound(x_t, eps, coef, pos, thr, frame)
        d = self._ddim_desc(x_t, eps, coef, tau, pos, 0, noise=noise, out=out, seed=self.fresh_seed() if seed is None else seed,
                            x0_bound=bound)
        check(self._update_call("ddim_update", d, frame, torch.cuda.current_stream().cuda_stream), "ddim_update")
        return out

    def _step_rules(self, x_t, pred_noise, t, t_prev, noise, prediction, clip_x0, dynamic_threshold, threshold_max, x0_prev=None):
        """The argument rules ddim_step and dpm_step share, checked before any device buffer is made: x_t / pred_noise (and ``noise`` /
        ``x0_prev``, where given) of one shape with a multiple of 4 elements per sample, -1 <= t_prev < t < timesteps, ``prediction``
        and the threshold's.  Returns (x_t, pred_noise, noise, x0_prev) as float32 host tensors (None stays None), t and t_prev as
        host int64 [B], and the host tables of threshold_tables() (None without dynamic_threshold)."""
        x_t, eps = torch.as_tensor(x_t, dtype=torch.float32), torch.as_tensor(pred_noise, dtype=torch.float32)
        B = x_t.shape[0]
        if eps.shape != x_t.shape or x_t[0].numel() % 4:
            raise ValueError("x_t / pred_noise disagree")
        self._frame_rules(prediction)
        t, tp = _indices(t, B), _indices(t_prev, B)
        if t.min() < 0 or t.max() >= self.timesteps or tp.min() < -1 or np.any(tp >= t):
            raise ValueError("t must lie in [0, timesteps) and t_prev in [-1, t)")
        thr = self._threshold_rules(B, x_t[0].numel(), clip_x0, dynamic_threshold, threshold_max)
        like = []
        for name, v in (("noise", noise), ("x0_prev", x0_prev)):
            if v is not None:
                v = torch.as_tensor(v, dtype=torch.float32)
                if v.shape != x_t.shape:
                    raise ValueError(f"{name} must have x_t's shape")
            like.append(v)
        return (x_t, eps, *like), t, tp, thr

    def _staged(self, tensors):
        """Host tensors on the device, contiguous (None stays None): what a single-call form hands its descriptor."""
        return [None if v is None else v.to(self.device).contiguous() for v in tensors]

    def _ddim_table(self, src, dst, eta, clip_x0) -> torch.Tensor:
        """The [n, 8] float32 coefficient rows of dm3d_ddim_desc, from the float32 alpha_bar table the kernels use, in float64."""
        tab = np.zeros((len(src), 8), dtype=np.float64)
        tab[:, :5] = ddim_coefficients(self.b.alpha_bar, src, dst, eta)
        tab[:, 5] = 1.0 if clip_x0 else 0.0
        return torch.from_numpy(tab.astype(np.float32))

    @staticmethod
    def _update_call(entry, desc, frame, st):
        """One launch of dm3d_<entry> (``frame`` None) or of dm3d_<entry>_frame with the frame rows ``frame`` (a device tensor the caller
        keeps alive): the raw-prediction form of the DDIM and DPM-Solver++ updates."""
        if frame is None:
            return getattr(lib(), "dm3d_" + entry)(C.byref(desc), st)
        return getattr(lib(), "dm3d_" + entry + "_frame")(C.byref(desc), frame.data_ptr(), st)

    def _ddim_desc(self, x, eps, coef, tau, pos, mode, noise=None, out=None, t_next=None, t_idx=None, seed=0, x0_bound=None) -> DdimDesc:
        d = _fill(DdimDesc(), x=x, eps=eps, noise=noise, out=out, coef=coef, tau=tau, pos=pos, t_next=t_next, t_idx=t_idx, x0_bound=x0_bound)
        d.batch, d.per_sample, d.rows = x.shape[0], x[0].numel(), coef.shape[0]
        d.seed, d.mode = int(seed) & (2 ** 64 - 1), mode
        return d

    def dpm_step(self, x_t, pred_noise, t, t_prev, x0_prev=None, t_before=None, *, clip_x0=True, dynamic_threshold=None,
                 threshold_max=None, prediction=None, sde_eta=None, noise=None, seed=None):
        """One DPM-Solver++(2M) update (include/dm3d.h, dm3d_dpm_desc, mode 0): x_t at timestep ``t`` -> x at ``t_prev`` (-1: the x0
        estimate), the single-call counterpart of a sampler="dpmpp" chain's step, as ddim_step is of a DDIM chain.  Returns
        (x_next, x0), x0 being this step's (clipped) estimate: the ``x0_prev`` of the next call.  With ``x0_prev`` and ``t_before``
        (the estimate and the timestep of the step before; given together or not at all) the step is second order, else first order
        (= ddim_step at eta = 0 where the x0 estimate is not clipped).  ``t`` / ``t_prev`` / ``t_before``: one index or one per sample, -1 <= t_prev < t < t_before.
        ``dynamic_threshold`` / ``threshold_max``: the x0 estimate (the one returned too) is thresholded dynamically, as in generate().
        ``pred_noise`` is eps, whatever the model's ``prediction``: predict_eps() converts a v- or x0-model's output first.
        ``prediction="v"`` / ``"x0"`` (None: today's call): ``pred_noise`` is the network's raw output in that frame, as ddim_step.
        ``sde_eta`` (None: today's launch of dm3d_dpm_update): the step of a sampler="dpmpp_sde" chain at that eta instead (include/dm3d.h,
        dm3d_dpm_sde_desc, mode 0; finite, >= 0; 0 is the ODE step bitwise).  ``noise`` (optional): z of the step; None draws it from
        Philox under ``seed`` (None: a fresh key).  ``noise`` / ``seed`` need ``sde_eta``."""
        if (x0_prev is None) != (t_before is None):
            raise ValueError("x0_prev and t_before are given together or not at all")
        if sde_eta is None and (noise is not None or seed is not None):
            raise ValueError("noise / seed belong to the stochastic step: give sde_eta")
        sde_eta = self._sde_eta_rules(sde_eta)
        host, t, tp, thr = self._step_rules(x_t, pred_noise, t, t_prev, noise, prediction, clip_x0, dynamic_threshold, threshold_max, x0_prev)
        B = host[0].shape[0]
        tb = np.full(B, -1, dtype=np.int64) if t_before is None else _indices(t_before, B)
        if t_before is not None and (np.any(tb <= t) or tb.max() >= self.timesteps):
            raise ValueError("t_before must lie in (t, timesteps)")
        dev = self.device
        x_t, eps, noise, hist = self._staged(host)
        coef = self._dpm_sde_table(t, tp, tb, 2, clip_x0, sde_eta).to(dev)
        pos = torch.arange(B, dtype=torch.int32, device=dev)
        out, x0 = torch.empty_like(x_t), torch.empty_like(x_t)
        frame = self._frame_rows(prediction, t)
        bound = None if thr is None else self._x0_bound(x_t, eps, coef, pos, thr, frame)
        if sde_eta is None:
            entry, d = "dpm_update", self._dpm_desc(x_t, eps, hist, coef, pos, 0, out=out, x0_out=x0, x0_bound=bound)
        else:
            tau = torch.from_numpy(t.astype(np.int32)).to(dev)
            entry, d = "dpm_sde_update", self._dpm_sde_desc(x_t, eps, hist, coef, tau, pos, 0, noise=noise, out=out, x0_out=x0,
                                                            seed=self.fresh_seed() if seed is None else seed, x0_bound=bound)
        check(self._update_call(entry, d, frame, torch.cuda.current_stream().cuda_stream), entry)
        return out, x0

    @staticmethod
    def _sde_eta_rules(sde_eta):
        """The argument rule of ``sde_eta``, checked before any device buffer is made: None stays None, else a finite float >= 0."""
        if sde_eta is None:
            return None
        eta = float(sde_eta)
        if not (eta >= 0 and np.isfinite(eta)):              # (a NaN fails the comparison too)
            raise ValueError(f"sde_eta must be finite and >= 0, got {sde_eta!r}")
        return eta

    def _dpm_table(self, src, dst, prev, order, clip_x0) -> torch.Tensor:
        """The [n, 8] float32 coefficient rows of dm3d_dpm_desc, from the float32 alpha_bar table the kernels use, in float64."""
        return DiffusionModel._dpm_sde_table(self, src, dst, prev, order, clip_x0)         # (of ``self`` only ``b`` is read)

    def _dpm_sde_table(self, src, dst, prev, order, clip_x0, eta=None) -> torch.Tensor:
        """The [n, 8] float32 coefficient rows of dm3d_dpm_sde_desc: _dpm_table's with c_z in column 6, which ``eta`` None (the ODE
        solver's table) leaves at 0, as eta = 0 does: dpm_sde_coefficients returns dpm_coefficients' own rows then."""
        tab = np.zeros((len(src), 8), dtype=np.float64)
        tab[:, :2] = ddim_coefficients(self.b.alpha_bar, src, dst)[:, :2]
        rows = dpm_sde_coefficients(self.b.alpha_bar, src, dst, prev, order, 0.0 if eta is None else eta)
        tab[:, 2:5], tab[:, 6] = rows[:, :3], rows[:, 3]
        tab[:, 5] = 1.0 if clip_x0 else 0.0
        return torch.from_numpy(tab.astype(np.float32))

    def _dpm_desc(self, x, eps, hist, coef, pos, mode, out=None, x0_out=None, t_next=None, t_idx=None, x0_bound=None, desc=DpmDesc,
                  **own) -> DpmDesc:
        """A dm3d_dpm_desc; ``desc`` and ``own`` are _dpm_sde_desc's: the extended descriptor and the pointers only it has."""
        d = _fill(desc(), x=x, eps=eps, hist=hist, out=out, x0_out=x0_out, coef=coef, pos=pos, t_next=t_next, t_idx=t_idx,
                  x0_bound=x0_bound, **own)
        d.batch, d.per_sample, d.rows, d.mode = x.shape[0], x[0].numel(), coef.shape[0], mode
        return d

    def _dpm_sde_desc(self, x, eps, hist, coef, tau, pos, mode, noise=None, out=None, x0_out=None, t_next=None, t_idx=None, seed=0,
                      x0_bound=None) -> DpmSdeDesc:
        d = self._dpm_desc(x, eps, hist, coef, pos, mode, out, x0_out, t_next, t_idx, x0_bound, desc=DpmSdeDesc, noise=noise, tau=tau)
        d.seed = int(seed) & (2 ** 64 - 1)
        return d

    # -- UniPC ---------------------------------------------------------------------------------------------------------------------
    def unipc_step(self, x_t, pred_noise, t, t_prev, hist=(), t_hist=(), x_before=None, *, solver_order=1, corrector_order=0,
                   clip_x0=True, unipc_variant="bh2", dynamic_threshold=None, threshold_max=None):
        """One launch of the UniPC update (include/dm3d.h, dm3d_unipc_desc, mode 0): the single-call counterpart of a sampler="unipc"
        chain's step, as dpm_step is of a "dpmpp" chain's.  ``x_t`` is the predicted state at timestep ``t`` and ``pred_noise`` the
        network's eps on it (predict_eps() converts a v- or x0-model's output first).  Returns (x_next, x_corr, x0): the predicted
        state at ``t_prev`` (-1: the x0 estimate itself), the corrected state at ``t`` and this level's (clipped) x0 estimate.
        ``hist`` / ``t_hist``: up to three x0 estimates of the levels before, newest first, and their timesteps, t < t_hist[0] <
        t_hist[1] < ...; ``x_before``: the corrected state at t_hist[0].  ``corrector_order`` = c in 0..3 (0: no corrector, x_corr is
        x_t): the corrector at ``t``, reached from t_hist[0], uses x_before and hist[:c].  ``solver_order`` = p in 1..3: the predictor
        from the corrected state uses this call's estimate and hist[:p-1] (p = 1: the DDIM eta = 0 step).  ``t`` / ``t_prev`` and every
        entry of ``t_hist``: one index or one per sample.  ``unipc_variant``, ``clip_x0``, ``dynamic_threshold`` / ``threshold_max``: as
        generate().  The inputs are left untouched."""
        _check_unipc(solver_order, unipc_variant)
        if corrector_order not in (0, 1, 2, 3):
            raise ValueError(f"corrector_order must be 0, 1, 2 or 3, got {corrector_order!r}")
        if self.zero_terminal_snr:
            raise ValueError("unipc_step needs a finite log-SNR at every level, which a zero_terminal_snr model's last timestep lacks: use dpm_step")
        hist, t_hist = list(hist), list(t_hist)
        need = max(solver_order - 1, corrector_order)
        if len(hist) != len(t_hist) or len(hist) > 3 or len(hist) < need:
            raise ValueError(f"hist / t_hist must hold the same number (at most 3) of estimates and timesteps, at least {need} for these orders")
        if corrector_order and x_before is None:
            raise ValueError("a corrector needs x_before, the corrected state at t_hist[0]")
        host, t, tp, thr = self._step_rules(x_t, pred_noise, t, t_prev, None, None, clip_x0, dynamic_threshold, threshold_max, x_before)
        B = host[0].shape[0]
        levels, last = [], t
        for k, v in enumerate(t_hist):
            v = _indices(v, B)
            if np.any(v <= last) or v.max() >= self.timesteps:
                raise ValueError("t_hist must lie in (t, timesteps), strictly increasing")
            levels.append(v)
            last = v
            hist[k] = torch.as_tensor(hist[k], dtype=torch.float32)
            if hist[k].shape != host[0].shape:
                raise ValueError("every entry of hist must have x_t's shape")
        ab = np.asarray(self.b.alpha_bar, dtype=np.float64)
        rows = np.zeros((B, 10), dtype=np.float64)
        for b in range(B):
            before = [int(v[b]) for v in levels]
            rows[b, :4] = unipc_predictor(ab, int(t[b]), int(tp[b]), before[:solver_order - 1], unipc_variant)
            if corrector_order:
                rows[b, 4:9] = unipc_corrector(ab, before[0], int(t[b]), before[1:corrector_order], unipc_variant)
        dev = self.device
        coef, corr = (v.to(dev) for v in self._unipc_table(t, rows, clip_x0))
        x_t, eps, _, xc = self._staged(host)
        slots = self._staged(hist) + [None] * (3 - len(hist))
        pos = torch.arange(B, dtype=torch.int32, device=dev)
        out, xc_out, x0 = torch.empty_like(x_t), torch.empty_like(x_t), torch.empty_like(x_t)
        bound = None if thr is None else self._x0_bound(x_t, eps, coef, pos, thr)
        d = self._unipc_desc(x_t, eps, xc, slots[::-1], coef, corr, pos, 0, out=out, xc_out=xc_out, x0_out=x0, x0_bound=bound)
        check(lib().dm3d_unipc_update(C.byref(d), torch.cuda.current_stream().cuda_stream), "unipc_update")
        return out, xc_out, x0

    def _unipc_table(self, src, rows, clip_x0):
        """The two [n, 8] float32 tables of dm3d_unipc_desc from unipc_coefficients' float64 rows for the levels ``src``: coef =
        (sqrt(a), sqrt(1-a), p_x, p_0, p_1, clip, p_2, rot) and corr = (k_x, k_0, k_1, k_2, k_t, 0, 0, 0), rounded once."""
        coef, corr = np.zeros((len(src), 8), dtype=np.float64), np.zeros((len(src), 8), dtype=np.float64)
        coef[:, :2] = ddim_coefficients(self.b.alpha_bar, src, np.full(len(src), -1, dtype=np.int64))[:, :2]
        coef[:, 2:5], coef[:, 6], coef[:, 7] = rows[:, :3], rows[:, 3], rows[:, 9]
        coef[:, 5] = 1.0 if clip_x0 else 0.0
        corr[:, :5] = rows[:, 4:9]
        return torch.from_numpy(coef.astype(np.float32)), torch.from_numpy(corr.astype(np.float32))

    def _unipc_desc(self, x, eps, xc, slots, coef, corr, pos, mode, out=None, xc_out=None, x0_out=None, t_next=None, t_idx=None,
                    x0_bound=None) -> UniPcDesc:
        """A dm3d_unipc_desc; ``slots``: the three history slots in the descriptor's order (None: a null slot)."""
        d = _fill(UniPcDesc(), x=x, eps=eps, xc=xc, out=out, xc_out=xc_out, x0_out=x0_out, coef=coef, corr=corr, pos=pos, t_next=t_next,
                  t_idx=t_idx, x0_bound=x0_bound)
        for k, s in enumerate(slots):
            d.hist[k] = None if s is None else s.data_ptr()
        d._keep += tuple(slots)
        d.batch, d.per_sample, d.rows, d.mode = x.shape[0], x[0].numel(), coef.shape[0], mode
        return d

    # -- dynamic thresholding of the x0 estimate ----------------------------------------------------------------------------------
    @staticmethod
    def _threshold_rules(B, per_sample, clip_x0, dynamic_threshold, threshold_max, kind=None):
        """The argument rules of dynamic thresholding, checked before any plan or device buffer is made: None for a call without it,
        else the host tables (rank, frac, smax) of threshold_tables()."""
        if dynamic_threshold is None:
            if threshold_max is not None:
                raise ValueError("threshold_max needs dynamic_threshold")
            return None
        if kind is not None and kind not in ("ddim", "dpmpp", "dpmpp_sde", "unipc"):
            raise ValueError("dynamic_threshold / threshold_max belong to sampler='ddim' and 'dpmpp' (and 'dpmpp_sde', 'unipc')")
        if not clip_x0:
            raise ValueError("dynamic_threshold needs clip_x0=True: it replaces the static clamp of the x0 estimate")
        return threshold_tables(B, per_sample, dynamic_threshold, threshold_max)

    def _thresh_desc(self, x, eps, coef, pos, rank, frac, smax, bound, scratch, frame=None) -> ThreshDesc:
        d = _fill(ThreshDesc(), x=x, eps=eps, coef=coef, pos=pos, rank=rank, frac=frac, smax=smax, bound=bound, scratch=scratch, frame=frame)
        d.batch, d.per_sample, d.rows = x.shape[0], x[0].numel(), coef.shape[0]
        return d

    def _thresh_scratch(self, B, per_sample) -> torch.Tensor:
        n = int(lib().dm3d_x0_threshold_scratch_bytes(B, per_sample))
        return torch.empty((n + 15) // 16 * 2, dtype=torch.int64, device=self.device)

    def _x0_bound(self, x, eps, coef, pos, tables, frame=None) -> torch.Tensor:
        """One dm3d_x0_threshold outside a chain: s [B] of x / eps (device, contiguous) under the coefficient rows coef[pos] (and the
        frame rows frame[pos], where eps is a raw prediction)."""
        dev, B = self.device, x.shape[0]
        rank, frac, smax = (torch.from_numpy(t).to(dev) for t in tables)
        bound = torch.empty(B, dtype=torch.float32, device=dev)
        d = self._thresh_desc(x, eps, coef, pos, rank, frac, smax, bound, self._thresh_scratch(B, x[0].numel()), frame)
        check(lib().dm3d_x0_threshold(C.byref(d), torch.cuda.current_stream().cuda_stream), "x0_threshold")
        return bound

    def x0_threshold(self, x_t, pred_noise, t, dynamic_threshold, threshold_max=None, *, clip_x0=True, prediction=None):
        """The dynamic threshold of one x0 estimate (include/dm3d.h, dm3d_thresh_desc): s [B] float32, per volume the
        ``dynamic_threshold`` quantile of |x0| with x0 = (x_t - sqrt(1-a) pred_noise) / sqrt(a) at timestep ``t`` (one index or one
        per volume), raised to 1 and capped at ``threshold_max``; the single-call counterpart of a thresholded chain's step, as
        ddim_step is of a DDIM chain.  The quantile is exact (numpy's "linear" interpolation between two order statistics, in
        float32).  ``clip_x0=False`` describes a step that does not clip: s = 1 and nothing is ranked.  ``pred_noise`` is eps, whatever
        the model's ``prediction``: predict_eps() converts a v- or x0-model's output first.  ``prediction="v"`` / ``"x0"`` (None: today's
        call): ``pred_noise`` is the network's raw output in that frame and x0 = k0x x_t + k0p pred_noise, as ddim_step."""
        x_t, eps = torch.as_tensor(x_t, dtype=torch.float32), torch.as_tensor(pred_noise, dtype=torch.float32)
        if x_t.dim() < 2 or eps.shape != x_t.shape or x_t[0].numel() % 4:
            raise ValueError("x_t / pred_noise must share one shape [B, ...] with a multiple of 4 elements per volume")
        self._frame_rules(prediction)
        B = x_t.shape[0]
        t = _indices(t, B)
        if t.min() < 0 or t.max() >= self.timesteps:
            raise ValueError("t must lie in [0, timesteps)")
        if dynamic_threshold is None:
            raise ValueError("x0_threshold needs dynamic_threshold")
        tables = self._threshold_rules(B, x_t[0].numel(), True, dynamic_threshold, threshold_max)    # clip_x0=False is legal here
        dev = self.device
        coef = self._ddim_table(t, np.full(B, -1, dtype=np.int64), 0.0, bool(clip_x0)).to(dev)
        pos = torch.arange(B, dtype=torch.int32, device=dev)
        return self._x0_bound(x_t.to(dev).contiguous(), eps.to(dev).contiguous(), coef, pos, tables, self._frame_rows(prediction, t))

    # -- what the network predicts -------------------------------------------------------------------------------------------------
    def _prediction_table(self) -> torch.Tensor:
        """The model's [T, 2] device table of dm3d_pred_desc (schedules.py, prediction_table), made on first use."""
        if self._pred_table is None:
            self._pred_table = torch.from_numpy(prediction_table(self.b.alpha_bar, self.prediction)).to(self.device)
        return self._pred_table

    def _frame_rules(self, prediction):
        """The argument rule of the single-call forms' ``prediction=``, checked before any device buffer is made."""
        if prediction is not None and prediction not in ("v", "x0"):
            raise ValueError(f"prediction must be None (pred_noise is eps), 'v' or 'x0' (pred_noise is the raw output), got {prediction!r}")

    def _frame_table(self, prediction=None) -> torch.Tensor:
        """The [T, 4] device table of the updates' ``frame`` for ``prediction`` (None: the model's own; schedules.py,
        frame_table), made on first use."""
        prediction = self.prediction if prediction is None else prediction
        if prediction not in self._frame_tables:
            self._frame_tables[prediction] = torch.from_numpy(frame_table(self.b.alpha_bar, prediction)).to(self.device)
        return self._frame_tables[prediction]

    def _frame_rows(self, prediction, t):
        """The frame rows of a single call at the timesteps ``t`` (host int64 [B]); None without ``prediction``."""
        if prediction is None:
            return None
        return self._frame_table(prediction)[torch.from_numpy(np.ascontiguousarray(t)).to(self.device)].contiguous()

    def _pred_desc(self, pred, x, t_idx, out=None) -> PredDesc:
        d = _fill(PredDesc(), pred=pred, x=x, out=out, table=self._prediction_table(), t_idx=t_idx)
        d.batch, d.per_sample, d.timesteps = x.shape[0], x[0].numel(), self.timesteps
        return d

    def predict_eps(self, x_t, pred, t):
        """The network's output ``pred`` on ``x_t`` at timestep ``t`` (one index or one per volume) as eps (include/dm3d.h,
        dm3d_pred_desc): c_p pred + c_x x_t with the model's ``prediction`` table, in float32 (mul, mul, add); the single-call
        counterpart of the conversion every chain of a v- or x0-model runs after its U-Net, as ddim_step is of a DDIM chain.  An eps
        model's table is (1, 0).  Returns a new tensor; the inputs are left untouched."""
        x_t, pred = torch.as_tensor(x_t, dtype=torch.float32), torch.as_tensor(pred, dtype=torch.float32)
        if x_t.dim() < 2 or pred.shape != x_t.shape or x_t[0].numel() % 4:
            raise ValueError("x_t / pred must share one shape [B, ...] with a multiple of 4 elements per volume")
        B = x_t.shape[0]
        t = _indices(t, B)
        if t.min() < 0 or t.max() >= self.timesteps:
            raise ValueError("t must lie in [0, timesteps)")
        dev = self.device
        x_t, pred = x_t.to(dev).contiguous(), pred.to(dev).contiguous()
        out = torch.empty_like(pred)
        d = self._pred_desc(pred, x_t, torch.from_numpy(t.astype(np.int32)).to(dev), out=out)
        check(lib().dm3d_pred_to_eps(C.byref(d), torch.cuda.current_stream().cuda_stream), "pred_to_eps")
        return out

    def q_sample(self, x0, t, noise=None, *, seed=None):
        """Forward noising (include/dm3d.h, dm3d_edit_desc, mode 0): sqrt(a) x0 + sqrt(1-a) z with a = alpha_bar[t], in the
        reference's order (conditional_dm3d.py:484-491); the single-call counterpart of edit()'s known latent, as ddim_step is of a
        DDIM chain.  ``t``: one index or one per sample in [-1, timesteps); -1 (clean) returns x0 bitwise.  ``noise`` (optional): z;
        None draws it from Philox under ``seed`` (None: a fresh key)."""
        return self._edit_call(x0, t, 0, noise=noise, seed=seed)

    def _edit_call(self, x0, t, mode, x=None, keep=None, noise=None, seed=None):
        """One dm3d_edit_update outside a chain, one level per sample; mode 1 blends into a copy of ``x`` with keep weights
        ``keep`` [B, per_sample / C]."""
        x0 = torch.as_tensor(x0, dtype=torch.float32).to(self.device).contiguous()
        B = x0.shape[0]
        if x0.dim() < 2 or x0[0].numel() % 4:
            raise ValueError("x0 must be [B, ...] with a multiple of 4 elements per sample")
        t = _indices(t, B)
        if t.min() < -1 or t.max() >= self.timesteps:
            raise ValueError("t must lie in [-1, timesteps)")
        if noise is not None:
            noise = torch.as_tensor(noise, dtype=torch.float32).to(self.device).contiguous()
            if noise.shape != x0.shape:
                raise ValueError("noise must have x0's shape")
        out = None
        if mode == 1:
            x = torch.as_tensor(x, dtype=torch.float32).to(self.device).contiguous().clone()
            keep = torch.as_tensor(keep, dtype=torch.float32).to(self.device).contiguous()
            if x.shape != x0.shape or keep.numel() * x0.shape[-1] != x0.numel():
                raise ValueError("x / keep disagree with x0")
        else:
            out = torch.empty_like(x0)
        levels = self._edit_table(t).to(self.device)
        pos = torch.arange(B, dtype=torch.int32, device=self.device)
        d = self._edit_desc(x0, levels, pos, mode, x=x, w=keep, noise=noise, out=out, seed=self.fresh_seed() if seed is None else seed)
        check(lib().dm3d_edit_update(C.byref(d), torch.cuda.current_stream().cuda_stream), "edit_update")
        return out if mode == 0 else x

    def _edit_table(self, levels) -> torch.Tensor:
        """The [n, 4] float32 level rows of dm3d_edit_desc (sqrt(a'), sqrt(1-a'), level, 0), from the float32 alpha_bar table the
        kernels use, in float64, rounded once."""
        tab = np.zeros((len(levels), 4), dtype=np.float64)
        tab[:, :2] = edit_levels(self.b.alpha_bar, levels)
        tab[:, 2] = np.maximum(np.asarray(levels, dtype=np.int64), -1)
        return torch.from_numpy(tab.astype(np.float32))

    def _edit_desc(self, x0, levels, pos, mode, x=None, w=None, noise=None, out=None, seed=0) -> EditDesc:
        d = _fill(EditDesc(), x0=x0, levels=levels, pos=pos, x=x, w=w, noise=noise, out=out)
        d.batch, d.per_sample, d.channels, d.rows = x0.shape[0], x0[0].numel(), x0.shape[-1], levels.shape[0]
        d.seed, d.mode = int(seed) & (2 ** 64 - 1), mode
        return d

    def _guide_desc(self, mode, batch, per_sample, eps_pos=None, eps_neg=None, out=None, scale=None, rescale=None, partials=None,
                    x=None, t_idx=None) -> GuideDesc:
        d = _fill(GuideDesc(), eps_pos=eps_pos, eps_neg=eps_neg, out=out, scale=scale, rescale=rescale, partials=partials, x=x, t_idx=t_idx)
        d.batch, d.per_sample, d.mode = int(batch), int(per_sample), mode
        return d

    _guide_tables = staticmethod(guide_tables)

    def _guidance(self, B, guidance_scale, negative_context, guidance_rescale):
        """The argument rules of classifier-free guidance, checked before any plan or device buffer is made: None for an unguided
        call, else (w [B] float32, phi [B] float32, negative ids [B] int32)."""
        rescaled = guidance_rescale is not None and bool(np.any(np.asarray(_host(guidance_rescale)) != 0))
        if guidance_scale is None:
            if negative_context is not None or rescaled:
                raise ValueError("negative_context / guidance_rescale need guidance_scale")
            return None
        if not self.conditional:
            raise ValueError("classifier-free guidance needs the conditional model: there is no context to guide with")
        if negative_context is None:
            if self.null_context is None:
                raise ValueError("guidance_scale needs negative_context (the model has no reserved null context)")
            negative_context = self.null_context        # compile(null_context=...): the unconditional branch context dropout trains
        w, phi = self._guide_tables(B, guidance_scale, 0.0 if guidance_rescale is None else guidance_rescale)
        neg = self._context_ids(negative_context, B)
        return w, phi, np.ascontiguousarray(np.broadcast_to(neg, (B,)))

    def guide_eps(self, eps_pos, eps_neg, guidance_scale, guidance_rescale=0.0):
        """Classifier-free guidance of one noise prediction (include/dm3d.h, dm3d_guide_desc): eps_neg + w (eps_pos - eps_neg) in
        float32 (sub, mul, add), then with guidance_rescale = phi != 0 scaled by phi std(eps_pos) / std(eps_g) + (1 - phi) per
        volume (population standard deviations over the whole volume); the single-call counterpart of a guided chain's step, as
        ddim_step is of a DDIM chain.  ``guidance_scale`` / ``guidance_rescale``: one value or one per volume.  Returns a new
        tensor; the inputs are left untouched.  Both inputs are eps, whatever the model's ``prediction`` (a chain guides the converted
        eps; Lin et al. 2023 state the rescale for v-prediction models, where it acts on the same quantity)."""
        eps_pos = torch.as_tensor(eps_pos, dtype=torch.float32)
        eps_neg = torch.as_tensor(eps_neg, dtype=torch.float32)
        if eps_pos.dim() < 2 or eps_neg.shape != eps_pos.shape or eps_pos[0].numel() % 4:
            raise ValueError("eps_pos / eps_neg must share one shape [B, ...] with a multiple of 4 elements per volume")
        B, per = eps_pos.shape[0], eps_pos[0].numel()
        w, phi = self._guide_tables(B, guidance_scale, guidance_rescale)
        dev = self.device
        eps_pos, eps_neg = eps_pos.to(dev).contiguous(), eps_neg.to(dev).contiguous()
        out = torch.empty_like(eps_pos)
        w_d, phi_d = torch.from_numpy(w).to(dev), torch.from_numpy(phi).to(dev)
        st = torch.cuda.current_stream().cuda_stream
        partials = None
        if phi.any():
            partials = torch.empty(B * _lib.GUIDE_PARTIAL_BLOCKS * 4, dtype=torch.float64, device=dev)
        d = self._guide_desc(0, B, per, eps_pos=eps_pos, eps_neg=eps_neg, out=out, scale=w_d, rescale=phi_d, partials=partials)
        check(lib().dm3d_guide_update(C.byref(d), st), "guide_update")
        if partials is not None:
            d = self._guide_desc(1, B, per, out=out, rescale=phi_d, partials=partials)
            check(lib().dm3d_guide_update(C.byref(d), st), "guide_update")
        return out

    # -- a14: generate ----------------------------------------------------------------------------------------------
    def _context_ids(self, context_value, batch=None):
        """The reference takes one scalar id and broadcasts it (conditional_dm3d.py:552); an array of shape [B], [B,1] or [B,1,1]
        gives every volume of the batch its own context."""
        if context_value is None:
            # the reference builds tf.constant([[None]]) here and fails (conditional_dm3d.py:552, 586-589)
            raise ValueError("context_value is required for the conditional model")
        ids = np.asarray(_host(context_value)).astype(np.int64).reshape(-1)
        if ids.size != 1 and batch is not None and ids.size != batch:
            raise ValueError(f"context_value must hold one id or one per volume ({batch}), got {ids.size}")
        if ids.min() < 0 or ids.max() > self.network.cfg.context_dim:
            raise ValueError(f"context ids must lie in [0, {self.network.cfg.context_dim}]")
        return ids.astype(np.int32)

    @staticmethod
    def fresh_seed() -> int:
        """A new 64-bit Philox key from the host's entropy source (the reference draws fresh tf.random.normal noise per call)."""
        import secrets
        return secrets.randbits(64)

    def sampler(self, shape, context_value=None, *, seed=None, use_graph=True, kind="ddpm", num_steps=None, timesteps=None,
                eta=0.0, clip_x0=True, guidance_scale=None, negative_context=None, guidance_rescale=0.0, solver_order=2,
                lower_order_final=True, dynamic_threshold=None, threshold_max=None, sde_eta=None, unipc_variant=None) -> "Sampler":
        """The state of one generate() call: plan, tables, context rows and the captured step graph.  There is one live
        Sampler per (batch, context mode): creating another one for the same plan retires the older (its step() raises).
        ``kind="ddim"``: a DDIM chain over ``ddim_timesteps(T, num_steps, timesteps)`` (S steps) with ``eta`` / ``clip_x0``.
        ``kind="dpmpp"``: a DPM-Solver++(2M) chain over the same schedule with ``clip_x0`` / ``solver_order`` / ``lower_order_final``.
        ``kind="dpmpp_sde"``: its stochastic form at ``sde_eta`` (None: 1.0), as generate(); step(noise=) injects a step's z.
        ``kind="unipc"``: a UniPC chain over the same schedule with ``clip_x0`` / ``solver_order`` (1-3) / ``lower_order_final`` /
        ``unipc_variant``, as generate().
        ``guidance_scale`` / ``negative_context`` / ``guidance_rescale``: a guided chain, as generate().
        ``dynamic_threshold`` / ``threshold_max``: a dynamically thresholded DDIM or DPM-Solver++ chain, as generate()."""
        shape = self._sampler_shape(shape)
        taus, opts = self._solver_rules(kind, num_steps, timesteps, eta, clip_x0, solver_order, lower_order_final,
                                        dynamic_threshold=dynamic_threshold, threshold_max=threshold_max, shape=shape, sde_eta=sde_eta,
                                        unipc_variant=unipc_variant)
        ctx, guide = self._contexts(shape[0], context_value, guidance_scale, negative_context, guidance_rescale)
        return _chain_class(kind, False, bool(guide))(self, shape, ctx, seed, use_graph, taus, **opts, **guide)

    def _solver_rules(self, kind, num_steps, timesteps, eta, clip_x0, solver_order, lower_order_final, noise=None, what="sampler kind",
                      dynamic_threshold=None, threshold_max=None, shape=None, sde_eta=None, unipc_variant=None, edit=False):
        """The argument rules of the solvers ("dpmpp_sde": the DPM-Solver++ chain in its stochastic mode, ``sde_eta`` among its
        keywords), checked before any plan or device buffer is made.  Returns the chain's schedule
        (``kind="ddpm"``: every timestep) and the keywords its sampler class takes besides.  ``noise``: the caller's injected z.
        ``dynamic_threshold`` / ``threshold_max`` (with the chain's ``shape``) add ``threshold=`` (the host tables of
        threshold_tables()) to those keywords; without them the keywords are what they always were.  ``unipc_variant`` (None: "bh2")
        belongs to "unipc", which ``edit`` chains and zero-terminal-SNR models do not have."""
        if kind not in ("ddpm", "ddim", "dpmpp", "dpmpp_sde", "unipc"):
            raise ValueError(f"{what} must be 'ddpm', 'ddim', 'dpmpp', 'dpmpp_sde' or 'unipc', got {kind!r}")
        if kind == "ddpm" and self.zero_terminal_snr:
            raise ValueError("a zero_terminal_snr model has no DDPM ancestral chain (its posterior divides by alpha_bar[T-1] = 0): "
                             "use sampler='ddim', eta=1.0, or sampler='dpmpp_sde'")
        sde, unipc = kind == "dpmpp_sde", kind == "unipc"
        if sde_eta is not None and not sde:
            raise ValueError("sde_eta belongs to sampler='dpmpp_sde'" + (": sampler='unipc' is a deterministic solver" if unipc else ""))
        if unipc_variant is not None and not unipc:
            raise ValueError("unipc_variant belongs to sampler='unipc'")
        if unipc:
            if edit:
                raise ValueError("edit(sampler='unipc') is not supported: where RePaint's replacement step goes between the corrector and "
                                 "the predictor is undecided; use sampler='dpmpp'")
            if self.zero_terminal_snr:
                raise ValueError("sampler='unipc' needs a finite log-SNR at every level: a zero_terminal_snr model's start level has "
                                 "lambda = -inf, which breaks the corrector's h; use sampler='dpmpp'")
            if eta != 0:
                raise ValueError("sampler='unipc' is a deterministic solver: eta must be 0 (sampler='ddim' takes eta, sampler='dpmpp_sde' is "
                                 "the stochastic multistep solver)")
            if noise is not None:
                raise ValueError("sampler='unipc' draws no noise: noise= does not apply (x_T= sets the start; sampler='dpmpp_sde' draws)")
            unipc_variant = "bh2" if unipc_variant is None else unipc_variant
            _check_unipc(solver_order, unipc_variant)
        if sde:
            sde_eta = self._sde_eta_rules(1.0 if sde_eta is None else sde_eta)
        thr = None
        if dynamic_threshold is not None or threshold_max is not None:
            thr = self._threshold_rules(shape[0], int(np.prod(shape[1:])), clip_x0, dynamic_threshold, threshold_max, kind)
        thr = {} if thr is None else dict(threshold=thr)
        if kind not in ("dpmpp", "dpmpp_sde", "unipc") and (solver_order != 2 or lower_order_final is not True):
            raise ValueError("solver_order / lower_order_final belong to sampler='dpmpp' and 'dpmpp_sde' (and 'unipc')")
        if kind == "ddpm":
            if num_steps is not None or timesteps is not None or eta != 0.0 or clip_x0 is not True:
                raise ValueError("num_steps / timesteps / eta / clip_x0 belong to sampler='ddim' and 'dpmpp'")
            return np.arange(self.timesteps, dtype=np.int64), {}
        if kind in ("dpmpp", "dpmpp_sde"):
            if eta != 0 and sde:
                raise ValueError("eta is DDIM's keyword and must stay 0 for sampler='dpmpp_sde': its noise level is sde_eta")
            if eta != 0:
                raise ValueError("sampler='dpmpp' is the deterministic solver: eta must be 0 (sampler='dpmpp_sde' is its stochastic form)")
            if solver_order not in (1, 2):
                raise ValueError(f"solver_order must be 1 or 2, got {solver_order!r}")
            if noise is not None and not sde:
                raise ValueError("sampler='dpmpp' draws no noise: noise= does not apply (x_T= sets the start; sampler='dpmpp_sde' draws)")
        taus = ddim_timesteps(self.timesteps, num_steps, timesteps)
        if not eta >= 0:
            raise ValueError("eta must be >= 0")
        if sde:
            thr = dict(thr, sde_eta=sde_eta)
        if unipc:
            thr = dict(thr, variant=unipc_variant)
        if kind in ("dpmpp", "dpmpp_sde", "unipc"):
            return taus, dict(clip_x0=clip_x0, solver_order=solver_order, lower_order_final=lower_order_final, **thr)
        return taus, dict(eta=eta, clip_x0=clip_x0, **thr)

    def _contexts(self, B, context_value, guidance_scale, negative_context, guidance_rescale):
        """The context and guidance rules, checked before any plan or device buffer is made: (context rows of the chain's plan, the
        ``guide=`` keyword of a guided sampler class or nothing)."""
        guide = self._guidance(B, guidance_scale, negative_context, guidance_rescale)
        ctx = self._context_ids(context_value, B) if self.conditional else None
        if guide is None:
            return ctx, {}
        return _guided_ids(ctx, guide[2]), dict(guide=guide[:2])

    def _sampler_shape(self, shape):
        cfg = self.network.cfg
        shape = tuple(int(s) for s in shape)
        if len(shape) != 5 or shape[1:] != (cfg.img_size,) * 3 + (cfg.img_channels,):
            raise ValueError(f"shape must be (B,{cfg.img_size},{cfg.img_size},{cfg.img_size},{cfg.img_channels})")
        return shape

    def generate(self, shape=(1, 16, 16, 16, 16), last_step=0, context_value=None, *, x_T=None, noise=None, seed=None,
                 use_graph=True, steps=None, sampler="ddpm", num_steps=None, timesteps=None, eta=0.0, clip_x0=True,
                 guidance_scale=None, negative_context=None, guidance_rescale=0.0, solver_order=2, lower_order_final=True,
                 dynamic_threshold=None, threshold_max=None, sde_eta=None, unipc_variant=None):
        """conditional_dm3d.py:550-575.  For shape[0] > 1 the single context row is broadcast to every sample.
        ``seed`` (optional): Philox key of x_T and of every step's noise; None (default) draws a fresh key per call, as the
        reference draws fresh tf.random.normal noise, an integer makes the call reproducible.
        ``noise`` (optional): tensor [timesteps, *shape]; row i is the draw of step i.  ``steps`` (optional) stops
        after that many steps (benchmarks time a prefix of the chain).
        ``sampler="ddim"``: the DDIM chain over ``ddim_timesteps(T, num_steps, timesteps)`` = tau_0 < ... < tau_{S-1}, S U-Net
        evaluations, ``eta`` (0: deterministic), ``clip_x0`` (clamp the x0 estimate to [-1, 1], as the reference's DDPM loop
        clips); ``noise`` is then [S, *shape] with row k the z of the step from tau_k; last_step must be 0.
        ``sampler="dpmpp"``: DPM-Solver++(2M) (Lu et al. 2022) over the same schedule, S U-Net evaluations like DDIM at eta = 0 but
        second order: it reuses the x0 estimate of the step before (include/dm3d.h, dm3d_dpm_desc).  The first step of a chain and
        the step to the clean sample are first order; with ``lower_order_final`` (default) the step tau_1 -> tau_0 before it too:
        these schedules end in timestep 0, which that step reaches over a log-SNR gap several times the previous step's, and
        extrapolating over it costs more than the second order gains.  ``solver_order=1`` makes every step first order: DDIM at
        eta = 0 wherever the x0 estimate is not clipped (where it is, DDIM carries the model's eps on, this solver the eps the
        clipped estimate implies).  eta must be 0, last_step 0, and ``noise`` does not apply (the chain draws none; ``x_T`` / ``seed`` set the start).
        ``sampler="dpmpp_sde"``: the stochastic form of that solver (Lu et al. 2022, appendix; k-diffusion's dpmpp_2m_sde; include/dm3d.h,
        dm3d_dpm_sde_desc): every step but the one to the clean sample adds c_z z, and x and the x0 estimates weigh accordingly.
        ``sde_eta`` >= 0 (None: 1.0, the paper's solver; 0: the "dpmpp" chain bitwise) sets the noise level; ``eta`` stays DDIM's keyword
        and must be 0.  ``solver_order`` / ``lower_order_final`` / ``clip_x0``, guidance and thresholding apply as for "dpmpp";
        ``noise`` is [S, *shape] with row k the z of the step from tau_k, as for DDIM (such a call runs eagerly); ``sde_eta`` with any
        other sampler is an error.  A zero_terminal_snr model runs the chain natively: its first step is alpha_t x0 + sigma_t z.
        ``sampler="unipc"``: UniPC (Zhao et al. 2023; the data-prediction multistep form; include/dm3d.h, dm3d_unipc_desc) over the same
        schedule, S U-Net evaluations like "dpmpp".  Each step predicts the next level at order p from the last p x0 estimates and,
        once the U-Net has run there, corrects that level with the new estimate at no further U-Net pass: the accuracy order is p + 1.
        ``solver_order`` = 1, 2 (default) or 3; step j of a chain (from 0) has order min(solver_order, j + 1), with ``lower_order_final``
        (default) at most the number of steps left, and the step to the clean sample returns the x0 estimate.  ``unipc_variant`` = "bh2"
        (None: the default) or "bh1" picks B(h) = expm1(-h) or -h; with any other sampler it is an error.  The solver is deterministic:
        eta must be 0 and ``noise`` / ``sde_eta`` do not apply (``x_T`` / ``seed`` set the start); last_step must be 0.  ``clip_x0``,
        guidance and thresholding apply as for "dpmpp".  edit() and zero_terminal_snr models do not have it: use "dpmpp" there.
        ``guidance_scale`` = w (None, the default: no guidance, today's path): classifier-free guidance, for either sampler.  Every
        step evaluates the U-Net under ``context_value`` and under ``negative_context`` (one id or one per volume; None stands for
        compile()'s ``null_context`` and is an error on a model without one) in one pass over a plan of 2 B rows and continues from eps_neg + w (eps_pos - eps_neg);
        ``guidance_rescale`` = phi in [0, 1] then scales it by phi std(eps_pos) / std(eps_g) + (1 - phi) per volume (Lin et al. 2023).
        w and phi take one value or one per volume; w < 0 and w > 1 are legal, w = 1 is the plain chain under context_value.  The
        chain draws the x_T and the per-step z of the unguided call of the same B volumes and seed.
        ``dynamic_threshold`` = p in (0, 1] (None, the default: the static clamp, today's path), for ``sampler="ddim"`` and
        ``"dpmpp"`` with ``clip_x0=True``: dynamic thresholding of the x0 estimate (Saharia et al. 2022, "Imagen", section 2.3;
        include/dm3d.h, dm3d_thresh_desc).  Every step takes s = the exact p-quantile of |x0| over each volume, raised to 1 and
        capped at ``threshold_max`` (>= 1; None: no cap), and continues from clamp(x0, -s, s) / s instead of clamp(x0, -1, 1): a
        guided chain at a high scale keeps its contrast instead of saturating at +-1.  p and the cap take one value or one per
        volume; a guided chain ranks the x0 of the guided eps.  DDIM carries the model's eps on, DPM-Solver++ uses (and remembers)
        the thresholded estimate."""
        if not 0 <= last_step <= self.timesteps:
            raise ValueError("last_step out of range")
        shape = self._sampler_shape(shape)
        taus, opts = self._solver_rules(sampler, num_steps, timesteps, eta, clip_x0, solver_order, lower_order_final, noise,
                                        dynamic_threshold=dynamic_threshold, threshold_max=threshold_max, shape=shape, sde_eta=sde_eta,
                                        unipc_variant=unipc_variant)
        if noise is not None and sampler != "ddpm" and tuple(noise.shape) != (len(taus),) + shape:      # (_run repeats it for every chain)
            raise ValueError(f"noise must be [S={len(taus)}, *shape] for sampler={sampler!r}")
        if sampler != "ddpm" and last_step != 0:
            raise ValueError(f"sampler={sampler!r} runs whole chains: last_step must be 0")
        ctx, guide = self._contexts(shape[0], context_value, guidance_scale, negative_context, guidance_rescale)
        self.weights.refresh()
        smp = _chain_class(sampler, False, bool(guide))(self, shape, ctx, seed, use_graph and noise is None, taus, **opts, **guide)
        return self._run(smp, (x_T,), noise, steps=steps, last_step=last_step)

    def _run(self, smp, start, noise=None, known_noise=None, steps=None, last_step=0):
        """Drives one chain of ``smp`` from reset(*start): all its steps but the last ``last_step``, at most ``steps`` of them.  Row i
        of ``noise`` [n_steps, *shape] and of ``known_noise`` goes to the step from the schedule's entry i (the first step takes the
        last row).  Returns a copy of the chain's latents, after the range check of the steps taken."""
        n = smp.n_steps
        if noise is not None:
            noise = torch.as_tensor(noise, dtype=torch.float32).to(self.device)
            if tuple(noise.shape) != (n,) + smp.shape:
                raise ValueError("noise must be [timesteps, *shape]" if smp.SOLVER == "ddpm" else f"noise must be [S={n}, *shape] for sampler={smp.SOLVER!r}")
        smp.reset(*start)
        row = lambda rows, i: None if rows is None else rows[i].contiguous()
        count = n - last_step if steps is None else min(int(steps), n - last_step)
        for i in range(n - 1, n - 1 - count, -1):
            smp.step(row(noise, i), row(known_noise, i))
        out = smp.x.clone()
        self.network.check_range(smp.plan)
        return out

    def invert(self, x0, context_value=None, *, num_steps=None, timesteps=None, use_graph=True, seed=None):
        """DDIM inversion: ``x0`` taken as the state at tau_0 of ``ddim_timesteps(T, num_steps, timesteps)``, then for
        i = 0..S-2 eps = U-Net(x, tau_i) and the deterministic update (sigma = 0, no clip) to tau_{i+1}: S-1 U-Net evaluations.
        Returns x at tau_{S-1}, which sampler='ddim' with eta=0 (clip_x0=False) maps back near ``x0``.  ``seed`` only keys the
        (unused) Philox stream."""
        if self.zero_terminal_snr:
            raise ValueError("invert() needs sqrt(1 - a/a') at its last target level, where a' = 0 in a zero_terminal_snr model: "
                             "invert with a model on the plain schedule, or edit(strength < 1) from q_sample's start")
        x0 = torch.as_tensor(x0, dtype=torch.float32)
        shape = self._sampler_shape(x0.shape)
        taus = ddim_timesteps(self.timesteps, num_steps, timesteps)
        ctx = self._context_ids(context_value, shape[0]) if self.conditional else None
        self.weights.refresh()
        smp = DdimSampler(self, shape, ctx, seed, use_graph, taus, clip_x0=False, invert=True)
        return self._run(smp, (x0,))

    def edit(self, x0, context_value=None, *, mask=None, strength=1.0, sampler="ddpm", num_steps=None, timesteps=None, eta=0.0,
             clip_x0=True, seed=None, use_graph=True, noise=None, known_noise=None, steps=None, guidance_scale=None,
             negative_context=None, guidance_rescale=0.0, solver_order=2, lower_order_final=True, dynamic_threshold=None,
             threshold_max=None, sde_eta=None):
        """Inpainting and image-to-image editing (SDEdit) of latents ``x0`` [B, S, S, S, C]; returns latents of x0's shape.

        ``mask`` (1 = regenerate, 0 = keep, in [0, 1]; None: regenerate everything) is pooled to the latent by latent_mask() and
        kept with weight w = 1 - mask: after every step of the chain the known latent, noised to the level the step reached, is put
        back, x <- w known_t + (1-w) x (RePaint's replacement step), so the last step leaves x0 bitwise where w = 1.
        ``strength`` in (0, 1]: the chain keeps the first n = edit_steps(strength, N) entries sched_0 < ... < sched_{n-1} of its
        schedule (DDPM: 0..T-1, N = T; DDIM: ddim_timesteps(T, num_steps, timesteps), N = S).  At n = N it starts from the x_T that
        generate() draws under the same seed (x0 unused); otherwise from q_sample(x0, sched_{n-1}) over the whole volume.
        ``sampler`` / ``num_steps`` / ``timesteps`` / ``eta`` / ``clip_x0`` / ``seed`` / ``use_graph`` / ``steps``: as generate();
        context_value: one id or one per volume, as generate().
        ``noise`` (optional): [n, *x0.shape], row i the sampler's z of the step from sched_i (generate's rows at n = N).
        ``known_noise`` (optional): [n+1, *x0.shape], row j the z of the known latent at level L_j of L = (clean, sched_0, ...,
        sched_{n-1}): row i is the blend after the step from sched_i (row 0, clean, draws none) and row n the start (unused at n = N).
        ``guidance_scale`` / ``negative_context`` / ``guidance_rescale``: classifier-free guidance of the chain's eps, as generate();
        the known latent, the blend and every draw are those of the unguided edit.
        ``sampler="dpmpp"`` / ``solver_order`` / ``lower_order_final``: the DPM-Solver++(2M) chain of generate() over the kept
        schedule; its first step (from x_T or from the q_sample start) is first order, the blend runs after every update as for the
        other samplers, and the solver's history keeps the model's own x0 estimate, unblended.  ``noise`` does not apply.
        ``sampler="dpmpp_sde"`` / ``sde_eta``: the stochastic form of that chain, as generate(); ``noise`` / ``known_noise`` as for DDIM.
        ``dynamic_threshold`` / ``threshold_max``: dynamic thresholding of the chain's x0 estimate over the whole volume, as generate();
        the blend follows the thresholded update.
        ``sampler="unipc"`` is refused: where the replacement step goes between its corrector and predictor is undecided; use "dpmpp"."""
        x0 = torch.as_tensor(x0, dtype=torch.float32)
        shape = self._sampler_shape(x0.shape)
        sched, opts = self._solver_rules(sampler, num_steps, timesteps, eta, clip_x0, solver_order, lower_order_final, noise, what="sampler",
                                         dynamic_threshold=dynamic_threshold, threshold_max=threshold_max, shape=shape, sde_eta=sde_eta,
                                         edit=True)
        n = edit_steps(strength, len(sched))
        full, sched = n == len(sched), sched[:n]
        mask = None if mask is None else latent_mask(mask, shape)
        ctx, guide = self._contexts(shape[0], context_value, guidance_scale, negative_context, guidance_rescale)
        for name, arr, rows in (("noise", noise, n), ("known_noise", known_noise, n + 1)):
            if arr is not None and tuple(arr.shape) != (rows,) + shape:
                raise ValueError(f"{name} must be [{rows}, *x0.shape] for this chain")
        if steps is not None and int(steps) < 0:
            raise ValueError("steps must be >= 0")
        # device work from here on
        self.weights.refresh()
        dev = self.device
        keep = torch.zeros(shape[:4], dtype=torch.float32, device=dev) if mask is None else 1 - mask.to(dev)
        if known_noise is not None:
            known_noise = torch.as_tensor(known_noise, dtype=torch.float32).to(dev)
        eager = noise is not None or known_noise is not None
        smp = _chain_class(sampler, True, bool(guide))(self, shape, ctx, seed, use_graph and not eager, sched, full, **opts, **guide)
        start = (x0.to(dev), keep, None if known_noise is None else known_noise[n].contiguous())
        return self._run(smp, start, noise, known_noise, steps)

    MAX_GRAPHS = 8      # captured step graphs kept per model (one per plan); the least recently used one is destroyed

    def _capture(self, smp: "Sampler"):
        """Capture one step of ``smp`` into a HIP graph, cached per (plan, sampler kind; a dynamically thresholded chain's kind is its
        own, so it and the plain chain of its class never replay each other's graph): the Philox key lives in a device scalar of
        the plan (dm3d_ddpm_desc.seed_dev), a DDIM chain's schedule, eta and clip and a guided chain's scale and rescale in the
        plan's tables, so one graph serves every seed, every DDIM schedule and every guidance scale."""
        key = (id(smp.plan), smp.graph_kind)
        if key in self._graphs:
            self._graphs[key] = self._graphs.pop(key)                  # most recently used last
            return self._graphs[key][0]
        torch.cuda.synchronize()
        cap = torch.cuda.Stream()
        g = C.c_void_p()
        check(lib().dm3d_graph_begin(cap.cuda_stream), "graph_begin")
        try:
            smp._enqueue(cap.cuda_stream, smp.desc)     # desc reads the key through plan.seed_buf
        finally:
            rc = lib().dm3d_graph_end(cap.cuda_stream, C.byref(g))
        check(rc, "graph_end")
        self._graphs[key] = (g, smp.desc, cap, smp.plan)               # the graph references the descriptor's and plan's memory
        while len(self._graphs) > self.MAX_GRAPHS:
            old = next(iter(self._graphs))
            torch.cuda.synchronize()
            lib().dm3d_graph_destroy(self._graphs.pop(old)[0])
        return g

    def test(self, test_prefix, context=None):
        """conditional_dm3d.py:577-594: generate 10 latents, decode them, np.save the images.  The reference hard-codes the
        latent shape (10,16,16,16,64); here it is (10, latent_size^3, latent_channels), identical for its test setting."""
        import os
        for i in [self.timesteps]:
            print(f"Generating for {i} rsteps")
            if self.vqvae_load_ckpt is not None:
                self.vqvae_trainer.load_weights(self.vqvae_load_ckpt)
            e = self.network.cfg.img_size
            img_latents = self.generate((10, e, e, e, self.lc), last_step=self.timesteps - i, context_value=context)
            images = self.vqvae_trainer.decoder(img_latents)
            os.makedirs("./generated_images_dm3d", exist_ok=True)
            np.save(f"./generated_images_dm3d/{test_prefix}-{i}rsteps.npy", images.cpu().numpy())
        return images


class UnconditionalDiffusionModel(DiffusionModel):
    """networks/dm3d.py:379-545: no context input, self-attention blocks, first_conv_channels = 64."""

    conditional = False

    def _context_ids(self, context_value, batch=None):
        return None

    def generate(self, shape=(1, 16, 16, 16, 16), last_step=0, **kw):
        kw.pop("context_value", None)
        return super().generate(shape, last_step, None, **kw)

    def edit(self, x0, **kw):
        kw.pop("context_value", None)
        return super().edit(x0, None, **kw)

    def test(self, test_prefix):
        return super().test(test_prefix, None)


class Sampler:
    """One DDPM chain over a fixed batch (the loop body of generate, conditional_dm3d.py:559-573), and the frame of every chain.

    ``step()`` enqueues U-Net forward + posterior update + index decrement on the current stream and never synchronises;
    with ``use_graph`` the three are one HIP-graph replay.  A chain has ``n_steps`` steps (T): step() past its end raises until reset().
    The plan (buffers, step index, Philox key) belongs to the newest Sampler made for it; an older one raises on use.

    reset(), step() and _enqueue() exist once, here; a step is U-Net, predict (a v- or x0-model's output -> eps), guide, threshold,
    update, blend, mirror, decrement.  A solver subclass names its update entry point (UPDATE) and its device row counter
    (_pos), builds its descriptor (_desc) and writes its tables (_schedule, _coefficients); _EditChain adds the blend after the update and
    _GuidedChain fills the hooks around it (_guide, _mirror, _head).  _CHAINS lists the combinations."""

    KIND = "ddpm"                             # the step graph's cache key beside the plan: one per class
    SOLVER = "ddpm"                           # generate()'s ``sampler=``; the roctx label of a step (an edit chain's: KIND)
    UPDATE = "ddpm_update"                    # the dm3d_* entry point of the solver's update
    COPIES = 1                                # rows of the plan per volume of the chain (a guided chain: 2)
    DRAWS = True                              # whether the update takes a z: step(noise=) applies
    edit = None                               # an edit chain: the blend's descriptor
    threshold = None                          # a dynamically thresholded DDIM / DPM-Solver++ chain: its host tables (rank, frac, smax)
    native = False                            # a zero-terminal-SNR model's chain: the update reads the raw output through frame rows
    sde_eta = None                            # a DPM-Solver++ chain in its stochastic mode: the noise level (None: the ODE solver)

    def __init__(self, model: DiffusionModel, shape, ctx_ids, seed, use_graph, taus=None):
        self.model, self.shape, self.use_graph = model, shape, use_graph
        self.seed = (model.fresh_seed() if seed is None else int(seed)) & (2 ** 64 - 1)
        net, T = model.network, model.timesteps
        # the schedule, lowest timestep first; a DDPM chain walks t = n-1 .. 0 (an edit chain keeps the prefix its strength asks for)
        self.taus = np.arange(T, dtype=np.int64) if taus is None else np.asarray(taus, dtype=np.int64)
        self.n_steps = len(self.taus)
        # one context row per volume, or one broadcast; "sampler": never the plan UNet.__call__ fills with its own time rows
        self.plan = net.plan(shape[0] * self.COPIES, T, ctx_ids is not None and len(ctx_ids) > 1, purpose="sampler")
        plan = self.plan
        if getattr(plan, "_time_filled", None) is not net.P:
            net.fill_time_table(np.arange(T), plan.vec)
            plan._time_filled = net.P
        if ctx_ids is not None:
            plan.set_context(ctx_ids)
        _plan_buffer(plan, "seed_buf", lambda: torch.zeros(1, dtype=torch.int64, device=model.device))
        plan._owner_gen = getattr(plan, "_owner_gen", 0) + 1
        self._gen = plan._owner_gen
        # a v- or x0-model: every row of the plan (a guided chain: both halves) becomes eps right after the U-Net
        # (a zero-terminal-SNR model's chains convert nothing: their update kernels read the raw output through the frame rows)
        self.native = bool(model.zero_terminal_snr)
        self._pred_d = None if model.prediction == "eps" or self.native else model._pred_desc(plan.eps, plan.x, plan.t_idx)
        # the update's entry, bound once: a native chain's takes the frame rows between the descriptor and the stream
        self._launch = getattr(lib(), "dm3d_" + self.UPDATE + ("_frame" if self.native else ""))
        self.desc = self._desc()
        self.desc.seed_dev = plan.seed_buf.data_ptr()
        self._t = -1                          # host mirror of the device step index; -1: no chain in progress

    def _head(self, t):
        """The rows of a plan buffer this chain updates and returns: all of them (a guided chain: the first half)."""
        return t

    @property
    def x(self):
        """The chain's latents [B, ...]: a view of the plan's state."""
        return self._head(self.plan.x)

    @property
    def graph_kind(self):
        """The step graph's cache key beside the plan: KIND, and a thresholded chain's and a converting chain's own (their steps
        hold more launches), a native-frame chain's (its update and threshold carry the frame rows) and a stochastic DPM-Solver++
        chain's (another update entry and descriptor)."""
        return (self.KIND + ("" if getattr(self, "sde_eta", None) is None else "+sde") + ("" if self.threshold is None else "+thr") + ("" if getattr(self, "_pred_d", None) is None else "+pred")
                + ("+frame" if getattr(self, "native", False) else ""))

    def _predict(self, st):
        """Between the U-Net and the guidance: nothing for an eps model; a v- or x0-model's output becomes eps in place, on every row
        of the plan (t_idx is still the timestep the network was evaluated at: the update moves it)."""
        if self._pred_d is not None:
            check(lib().dm3d_pred_to_eps(C.byref(self._pred_d), st), "pred_to_eps")

    def _guide(self, st):
        """Between the U-Net and the update: nothing (a guided chain: eps <- the guided eps)."""

    def _frame(self):
        """The frame rows the update and the threshold read: the plan's in a zero-terminal-SNR model's chain, else nothing (eps is eps)."""
        return self.plan.frame if self.native else None

    def _threshold(self, st):
        """Between the guidance and the update: the x0 estimate's dynamic bound, where the chain asks for one."""
        if self.threshold is not None:
            check(lib().dm3d_x0_threshold(C.byref(self._thr_desc), st), "x0_threshold")

    def _mirror(self, st):
        """After the update and the blend, before the counter's decrement: nothing (a guided chain: the second half follows)."""

    def _desc(self, noise=None):
        return self.model._ddpm_desc(self.x, self._head(self.plan.eps), self.plan.t_idx, 1, noise=noise, seed=self.seed)

    def _pos(self):
        """The device counter a step decrements (and an edit chain's blend reads first): here the timestep itself."""
        return self.plan.t_idx

    def _own(self):
        if self._gen != self.plan._owner_gen:
            raise RuntimeError("this Sampler was retired: a newer Sampler (generate() call) took over its plan")

    def reset(self, x_T=None):
        self._own()
        self._start(x_T)
        self._schedule()
        if self.plan.range_flag is not None:
            self.plan.range_flag.zero_()
        self._t = self.n_steps - 1

    def _start(self, x_T):
        """Philox key and x_T (given, or drawn under the key) of a new chain."""
        plan = self.plan
        st = torch.cuda.current_stream().cuda_stream
        seed_i64 = self.seed - (1 << 64) if self.seed >= (1 << 63) else self.seed
        plan.seed_buf.fill_(seed_i64)
        if x_T is not None:
            self.x.copy_(torch.as_tensor(x_T, dtype=torch.float32).reshape(self.shape))
        else:
            check(lib().dm3d_randn(self.x.data_ptr(), self.x.numel(), self.seed, 0x7fffffff, st), "randn")

    def _schedule(self):
        """The device tables and counters of a new chain: here the first timestep."""
        self.plan.t_idx.fill_(self.n_steps - 1)

    def _enqueue(self, st, desc, edit=None):
        self.plan.run(st)
        push, pop = _lib.roctx()
        push(self.SOLVER if self.edit is None else self.KIND)
        self._predict(st)
        self._guide(st)
        self._threshold(st)
        check(self._launch(C.byref(desc), *((self.plan.frame.data_ptr(),) if self.native else ()), st), self.UPDATE)
        if self.edit is not None:
            check(lib().dm3d_edit_update(C.byref(self.edit if edit is None else edit), st), "edit_update")
        self._mirror(st)
        check(lib().dm3d_add_i32(self._pos().data_ptr(), self.plan.B, -1, st), "add_i32")
        pop()

    def prepare(self):
        """Capture the step graph now (setup cost: the first step() otherwise pays for it)."""
        if self.use_graph:
            self.model._capture(self)
        return self

    def step(self, noise=None, known_noise=None):
        """One step; ``noise`` injects the update's z and ``known_noise`` (edit chains) the z of the blend's known latent: such a step
        is enqueued eagerly with descriptors of its own."""
        if noise is not None and not self.DRAWS:
            raise ValueError(f"a {self.SOLVER!r} chain draws no noise")
        if known_noise is not None and self.edit is None:
            raise TypeError("known_noise belongs to an edit chain")
        self._own()
        if self._t < 0:
            raise RuntimeError("the chain is finished (or was never started): call reset() before step()")
        st = torch.cuda.current_stream().cuda_stream
        if noise is not None or known_noise is not None:
            self._enqueue(st, self.desc if noise is None else self._desc(noise), None if known_noise is None else self._edit_d(known_noise))
        elif self.use_graph:
            # resolved through the model's cache on every step: load_weights / LRU eviction destroy graphs, never under a live handle
            check(lib().dm3d_graph_launch(self.model._capture(self), st), "graph_launch")
        else:
            self._enqueue(st, self.desc)
        self._t -= 1
        if self._t < 0:
            self.finish()                     # the chain's last step: the one host read of a chain driven through step()

    def finish(self):
        """Reads the H3 range flag of the steps taken so far (one 4-byte device read) and raises if an activation left the
        range the arithmetic covers or turned NaN — what generate() does at its end; step() calls it after a chain's last step, a
        caller that stops a chain early calls it itself."""
        self._own()
        self.model.network.check_range(self.plan)


class DdimSampler(Sampler):
    """One DDIM chain over a fixed batch: S steps tau_{S-1} -> ... -> tau_0 -> x0 (``invert``: S-1 steps tau_0 -> ... -> tau_{S-1}).

    It drives the DDPM Sampler's plan (its full T-row time table serves any schedule) and keeps the chain in tables of that
    plan, rewritten by reset(): coefficient rows, the timestep of each row, the next step's timestep and the device row counter.
    Row n-1 is the first step and row 0 the last, so one step is U-Net + dm3d_ddim_update (which also moves t_idx to the next
    step's timestep) + counter decrement in either direction, and one captured graph serves every schedule, eta and clip.

    ``threshold`` (the host tables of threshold_tables()) makes the chain, and every chain built on it, a dynamically thresholded one:
    dm3d_x0_threshold runs before the update, whose descriptor reads the bound it leaves.  Ranks, fractions and caps are tables of
    the plan, rewritten by reset(): one captured graph (of a kind of its own) serves every ratio and cap."""

    KIND = SOLVER = "ddim"
    UPDATE = "ddim_update"

    def __init__(self, model, shape, ctx_ids, seed, use_graph, taus, eta=0.0, clip_x0=True, invert=False, threshold=None):
        self.eta, self.clip_x0, self.invert = float(eta), bool(clip_x0), bool(invert)
        if threshold is not None:
            self.threshold = threshold
        super().__init__(model, shape, ctx_ids, seed, use_graph, taus)
        self.n_steps = len(self.taus) - int(self.invert)

    def _tables(self, coef):
        """The plan's schedule tables, sized for the longest chain (S = T) so that one graph serves every S; ``coef``: the solver's own."""
        plan, T, dev = self.plan, self.model.timesteps, self.model.device
        _plan_buffer(plan, coef, lambda: torch.zeros(T, 8, dtype=torch.float32, device=dev))
        for name in ("ddim_tau", "ddim_next"):
            _plan_buffer(plan, name, lambda: torch.zeros(T, dtype=torch.int32, device=dev))
        _plan_buffer(plan, "ddim_pos", lambda: torch.zeros(plan.B, dtype=torch.int32, device=dev))
        if self.native:
            _plan_buffer(plan, "frame", lambda: torch.zeros(T, 4, dtype=torch.float32, device=dev))
        if self.threshold is not None and getattr(self, "_thr_desc", None) is None:
            # sized for the plan's rows (a guided chain uses the first half, as of every buffer)
            _plan_buffer(plan, "thr_rank", lambda: torch.zeros(plan.B, dtype=torch.int32, device=dev))
            for name in ("thr_frac", "thr_smax", "thr_bound"):
                _plan_buffer(plan, name, lambda: torch.ones(plan.B, dtype=torch.float32, device=dev))
            _plan_buffer(plan, "thr_scratch", lambda: self.model._thresh_scratch(plan.B, plan.x[0].numel()))
            h = self._head
            self._thr_desc = self.model._thresh_desc(self.x, h(plan.eps), getattr(plan, coef), h(plan.ddim_pos), h(plan.thr_rank),
                                                     h(plan.thr_frac), h(plan.thr_smax), h(plan.thr_bound), plan.thr_scratch, self._frame())
        return plan

    def _bound(self):
        """The update descriptor's x0_bound: the plan's bound buffer in a thresholded chain, else nothing (the static clamp)."""
        return None if self.threshold is None else self._head(self.plan.thr_bound)

    def _desc(self, noise=None):
        plan = self._tables("ddim_coef")
        d = self.model._ddim_desc(self.x, self._head(plan.eps), plan.ddim_coef, plan.ddim_tau, plan.ddim_pos, 1, noise=noise,
                                  t_next=plan.ddim_next, t_idx=plan.t_idx, seed=self.seed, x0_bound=self._bound())
        d.seed_dev = plan.seed_buf.data_ptr()
        return d

    def _pos(self):
        return self.plan.ddim_pos

    def _rows(self):
        """(src, dst) timesteps of rows 0..n-1 (row n-1 runs first); dst -1: the x0 target of a sampling chain's last step."""
        t = self.taus
        if self.invert:
            return t[:-1][::-1], t[1:][::-1]
        return t, np.concatenate([[-1], t[:-1]])

    def _start(self, x_T):
        if self.invert and x_T is None:
            raise ValueError("an inversion chain starts from a given x0")
        super()._start(x_T)

    def _coefficients(self, src, dst):
        """(the solver's coefficient buffer of the plan, its float32 rows for the steps src[r] -> dst[r])."""
        return self.plan.ddim_coef, self.model._ddim_table(src, dst, self.eta, self.clip_x0 and not self.invert)

    def _schedule(self):
        """Rows 0..n-1 of the chain: the solver's coefficients, each row's timestep, the timestep the step after it evaluates, the
        row counter at the first step (row n-1) and that step's timestep."""
        plan, n = self.plan, self.n_steps
        if n > 0:
            src, dst = self._rows()
            coef, table = self._coefficients(src, dst)
            coef[:n].copy_(table)
            plan.ddim_tau[:n].copy_(torch.from_numpy(src.astype(np.int32)))
            plan.ddim_next[:n].copy_(torch.from_numpy(np.maximum(dst, 0).astype(np.int32)))
            plan.ddim_pos.fill_(n - 1)
            plan.t_idx.fill_(int(src[n - 1]))
            if self.native:                           # row r reads the network's output at src[r]
                plan.frame[:n].copy_(self.model._frame_table()[torch.from_numpy(np.ascontiguousarray(src)).to(self.model.device)])
        if self.threshold is not None:
            for buf, table in zip((plan.thr_rank, plan.thr_frac, plan.thr_smax), self.threshold):
                self._head(buf).copy_(torch.from_numpy(table))


class DpmSampler(DdimSampler):
    """One DPM-Solver++(2M) chain over a fixed batch: S steps tau_{S-1} -> ... -> tau_0 -> x0, one U-Net pass each, as a DDIM chain.

    It shares the DDIM chain's frame: the plan's schedule tables (ddim_tau / ddim_next / ddim_pos) and row counter, with a
    coefficient table of its own (plan.dpm_coef, rows (sqrt(a), sqrt(1-a), c_x, c_0, c_1, clip, 0, 0)) and the history buffer
    plan.dpm_hist, the x0 estimate of the step before.  reset() rewrites the tables, so one captured graph serves every schedule,
    order and lower_order_final.  The history is never cleared: the first row of every chain has c_1 = 0 and does not read it.

    ``sde_eta`` (None: the ODE solver) makes the chain, and every chain built on it, the stochastic form (generate(sampler="dpmpp_sde")):
    the update is dm3d_dpm_sde_update on a dm3d_dpm_sde_desc that adds the DDIM chain's plan.ddim_tau and the plan's Philox key, the rows
    (..., c_z in column 6) come from dpm_sde_coefficients into a table of their own, plan.dpm_sde_coef, and step(noise=) applies.  eta,
    like schedule and order, is table contents: one captured graph, of a kind of its own ("+sde"), serves every sde_eta."""

    KIND = SOLVER = "dpmpp"
    UPDATE = "dpm_update"
    DRAWS = False
    COEF = "dpm_coef"                         # the plan's coefficient table; the stochastic form keeps one of its own

    def __init__(self, model, shape, ctx_ids, seed, use_graph, taus, clip_x0=True, solver_order=2, lower_order_final=True, threshold=None,
                 sde_eta=None):
        if solver_order not in (1, 2):
            raise ValueError(f"solver_order must be 1 or 2, got {solver_order!r}")
        self.solver_order, self.lower_order_final = int(solver_order), bool(lower_order_final)
        if sde_eta is not None:
            self.sde_eta = model._sde_eta_rules(sde_eta)
            self.UPDATE, self.DRAWS, self.SOLVER, self.COEF = "dpm_sde_update", True, "dpmpp_sde", "dpm_sde_coef"
        super().__init__(model, shape, ctx_ids, seed, use_graph, taus, eta=0.0, clip_x0=clip_x0, threshold=threshold)

    def _desc(self, noise=None):
        plan = self._tables(self.COEF)
        _plan_buffer(plan, "dpm_hist", lambda: torch.zeros_like(plan.x))
        args = self.x, self._head(plan.eps), self._head(plan.dpm_hist), getattr(plan, self.COEF)
        kw = dict(t_next=plan.ddim_next, t_idx=plan.t_idx, x0_bound=self._bound())
        if self.sde_eta is None:
            return self.model._dpm_desc(*args, plan.ddim_pos, 1, **kw)
        d = self.model._dpm_sde_desc(*args, plan.ddim_tau, plan.ddim_pos, 1, noise=noise, seed=self.seed, **kw)
        d.seed_dev = plan.seed_buf.data_ptr()
        return d

    def _prev(self):
        """The level the step before row r started from (row n-1 runs first), -1 where the row is first order: the chain's first
        step, with lower_order_final the step into the schedule's lowest level (row 1), and every row at solver_order 1.  (Row 0,
        the step to clean, is first order by its target.)"""
        prev = np.concatenate([self.taus[1:], [-1]])
        if self.solver_order == 1:
            prev[:] = -1
        if self.lower_order_final and len(prev) > 1:
            prev[1] = -1
        return prev

    def _coefficients(self, src, dst):
        return getattr(self.plan, self.COEF), self.model._dpm_sde_table(src, dst, self._prev(), self.solver_order, self.clip_x0, self.sde_eta)


class _EditChain:
    """The known-latent half of an edit chain (DiffusionModel.edit), mixed in before a solver's class: ``sched`` is the kept prefix of
    its schedule and ``full`` whether that is all of it.  After every update of the chain's kind, dm3d_edit_update
    (mode 1) blends the known latent, noised to the level the step reached, into the kept region, before the row counter's
    decrement.  The known latent, the keep weights and the level table are buffers of the plan, rewritten by reset(), so one captured
    graph per (plan, kind) serves every x0, mask, strength and seed.  Level row j holds L_j of L = (clean, sched_0, ..., sched_{n-1}):
    the blend after the step from sched_i reads row i through the chain's own row counter (_pos, still undecremented: t_idx in a
    DDPM chain, where row t is level t-1; ddim_pos otherwise, where row r is its target dst[r]), the start (q_sample) row n."""

    def __init__(self, model, shape, ctx_ids, seed, use_graph, sched, full, **kw):
        self.full = bool(full)
        super().__init__(model, shape, ctx_ids, seed, use_graph, sched, **kw)
        plan, dev = self.plan, model.device
        _plan_buffer(plan, "edit_known", lambda: torch.zeros_like(plan.x))
        _plan_buffer(plan, "edit_keep", lambda: torch.zeros(plan.B, plan.x[0].numel() // plan.x.shape[-1], dtype=torch.float32, device=dev))
        _plan_buffer(plan, "edit_levels", lambda: torch.zeros(model.timesteps + 1, 4, dtype=torch.float32, device=dev))
        _plan_buffer(plan, "edit_start", lambda: torch.zeros(plan.B, dtype=torch.int32, device=dev))
        self.edit = self._edit_d()

    def _edit_d(self, noise=None, start=False):
        plan = self.plan
        known = self._head(plan.edit_known)                      # (a guided chain: the first half of every buffer)
        if start:
            d = self.model._edit_desc(known, plan.edit_levels, plan.edit_start, 0, noise=noise, out=plan.x, seed=self.seed)
        else:
            d = self.model._edit_desc(known, plan.edit_levels, self._pos(), 1, x=plan.x, w=plan.edit_keep, noise=noise, seed=self.seed)
        d.seed_dev = plan.seed_buf.data_ptr()
        return d

    def reset(self, x0, keep, start_noise=None):
        """A new chain from known latent ``x0`` (device, the plan's shape) with keep weights ``keep`` [B, D, H, W]."""
        self._own()
        plan, n = self.plan, self.n_steps
        known, kept = self._head(plan.edit_known), self._head(plan.edit_keep)
        known.copy_(x0.reshape(known.shape))
        kept.copy_(keep.reshape(kept.shape))
        plan.edit_levels[:n + 1].copy_(self.model._edit_table(np.concatenate([[-1], self.taus])))
        plan.edit_start.fill_(n)
        super().reset(None if self.full else known)
        if not self.full:                                        # SDEdit's start: the whole volume noised to sched_{n-1}
            st = torch.cuda.current_stream().cuda_stream
            check(lib().dm3d_edit_update(C.byref(self._edit_d(start_noise, start=True)), st), "edit_update")


class EditSampler(_EditChain, Sampler):
    """A DDPM edit chain of n steps from t = n-1 (DiffusionModel.edit)."""
    KIND = "ddpm-edit"


class DdimEditSampler(_EditChain, DdimSampler):
    """A DDIM edit chain over the first n entries of a schedule (DiffusionModel.edit)."""
    KIND = "ddim-edit"


class DpmEditSampler(_EditChain, DpmSampler):
    """A DPM-Solver++(2M) edit chain over the first n entries of a schedule (DiffusionModel.edit): the blend follows each update as
    in DdimEditSampler; the history holds the model's x0 estimates, unblended."""
    KIND = "dpmpp-edit"


def _guided_ids(ctx, neg) -> np.ndarray:
    """The context rows of a guided chain's plan: B rows of the wanted ids, then B rows of the negative ones."""
    B = len(neg)
    return np.concatenate([np.broadcast_to(ctx, (B,)), neg]).astype(np.int32)


class _GuidedChain:
    """Classifier-free guidance of a chain (include/dm3d.h, dm3d_guide_desc).  The chain of B volumes drives a plan of 2 B rows with
    one context row per volume: rows :B run under context_value, rows B: under negative_context on the same x, so one U-Net pass
    gives both predictions.  A step is U-Net, guide (eps[:B] <- eps_out in place), the chain's own update and blend on rows :B
    (their descriptors carry batch = B, so the Philox counters are those of the unguided B-row chain), mirror (x and t_idx of rows
    :B to rows B:), counter decrement.  The scales and rescales are tables of the plan, rewritten by reset(): one captured graph per
    (plan, kind) serves every scale, and its kind keeps it apart from the plain step of the same 2 B-row plan.  The graph always
    holds the rescale launch (rows with phi = 0 return at once); an eager chain launches it only if some phi != 0."""

    COPIES = 2

    def __init__(self, *args, guide, **kw):
        self.w, self.phi = guide
        super().__init__(*args, **kw)
        plan, dev, B = self.plan, self.model.device, self.shape[0]
        for name in ("guide_w", "guide_phi"):
            _plan_buffer(plan, name, lambda: torch.zeros(B, dtype=torch.float32, device=dev))
        _plan_buffer(plan, "guide_partials", lambda: torch.zeros(B * _lib.GUIDE_PARTIAL_BLOCKS * 4, dtype=torch.float64, device=dev))
        per, mk = plan.x[0].numel(), self.model._guide_desc
        self._rescales = bool(self.use_graph or self.phi.any())
        self._guide_descs = [mk(0, B, per, eps_pos=plan.eps, eps_neg=plan.eps[B:], out=plan.eps, scale=plan.guide_w,
                                rescale=plan.guide_phi, partials=plan.guide_partials)]
        if self._rescales:
            self._guide_descs.append(mk(1, B, per, out=plan.eps, rescale=plan.guide_phi, partials=plan.guide_partials))
        self._mirror_desc = mk(2, B, per, x=plan.x, t_idx=plan.t_idx)

    def _head(self, t):
        return t[:self.shape[0]]

    def reset(self, *args, **kw):
        super().reset(*args, **kw)
        self.plan.guide_w.copy_(torch.from_numpy(self.w))
        self.plan.guide_phi.copy_(torch.from_numpy(self.phi))
        self._mirror(torch.cuda.current_stream().cuda_stream)      # x_T (or the q_sample start) and t_idx, first half to second

    def _guide(self, st):
        for d in self._guide_descs:
            check(lib().dm3d_guide_update(C.byref(d), st), "guide_update")

    def _mirror(self, st):
        check(lib().dm3d_guide_update(C.byref(self._mirror_desc), st), "guide_update")


class GuidedSampler(_GuidedChain, Sampler):
    KIND = "ddpm-cfg"


class GuidedDdimSampler(_GuidedChain, DdimSampler):
    KIND = "ddim-cfg"


class GuidedEditSampler(_GuidedChain, EditSampler):
    KIND = "ddpm-edit-cfg"


class GuidedDdimEditSampler(_GuidedChain, DdimEditSampler):
    KIND = "ddim-edit-cfg"


class GuidedDpmSampler(_GuidedChain, DpmSampler):
    KIND = "dpmpp-cfg"


class GuidedDpmEditSampler(_GuidedChain, DpmEditSampler):
    KIND = "dpmpp-edit-cfg"


class UniPcSampler(DdimSampler):
    """One UniPC chain over a fixed batch (Zhao et al. 2023; data prediction, multistep, "bh1" / "bh2"): S steps tau_{S-1} -> ... ->
    tau_0 -> x0, one U-Net pass each, as a DPM-Solver++ chain.

    It shares the DDIM chain's frame (plan.ddim_tau / ddim_next / ddim_pos and the row counter).  One launch of dm3d_unipc_update per
    step, after the U-Net, the guidance and the threshold, forms the x0 estimate at the row's level, corrects that level's state with
    it and predicts the next level from the corrected state.  plan.x carries the predicted states (what the U-Net sees), plan.unipc_xc
    the corrected ones and plan.unipc_hist three x0 estimates (order 2 reads two of them); which slot plays which role at a row is
    column 7 of plan.unipc_coef, so no pointer changes between replays.  reset() rewrites plan.unipc_coef and plan.unipc_corr: one
    captured graph serves every schedule, order, variant, lower_order_final and clip.  Nothing is cleared between chains: a chain's
    first row has no corrector and reads no history, and every later row reads only what its chain wrote."""

    KIND = SOLVER = "unipc"
    UPDATE = "unipc_update"
    DRAWS = False

    def __init__(self, model, shape, ctx_ids, seed, use_graph, taus, clip_x0=True, solver_order=2, lower_order_final=True, threshold=None,
                 variant="bh2"):
        _check_unipc(solver_order, variant)
        if model.zero_terminal_snr:
            raise ValueError("sampler='unipc' needs a finite log-SNR at every level, which a zero_terminal_snr model lacks: use sampler='dpmpp'")
        self.solver_order, self.lower_order_final, self.variant = int(solver_order), bool(lower_order_final), variant
        super().__init__(model, shape, ctx_ids, seed, use_graph, taus, eta=0.0, clip_x0=clip_x0, threshold=threshold)

    def _desc(self, noise=None):
        plan, T, dev = self._tables("unipc_coef"), self.model.timesteps, self.model.device
        _plan_buffer(plan, "unipc_corr", lambda: torch.zeros(T, 8, dtype=torch.float32, device=dev))
        _plan_buffer(plan, "unipc_xc", lambda: torch.zeros_like(plan.x))
        _plan_buffer(plan, "unipc_hist", lambda: torch.zeros((3,) + tuple(plan.x.shape), dtype=torch.float32, device=dev))
        h = self._head
        return self.model._unipc_desc(self.x, h(plan.eps), h(plan.unipc_xc), [h(plan.unipc_hist[k]) for k in range(3)], plan.unipc_coef,
                                      plan.unipc_corr, plan.ddim_pos, 1, t_next=plan.ddim_next, t_idx=plan.t_idx, x0_bound=self._bound())

    def _coefficients(self, src, dst):
        rows = unipc_coefficients(self.model.b.alpha_bar, self.taus, self.solver_order, self.lower_order_final, self.variant)
        coef, self._corr_rows = self.model._unipc_table(src, rows, self.clip_x0)
        return self.plan.unipc_coef, coef

    def _schedule(self):
        super()._schedule()
        if self.n_steps > 0:
            self.plan.unipc_corr[:self.n_steps].copy_(self._corr_rows)


class GuidedUniPcSampler(_GuidedChain, UniPcSampler):
    KIND = "unipc-cfg"


# (generate()'s ``sampler=``, edit chain?, guided?) -> the chain's class: the one place that picks it ("dpmpp_sde" is the "dpmpp"
# classes' stochastic mode, not a class: _chain_class maps the name)
_CHAINS = {(c.SOLVER, issubclass(c, _EditChain), issubclass(c, _GuidedChain)): c
           for c in (Sampler, DdimSampler, DpmSampler, EditSampler, DdimEditSampler, DpmEditSampler, GuidedSampler, GuidedDdimSampler,
                     GuidedDpmSampler, GuidedEditSampler, GuidedDdimEditSampler, GuidedDpmEditSampler)}


# UniPC's chains, in a table of their own beside the twelve the three earlier solvers share: it has no edit form
_UNIPC_CHAINS = {(c.SOLVER, issubclass(c, _EditChain), issubclass(c, _GuidedChain)): c for c in (UniPcSampler, GuidedUniPcSampler)}


def _chain_class(sampler, edit, guided):
    """The chain class of a public sampler name: "dpmpp_sde" runs the "dpmpp" classes (with ``sde_eta`` among their keywords)."""
    key = "dpmpp" if sampler == "dpmpp_sde" else sampler, edit, guided
    return _UNIPC_CHAINS[key] if key in _UNIPC_CHAINS else _CHAINS[key]
