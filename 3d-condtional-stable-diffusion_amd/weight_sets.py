"""``WeightSets`` — where a DiffusionModel's live weights and their average are, and which of the two the sampling network holds.

One object per model (``model.weights``) owns the whole lifecycle: checkpoints coming in and going out, the lazily built Trainer, the
switch between the live and the averaged set (use_ema) and the reload that brings either back into the sampling network.  Its state:

    trainer            None or the Trainer: once it exists it is the one home of the live weights, and of the average once it keeps one
    held               "live" | "ema": the set network.state holds now
    want               "live" | "ema": what use_ema() asked for; refresh() brings ``held`` to it
    dirty              the Trainer's weights moved since the network was last loaded from them
    parked_live        host copy of the live weights while the network holds the averaged ones and no Trainer exists
    pending_optimizer  ``optimizer/`` entries of a loaded checkpoint, waiting for a Trainer
    pending_ema        its ``ema/`` entries likewise (the network samples from them as they are)

and the rules ``_check()`` enforces after every change:

    * the live weights are in exactly one place: the Trainer, else ``parked_live`` when held == "ema", else network.state; so
      ``parked_live`` is set exactly when there is no Trainer and held == "ema";
    * the average is in at most one place: ``trainer.ema`` or ``pending_ema``;
    * want == "ema" needs an average, and so does held == "ema" — but for one case: a train step under compile(ema_decay=None) frees the
      Trainer's average while the network still holds a copy of it.  That needs want == "live", so the next refresh() replaces the copy.
"""
from __future__ import annotations

import numpy as np

SETS = ("live", "ema")


class WeightSets:
    def __init__(self, network, make_trainer, on_reload):
        """``make_trainer(live, lr)`` builds a Trainer on the live weights; ``on_reload()`` runs whenever network.state was replaced."""
        self.network, self._make_trainer, self._on_reload = network, make_trainer, on_reload
        self.trainer = None
        self.held = self.want = "live"
        self.dirty = False
        self.parked_live = None
        self.pending_optimizer = self.pending_ema = None

    def _check(self):
        tr = self.trainer
        if self.held not in SETS or self.want not in SETS:
            raise AssertionError(f"weight sets: held {self.held!r}, want {self.want!r}")
        if (self.parked_live is not None) != (tr is None and self.held == "ema"):
            raise AssertionError(f"weight sets: parked live weights {'present' if self.parked_live is not None else 'absent'} with "
                                 f"{'no' if tr is None else 'a'} Trainer and the network holding {self.held!r}")
        if tr is None and self.dirty:
            raise AssertionError("weight sets: dirty without a Trainer")
        if tr is not None and tr.ema is not None and self.pending_ema is not None:
            raise AssertionError("weight sets: an average in the Trainer and another waiting on the host")
        if not self.has_average():
            if self.want == "ema":
                raise AssertionError("weight sets: use_ema(True) without an average")
            if self.held == "ema" and tr is None:
                raise AssertionError("weight sets: the network holds averaged weights no Trainer ever kept")

    # -- the questions ------------------------------------------------------------------------------------------------------
    def trainable_names(self):
        """Names of the parameters Adam updates (everything but the BatchNormalization moving statistics)."""
        from .train import is_trainable
        return [n for n in self.network.spec if is_trainable(n)]

    def has_average(self) -> bool:
        return (self.trainer is not None and self.trainer.ema is not None) or self.pending_ema is not None

    def live(self):
        """The live weights by name (host), from the one place they are in."""
        if self.trainer is not None:
            return self.trainer.state_dict()
        return dict(self.parked_live if self.held == "ema" else self.network.state)

    def averaged(self):
        """The averaged model by name (host): the live weights with every trainable entry replaced by its average."""
        if self.trainer is not None and self.trainer.ema is not None:
            return self.trainer.ema_state_dict()
        return {**self.live(), **{k[len("ema/"):]: v for k, v in self.pending_ema.items() if k != "ema/num_updates"}}

    def ema_entries(self):
        """The ``ema/...`` checkpoint entries of the model, {} without an average."""
        if self.trainer is not None and self.trainer.ema is not None:
            return self.trainer.ema_state()
        return dict(self.pending_ema or {})

    # -- the switch and the reload ------------------------------------------------------------------------------------------
    def select(self, flag) -> bool:
        """use_ema(): asks for the averaged (True) or the live set; the network takes it at its next refresh().  Returns the previous setting."""
        prev = self.want == "ema"
        if flag and not self.has_average():
            raise ValueError("use_ema(True): the model has no averaged weights (train with compile(ema_decay=...) or load a "
                             "checkpoint that carries ema/ entries)")
        self.want = "ema" if flag else "live"
        if __debug__:
            self._check()
        return prev

    def _reload(self, state, held, strict=True):
        """network.state becomes ``state``, a ``held`` set; live weights with no other home are parked first."""
        park = self.live() if held == "ema" and self.trainer is None else None
        self.network.load_state_dict(state, strict)
        self.held, self.parked_live, self.dirty = held, park, False
        self._on_reload()

    def refresh(self):
        """Before the sampling network is used (network._before_use): the set use_ema() asked for, with what train steps changed, flows
        back into it (folded norms, packed images, tables).  Nothing is reloaded while the network is up to date."""
        if self.held == self.want and not self.dirty:
            return
        self._reload(self.averaged() if self.want == "ema" else self.live(), self.want)
        if __debug__:
            self._check()

    # -- checkpoints ----------------------------------------------------------------------------------------------------------
    def load(self, sd, strict=True):
        """load_state_dict(): weights by name, with the ``optimizer/`` and ``ema/`` entries beside them.  Both groups are validated
        BEFORE anything is touched: a checkpoint with partial slots fails with the model as it was (new weights with the old Adam
        state gone would be a half-loaded model)."""
        names = self.trainable_names()
        opt = {k: v for k, v in sd.items() if k.startswith("optimizer/")}
        if opt:
            missing = [k for k in ["optimizer/iter"] + [f"optimizer/{slot}/{n}" for n in names for slot in ("m", "v")] if k not in opt]
            if missing:
                raise ValueError(f"checkpoint carries optimizer state but {len(missing)} entries are missing (first: {missing[:3]}); "
                                 "drop every optimizer/ entry to load the weights alone")
        ema = {k: v for k, v in sd.items() if k.startswith("ema/")}
        if ema:
            want = {"ema/num_updates": ()}
            want.update({f"ema/{n}": tuple(self.network.spec[n]) for n in names})
            missing = [k for k in want if k not in ema]
            extra = [k for k in ema if k not in want]
            wrong = [k for k in want if k in ema and k != "ema/num_updates" and tuple(np.shape(ema[k])) != want[k]]
            if missing or extra or wrong:
                raise ValueError(f"checkpoint carries averaged weights but {len(missing)} entries are missing (first: {missing[:3]}), "
                                 f"{len(extra)} are unknown (first: {extra[:3]}) and {len(wrong)} have another shape (first: {wrong[:3]}); "
                                 "drop every ema/ entry to load the weights alone")
        if self.held == "ema" or self.dirty:                       # a non-strict load fills missing names from the CURRENT live weights
            self._reload(self.live(), "live")
        self._reload({k: v for k, v in sd.items() if not k.startswith(("optimizer/", "ema/"))}, "live", strict)
        self.trainer = None                                        # Adam moments belong to the weights they were built for
        # the slots wait until a Trainer exists (an inference-only load builds none: theta, gradients and moments are four copies of the weights)
        self.pending_optimizer = opt or None
        self.pending_ema = {k: np.array(v, dtype=np.int64 if k == "ema/num_updates" else np.float32) for k, v in ema.items()} or None
        if not ema:
            self.want = "live"                                     # a checkpoint without an average takes the switch back with it
        if __debug__:
            self._check()

    def checkpoint(self, which):
        """(state, optimizer entries, ema entries) for save_weights(): the live weights with everything a resumed run needs, or
        (``which`` = "ema") the averaged model alone."""
        if which == "ema":
            return self.averaged(), {}, {}
        # with the live set asked for and held, a reload that is due happens now and the state is the network's; otherwise it comes from
        # where the live weights are and the network is left as it is
        state = self.network.state_dict() if self.held == "live" == self.want else self.live()
        # the Adam slots and step count travel with the weights, as in the reference's save_weights_only TF checkpoints of a compiled model
        stepped = self.trainer is not None and self.trainer.step_count > 0
        return state, self.trainer.optimizer_state() if stepped else (self.pending_optimizer or {}), self.ema_entries()

    # -- training ---------------------------------------------------------------------------------------------------------------
    def ensure_trainer(self, lr, ema_decay, ema_warmup, *, step=False):
        """The training engine (train.py), built on first use from the live weights, with the waiting optimizer slots.  A new one, and
        one about to take a train step (``step``), gets compile()'s settings: the learning rate and the average's decay and warm-up
        (None: no average is kept); a loaded average continues in it.  (compile()'s clipping and accumulation settings go to the
        Trainer from train_step itself, Trainer.set_clipping: they own no weights and need no rule here.  A Trainer dropped by load()
        takes its half-filled accumulation cycle with it.)"""
        tr, new = self.trainer, self.trainer is None
        if new:
            tr = self.trainer = self._make_trainer(self.live(), lr)
            self.parked_live = None
            if self.pending_optimizer:
                tr.load_optimizer_state(self.pending_optimizer)
                self.pending_optimizer = None
        if new or step:
            tr.lr = lr
            if ema_decay is not None:
                tr.set_ema(ema_decay, ema_warmup)
                if self.pending_ema is not None:
                    tr.load_ema_state(self.pending_ema)
                    self.pending_ema = None
            elif tr.ema is not None:
                if self.want == "ema":
                    raise ValueError("compile(ema_decay=None) would drop the averaged weights the sampling network runs on: use_ema(False) first")
                tr.set_ema(None)
        if __debug__:
            self._check()
        return tr

    def engine_for_training_forward(self, lr, ema_decay, ema_warmup):
        """``network(..., training=True)`` outside train_step (network._training_engine) runs on the model's own Trainer when it has one,
        so the moving statistics it updates are the ones the next train_step continues from (in Keras both are the same variables).
        Under use_ema(True) the network holds the averaged weights: the live ones need a Trainer, so one is built."""
        if self.trainer is None and self.want == "live":
            return None
        tr = self.ensure_trainer(lr, ema_decay, ema_warmup)
        self.dirty = True
        return tr

    def trained(self):
        """A train step moved the Trainer's weights (and its average): the network is out of date."""
        self.dirty = True
        if __debug__:
            self._check()
