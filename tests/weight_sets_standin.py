"""A host-only stand-in for dm3d_amd.train.Trainer with its lifecycle surface (constructor, lr, step_count, forward_only, state_dict,
optimizer_state / load_optimizer_state, set_ema, ema, ema_updates, ema_state_dict, ema_state / load_ema_state, adam_step), for
tools/weight_sets_trace.py and tests/test_weight_sets.py: the weight lifecycle of a DiffusionModel can then be driven on a CPU-built model.
Weights are kept by name in numpy arrays; adam_step moves every trainable entry by STEP, exactly, and advances the average as the real
one does (float32(1 - ema_decay_at(...)))."""
import numpy as np

STEP = np.float32(2.0 ** -7)


class HostTrainer:
    def __init__(self, cfg, state, device, lr=1e-4, bn_moving_unbiased=True, forward_only=False, ema_decay=None, ema_warmup=True):
        from dm3d_amd.train import is_trainable
        from dm3d_amd.weights import walk
        self.cfg, self.device, self.lr, self.forward_only = cfg, device, float(lr), bool(forward_only)
        self.spec = walk(cfg)[1]
        self.names = [n for n in self.spec if is_trainable(n)]
        self.values = {n: np.array(state[n], dtype=np.float32).reshape(self.spec[n]) for n in self.spec}
        self.m = {n: np.zeros(self.spec[n], np.float32) for n in self.names}
        self.v = {n: np.zeros(self.spec[n], np.float32) for n in self.names}
        self.step_count = 0
        self.ema, self.ema_decay, self.ema_warmup, self.ema_updates = None, None, True, 0
        if ema_decay is not None:
            self.set_ema(ema_decay, ema_warmup)

    def state_dict(self):
        return {n: v.copy() for n, v in self.values.items()}

    def optimizer_state(self):
        out = {"optimizer/iter": np.asarray(self.step_count, dtype=np.int64)}
        for n in self.names:
            out[f"optimizer/m/{n}"], out[f"optimizer/v/{n}"] = self.m[n].copy(), self.v[n].copy()
        return out

    def load_optimizer_state(self, st):
        self.step_count = int(np.asarray(st["optimizer/iter"]).reshape(-1)[0])
        for n in self.names:
            for slot, buf in (("m", self.m), ("v", self.v)):
                arr = np.ascontiguousarray(st[f"optimizer/{slot}/{n}"], dtype=np.float32)
                if arr.size != buf[n].size:
                    raise ValueError(f"optimizer slot {slot} of {n}: {arr.size} values for a parameter of {buf[n].size}")
                buf[n] = arr.reshape(self.spec[n]).copy()

    def adam_step(self):
        from dm3d_amd.train import ema_decay_at
        self.step_count += 1
        for n in self.names:
            self.values[n] += STEP
            self.m[n] += STEP
            self.v[n] += STEP * STEP
        if self.ema is None:
            return
        rate = np.float32(1.0 - ema_decay_at(self.ema_decay, self.ema_updates, self.ema_warmup))
        for n in self.names:
            self.ema[n] += rate * (self.values[n] - self.ema[n])
        self.ema_updates += 1

    def set_ema(self, decay, warmup=True):
        from dm3d_amd.train import _check_ema_decay
        if decay is None:
            self.ema, self.ema_decay, self.ema_updates = None, None, 0
            return
        decay = _check_ema_decay(decay)
        if self.forward_only:
            raise ValueError("a forward_only Trainer takes no optimizer step: it keeps no weight average")
        self.ema_decay, self.ema_warmup = decay, bool(warmup)
        if self.ema is None:
            self.ema = {n: self.values[n].copy() for n in self.names}
            self.ema_updates = 0

    def ema_state_dict(self):
        if self.ema is None:
            raise ValueError("no weight average is kept (set_ema)")
        return {n: (self.ema[n] if n in self.ema else v).copy() for n, v in self.values.items()}

    def ema_state(self):
        if self.ema is None:
            raise ValueError("no weight average is kept (set_ema)")
        return {"ema/num_updates": np.asarray(self.ema_updates, dtype=np.int64), **{f"ema/{n}": self.ema[n].copy() for n in self.names}}

    def load_ema_state(self, st):
        if self.ema is None:
            raise ValueError("no weight average is kept (set_ema) to load into")
        for n in self.names:
            arr = np.ascontiguousarray(st[f"ema/{n}"], dtype=np.float32)
            if arr.size != self.ema[n].size:
                raise ValueError(f"averaged {n}: {arr.size} values for a parameter of {self.ema[n].size}")
            self.ema[n] = arr.reshape(self.spec[n]).copy()
        self.ema_updates = int(np.asarray(st["ema/num_updates"]).reshape(-1)[0])
