"""The weight lifecycle of a DiffusionModel as a caller observes it, recorded from one tree and replayed on another.

A ``device="cpu"`` conditional model (``_model(context_dim=2)`` of tests/test_ema_host.py) is driven through fixed sequences of the
operations that move its weights: load_state_dict (plain, with optimizer/ entries, with ema/ entries, with both, non-strict partial, an
invalid partial ema/ set), use_ema, compile(ema_decay=), the first access of ``trainer``, a train step (what train_step does after
loss_and_grad: learning rate, average settings, adam_step, mark trained), the engine request of network(..., training=True), a use of
the sampling network (network.state_dict()) and save_weights to .npz (live and averaged).  dm3d_amd.train.Trainer is replaced by the
host-only stand-in of tests/weight_sets_standin.py, so no device is needed.  After every operation the recorder keeps

    [exception "Type: message" or null, returned value, _has_ema(), whether a Trainer exists, reloads of the network in this operation]

where the returned value of a use is one digest folded over every entry of the state (name, dtype, shape, bytes), and that of a save
is [number of keys, number of optimizer/ keys, number of ema/ keys, digest folded over every key in sorted order].  A reload re-packs
every weight on the device and drops the captured graphs: the reload count is the speed of this code.  The recorder also reports which
combinations of (Trainer: none | built) x (network holds: live | ema) x (average: none | host | trainer) the sequences visited.

    python tools/weight_sets_trace.py record [--tree DIR] [golden.json]    record from the tree DIR (default: this one)
    python tools/weight_sets_trace.py replay [--tree DIR]                  replay and compare with the golden file

tests/golden/weight_sets_trace.json was recorded from the commit before ``WeightSets`` existed (--tree pointing at a checkout of it);
tests/test_weight_sets.py replays it on the current code.  The two spellings of the steps that differ between the trees are the
adapters ``_Loose`` (nine attributes on the model) and ``_Owned`` (model.weights).
"""
import hashlib
import json
import os
import random
import sys
from unittest import mock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "weight_sets_trace.json")
LOADS = ("plain", "opt", "ema", "both", "partial", "bad_ema")
OPS = tuple(f"load:{v}" for v in LOADS) + ("use_ema:1", "use_ema:0", "compile:ema", "compile:none", "trainer", "step", "engine", "use",
                                            "save:live", "save:ema")
# every combination that can occur: an average in the Trainer needs a Trainer, averaged weights in the network need an average -- but for
# ("built", "ema", "none"): a step under compile(ema_decay=None) freed the average the network still holds a copy of
COMBINATIONS = (("none", "live", "none"), ("none", "live", "host"), ("none", "ema", "host"), ("built", "live", "none"),
                ("built", "live", "host"), ("built", "live", "trainer"), ("built", "ema", "host"), ("built", "ema", "trainer"),
                ("built", "ema", "none"))


def sequences():
    """Three written sequences that walk through every combination, and two seeded random walks over all operations."""
    a = ["use", "use_ema:1", "save:ema", "load:ema", "use", "save:live", "use_ema:1", "use", "save:live", "save:ema", "engine", "use",
         "use_ema:0", "use", "load:both", "use_ema:1", "use", "trainer", "use", "step", "use", "compile:ema", "step", "use", "save:live",
         "use_ema:0", "compile:none", "step", "use_ema:1", "use", "load:bad_ema", "load:partial", "use", "save:live", "compile:none", "use"]
    b = ["compile:ema", "trainer", "use", "step", "step", "use", "use_ema:1", "use", "save:live", "compile:none", "step", "use_ema:0",
         "save:ema", "step", "use", "use_ema:1", "load:opt", "trainer", "save:live", "compile:ema", "step", "use_ema:1", "use",
         "load:plain", "use", "engine", "load:ema", "use_ema:1", "use", "load:partial", "use", "load:plain", "use"]
    c = ["load:both", "trainer", "use_ema:1", "use", "engine", "use", "save:ema", "use_ema:0", "use", "compile:ema", "step", "save:live",
         "load:bad_ema", "use_ema:1", "load:opt", "use", "load:ema", "use_ema:1", "load:both", "use", "step", "use", "save:ema",
         "load:partial", "engine", "use", "load:bad_ema", "save:live", "compile:none", "load:partial", "use"]
    out = [a, b, c]
    for seed in (1, 2):
        rng = random.Random(seed)
        out.append([rng.choice(OPS) for _ in range(30)])
    return out


def _digest(items):
    """One digest folded over (name, array) pairs."""
    h = hashlib.sha1()
    for k, v in items:
        v = np.ascontiguousarray(v)
        h.update(f"{k}|{v.dtype}|{v.shape}|".encode())
        h.update(v.tobytes())
    return h.hexdigest()[:16]


class _Loose:
    """The tree whose DiffusionModel keeps the lifecycle in loose attributes."""

    def __init__(self, m):
        self.m, self.held = m, "live"

    def step(self):
        m = self.m
        tr = m.trainer
        tr.lr = m._learning_rate()
        m._configure_ema(tr)
        tr.adam_step()
        m._trainer_dirty = True
        return tr

    def trainer(self):
        return self.m._trainer

    def pending_ema(self):
        return self.m._pending_ema

    def reloaded(self, in_load):
        # every reload outside load_state_dict is _sync_from_trainer's, which loads the set use_ema() named; load_state_dict loads live ones
        self.held = "live" if in_load or not self.m._use_ema else "ema"

    def check(self):
        pass


class _Owned:
    """The tree with model.weights."""

    def __init__(self, m):
        self.m = m

    def step(self):
        m = self.m
        tr = m.weights.ensure_trainer(*m._training_settings(), step=True)
        tr.adam_step()
        m.weights.trained()
        return tr

    def trainer(self):
        return self.m.weights.trainer

    def pending_ema(self):
        return self.m.weights.pending_ema

    def reloaded(self, in_load):
        pass

    held = property(lambda self: self.m.weights.held)

    def check(self):
        self.m.weights._check()


class Driver:
    """One model and the operations on it; ``run(op)`` returns the record of that operation."""

    def __init__(self, make_model):
        self.m = make_model()
        self.side = (_Owned if hasattr(self.m, "weights") else _Loose)(self.m)
        self.init = {k: v.copy() for k, v in self.m.network.state.items()}
        self.names = list(self.m._trainable_names())
        self.loads = self.reloads = 0
        self.in_load = False
        self.visited = set()
        inner = self.m.network.load_state_dict

        def counted(sd, strict=True):
            inner(sd, strict)
            self.reloads += 1
            self.side.reloaded(self.in_load)
        self.m.network.load_state_dict = counted

    def _checkpoint(self, variant):
        """A fresh set of weights (the initial ones, shifted by an exact amount that differs from load to load) with the entries of
        ``variant``."""
        self.loads += 1
        k = np.float32(self.loads * 2.0 ** -5)
        names = list(self.init)[::3] if variant == "partial" else list(self.init)
        sd = {n: self.init[n] + k for n in names}
        if variant in ("opt", "both"):
            sd["optimizer/iter"] = np.asarray(self.loads, dtype=np.int64)
            for n in self.names:
                sd[f"optimizer/m/{n}"], sd[f"optimizer/v/{n}"] = self.init[n] * np.float32(0.5), self.init[n] * self.init[n]
        if variant in ("ema", "both", "bad_ema"):
            sd["ema/num_updates"] = np.asarray(10 + self.loads, dtype=np.int64)
            for n in self.names[3 if variant == "bad_ema" else 0:]:
                sd[f"ema/{n}"] = self.init[n] - k
        return sd

    def _call(self, op):
        m = self.m
        kind, _, arg = op.partition(":")
        if kind == "load":
            self.in_load = True
            try:
                return m.load_state_dict(self._checkpoint(arg), strict=arg != "partial")
            finally:
                self.in_load = False
        if kind == "use_ema":
            return m.use_ema(arg == "1")
        if kind == "compile":
            return m.compile(optimizer=1e-3, ema_decay=0.75 if arg == "ema" else None)
        if kind == "trainer":
            return type(m.trainer).__name__
        if kind == "step":
            tr = self.side.step()
            return [tr.step_count, tr.ema_updates]
        if kind == "engine":
            m.network._fresh()                                  # as network(..., training=True) does before it asks
            return type(m.network._training_engine()).__name__
        if kind == "use":
            return _digest(m.network.state_dict().items())
        assert kind == "save", op
        saved = {}
        with mock.patch.object(np, "savez", lambda path, **arrays: saved.update(arrays)):       # what the file would hold
            m.save_weights("trace.npz", weights=arg)
        keys = sorted(saved)
        return [len(keys), sum(k.startswith("optimizer/") for k in keys), sum(k.startswith("ema/") for k in keys),
                _digest((k, saved[k]) for k in keys)]

    def run(self, op):
        self.reloads = 0
        error = value = None
        try:
            value = self._call(op)
        except Exception as e:
            error = f"{type(e).__name__}: {e}"
        self.side.check()
        tr = self.side.trainer()
        average = "trainer" if tr is not None and tr.ema is not None else "host" if self.side.pending_ema() is not None else "none"
        self.visited.add(("none" if tr is None else "built", self.side.held, average))
        return [error, value, bool(self.m._has_ema()), tr is not None, self.reloads]


def import_tree(tree):
    """``import dm3d_amd`` from ``tree``, with the stand-in Trainer in place of the real one; returns _model of its test_ema_host.py."""
    for p in (os.path.join(ROOT, "tests"), os.path.join(tree, "tests"), tree):         # (the stand-in is this tree's)
        sys.path.insert(0, p)
    import dm3d_amd.train
    from weight_sets_standin import HostTrainer
    from test_ema_host import _model
    assert os.path.dirname(os.path.abspath(dm3d_amd.__file__)).startswith(os.path.abspath(tree)), dm3d_amd.__file__
    dm3d_amd.train.Trainer = HostTrainer
    return lambda: _model(context_dim=2)


def trace(make_model):
    records, visited = [], set()
    for seq in sequences():
        d = Driver(make_model)
        records.append([d.run(op) for op in seq])
        visited |= d.visited
    return records, sorted(visited)


def differences(golden, records):
    """Where a replay departs from the recording: anything but a reload count that went down."""
    out = []
    for s, (seq, want, got) in enumerate(zip(golden["sequences"], golden["records"], records)):
        for i, (op, w, g) in enumerate(zip(seq, want, got)):
            if w[:4] != g[:4] or g[4] > w[4]:
                out.append(f"sequence {s} operation {i} ({op}): recorded {w}, now {g}")
    return out


def main(argv):
    mode, rest = argv[1], argv[2:]
    tree = ROOT
    if rest[:1] == ["--tree"]:
        tree, rest = os.path.abspath(rest[1]), rest[2:]
    path = rest[0] if rest else GOLDEN
    records, visited = trace(import_tree(tree))
    counts = {op: sum(seq.count(op) for seq in sequences()) for op in OPS}
    print("operations:", counts)
    print("combinations visited:", visited)
    print("combinations missed:", [c for c in COMBINATIONS if list(c) not in [list(v) for v in visited]])
    if mode == "record":
        with open(path, "w") as f:
            f.write('{"sequences": %s,\n "visited": %s,\n "records": [\n%s]}\n' % (
                json.dumps(sequences()), json.dumps(visited), ",\n".join(json.dumps(r, separators=(",", ":")) for r in records)))
        print(f"{path}: {sum(map(len, records))} operations, {os.path.getsize(path)} bytes")
        return 0
    assert mode == "replay", mode
    with open(path) as f:
        golden = json.load(f)
    bad = differences(golden, json.loads(json.dumps(records)))
    print("\n".join(bad) if bad else "replay matches the recording")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
