"""The weight lifecycle of DiffusionModel against a recording of it (CPU only).

tests/golden/weight_sets_trace.json holds what a caller observed, operation by operation, when the model still kept its live and
averaged weights in nine loose attributes (tools/weight_sets_trace.py: the operations, the sequences, the record format and the
recorder; tests/weight_sets_standin.py: the host-only Trainer both use).  ``WeightSets`` must show the same: every exception and message,
every digest, key count and dtype, _has_ema() and the existence of a Trainer, with no more reloads of the network in any operation than
were recorded, and with its own rules (``_check``) holding after every operation."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("weight_sets_trace", os.path.join(ROOT, "tools", "weight_sets_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
with open(TOOL.GOLDEN) as _f:
    GOLDEN = json.load(_f)


def test_the_recording_is_the_tools_and_covers_the_issue():
    assert GOLDEN["sequences"] == TOOL.sequences() and [len(r) for r in GOLDEN["records"]] == [len(s) for s in GOLDEN["sequences"]]
    for op in TOOL.OPS:
        assert sum(seq.count(op) for seq in GOLDEN["sequences"]) >= 5, op
    assert sorted(map(tuple, GOLDEN["visited"])) == sorted(TOOL.COMBINATIONS)
    assert os.path.getsize(TOOL.GOLDEN) < 64 * 1024


def test_replay_matches_the_recording(monkeypatch):
    import dm3d_amd.train
    from test_ema_host import _model
    from weight_sets_standin import HostTrainer
    monkeypatch.setattr(dm3d_amd.train, "Trainer", HostTrainer)
    records, visited = [], set()
    for seq in GOLDEN["sequences"]:
        d = TOOL.Driver(lambda: _model(context_dim=2))
        assert isinstance(d.side, TOOL._Owned)
        records.append([d.run(op) for op in seq])               # (run() calls weights._check() after every operation)
        visited |= d.visited
    bad = TOOL.differences(GOLDEN, json.loads(json.dumps(records)))
    assert not bad, f"{len(bad)} operations differ:\n" + "\n".join(bad[:10])
    assert sorted(visited) == sorted(TOOL.COMBINATIONS)


def test_check_raises_on_a_broken_rule():
    from test_ema_host import _model
    w = _model(context_dim=2).weights
    w._check()
    for field, value in (("held", "ema"), ("want", "ema"), ("parked_live", {}), ("dirty", True), ("held", "both")):
        keep = getattr(w, field)
        setattr(w, field, value)
        with pytest.raises(AssertionError, match="weight sets"):
            w._check()
        setattr(w, field, keep)
    w._check()
