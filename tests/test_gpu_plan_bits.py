"""The plan builder against what it built at the commit before its attention half was rewritten (tests/golden/plan_bits.json, written
by tests/golden/make_plan_bits.py, which also holds the fifteen cases and runs them): the same launches in the same order with the same
descriptions and FLOP / byte counts, the same kind counts, ``uses_wino`` and ``range_limit``, and, the kernels being deterministic,
the same bytes in ``eps``.  tests/test_plan_bits_host.py checks the recording itself."""
import hashlib
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_plan_bits", os.path.join(HERE, "golden", "make_plan_bits.py"))
mpb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mpb)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "golden", "plan_bits.json")) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", list(mpb.CASES))
def test_plan_and_eps_replay(recorded, case_id, monkeypatch):
    import torch
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    for k in mpb.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in mpb.CASES[case_id]["env"].items():
        monkeypatch.setenv(k, v)
    want = recorded[case_id]
    rec, eps = mpb.run_case(case_id)
    got = json.loads(json.dumps(rec))                        # tuples as lists, as the file has them
    assert got.pop("repeats"), f"{case_id}: two forwards of one net differ"
    assert got["seed"] == want["seed"]
    assert len(got["launches"]) == len(want["launches"]), (got["count"], want["count"])
    for i, (g, w) in enumerate(zip(got["launches"], want["launches"])):
        assert g == w, f"{case_id}: launch {i} is {g}, recorded {w}"
    for k in ("count", "uses_wino", "range_limit", "final_h2in"):
        assert got[k] == want[k], (case_id, k, got[k], want[k])
    if "sha256" in want:                                     # (left out only where eps did not repeat at the recorded commit)
        assert got["sha256"] == want["sha256"], f"{case_id}: eps differs from the recording"
    if "eps_hex" in want:
        assert eps == bytes.fromhex(want["eps_hex"]) and hashlib.sha256(eps).hexdigest() == want["sha256"]
