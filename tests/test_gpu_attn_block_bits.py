"""dm3d_attn_front, dm3d_mlp_fused and the two weight tilers against the bits they left at the commit before their shared parts moved
into csrc/dm3d_frag.h (tests/golden/attn_block_bits.json, written by tests/golden/make_attn_block_bits.py, which also holds the cases and
runs them): every output buffer and every 32-row block of it has the recorded SHA-256, so a mismatch names the output and the tile.
tests/test_attn_block_bits_host.py checks the recording itself."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_attn_block_bits", os.path.join(HERE, "golden", "make_attn_block_bits.py"))
mab = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mab)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "golden", "attn_block_bits.json")) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", list(mab.CASES))
def test_bits_replay(recorded, case_id, monkeypatch):
    import torch
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    monkeypatch.delenv("DM3D_FRONT_MR", raising=False)
    want = recorded[case_id]
    got, repeats = mab.run_case(case_id)
    assert repeats, f"{case_id}: two runs differ"
    assert got["seed"] == want["seed"] and set(got["outputs"]) == set(want["outputs"])
    for name, w in want["outputs"].items():
        g = got["outputs"][name]
        bad = [i for i, (a, b) in enumerate(zip(g["blocks"], w["blocks"])) if a != b]
        assert len(g["blocks"]) == len(w["blocks"]) and not bad, f"{case_id}: {name} differs from the recording in 32-row blocks {bad}"
        assert g["all"] == w["all"], f"{case_id}: {name} differs from the recording"
