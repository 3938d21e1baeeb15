"""tests/golden/attn_block_bits.json itself, without a GPU: it holds the cases of tests/golden/make_attn_block_bits.py and nothing else,
with their seeds, and every output has one digest for the whole buffer and one per 32-row block of the shape its case gives it."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_attn_block_bits", os.path.join(HERE, "golden", "make_attn_block_bits.py"))
mab = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mab)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "golden", "attn_block_bits.json")) as f:
        return json.load(f)


def test_the_case_list():
    ids = set(mab.CASES)
    assert {f"front-m{m}-mr{mr}" for m, mr in ((64, 1), (64, 2), (128, 2))} <= ids
    assert {f"mlp-m{m}-{f}" for m in (64, 200) for f in ("f32-res", "f32-nores", "h2out", "tail-res3", "tail-nores3")} <= ids
    assert {"tile-front-n256", "tile-front-n512", "tile-mlp-which0", "tile-mlp-which1"} <= ids and len(ids) == 17


def _rows(case_id, name):
    spec = mab.CASES[case_id]
    if spec["kind"] == "front":
        return mab.U if name == "vt" else spec["m"]
    if spec["kind"] == "mlp":
        return spec["m"]
    return (spec["n"] if spec["kind"] == "tile_front" else 4 * mab.U) * mab.U // 256       # images are digested as rows of 256 words


@pytest.mark.parametrize("case_id", list(mab.CASES))
def test_recorded_case(recorded, case_id):
    assert set(recorded) == set(mab.CASES)
    rec = recorded[case_id]
    assert rec["seed"] == mab.seed_of(case_id)
    kind = mab.CASES[case_id]["kind"]
    assert set(rec["outputs"]) == (set(mab.FRONT_OUTPUTS) if kind == "front" else {"out"} if kind == "mlp" else {"image"})
    for name, d in rec["outputs"].items():
        assert len(d["blocks"]) == -(-_rows(case_id, name) // 32)
        assert all(re.fullmatch(r"[0-9a-f]{64}", h) for h in [d["all"], *d["blocks"]])


def test_digests_name_the_block():
    buf = np.arange(70 * 8, dtype=np.int32).reshape(70, 8)
    a = mab.digests(buf)
    buf[40, 3] ^= 1
    b = mab.digests(buf)
    assert len(a["blocks"]) == 3 and a["all"] != b["all"] and [x != y for x, y in zip(a["blocks"], b["blocks"])] == [False, True, False]
