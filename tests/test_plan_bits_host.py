"""tests/golden/plan_bits.json itself, without a GPU: it holds the fifteen cases of tests/golden/make_plan_bits.py and nothing else, every
recorded plan took the path its case is there for, and the stored bytes are the ones the digests name — so that a recording made from a
plan that never reached the fused, fall-back, float32, GroupNorm or hand-off arm cannot become the standard of test_gpu_plan_bits.py."""
import hashlib
import importlib.util
import json
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_plan_bits", os.path.join(HERE, "golden", "make_plan_bits.py"))
mpb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mpb)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "golden", "plan_bits.json")) as f:
        return json.load(f)


def test_the_recording_holds_the_fifteen_cases(recorded):
    assert len(mpb.CASES) == 15 and set(recorded) == set(mpb.CASES)
    for case_id, rec in recorded.items():
        assert rec["seed"] == mpb.seed_of(case_id), case_id


@pytest.mark.parametrize("case_id", list(mpb.CASES))
def test_recorded_case(recorded, case_id):
    rec = recorded[case_id]
    assert rec["launches"] and all(len(launch) == 5 and launch[0] for launch in rec["launches"])
    kinds = mpb.kinds_of(rec["launches"])
    assert kinds == rec["count"]
    assert mpb.expect_failures(case_id, kinds, rec["final_h2in"]) == []
    assert re.fullmatch(r"[0-9a-f]{64}", rec["sha256"])         # every case repeated at the recorded commit: none lacks its digest
    if "eps_hex" in rec:
        eps = bytes.fromhex(rec["eps_hex"])
        assert 0 < len(eps) <= mpb.FULL_BYTES and hashlib.sha256(eps).hexdigest() == rec["sha256"]
    assert isinstance(rec["uses_wino"], bool) and rec["range_limit"] >= 1.0


def test_expect_rules_can_fail():
    """The rule checker itself: a plan without the fused launches, or with an unequal pair, or the wrong final hand-off, is reported."""
    assert mpb.expect_failures("01-wide-fused", {"attn_front": 4, "attn_fused": 4, "mlp_fused": 4}, False) == []
    assert mpb.expect_failures("01-wide-fused", {"attn_front": 4, "gemm_h3": 4}, False) == ["no attn_fused", "no mlp_fused", "has gemm_h3"]
    assert mpb.expect_failures("04-wide-no-tail", {"mlp_fused": 4, "gemm_h3": 3}, False) == ["gemm_h3 x3 != mlp_fused x4"]
    assert mpb.expect_failures("14-res-handoff", {"conv_k3s1": 2}, False) == ["no *_h2in", "final_h2in is False"]
    assert mpb.expect_failures("15-res-no-handoff", {"conv_wino_h2in": 1}, False) == ["has *_h2in"]
