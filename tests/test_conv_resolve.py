"""The conv queries of the C ABI (dm3d_conv_tile_form, dm3d_conv_scratch_bytes, dm3d_conv_split_counter_words) against a recording.

The launch and the three queries read one resolved description of a conv (dm3d_conv_resolve, csrc/dm3d_conv.hip).  tests/golden/conv_resolve.json
holds what the library answered, before that function existed, for a grid of 1969 descriptors (tools/conv_resolve_grid.py: the grid, the
file format and the recorder), and for a 50-row sub-grid under each policy knob of the environment.  The answers must be the same value
for value, with one deliberate exception: a DM3D_WL_PAIR k3 / stride-1 descriptor with cout <= 32 now answers form 4 — the narrow 4-slice forms the
launch runs and include/dm3d.h documents — where the recording named the wide form's brick depth (flagged rows; their recorded value stays
in the file).  No device is needed: the queries only read the descriptor."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("conv_resolve_grid", os.path.join(ROOT, "tools", "conv_resolve_grid.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
with open(TOOL.GOLDEN) as _f:
    GOLDEN = json.load(_f)
NCOL = len(TOOL.COLUMNS)


def _expected(recorded):
    form, nbytes, words, narrow = recorded
    return [4 if narrow else form, nbytes, words, narrow]


def _mismatches(rows, answers):
    return [(row[:NCOL], got, _expected(row[NCOL:])) for row, got in zip(rows, answers) if got != _expected(row[NCOL:])]


def test_the_recorded_grid_is_the_grid_of_the_tool():
    assert [tuple(r[:NCOL]) for r in GOLDEN["rows"]] == TOOL.grid() and GOLDEN["sub"] == TOOL.sub_grid(TOOL.grid())
    assert len(GOLDEN["rows"]) <= 2000 and os.path.getsize(TOOL.GOLDEN) < 200 * 1024
    assert sorted(GOLDEN["env"]) == sorted(TOOL.ENV_KEYS) and all(len(v) == 50 for v in GOLDEN["env"].values())


def test_queries_answer_as_recorded(built_library, monkeypatch):
    for key in TOOL.ENV_KEYS:
        monkeypatch.delenv(key.split("=")[0], raising=False)
    mod = TOOL.load_lib_module()
    handle = TOOL.open_lib(mod, built_library)
    answers = [TOOL.query(mod, handle, tuple(r[:NCOL])) for r in GOLDEN["rows"]]
    bad = _mismatches(GOLDEN["rows"], answers)
    assert not bad, f"{len(bad)} of {len(answers)} descriptors (descriptor, answer, expected): {bad[:5]}"
    # the rows measured by hand on the library of record: the U-Net's conv_in / conv_out at the benchmark shape and the policy's thresholds
    table = [(8, 0, 0), (8, 0, 0), (4, 262144, 2), (10, 33554432, 256), (4, 33554432, 256), (10, 0, 0), (8, 0, 0), (8, 0, 0), (4, 0, 0), (0, 0, 0),
             (4, 0, 0)]
    assert [tuple(r[NCOL:NCOL + 3]) for r in GOLDEN["rows"][:len(table)]] == table
    assert [tuple(a[:3]) for a in answers[:2]] == [(4, 0, 0), (4, 0, 0)]         # conv_in 8 -> 32 and conv_out 64 -> 8: the narrow forms


@pytest.mark.parametrize("env_key", TOOL.ENV_KEYS)
def test_queries_under_a_policy_knob(built_library, monkeypatch, env_key):
    """One fresh process per knob: DM3D_CONV_PAIR, DM3D_CONV_KSPLIT and DM3D_CONV_WINO_SPLIT are read once per process."""
    for key in TOOL.ENV_KEYS:
        monkeypatch.delenv(key.split("=")[0], raising=False)
    monkeypatch.setenv("DM3D_LIB", built_library)
    rows = [GOLDEN["rows"][i][:NCOL] + rec for i, rec in zip(GOLDEN["sub"], GOLDEN["env"][env_key])]
    bad = _mismatches(rows, TOOL.replay(env_key))
    assert not bad, f"{env_key}: (descriptor, answer, expected) {bad[:5]}"
