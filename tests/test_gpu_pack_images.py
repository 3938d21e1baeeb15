"""Every conv weight packer of the C ABI, bitwise: each case of tests/pack_image_cases.py packs into a guarded buffer of exactly the queried
size, and the queried size and the SHA-256 of the image must be those recorded in tests/golden/pack_images.json (recorded once on the MI355X
by tests/golden/make_pack_images.py at the commit that file names).  A change to a packer that moves one byte of one image fails the case
that names the entry, the shape, the taps, the exponent and whether in_scale was given.  The guard bands around the image must be intact and
the inputs unwritten (run_case asserts both).

dm3d_pack_weights_up_h3 / dm3d_pack_weights_convt_h3 write the layout dm3d_conv_weight_layout names; their DM3D_WL_TAP branch runs in one
fresh child process under DM3D_CONV_PAIR=0 (read once per process) and has digests of its own."""
import json
import os

import pytest

import pack_image_cases as pic

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_images.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def ctx():
    return pic._device()


def test_case_list_is_the_recorded_one():
    assert sorted(GOLDEN["images"]) == sorted(c["name"] for c in pic.CASES)
    assert sorted(GOLDEN["images_tap_layout"]) == sorted(c["name"] for c in pic.TAP_CASES)
    assert sorted(GOLDEN["queries"]) == sorted(pic.query_key(q, a) for q, a in pic.QUERY_CASES)


def test_size_queries_at_non_positive_arguments(ctx):
    got = pic.run_queries(ctx[0])
    assert got == GOLDEN["queries"] and set(got.values()) == {0}


@pytest.mark.parametrize("case", pic.CASES, ids=[c["name"] for c in pic.CASES])
def test_pack_image(ctx, case):
    lib, dev = ctx
    key = "images"
    if case["entry"] in pic.LAYOUT_ENTRIES and lib.lib().dm3d_conv_weight_layout(3, 1, 1, 0, case["cout"]) == lib.WL_TAP:
        key = "images_tap_layout"                    # (this process itself runs under DM3D_CONV_PAIR=0)
    nbytes, digest = pic.run_case(lib, dev, case)
    want_bytes, want_digest = GOLDEN[key][case["name"]]
    assert nbytes == want_bytes
    assert digest == want_digest, f"{case['name']}: the image differs from the one recorded at {GOLDEN['commit']}"


def test_pack_image_tap_layout_child(ctx):
    got = pic.tap_layout_child()
    assert got == GOLDEN["images_tap_layout"], sorted(k for k in GOLDEN["images_tap_layout"] if got.get(k) != GOLDEN["images_tap_layout"][k])
