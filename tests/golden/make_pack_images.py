"""Records tests/golden/pack_images.json: per case of tests/pack_image_cases.py the byte count its size query returned and the SHA-256 of
the image the packer wrote, on the MI355X, at the commit named on the command line (the recorded file says which).

    python tests/golden/make_pack_images.py <commit the working tree is at>

Keys: "commit"; "queries" (every size query at a non-positive argument); "images" (every case in this process, the default
DM3D_WL_PAIR layout of the two entries that ask dm3d_conv_weight_layout); "images_tap_layout" (those two entries' cases again in a fresh
process under DM3D_CONV_PAIR=0).  The file pins what the packers wrote when it was recorded: re-record it only with a change that means
to move bytes of an image, and say which."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import pack_image_cases as pic  # noqa: E402


def main():
    assert len(sys.argv) == 2, __doc__
    assert os.environ.get("DM3D_CONV_PAIR") != "0", "record the default layout in this process; the tap-layout child sets the variable itself"
    lib, dev = pic._device()
    rec = {"commit": sys.argv[1], "queries": pic.run_queries(lib),
           "images": {c["name"]: list(pic.run_case(lib, dev, c)) for c in pic.CASES},
           "images_tap_layout": pic.tap_layout_child()}
    assert len(rec["images"]) == len(pic.CASES), "case names must be unique"
    out = os.path.join(HERE, "pack_images.json")
    with open(out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(rec['images'])} images, {len(rec['images_tap_layout'])} tap-layout images, {len(rec['queries'])} queries")


if __name__ == "__main__":
    main()
