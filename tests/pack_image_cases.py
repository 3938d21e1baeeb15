"""The conv weight packers' images, case by case (plain helper, no test in it): the shared case list of tests/test_gpu_pack_images.py and
of the recorder tests/golden/make_pack_images.py, so that the commit that recorded tests/golden/pack_images.json and every later one pack the
same floats.

A case is one call of one packer entry of the C ABI.  Its inputs come from numpy.random.default_rng seeded by the case itself (entry,
taps, cin, cout); `run_case` packs them into a guarded buffer (tests/guarded_buffers.py) of exactly the queried size that starts out as
sentinel words, checks the guard bands and that the inputs were not written, and returns (queried bytes, SHA-256 of the image).

Shapes: (cin, cout) = (4, 8) one chunk and one column tile, both padded; (20, 72) a half-empty second chunk (also a half-empty skip pair) and
two column tiles; (48, 130) three chunks (an odd number for the skip pairs) and three column tiles.  Every entry that takes in_scale runs
without and with it, every entry that takes w_exp with 0, -3 and 9.

dm3d_pack_weights_up_h3 / dm3d_pack_weights_convt_h3 write the layout dm3d_conv_weight_layout names, and DM3D_CONV_PAIR=0 (read once per
process) turns that into DM3D_WL_TAP: `tap_layout_child` runs their cases once more in one fresh interpreter with that variable set
(this file is its program: `python pack_image_cases.py --tap-child` prints the records as JSON)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

SHAPES = ((4, 8), (20, 72), (48, 130))
W_EXPS = (0, -3, 9)
PLAIN, UP, CONVT = 0, 1, 2          # which Keras kernel an entry reads: [taps][cin][cout], [27][cin][cout], [64][cout][cin]

# entry -> (size query, bytes per queried unit, kernel kind, takes taps, takes w_exp, takes in_scale)
ENTRIES = {
    "dm3d_pack_weights":          ("dm3d_packed_weight_elems", 4, PLAIN, True, False, True),
    "dm3d_pack_weights_h3":       ("dm3d_packed_weight_h3_bytes", 1, PLAIN, True, True, True),
    "dm3d_pack_weights_h3p":      ("dm3d_packed_weight_h3p_bytes", 1, PLAIN, True, True, True),
    "dm3d_pack_weights_h3w":      ("dm3d_packed_weight_h3w_bytes", 1, UP, False, True, True),
    "dm3d_pack_weights_up":       ("dm3d_packed_weight_up_elems", 4, UP, False, False, False),
    "dm3d_pack_weights_convt":    ("dm3d_packed_weight_up_elems", 4, CONVT, False, False, False),
    "dm3d_pack_weights_up_h3":    ("dm3d_packed_weight_up_h3_bytes", 1, UP, False, True, False),
    "dm3d_pack_weights_convt_h3": ("dm3d_packed_weight_up_h3_bytes", 1, CONVT, False, True, False),
    "dm3d_pack_weights_skip_h3p": ("dm3d_packed_weight_skip_h3p_bytes", 1, PLAIN, False, True, False),
    "dm3d_pack_weights_skip_h3f": ("dm3d_packed_weight_skip_h3p_bytes", 1, PLAIN, False, True, False),
}
LAYOUT_ENTRIES = ("dm3d_pack_weights_up_h3", "dm3d_pack_weights_convt_h3")       # the two that ask dm3d_conv_weight_layout


def _case(entry, cin, cout, taps=None, mode=None, w_exp=None, scaled=False):
    name = entry[len("dm3d_pack_weights"):].lstrip("_") or "f32"
    name += f" cin{cin} cout{cout}"
    if taps is not None:
        name += f" taps{taps}"
    if mode is not None:
        name += f" mode{mode}"
    if w_exp is not None:
        name += f" e{w_exp}"
    if scaled:
        name += " in_scale"
    return dict(name=name, entry=entry, cin=cin, cout=cout, taps=taps, mode=mode, w_exp=w_exp, scaled=scaled)


def _cases():
    out = []
    for cin, cout in SHAPES:
        for scaled in (False, True):
            for taps in (1, 27, 64):
                out.append(_case("dm3d_pack_weights", cin, cout, taps=taps, scaled=scaled))
                out += [_case("dm3d_pack_weights_h3", cin, cout, taps=taps, w_exp=e, scaled=scaled) for e in W_EXPS]
            for taps, mode in ((1, 0), (27, 0), (8, 1), (8, 2)):
                out += [_case("dm3d_pack_weights_h3p", cin, cout, taps=taps, mode=mode, w_exp=e, scaled=scaled) for e in W_EXPS]
            out += [_case("dm3d_pack_weights_h3w", cin, cout, w_exp=e, scaled=scaled) for e in W_EXPS]
        out += [_case("dm3d_pack_weights_up", cin, cout), _case("dm3d_pack_weights_convt", cin, cout)]
        for entry in LAYOUT_ENTRIES + ("dm3d_pack_weights_skip_h3p", "dm3d_pack_weights_skip_h3f"):
            out += [_case(entry, cin, cout, w_exp=e) for e in W_EXPS]
    return out


CASES = _cases()
TAP_CASES = [c for c in CASES if c["entry"] in LAYOUT_ENTRIES]

# every size query at a non-positive argument: the answer is 0
QUERY_CASES = [(q, args) for q, base in (("dm3d_packed_weight_elems", (27, 4, 8)), ("dm3d_packed_weight_h3_bytes", (27, 4, 8)),
                                         ("dm3d_packed_weight_h3p_bytes", (27, 4, 8)), ("dm3d_packed_weight_up_elems", (4, 8)),
                                         ("dm3d_packed_weight_up_h3_bytes", (4, 8)), ("dm3d_packed_weight_h3w_bytes", (4, 8)),
                                         ("dm3d_packed_weight_skip_h3p_bytes", (4, 8)))
               for i in range(len(base)) for bad in (0, -3) for args in (base[:i] + (bad,) + base[i + 1:],)]


def query_key(query, args):
    return f"{query}({', '.join(map(str, args))})"


def inputs(case):
    """(kernel, in_scale or None) of a case: float32, seeded by the case.  The kernel kind decides the Keras shape."""
    entry, cin, cout = case["entry"], case["cin"], case["cout"]
    kind = ENTRIES[entry][2]
    if case["mode"] in (UP, CONVT):
        kind = case["mode"]
    rng = np.random.default_rng([list(ENTRIES).index(entry), case["taps"] or 0, case["mode"] or 0, cin, cout])
    shape = {PLAIN: (case["taps"] or 1, cin, cout), UP: (27, cin, cout), CONVT: (64, cout, cin)}[kind]
    kernel = (rng.standard_normal(shape) * 0.1).astype(np.float32)
    scale = (rng.random(cin) + 0.5).astype(np.float32)
    return kernel, (scale if case["scaled"] else None)


def run_case(lib, dev, case):
    """Packs one case on `dev` through the ctypes handle `lib` (dm3d_amd._lib): (queried bytes, SHA-256 hex digest of the image)."""
    from guarded_buffers import IN, OUT, Guarded
    entry, cin, cout, taps = case["entry"], case["cin"], case["cout"], case["taps"]
    query, unit, _, has_taps, has_exp, has_scale = ENTRIES[entry]
    h = lib.lib()
    nbytes = unit * getattr(h, query)(*(((taps,) if has_taps else ()) + (cin, cout)))
    if case["mode"] in (UP, CONVT):                    # eight parity images of eight taps
        nbytes *= 8
        assert nbytes == h.dm3d_packed_weight_up_h3_bytes(cin, cout)
    assert nbytes > 0 and nbytes % 4 == 0, nbytes
    kernel, scale = inputs(case)
    bk = Guarded(kernel, dev, IN)
    bs = Guarded(scale, dev, IN) if scale is not None else None
    img = Guarded(np.zeros(nbytes // 4, np.int32), dev, OUT)
    img.t.fill_(img.fill)                              # the window starts out as sentinel words too: what the packer leaves unwritten shows
    args = (bk.ptr,) + ((taps,) if has_taps else ()) + (cin, cout) + ((case["w_exp"],) if has_exp else ())
    args += ((bs.ptr if bs else None,) if has_scale else ()) + (img.ptr,)
    args += (case["mode"],) if entry == "dm3d_pack_weights_h3p" else ()
    lib.check(getattr(h, entry)(*args, None), entry)
    image = img.get()                                  # (asserts the guard bands)
    bk.unchanged()
    if bs:
        bs.unchanged()
    return int(nbytes), hashlib.sha256(image.tobytes()).hexdigest()


def run_queries(lib):
    return {query_key(q, a): int(getattr(lib.lib(), q)(*a)) for q, a in QUERY_CASES}


def _device():
    import torch
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    return _lib, torch.device("cuda:0")


def tap_layout_child(timeout=300):
    """The TAP_CASES in one fresh interpreter under DM3D_CONV_PAIR=0: {case name: [bytes, digest]}.  The child has its own time limit and
    its exit status is checked."""
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, here, "--tap-child"], env=dict(os.environ, DM3D_CONV_PAIR="0"), capture_output=True, text=True,
                       timeout=timeout, cwd=os.path.dirname(os.path.dirname(here)))
    assert r.returncode == 0, f"tap-layout child exited with {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    assert sys.argv[1:] == ["--tap-child"] and os.environ.get("DM3D_CONV_PAIR") == "0"
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
    lib_, dev_ = _device()
    assert lib_.lib().dm3d_conv_weight_layout(3, 1, 1, 0, 64) == lib_.WL_TAP and lib_.lib().dm3d_conv_weight_layout(4, 2, 0, 1, 64) == lib_.WL_TAP
    print(json.dumps({c["name"]: list(run_case(lib_, dev_, c)) for c in TAP_CASES}))
