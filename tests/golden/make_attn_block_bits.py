"""Records tests/golden/attn_block_bits.json: the bits dm3d_attn_front, dm3d_mlp_fused (with and without its proj_out tail) and the two
weight tilers leave at the smallest shapes at which they can go wrong, so that a change to dm3d_attn_front_h3.hip / dm3d_mlp_h3.hip /
dm3d_frag.h can be held against the commit before it.  The kernels are deterministic, so the same code gives the same bytes.  The file
holds SHA-256 digests only: one per output buffer (leading-dimension gaps included: they stay zero) and one per 32-row block of it, so a
mismatch names the tile.  tests/test_gpu_attn_block_bits.py replays every case through ``run_case``; tests/test_attn_block_bits_host.py
checks the recording itself without a GPU.

    python tests/golden/make_attn_block_bits.py [--root TREE] [--out FILE]

``--root TREE`` imports the package of another tree (an export of the commit to record, built there); DM3D_LIB selects another build of
the library under this tree's bindings.  Inputs and weights are not stored: they are drawn from the seed the file keeps.  Needs a GPU.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
U = 256
FRONT_OUTPUTS = ("y", "qk", "vt", "q2", "n3")
# form -> (H2 output, residuals res + res2, tail, res3)
MLP_FORMS = {"f32-res": (False, True, False, False), "f32-nores": (False, False, False, False), "h2out": (True, True, False, False),
             "tail-res3": (False, True, True, True), "tail-nores3": (False, True, True, False)}

CASES = {}
for _m, _mr in ((64, 1), (64, 2), (128, 2)):            # two 32-row workgroups; one 64-row workgroup; two of them (a non-zero blockIdx)
    CASES[f"front-m{_m}-mr{_mr}"] = dict(kind="front", m=_m, mr=_mr)
for _m in (64, 200):                                    # one full workgroup; four, the last with 8 live rows (its padding rows re-read row m - 1)
    for _form in MLP_FORMS:
        CASES[f"mlp-m{_m}-{_form}"] = dict(kind="mlp", m=_m, form=_form)
for _n in (256, 512):                                   # 512: the second pass of the image
    CASES[f"tile-front-n{_n}"] = dict(kind="tile_front", n=_n)
for _which in (0, 1):
    CASES[f"tile-mlp-which{_which}"] = dict(kind="tile_mlp", which=_which)


def seed_of(case_id):
    return zlib.crc32(case_id.encode())


def h2_encode(x):
    """float32 [..., k] -> the uint32 words of its DM3D_FMT_H2 rows (tests/guarded_buffers.py has the same function for the parity tests)."""
    x = np.asarray(x, np.float32)
    k = x.shape[-1]
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    rec = np.stack([hi.reshape(x.shape[:-1] + (k // 16, 2, 8)), lo.reshape(x.shape[:-1] + (k // 16, 2, 8))], -3)
    return np.ascontiguousarray(rec).view(np.uint32).reshape(x.shape[:-1] + (k,))


def digests(buf):
    """buf: numpy [rows][ld] of 4-byte words as the device holds it -> {"all": sha, "blocks": [sha of rows 32 i .. 32 i + 31]}"""
    b = np.ascontiguousarray(buf)
    return dict(all=hashlib.sha256(b.tobytes()).hexdigest(), blocks=[hashlib.sha256(b[i:i + 32].tobytes()).hexdigest() for i in range(0, b.shape[0], 32)])


def _f32(rng, *shape, std=1.0):
    return (rng.standard_normal(shape) * std).astype(np.float32)


def _padded(arr, ld):
    out = np.zeros((arr.shape[0], ld), arr.dtype)
    out[:, :arr.shape[1]] = arr
    return out


def _launch_once(case_id):
    import torch
    from dm3d_amd import _lib
    spec, rng = CASES[case_id], np.random.default_rng(seed_of(case_id))
    lib, dev, keep = _lib.lib(), torch.device("cuda:0"), []

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t

    def zeros(rows, ld):
        return up(np.zeros((rows, ld), np.int32))

    def tiled(w, entry, *args):
        words = h2_encode(w)
        src, img = up(words), zeros(1, words.size)
        _lib.check(getattr(lib, entry)(src.data_ptr(), *args, img.data_ptr(), None), entry)
        return img

    kind, outs = spec["kind"], {}
    if kind == "tile_front":
        outs["image"] = tiled(_f32(rng, spec["n"], U, std=1 / 16), "dm3d_pack_front_weights", spec["n"], U).view(-1, 256)
    elif kind == "tile_mlp":
        shape = (4 * U, U) if spec["which"] == 0 else (U, 4 * U)
        outs["image"] = tiled(_f32(rng, *shape, std=1 / 16), "dm3d_pack_mlp_weights", U, spec["which"]).view(-1, 256)
    elif kind == "front":
        m = spec["m"]
        os.environ["DM3D_FRONT_MR"] = str(spec["mr"])             # read per call
        ld = dict(x=U + 4, y=U + 8, qk=2 * U + 16, vt=m + 16, q2=U + 16, n3=U + 32)       # the leading dimensions of tests/test_gpu_infer_kernels.py
        rows = dict(y=m, qk=m, vt=U, q2=m, n3=m)
        d = _lib.AttnFrontDesc()
        x = up(_padded(_f32(rng, m, U, std=2.0), ld["x"]))
        d.x, d.ldx = x.data_ptr(), ld["x"]
        d.w_in = tiled(_f32(rng, U, U, std=1 / 16), "dm3d_pack_front_weights", U, U).data_ptr()
        d.w_qk = tiled(_f32(rng, 2 * U, U, std=1 / 16), "dm3d_pack_front_weights", 2 * U, U).data_ptr()
        d.w_v = tiled(_f32(rng, U, U, std=1 / 16), "dm3d_pack_front_weights", U, U).data_ptr()
        d.b_in, d.b_qk, d.b_v = (up(_f32(rng, n, std=0.1)).data_ptr() for n in (U, 2 * U, U))
        for i in (1, 2, 3):
            setattr(d, f"g{i}", up((rng.random(U) + 0.5).astype(np.float32)).data_ptr())
            setattr(d, f"be{i}", up(_f32(rng, U, std=0.2)).data_ptr())
        d.eps, d.m, d.units = 1e-3, m, U
        for k in FRONT_OUTPUTS:
            outs[k] = zeros(rows[k], ld[k])
            setattr(d, k, outs[k].data_ptr())
            setattr(d, "ld" + k, ld[k])
        _lib.check(lib.dm3d_attn_front(C.byref(d), None), "attn_front")
        os.environ.pop("DM3D_FRONT_MR")
    else:
        m = spec["m"]
        out_h2, has_res, tail, has_r3 = MLP_FORMS[spec["form"]]
        ldx, ldr, ldr3, ldo = U + 16, U + 4, U + 8, (U + 16 if out_h2 else U + 12)
        d = _lib.MlpDesc()
        d.x, d.ldx = up(_padded(h2_encode(_f32(rng, m, U)), ldx)).data_ptr(), ldx
        d.w0 = tiled(_f32(rng, 4 * U, U, std=1 / 16), "dm3d_pack_mlp_weights", U, 0).data_ptr()
        d.w1 = tiled(_f32(rng, U, 4 * U, std=1 / 32), "dm3d_pack_mlp_weights", U, 1).data_ptr()
        d.b0, d.b1 = up(_f32(rng, 4 * U, std=0.1)).data_ptr(), up(_f32(rng, U, std=0.1)).data_ptr()
        r1, r2, r3 = (_padded(_f32(rng, m, U), ld_) for ld_ in (ldr, ldr, ldr3))      # always drawn: a form's stream does not depend on its residuals
        if has_res:
            d.res, d.res2, d.ldr = up(r1).data_ptr(), up(r2).data_ptr(), ldr
        w2, b2 = _f32(rng, U, U, std=1 / 16), _f32(rng, U, std=0.1)
        if tail:
            d.w2, d.b2 = tiled(w2, "dm3d_pack_front_weights", U, U).data_ptr(), up(b2).data_ptr()
            if has_r3:
                d.res3, d.ldr3 = up(r3).data_ptr(), ldr3
        outs["out"] = zeros(m, ldo)
        d.out, d.ldo, d.out_fmt, d.m, d.units = outs["out"].data_ptr(), ldo, (_lib.FMT_H2 if out_h2 else _lib.FMT_F32), m, U
        _lib.check(lib.dm3d_mlp_fused(C.byref(d), None), "mlp_fused")
    torch.cuda.synchronize()
    return {k: digests(v.cpu().numpy()) for k, v in outs.items()}


def run_case(case_id):
    """One case on the device, twice: (the record the golden file keeps for it, whether the two runs were equal)."""
    first, again = _launch_once(case_id), _launch_once(case_id)
    return dict(seed=seed_of(case_id), outputs=first), first == again


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT, help="the tree whose package is imported")
    ap.add_argument("--out", default=os.path.join(HERE, "attn_block_bits.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    out = {}
    for case_id in CASES:
        rec, repeats = run_case(case_id)
        assert repeats, f"{case_id}: two runs differ at this commit"
        out[case_id] = rec
        print(f"{case_id}: " + " ".join(f"{k}={v['all'][:12]}" for k, v in rec["outputs"].items()), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: {len(out)} cases, {os.path.getsize(args.out)} bytes (library {_lib.LIB_PATH})")


if __name__ == "__main__":
    main()
