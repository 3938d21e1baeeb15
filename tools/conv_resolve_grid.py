"""The descriptor grid of tests/test_conv_resolve.py and its recorder.

What the three conv queries of the C ABI (dm3d_conv_tile_form, dm3d_conv_scratch_bytes, dm3d_conv_split_counter_words) answer for a grid of
descriptors, recorded from one build of the library and replayed against another: the queries promise callers what dm3d_conv3d_ndhwc will
do (unet.Plan sizes its workspace and picks the float16 range guard from them), so a change of the conv launch policy has to show up here.
No device is needed: the queries only read the descriptor.

    python tools/conv_resolve_grid.py record [golden.json]     write the golden file from the library DM3D_LIB names (default: csrc/)
    python tools/conv_resolve_grid.py replay ENV_KEY            (used by the test) answers of the `env` sub-grid as JSON on stdout, in a
                                                               process that was started with the knob ENV_KEY ("NAME=value") set

File format: {"columns": [...], "rows": [[...], ...], "sub": [row indices], "env": {"NAME=value": [[form, bytes, words, flag], ...]}}.
A row is the descriptor (COLUMNS) followed by form, bytes, words, flag.  flag = 1 marks a DM3D_WL_PAIR k3 / stride-1 descriptor with
cout <= 32: the recorded form is kept, but the library of record named the wide form's brick depth there while the launch runs the narrow
4-slice forms (include/dm3d.h documents 4), so the test asserts 4 for those rows.
"""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "3d-condtional-stable-diffusion_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_resolve.json")

KINDS = ("k3s1", "k3s1_wino", "k3s1_skip", "k3s1_wino_skip_frag", "upsample", "k3s2", "k1", "transpose_k4s2")
FMTS = ("f32", "x1_h2", "out_h2", "post")
COLUMNS = ("batch", "in_d", "in_h", "in_w", "c1", "cout", "kind", "counters", "fmt")
BATCHES, C1S, COUTS = (1, 2, 4, 6, 32), (8, 16, 32, 64, 128, 256, 512), (8, 32, 64, 256)
EXTENTS = ((4, 4, 4), (8, 8, 8), (12, 12, 12), (16, 16, 16), (32, 32, 32), (36, 36, 36), (36, 32, 32))
ENV_KEYS = ("DM3D_CONV_WIDE_WGS=1", "DM3D_CONV_WINO=0", "DM3D_CONV_V3_TD=4", "DM3D_CONV_V3_TD=8", "DM3D_CONV_KSPLIT=0",
            "DM3D_CONV_WINO_SPLIT=0", "DM3D_CONV_PAIR=0")
# rows the grid must contain whatever the walk below picks (the U-Net's own convs at the benchmark shape and the policy's thresholds)
FIXED = [(32, 32, 32, 32, 8, 32, 0, 1, 0), (32, 32, 32, 32, 64, 8, 0, 1, 0), (1, 8, 8, 8, 64, 8, 0, 1, 0),
         (32, 8, 8, 8, 256, 256, 1, 1, 0), (32, 8, 8, 8, 256, 256, 0, 1, 0),
         (32, 32, 32, 32, 128, 64, 1, 1, 0), (32, 32, 32, 32, 128, 64, 0, 1, 0), (32, 32, 32, 32, 128, 64, 0, 0, 0),
         (32, 16, 16, 16, 128, 128, 4, 1, 0), (32, 32, 32, 32, 64, 64, 5, 1, 0), (4, 36, 36, 36, 64, 64, 1, 1, 0)]


def load_lib_module():
    """_lib.py by path: the ctypes mirrors without importing the package (and torch) — a replay process starts in well under a second."""
    spec = importlib.util.spec_from_file_location("dm3d_lib_mirror", os.path.join(PKG, "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def grid():
    """FIXED, then every 9th point of batch x extent x c1 x cout x kind x counters (9 is coprime to every axis length, so the walk visits
    every value of every axis evenly: 1743 rows), then the fused formats on the shapes that admit them (k3 / stride 1, whole 4x8x8 bricks,
    c1 % 16 == 0, cout % 64 == 0: 216 rows)."""
    rows, seen = [], set()

    def add(row):
        if row not in seen:
            seen.add(row)
            rows.append(row)

    for row in FIXED:
        add(row)
    full = [(b, *e, c1, co, kind, cnt, 0) for b in BATCHES for e in EXTENTS for c1 in C1S for co in COUTS for kind in range(len(KINDS))
            for cnt in (1, 0)]
    for row in full[::9]:
        add(row)
    for b in (1, 4, 32):
        for e in (8, 16, 32):
            for c1 in (64, 256):
                for co in (64, 256):
                    for kind in (0, 1):
                        for fmt in (1, 2, 3):
                            add((b, e, e, e, c1, co, kind, 1, fmt))
    return rows


def descriptor(mod, row):
    """The dm3d_conv_desc of a row, as ops.conv3d / unet.Plan fill it (the queries read no memory: the pointers are placeholders)."""
    b, d_, h, w, c1, cout, kind, counters, fmt = row
    name, ptr = KINDS[kind], 4096
    d = mod.ConvDesc()
    d.x1 = d.wpk = d.out = ptr
    d.c1, d.batch, d.in_d, d.in_h, d.in_w, d.cout = c1, b, d_, h, w, cout
    d.precision = mod.PREC_H3
    d.ksize, d.stride = 3, 1
    if name == "upsample":
        d.upsample = 1
    elif name == "k3s2":
        d.stride = 2
    elif name == "k1":
        d.ksize = 1
    elif name == "transpose_k4s2":
        d.ksize, d.stride, d.transpose = 4, 2, 1
    if "wino" in name:
        d.wpk_wino = ptr
    if "skip" in name:
        d.skip_wpk, d.skip_x1, d.skip_c1 = ptr, ptr, c1
        if "frag" in name:
            d.skip_wpk_frag = ptr
    if counters:
        d.split_counters, d.split_counter_words = ptr, 1 << 20
    if FMTS[fmt] == "x1_h2":
        d.x1_fmt = mod.FMT_H2
    elif FMTS[fmt] == "out_h2":
        d.out_fmt = mod.FMT_H2
    elif FMTS[fmt] == "post":
        d.post_scale = d.post_shift = ptr
    return d


def query(mod, handle, row):
    d = descriptor(mod, row)
    d.w_layout = handle.dm3d_conv_weight_layout(d.ksize, d.stride, d.upsample, d.transpose, d.cout)
    ref = C.byref(d)
    form = handle.dm3d_conv_tile_form(ref)
    narrow = int(KINDS[row[6]].startswith("k3s1") and row[5] <= 32 and d.w_layout == mod.WL_PAIR)
    return [form, handle.dm3d_conv_scratch_bytes(ref), handle.dm3d_conv_split_counter_words(ref), narrow]


def open_lib(mod, path=None):
    handle = C.CDLL(path or mod.LIB_PATH)
    for name in ("dm3d_conv_tile_form", "dm3d_conv_scratch_bytes", "dm3d_conv_split_counter_words", "dm3d_conv_weight_layout"):
        getattr(handle, name).restype, getattr(handle, name).argtypes = mod.SIGNATURES[name]
    return handle


def sub_grid(rows):
    """50 rows for the knob replays: FIXED and an even walk over the rest of the k3 / stride-1 and UpSample rows (the knobs touch no other)."""
    rest = [i for i, r in enumerate(rows) if i >= len(FIXED) and r[6] <= 4]
    return list(range(len(FIXED))) + rest[::len(rest) // (50 - len(FIXED))][:50 - len(FIXED)]


def replay(env_key, golden=GOLDEN):
    """In a fresh process with the knob set (the read-once knobs are read when the library first resolves a conv)."""
    name, value = env_key.split("=")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "replay", env_key, golden], env=dict(os.environ, **{name: value}),
                         check=True, capture_output=True, text=True).stdout
    return json.loads(out)


def main(argv):
    mod = load_lib_module()
    if argv[1] == "replay":
        name, value = argv[2].split("=")
        assert os.environ.get(name) == value, "start this process with the knob set"
        with open(argv[3] if len(argv) > 3 else GOLDEN) as f:
            g = json.load(f)
        handle = open_lib(mod)
        print(json.dumps([query(mod, handle, tuple(g["rows"][i][:len(COLUMNS)])) for i in g["sub"]]))
        return
    assert argv[1] == "record"
    path = argv[2] if len(argv) > 2 else GOLDEN
    for key in ENV_KEYS:
        assert key.split("=")[0] not in os.environ, "record without conv knobs in the environment"
    handle = open_lib(mod)
    rows = grid()
    g = {"columns": list(COLUMNS) + ["form", "scratch_bytes", "split_counter_words", "narrow_k3s1"], "kinds": list(KINDS), "fmts": list(FMTS),
         "rows": [list(r) + query(mod, handle, r) for r in rows], "sub": sub_grid(rows), "env": {}}
    with open(path, "w") as f:           # (the replays read rows and sub from the file)
        json.dump(g, f)
    for key in ENV_KEYS:
        g["env"][key] = replay(key, path)
    with open(path, "w") as f:
        f.write('{"columns": %s, "kinds": %s, "fmts": %s,\n "sub": %s,\n "env": {\n%s},\n "rows": [\n%s]}\n' % (
            json.dumps(g["columns"]), json.dumps(g["kinds"]), json.dumps(g["fmts"]), json.dumps(g["sub"]),
            ",\n".join('  "%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in g["env"].items()),
            ",\n".join(json.dumps(r, separators=(",", ":")) for r in g["rows"])))
    print(f"{path}: {len(rows)} rows, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv)
