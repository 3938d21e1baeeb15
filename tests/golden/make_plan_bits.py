"""Records tests/golden/plan_bits.json: what the U-Net plan builder (unet.py, ``Plan``) makes of fifteen small networks, and the bits one
forward through each plan leaves in ``eps``, so that a change to the builder can be held against the commit before it.  The kernels are
deterministic, so a plan with the same launches and the same descriptors gives the same bytes.  tests/test_gpu_plan_bits.py replays every
case through ``run_case`` below; tests/test_plan_bits_host.py checks the recording itself without a GPU.

    python tests/golden/make_plan_bits.py [--root TREE] [--out FILE]

``--root TREE`` imports the package of another tree (an export of the commit to record, built there); the cases are this tree's.  Inputs
and weights are not stored: they are drawn from the seed the file keeps.  A case's knobs are set in os.environ before its UNet is built.
Needs a GPU.
"""
import argparse
import hashlib
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

# every environment switch the plan builder or the UNet constructor reads: a case sets its own and runs with the others unset
KNOBS = ("DM3D_FUSED_MIN_ROWS", "DM3D_ATTN_FRONT", "DM3D_MLP_FUSED", "DM3D_ATTN_FUSED", "DM3D_MLP_TAIL",
         "DM3D_PRECISION", "DM3D_CONV_WINO", "DM3D_FUSE_SKIP", "DM3D_H2_HANDOFF")
FULL_BYTES = 64 * 1024                                       # eps is stored in full (hex) up to this size, else only its SHA-256

WIDE = dict(img_size=16, img_channels=4, widths=(256,), has_attention=(True,), num_res_blocks=1)               # L = 4096, u = 256
TWO = dict(img_size=8, img_channels=4, widths=(32, 64), has_attention=(False, True), num_res_blocks=1, first_conv_channels=16)
ODD = dict(img_size=24, img_channels=4, widths=(16, 32, 48), num_res_blocks=1, first_conv_channels=16)         # 6^3 = 216 tokens
SELF = dict(img_size=8, img_channels=4, widths=(64,), has_attention=(True,), num_res_blocks=1, conditional=False)
RES = dict(img_size=32, img_channels=4, widths=(64,), has_attention=(False,), num_res_blocks=1)
PER2, ONE = [[1], [0]], [[[1]]]                              # per-sample context ids of a batch of two; one id for the whole batch


def _case(cfg, batch, ctx, precision="h3", env=None, has=(), lacks=(), equal=(), final_h2in=None):
    """``has`` / ``lacks``: kinds the plan must / must not hold (a name that starts with ``*`` matches as a suffix); ``equal``: pairs of kinds
    with equal counts; ``final_h2in``: whether the output conv reads a DM3D_FMT_H2 input (the hand-off rule of ``Plan._build``)."""
    return dict(cfg=cfg, batch=batch, ctx=ctx, precision=precision, env=dict(env or {}), has=tuple(has), lacks=tuple(lacks),
                equal=tuple(equal), final_h2in=final_h2in)


CASES = {
    # the fused forms of the cross block at default knobs: M = 8192 rows, 2 * B * (L / 128) = 128 attention workgroups
    "01-wide-fused": _case(WIDE, 2, PER2, has=("attn_front", "attn_fused", "mlp_fused"), lacks=("gemm_h3", "layernorm", "softmax")),
    # each fall-back arm of the split-float16 body
    "02-wide-no-front": _case(WIDE, 2, PER2, env={"DM3D_ATTN_FRONT": "0"}, has=("layernorm", "gemm_h3", "mlp_fused", "attn_fused"),
                              lacks=("attn_front",)),
    "03-wide-no-mlp": _case(WIDE, 2, PER2, env={"DM3D_MLP_FUSED": "0"}, has=("attn_front", "gemm_h3"), lacks=("mlp_fused",)),
    "04-wide-no-tail": _case(WIDE, 2, PER2, env={"DM3D_MLP_TAIL": "0"}, has=("mlp_fused", "gemm_h3"), equal=(("gemm_h3", "mlp_fused"),)),
    "05-wide-no-attn": _case(WIDE, 2, PER2, env={"DM3D_ATTN_FUSED": "0"}, has=("softmax", "gemm_h3"), lacks=("attn_fused",)),   # 4096-column softmax
    "06-wide-min-rows": _case(WIDE, 2, PER2, env={"DM3D_FUSED_MIN_ROWS": "16384"}, has=("layernorm", "gemm_h3", "attn_fused"),
                              lacks=("attn_front", "mlp_fused")),
    "07-two-h3-broadcast": _case(TWO, 2, ONE, has=("gemm_h3", "layernorm", "softmax"), lacks=("gemm", "attn_front", "attn_fused", "mlp_fused")),
    "08-two-fp32": _case(TWO, 2, PER2, precision="fp32", has=("gemm", "layernorm", "softmax"), lacks=("gemm_h3",)),
    "09-odd-tokens": _case(ODD, 1, [[1]], has=("gemm", "layernorm", "softmax"), lacks=("gemm_h3",)),      # float32 intermediates under "h3"
    "10-self-h3": _case(SELF, 2, None, has=("gemm_h3", "affine", "softmax"), lacks=("gemm", "layernorm")),
    "11-self-fp32": _case(SELF, 2, None, precision="fp32", has=("gemm", "affine", "softmax"), lacks=("gemm_h3", "layernorm")),
    "12-two-group": _case(dict(TWO, norm="group"), 2, ONE, has=("groupnorm", "affine", "gemm_h3")),
    "13-self-group": _case(dict(SELF, norm="group"), 2, None, has=("groupnorm", "affine", "gemm_h3")),
    "14-res-handoff": _case(RES, 3, [[1], [0], [1]], has=("*_h2in",), final_h2in=True),                  # 3 * (32^3 / 256) = 384 > 256 bricks
    "15-res-no-handoff": _case(RES, 1, [[1]], lacks=("*_h2in",), final_h2in=False),
}


def seed_of(case_id):
    return zlib.crc32(case_id.encode())


def kinds_of(launches):
    out = {}
    for launch in launches:
        out[launch[0]] = out.get(launch[0], 0) + 1
    return out


def expect_failures(case_id, kinds, final_h2in):
    """What of the case's expect rule the kinds {name: count} of a plan miss (empty: the plan took the path the case is there for)."""
    spec, bad = CASES[case_id], []

    def present(name):
        return any(k.endswith(name[1:]) for k in kinds) if name.startswith("*") else name in kinds

    bad += [f"no {n}" for n in spec["has"] if not present(n)]
    bad += [f"has {n}" for n in spec["lacks"] if present(n)]
    bad += [f"{a} x{kinds.get(a, 0)} != {b} x{kinds.get(b, 0)}" for a, b in spec["equal"] if kinds.get(a, 0) != kinds.get(b, 0)]
    if spec["final_h2in"] is not None and bool(final_h2in) != spec["final_h2in"]:
        bad.append(f"final_h2in is {final_h2in}")
    return bad


_WEIGHTS = {}


def _weights(dm3d_amd, cfg_kw, seed):
    """Six cases share the wide configuration, whose context MLPs are large: drawn once."""
    key = (json.dumps(cfg_kw, sort_keys=True), seed)
    if key not in _WEIGHTS:
        _WEIGHTS.clear()
        _WEIGHTS[key] = dm3d_amd.synthetic_weights(dm3d_amd.UNetConfig(**cfg_kw), seed=seed)
    return _WEIGHTS[key]


def run_case(case_id):
    """One case on the device, with the environment as the caller set it: the record the golden file keeps for it."""
    import torch
    import dm3d_amd
    from dm3d_amd import _lib
    spec = CASES[case_id]
    seed = zlib.crc32(json.dumps(spec["cfg"], sort_keys=True).encode()) % 1000         # cases of one configuration share their weights
    cfg = dm3d_amd.UNetConfig(**spec["cfg"])
    net = dm3d_amd.UNet(cfg, weights=_weights(dm3d_amd, spec["cfg"], seed), precision=spec["precision"])
    B, S, c = spec["batch"], cfg.img_size, cfg.img_channels
    rng = np.random.default_rng(seed_of(case_id))
    x = torch.from_numpy(rng.standard_normal((B, S, S, S, c)).astype(np.float32))
    t = torch.from_numpy(rng.integers(0, 1000, size=B))
    inputs = [x, t] if spec["ctx"] is None else [x, t, torch.tensor(spec["ctx"])]
    first, again = (net(inputs).cpu().numpy().tobytes() for _ in range(2))
    ids = None if spec["ctx"] is None else np.asarray(spec["ctx"]).reshape(-1)
    per_sample = ids is not None and len(ids) == B and B > 1 and len(set(ids.tolist())) > 1
    plan = net.plan(B, B, per_sample)
    last = plan.ops[-1][1][0]._obj                           # the output conv's descriptor
    rec = dict(
        seed=seed_of(case_id), repeats=first == again, sha256=hashlib.sha256(first).hexdigest(),
        launches=[[op[2], op[3].get("desc", ""), op[3].get("flops", 0.0), op[3].get("exec_flops"), op[3].get("bytes")] for op in plan.ops],
        count=plan.count(), uses_wino=bool(plan.uses_wino), range_limit=float(plan.range_limit),
        final_h2in=int(last.x1_fmt) == _lib.FMT_H2)
    if len(first) <= FULL_BYTES:
        rec["eps_hex"] = first.hex()
    return rec, first


def set_knobs(case_id, environ=os.environ):
    for k in KNOBS:
        environ.pop(k, None)
    environ.update(CASES[case_id]["env"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT, help="the tree whose package is imported")
    ap.add_argument("--out", default=os.path.join(HERE, "plan_bits.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import time
    import torch
    import dm3d_amd  # noqa: F401
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    out = {}
    for case_id in CASES:
        t0 = time.time()
        set_knobs(case_id)
        rec, _ = run_case(case_id)
        bad = expect_failures(case_id, rec["count"], rec["final_h2in"])
        assert not bad, f"{case_id} did not reach its path: {bad}; kinds {rec['count']}"
        if not rec.pop("repeats"):
            print(f"{case_id}: eps does NOT repeat at this commit: its digest is left out", flush=True)
            rec.pop("sha256"), rec.pop("eps_hex", None)
        out[case_id] = rec
        print(f"{case_id}: {len(rec['launches'])} launches {rec['count']} wino={rec['uses_wino']} limit={rec['range_limit']:.6g} "
              f"sha={rec.get('sha256', '-')[:12]} {time.time() - t0:.1f} s", flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: {len(out)} cases, {os.path.getsize(args.out)} bytes (package {os.path.dirname(dm3d_amd.__file__)}, library {_lib.LIB_PATH})")


if __name__ == "__main__":
    main()
