#!/usr/bin/env python3
"""The dynamically thresholded DDIM step against the plain one on BASELINE config 3 (conditional U-Net, 32^3 x 8ch latents, B = 32,
T = 1000, seeded weights with the output conv scaled by 0.1 as in tools/ddim_bench.py): one JSON line.

    python tools/threshold_bench.py [--batch 32] [--steps 10] [--reps 5] [--num-steps 50] [--ratio 0.995] [--solver ddim]

  * ms/step of each kind: blocks of --steps graph replays (U-Net + [threshold] + update + counter), plain and thresholded blocks
    alternating --reps times in this one process on the same plan, each block timed by the host clock around a device synchronise;
    the median block is reported, and the thresholded step over the plain one.
  * s of the last timed step (min and max over the batch): the selection ran on real values.
Per-launch times of the selection kernels (thresh_clear_kernel, thresh_pass1_kernel, thresh_pass_kernel<2>, <3>, thresh_final_kernel)
come from a separate rocprofv3 --kernel-trace --stats run of this tool.  The plain step of another commit is measured with that
commit's tools/ddim_bench.py from a worktree of it (tools/tree_ab.sh's layout), on the same box in the same visit.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10, help="graph steps per timed block")
    ap.add_argument("--reps", type=int, default=5, help="plain / thresholded block pairs")
    ap.add_argument("--num-steps", type=int, default=50, help="S of the schedule")
    ap.add_argument("--ratio", type=float, default=0.995, help="dynamic_threshold")
    ap.add_argument("--solver", choices=("ddim", "dpmpp"), default="ddim")
    args = ap.parse_args()
    import numpy as np
    import torch
    import dm3d_amd
    from dm3d_amd import _lib
    from dm3d_amd.networks import conditional_dm3d as cdm
    from types import SimpleNamespace

    _lib.require_device()
    torch.cuda.set_device(0)
    B, S, C, T = args.batch, 32, 8, 1000
    if not 1 <= args.steps < args.num_steps:
        raise SystemExit("--steps must lie in [1, --num-steps)")
    cfg = dm3d_amd.UNetConfig(img_size=S, img_channels=C)
    W = dm3d_amd.synthetic_weights(cfg, seed=0)
    W = dict(W, **{k: W[k] * np.float32(0.1) for k in ("out.conv.kernel", "out.conv.bias")})       # tools/ddim_bench.py's weights
    model = cdm.DiffusionModel(S, 1024, C, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B), weights=W)
    shape = (B, S, S, S, C)
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda()

    def sampler(kind):
        kw = dict(dynamic_threshold=args.ratio) if kind == "thresholded" else {}
        return model.sampler(shape, context_value=1, seed=1234, kind=args.solver, num_steps=args.num_steps, **kw).prepare()

    blocks = {"plain": [], "thresholded": []}
    bound = None
    for rep in range(args.reps + 1):                    # rep 0 warms both kinds
        for kind in ("plain", "thresholded"):
            smp = sampler(kind)
            smp.reset(x_T)
            smp.step()                                  # the first step of a chain is not timed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                smp.step()
            torch.cuda.synchronize()
            if rep:
                blocks[kind].append((time.perf_counter() - t0) / args.steps * 1e3)
            if kind == "thresholded":
                bound = smp.plan.thr_bound.clone()
    ms = {k: statistics.median(v) for k, v in blocks.items()}
    print(json.dumps({
        "tool": "threshold_bench", "config": {"latent": f"{S}^3x{C}", "batch": B, "timesteps": T, "solver": args.solver,
                                              "num_steps": args.num_steps, "ratio": args.ratio, "precision": model.network.precision,
                                              "steps_per_block": args.steps, "reps": args.reps},
        "plain_ms_per_step": round(ms["plain"], 4), "thresholded_ms_per_step": round(ms["thresholded"], 4),
        "thresholded_over_plain_step": round(ms["thresholded"] / ms["plain"], 4),
        "thresholded_minus_plain_us": round((ms["thresholded"] - ms["plain"]) * 1e3, 1),
        "plain_ms_per_step_blocks": [round(v, 4) for v in blocks["plain"]],
        "thresholded_ms_per_step_blocks": [round(v, 4) for v in blocks["thresholded"]],
        "bound_min": float(bound.min()), "bound_max": float(bound.max()),
    }), flush=True)


if __name__ == "__main__":
    main()
