#!/usr/bin/env python3
"""Latent editing against plain sampling on BASELINE config 3 (conditional U-Net, 32^3 x 8ch latents, B = 32, T = 1000, seeded weights
with the output conv scaled by 0.1, as tools/ddim_bench.py): one JSON line.

    python tools/edit_bench.py [--batch 32] [--steps 10] [--reps 5] [--num-steps 50]

  * ms/step of each kind: blocks of --steps graph replays, the plain step (U-Net + update + counter) and the edit step (the same plus
    dm3d_edit_update) alternating --reps times in this one process, DDPM and DDIM, each block timed by the host clock around a device
    synchronise; the median block is reported.  The edit chains run with a mask that regenerates half of every volume (a box of half
    the depth, the rest kept) at strength 1.
  * one whole S = --num-steps DDIM edit chain (edit(sampler="ddim"), the same mask, strength 0.8: a q_sample start), wall clock around a
    synchronise, after one warm chain.
Kernel times (edit_kernel against ddim_kernel / ddpm_kernel) come from a separate rocprofv3 --kernel-trace --stats run of this tool.
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
    ap.add_argument("--reps", type=int, default=5, help="rounds of the four kinds' blocks")
    ap.add_argument("--num-steps", type=int, default=50, help="S of the DDIM schedule")
    args = ap.parse_args()
    import numpy as np
    import torch
    import dm3d_amd
    from dm3d_amd import _lib
    from dm3d_amd.diffusion import DdimEditSampler, EditSampler, ddim_timesteps, edit_steps
    from dm3d_amd.networks import conditional_dm3d as cdm
    from types import SimpleNamespace

    _lib.require_device()
    torch.cuda.set_device(0)
    B, S, C, T = args.batch, 32, 8, 1000
    if not 1 <= args.steps < args.num_steps:
        raise SystemExit("--steps must lie in [1, --num-steps)")
    cfg = dm3d_amd.UNetConfig(img_size=S, img_channels=C)
    W = dm3d_amd.synthetic_weights(cfg, seed=0)
    W = dict(W, **{k: W[k] * np.float32(0.1) for k in ("out.conv.kernel", "out.conv.bias")})
    model = cdm.DiffusionModel(S, 1024, C, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B), weights=W)
    shape = (B, S, S, S, C)
    g = torch.Generator().manual_seed(1)
    x_T = torch.randn(shape, generator=g).cuda()
    x0 = (torch.rand(shape, generator=g) * 2 - 1).cuda()
    mask = torch.zeros((1, 4 * S, 4 * S, 4 * S))
    mask[:, : 2 * S] = 1.0                                            # regenerate the lower half of D
    keep = torch.ones(shape[:4], device="cuda")
    keep[:, : S // 2] = 0.0
    ctx = model._context_ids(1, B)
    taus = ddim_timesteps(T, args.num_steps)

    def sampler(kind):
        if kind == "ddpm":
            return model.sampler(shape, context_value=1, seed=1234).prepare()
        if kind == "ddim":
            return model.sampler(shape, context_value=1, seed=1234, kind="ddim", num_steps=args.num_steps).prepare()
        if kind == "ddpm-edit":
            return EditSampler(model, shape, ctx, 1234, True, np.arange(T), True).prepare()
        return DdimEditSampler(model, shape, ctx, 1234, True, taus, True).prepare()

    kinds = ("ddpm", "ddpm-edit", "ddim", "ddim-edit")
    blocks = {k: [] for k in kinds}
    for rep in range(args.reps + 1):                    # rep 0 warms every kind
        for kind in kinds:
            smp = sampler(kind)
            if kind.endswith("edit"):
                smp.reset(x0, keep)
            else:
                smp.reset(x_T)
            smp.step()                                  # the first step of a chain is not timed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                smp.step()
            torch.cuda.synchronize()
            if rep:
                blocks[kind].append((time.perf_counter() - t0) / args.steps * 1e3)
    ms = {k: statistics.median(v) for k, v in blocks.items()}

    kw = dict(mask=mask, strength=0.8, sampler="ddim", num_steps=args.num_steps)
    model.edit(x0, 1, seed=7, **kw)                     # warm chain
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.edit(x0, 1, seed=8, **kw)
    torch.cuda.synchronize()
    chain_s = time.perf_counter() - t0
    kept = bool(torch.equal(out[:, S // 2:], x0[:, S // 2:]))

    print(json.dumps({
        "tool": "edit_bench", "config": {"latent": f"{S}^3x{C}", "batch": B, "timesteps": T, "ddim_steps": args.num_steps,
                                         "precision": model.network.precision, "steps_per_block": args.steps, "reps": args.reps,
                                         "mask": "lower half of D regenerated"},
        **{f"{k.replace('-', '_')}_ms_per_step": round(ms[k], 4) for k in kinds},
        "ddpm_edit_over_plain_step": round(ms["ddpm-edit"] / ms["ddpm"], 4),
        "ddim_edit_over_plain_step": round(ms["ddim-edit"] / ms["ddim"], 4),
        **{f"{k.replace('-', '_')}_ms_per_step_blocks": [round(v, 4) for v in blocks[k]] for k in kinds},
        "ddim_edit_chain_steps": edit_steps(0.8, args.num_steps), "ddim_edit_chain_s": round(chain_s, 4),
        "ddim_edit_chain_volumes_per_s": round(B / chain_s, 3), "kept_region_is_x0": kept,
    }), flush=True)


if __name__ == "__main__":
    main()
