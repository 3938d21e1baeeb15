#!/usr/bin/env python3
"""Classifier-free guidance against plain sampling on BASELINE config 3 (conditional U-Net, 32^3 x 8ch latents, T = 1000, seeded weights
with the output conv scaled by 0.1, as tools/ddim_bench.py: untrained, they would amplify eps out of the H3 range over a whole DDIM
chain; the launches and their cost do not depend on the values): one JSON line, also written to --out.

    python tools/guidance_bench.py [--batch 32] [--steps 10] [--reps 5] [--num-steps 50] [--out profiles/guidance_bench.json]

  * ms/step of each kind: blocks of --steps graph replays alternating --reps times in this one process, each block timed by the host
    clock around a device synchronise; the median block is reported.  The kinds: the guided DDPM and DDIM steps of B = --batch
    volumes (a plan of 2 B rows: U-Net, combine, rescale, update on B rows, mirror, counter; w = 3, phi = 0.7), the plain DDPM and DDIM
    steps of the same 2 B-row plan (U-Net, update on 2 B rows, counter), and the plain DDPM step of the B-row plan, from which the
    cost of guidance per guided volume can be read.
  * one whole guided DDIM chain (S = --num-steps steps of B volumes, generate(), reset and range check included), wall clock
    around a synchronise, after one warm chain: volumes/s.
Kernel times (guide_combine_kernel, guide_rescale_kernel, guide_mirror_kernel against ddim_kernel / ddpm_kernel) come from a
separate rocprofv3 --kernel-trace --stats run of this tool (--reps 1 --no-chain keeps it short).
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
    ap.add_argument("--batch", type=int, default=32, help="guided volumes B (the guided plan holds 2 B rows)")
    ap.add_argument("--steps", type=int, default=10, help="graph steps per timed block")
    ap.add_argument("--reps", type=int, default=5, help="rounds of the kinds' blocks")
    ap.add_argument("--num-steps", type=int, default=50, help="S of the DDIM schedule")
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--rescale", type=float, default=0.7)
    ap.add_argument("--no-chain", action="store_true", help="skip the whole guided chain (profiling runs)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
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
    W = dict(W, **{k: W[k] * np.float32(0.1) for k in ("out.conv.kernel", "out.conv.bias")})
    model = cdm.DiffusionModel(S, 1024, C, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B), weights=W)
    shape, shape2 = (B, S, S, S, C), (2 * B, S, S, S, C)
    g = torch.Generator().manual_seed(1)
    x_T = torch.randn(shape, generator=g).cuda()
    x_T2 = torch.cat([x_T, x_T])
    pos, neg = [1] * B, [0] * B
    guide = dict(guidance_scale=args.scale, negative_context=neg, guidance_rescale=args.rescale)
    ddim = dict(kind="ddim", num_steps=args.num_steps)

    def sampler(kind):                                                      # a new Sampler takes its plan over
        if kind == "ddpm_guided":
            return model.sampler(shape, pos, seed=1234, **guide).prepare(), x_T
        if kind == "ddim_guided":
            return model.sampler(shape, pos, seed=1234, **ddim, **guide).prepare(), x_T
        if kind == "ddpm_plain_2b":
            return model.sampler(shape2, pos + neg, seed=1234).prepare(), x_T2
        if kind == "ddim_plain_2b":
            return model.sampler(shape2, pos + neg, seed=1234, **ddim).prepare(), x_T2
        return model.sampler(shape, pos, seed=1234).prepare(), x_T          # ddpm_plain_b

    kinds = ("ddpm_guided", "ddpm_plain_2b", "ddim_guided", "ddim_plain_2b", "ddpm_plain_b")
    blocks = {k: [] for k in kinds}
    for rep in range(args.reps + 1):                    # rep 0 warms every kind
        for kind in kinds:
            smp, start = sampler(kind)
            smp.reset(start)
            smp.step()                                  # the first step of a chain is not timed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                smp.step()
            torch.cuda.synchronize()
            if rep:
                blocks[kind].append((time.perf_counter() - t0) / args.steps * 1e3)
    ms = {k: statistics.median(v) for k, v in blocks.items()}

    chain = {}
    if not args.no_chain:
        kw = dict(sampler="ddim", num_steps=args.num_steps, **guide)
        model.generate(shape, context_value=pos, seed=7, **kw)              # warm chain
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(shape, context_value=pos, seed=8, **kw)
        torch.cuda.synchronize()
        chain_s = time.perf_counter() - t0
        chain = {"ddim_guided_chain_s": round(chain_s, 4), "ddim_guided_chain_volumes_per_s": round(B / chain_s, 3),
                 "ddim_guided_chain_max_abs": round(float(out.abs().max()), 4)}

    line = json.dumps({
        "tool": "guidance_bench", "config": {"latent": f"{S}^3x{C}", "guided_volumes": B, "plan_rows": 2 * B, "timesteps": T,
                                             "ddim_steps": args.num_steps, "guidance_scale": args.scale,
                                             "guidance_rescale": args.rescale, "precision": model.network.precision,
                                             "steps_per_block": args.steps, "reps": args.reps,
                                             "weights": "seeded, output conv scaled by 0.1"},
        **{f"{k}_ms_per_step": round(ms[k], 4) for k in kinds},
        "ddpm_guided_over_plain_2b_step": round(ms["ddpm_guided"] / ms["ddpm_plain_2b"], 4),
        "ddim_guided_over_plain_2b_step": round(ms["ddim_guided"] / ms["ddim_plain_2b"], 4),
        "plain_2b_over_plain_b_step": round(ms["ddpm_plain_2b"] / ms["ddpm_plain_b"], 4),
        "ddpm_guided_ms_per_guided_volume": round(ms["ddpm_guided"] / B, 4),
        "ddpm_plain_b_ms_per_volume": round(ms["ddpm_plain_b"] / B, 4),
        **{f"{k}_ms_per_step_blocks": [round(v, 4) for v in blocks[k]] for k in kinds},
        **chain,
    })
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
