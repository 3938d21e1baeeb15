#!/usr/bin/env python3
"""DDIM against DDPM on BASELINE config 3 (conditional U-Net, 32^3 x 8ch latents, B = 32, T = 1000, seeded weights with the output
conv scaled by 0.1, see below): one JSON line.

    python tools/ddim_bench.py [--batch 32] [--steps 10] [--reps 5] [--num-steps 50]

  * ms/step of each kind: blocks of --steps graph replays (U-Net + update + counter), DDPM and DDIM blocks alternating --reps times
    in this one process, each block timed by the host clock around a device synchronise; the median block is reported.  The
    DDPM blocks run the T = 1000 chain from t = T-1 (Philox noise every step), the DDIM blocks the S = --num-steps chain at eta = 0.
  * one whole DDIM chain (S steps of B volumes, generate(sampler="ddim"), reset and range check included), wall clock around a
    synchronise, after one warm chain: volumes/s of the chain, next to the DDPM T = 1000 figure implied by its step time.
  * max |eps_ddpm - eps_ddim|: the U-Net output of the first step of each kind from the same x_T (t = T-1 in both): 0 when the two
    kinds run the same network on the same plan.
Kernel times (ddim_kernel against ddpm_kernel) come from a separate rocprofv3 --kernel-trace --stats run of this tool.
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
    ap.add_argument("--reps", type=int, default=5, help="DDPM / DDIM block pairs")
    ap.add_argument("--num-steps", type=int, default=50, help="S of the DDIM schedule")
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
    # bench.py's seeded weights with the output conv scaled by 0.1: untrained, they amplify eps ~3.5x per DDIM step near t = T-1 and a
    # whole chain would leave the H3 range (tests/test_gpu_ddim.py); the launches and their cost do not depend on the values
    W = dict(W, **{k: W[k] * np.float32(0.1) for k in ("out.conv.kernel", "out.conv.bias")})
    model = cdm.DiffusionModel(S, 1024, C, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B), weights=W)
    shape = (B, S, S, S, C)
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda()

    def sampler(kind):
        kw = dict(kind="ddim", num_steps=args.num_steps) if kind == "ddim" else {}
        return model.sampler(shape, context_value=1, seed=1234, **kw).prepare()       # a new Sampler takes the plan over

    # the same x, the same t = T-1: the two kinds' U-Net eps
    eps = {}
    for kind in ("ddpm", "ddim"):
        smp = sampler(kind)
        smp.reset(x_T)
        smp.step()
        torch.cuda.synchronize()
        eps[kind] = smp.plan.eps.clone()
    eps_diff = float((eps["ddpm"] - eps["ddim"]).abs().max())

    blocks = {"ddpm": [], "ddim": []}
    for rep in range(args.reps + 1):                    # rep 0 warms both kinds
        for kind in ("ddpm", "ddim"):
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
    ms = {k: statistics.median(v) for k, v in blocks.items()}

    model.generate(shape, context_value=1, seed=7, sampler="ddim", num_steps=args.num_steps)        # warm chain
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate(shape, context_value=1, seed=8, sampler="ddim", num_steps=args.num_steps)
    torch.cuda.synchronize()
    chain_s = time.perf_counter() - t0

    print(json.dumps({
        "tool": "ddim_bench", "config": {"latent": f"{S}^3x{C}", "batch": B, "timesteps": T, "ddim_steps": args.num_steps, "eta": 0.0,
                                         "precision": model.network.precision, "steps_per_block": args.steps, "reps": args.reps},
        "ddpm_ms_per_step": round(ms["ddpm"], 4), "ddim_ms_per_step": round(ms["ddim"], 4),
        "ddim_over_ddpm_step": round(ms["ddim"] / ms["ddpm"], 4),
        "ddpm_ms_per_step_blocks": [round(v, 4) for v in blocks["ddpm"]], "ddim_ms_per_step_blocks": [round(v, 4) for v in blocks["ddim"]],
        "ddim_chain_s": round(chain_s, 4), "ddim_chain_volumes_per_s": round(B / chain_s, 3),
        "ddpm_T1000_volumes_per_s_from_step": round(B / (T * ms["ddpm"] * 1e-3), 3),
        "eps_max_abs_diff": eps_diff,
    }), flush=True)


if __name__ == "__main__":
    main()
