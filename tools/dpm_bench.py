#!/usr/bin/env python3
"""DPM-Solver++(2M) against DDIM on BASELINE config 3 (conditional U-Net, 32^3 x 8ch latents, B = 32, T = 1000, seeded weights with the
output conv scaled by 0.1, as tools/ddim_bench.py: untrained, they would amplify eps out of the H3 range over a whole deterministic
chain; the launches and their cost do not depend on the values): one JSON line, also written to --out.

    python tools/dpm_bench.py [--batch 32] [--steps 10] [--reps 5] [--dpm-steps 20] [--ddim-steps 50] [--solver-order 2] [--out profiles/dpm_bench.json]

  * ms/step of each kind: blocks of --steps graph replays alternating --reps times in this one process, each block timed by the host
    clock around a device synchronise; the median block is reported.  The kinds: the plain DDIM (eta = 0) and dpmpp steps of B volumes
    (U-Net, update, counter), and the guided ones (a plan of 2 B rows: U-Net, combine, rescale, update on B rows, mirror, counter;
    w = 3, phi = 0.7).  Both kinds of a pair run the same U-Net on the same plan; they differ in the update kernel alone.
  * whole chains (generate(), reset and range check included), wall clock around a synchronise, after one warm chain each: dpmpp at
    S = --dpm-steps against DDIM at S = --ddim-steps, plain and guided: seconds and volumes/s.
  * self-convergence (--no-convergence skips it): max |x_S - x_ref| of the DDIM (eta = 0) and dpmpp chains at S in {10, 20, 50}, x_ref
    the S = T DDIM chain, all with clip_x0=False from one x_T, at 8^3 x 4ch, B = 2.  The weights are random: this illustrates the
    solver's order on this network's ODE, it is no statement about sample quality.
Kernel times (dpm_kernel against ddim_kernel) come from a separate rocprofv3 --kernel-trace --stats run of this tool
(--reps 1 --no-chain --no-convergence keeps it short).
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
    ap.add_argument("--batch", type=int, default=32, help="volumes B (a guided plan holds 2 B rows)")
    ap.add_argument("--steps", type=int, default=10, help="graph steps per timed block")
    ap.add_argument("--reps", type=int, default=5, help="rounds of the kinds' blocks")
    ap.add_argument("--dpm-steps", type=int, default=20, help="S of the dpmpp chains")
    ap.add_argument("--ddim-steps", type=int, default=50, help="S of the DDIM chains")
    ap.add_argument("--solver-order", type=int, default=2, choices=[1, 2], help="order of the dpmpp steps (1 with --dpm-steps equal to "
                    "--ddim-steps: the same chain as DDIM through the other update kernel, a control of the step-time comparison)")
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--rescale", type=float, default=0.7)
    ap.add_argument("--no-guided", action="store_true", help="skip the guided kinds and chains")
    ap.add_argument("--no-chain", action="store_true", help="skip the whole chains (profiling runs)")
    ap.add_argument("--no-convergence", action="store_true", help="skip the self-convergence figures")
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
    if not 1 <= args.steps < min(args.dpm_steps, args.ddim_steps):
        raise SystemExit("--steps must lie in [1, min(--dpm-steps, --ddim-steps))")

    def scaled(cfg):
        W = dm3d_amd.synthetic_weights(cfg, seed=0)
        return dict(W, **{k: W[k] * np.float32(0.1) for k in ("out.conv.kernel", "out.conv.bias")})

    def build(size, ch, batch):
        cfg = dm3d_amd.UNetConfig(img_size=size, img_channels=ch)
        return cdm.DiffusionModel(size, 1024, ch, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=batch), weights=scaled(cfg))

    model = build(S, C, B)
    shape = (B, S, S, S, C)
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda()
    pos, neg = [1] * B, [0] * B
    guide = dict(guidance_scale=args.scale, negative_context=neg, guidance_rescale=args.rescale)
    sched = {"ddim": dict(kind="ddim", num_steps=args.ddim_steps), "dpmpp": dict(kind="dpmpp", num_steps=args.dpm_steps, solver_order=args.solver_order)}

    def sampler(kind):                                                      # a new Sampler takes its plan over
        base, _, guided = kind.partition("_")
        return model.sampler(shape, pos, seed=1234, **sched[base], **(guide if guided else {})).prepare()

    kinds = ("ddim", "dpmpp") + (() if args.no_guided else ("ddim_guided", "dpmpp_guided"))
    blocks = {k: [] for k in kinds}
    for rep in range(args.reps + 1):                    # rep 0 warms every kind
        for kind in kinds:
            smp = sampler(kind)
            smp.reset(x_T)
            smp.step()                                  # the first step of a chain is not timed (and is first order)
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
        for kind in kinds:
            base, _, guided = kind.partition("_")
            kw = dict(context_value=pos, sampler=base, **{k: v for k, v in sched[base].items() if k != "kind"}, **(guide if guided else {}))
            model.generate(shape, seed=7, **kw)                             # warm chain
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(shape, seed=8, **kw)
            torch.cuda.synchronize()
            sec = time.perf_counter() - t0
            chain.update({f"{kind}_chain_steps": kw["num_steps"], f"{kind}_chain_s": round(sec, 4),
                          f"{kind}_chain_volumes_per_s": round(B / sec, 3), f"{kind}_chain_max_abs": round(float(out.abs().max()), 4)})
        chain["dpmpp_over_ddim_chain_speedup"] = round(chain["ddim_chain_s"] / chain["dpmpp_chain_s"], 3)
        if not args.no_guided:
            chain["dpmpp_over_ddim_guided_chain_speedup"] = round(chain["ddim_guided_chain_s"] / chain["dpmpp_guided_chain_s"], 3)

    conv = {}
    if not args.no_convergence:
        small = build(8, 4, 2)
        sshape = (2, 8, 8, 8, 4)
        xs = torch.randn(sshape, generator=torch.Generator().manual_seed(2)).cuda()
        kw = dict(context_value=[1, 0], x_T=xs, clip_x0=False)
        ref = small.generate(sshape, sampler="ddim", num_steps=T, **kw).double()
        conv = {"convergence_config": {"latent": "8^3x4", "batch": 2, "timesteps": T, "clip_x0": False, "reference": f"ddim S={T}",
                                       "weights": "seeded (random), output conv scaled by 0.1: an illustration, not a quality claim"},
                "convergence_ref_max_abs": round(float(ref.abs().max()), 4)}
        for s in (10, 20, 50):
            for name, skw in (("ddim", dict(sampler="ddim")), ("dpmpp", dict(sampler="dpmpp")),
                              ("dpmpp_no_lower_order_final", dict(sampler="dpmpp", lower_order_final=False))):
                out = small.generate(sshape, num_steps=s, **skw, **kw).double()
                conv[f"{name}_S{s}_max_abs_diff_to_ref"] = float(f"{float((out - ref).abs().max()):.4e}")

    line = json.dumps({
        "tool": "dpm_bench", "config": {"latent": f"{S}^3x{C}", "batch": B, "timesteps": T, "dpm_steps": args.dpm_steps,
                                        "ddim_steps": args.ddim_steps, "solver_order": args.solver_order, "guidance_scale": args.scale, "guidance_rescale": args.rescale,
                                        "precision": model.network.precision, "steps_per_block": args.steps, "reps": args.reps,
                                        "weights": "seeded, output conv scaled by 0.1"},
        **{f"{k}_ms_per_step": round(ms[k], 4) for k in kinds},
        "dpmpp_over_ddim_step": round(ms["dpmpp"] / ms["ddim"], 4),
        **({} if args.no_guided else {"dpmpp_over_ddim_guided_step": round(ms["dpmpp_guided"] / ms["ddim_guided"], 4)}),
        **{f"{k}_ms_per_step_blocks": [round(v, 4) for v in blocks[k]] for k in kinds},
        **chain, **conv,
    })
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
