#!/usr/bin/env python3
"""UniPC against DPM-Solver++(2M) on BASELINE config 3 (conditional U-Net, 32^3 x 8ch latents, B = 32, T = 1000, seeded weights with the
output conv scaled by 0.1, as tools/dpm_bench.py): one JSON line, also written to --out.

    python tools/unipc_bench.py [--batch 32] [--steps 8] [--reps 5] [--chain-steps 10 20] [--solver-order 2] [--kinds dpmpp unipc] [--out FILE]

  * us/launch of unipc_kernel and dpm_kernel in this one process: --launches back-to-back launches of each update on buffers of the
    chain's size (mode 1, a second-order row; UniPC at --solver-order with its corrector), alternating --reps times, each block timed
    by the host clock around a device synchronise; the median block is reported (back-to-back launches hide the launch latency, so
    this is the kernels' stream time).
  * ms/step of each kind of --kinds: blocks of --steps graph replays alternating --reps times, as tools/dpm_bench.py.  Both kinds run
    the same U-Net on the same plan; they differ in the update kernel alone.  --kinds with one name times that kind only: run the tool
    from two checkouts in alternating processes to compare a step across commits.
  * whole chains (generate(), reset and range check included) at every S of --chain-steps, wall clock around a synchronise, after one
    warm chain each: seconds and volumes/s.
"""
import argparse
import ctypes as C
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
    ap.add_argument("--steps", type=int, default=8, help="graph steps per timed block")
    ap.add_argument("--reps", type=int, default=5, help="rounds of the kinds' blocks")
    ap.add_argument("--launches", type=int, default=200, help="update launches per timed kernel block")
    ap.add_argument("--chain-steps", type=int, nargs="*", default=[10, 20], help="S of the whole chains (none: skip them)")
    ap.add_argument("--solver-order", type=int, default=2, choices=[1, 2, 3], help="order of the UniPC steps (dpmpp runs at min(order, 2))")
    ap.add_argument("--kinds", nargs="+", default=["dpmpp", "unipc"], choices=["dpmpp", "unipc"])
    ap.add_argument("--no-kernel", action="store_true", help="skip the per-launch kernel times")
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
    B, S, Cc, T = args.batch, 32, 8, 1000
    steps = max(args.chain_steps + [args.steps + 2])
    cfg = dm3d_amd.UNetConfig(img_size=S, img_channels=Cc)
    W = dm3d_amd.synthetic_weights(cfg, seed=0)
    W = dict(W, **{k: W[k] * np.float32(0.1) for k in ("out.conv.kernel", "out.conv.bias")})
    model = cdm.DiffusionModel(S, 1024, Cc, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B), weights=W)
    shape = (B, S, S, S, Cc)
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda()
    ctx = [1] * B
    order = {"dpmpp": min(args.solver_order, 2), "unipc": args.solver_order}

    kernel = {}
    if not args.no_kernel:
        lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
        bufs = [torch.randn(shape, generator=torch.Generator().manual_seed(2 + i)).cuda() for i in range(7)]
        pos = torch.zeros(B, dtype=torch.int32, device="cuda")
        taus = np.array([400, 450, 500, 550], dtype=np.int64)
        rows = dm3d_amd.diffusion.unipc_coefficients(model.b.alpha_bar, taus, args.solver_order, False)
        ucoef, ucorr = (t.cuda() for t in model._unipc_table(taus, rows, True))
        uni = model._unipc_desc(bufs[0], bufs[1], bufs[2], bufs[3:6], ucoef[1:2].contiguous(), ucorr[1:2].contiguous(), pos, 1)
        dcoef = model._dpm_table(taus[1:2], taus[0:1], taus[2:3], 2, True).cuda()
        dpm = model._dpm_desc(bufs[0].clone(), bufs[1], bufs[6], dcoef, pos, 1)
        calls = {"unipc_kernel": lambda: lib.dm3d_unipc_update(C.byref(uni), st), "dpm_kernel": lambda: lib.dm3d_dpm_update(C.byref(dpm), st)}
        blocks = {k: [] for k in calls}
        for rep in range(args.reps + 1):
            for name, call in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.launches):
                    _lib.check(call(), name)
                torch.cuda.synchronize()
                if rep:
                    blocks[name].append((time.perf_counter() - t0) / args.launches * 1e6)
        kernel = {f"{k}_us_per_launch": round(statistics.median(v), 2) for k, v in blocks.items()}
        kernel["unipc_over_dpm_kernel"] = round(kernel["unipc_kernel_us_per_launch"] / kernel["dpm_kernel_us_per_launch"], 3)

    blocks = {k: [] for k in args.kinds}
    for rep in range(args.reps + 1):                    # rep 0 warms every kind
        for kind in args.kinds:
            smp = model.sampler(shape, ctx, seed=1234, kind=kind, num_steps=steps, solver_order=order[kind]).prepare()
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
    for s in args.chain_steps:
        for kind in args.kinds:
            kw = dict(context_value=ctx, sampler=kind, num_steps=s, solver_order=order[kind])
            model.generate(shape, seed=7, **kw)                             # warm chain
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(shape, seed=8, **kw)
            torch.cuda.synchronize()
            sec = time.perf_counter() - t0
            chain.update({f"{kind}_S{s}_chain_s": round(sec, 4), f"{kind}_S{s}_chain_volumes_per_s": round(B / sec, 3),
                          f"{kind}_S{s}_chain_max_abs": round(float(out.abs().max()), 4)})

    line = json.dumps({
        "tool": "unipc_bench", "config": {"latent": f"{S}^3x{Cc}", "batch": B, "timesteps": T, "solver_order": args.solver_order,
                                          "precision": model.network.precision, "steps_per_block": args.steps, "reps": args.reps,
                                          "launches_per_block": args.launches, "weights": "seeded, output conv scaled by 0.1"},
        **kernel, **{f"{k}_ms_per_step": round(ms[k], 4) for k in args.kinds},
        **({"unipc_over_dpmpp_step": round(ms["unipc"] / ms["dpmpp"], 4)} if len(ms) == 2 else {}),
        **{f"{k}_ms_per_step_blocks": [round(v, 4) for v in blocks[k]] for k in args.kinds}, **chain,
    })
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
