#!/usr/bin/env python3
"""What v-prediction costs a sampling step and what the objective entry costs a train step: one JSON line per part.

    python tools/prediction_bench.py [--parts launch,step,train] [--batch 32] [--steps 10] [--reps 5] [--kinds eps,v] [--root TREE]

  * launch: us per dm3d_pred_to_eps launch at the step's shape (32^3 x 8ch, B = --batch; 12 B per element), and per
    dm3d_objective_loss_grad against dm3d_mse_loss_grad at the training shape (8^3 x 256ch, B = 8): blocks of 200 launches between two
    device events, the median of --reps blocks after one warm block.
  * step: ms per DDIM step (S = 50 of T = 1000, graph replay) of an eps model and a v model on the same weights (bench.py's seeded
    weights with the output conv scaled by 0.1, as tools/ddim_bench.py), blocks of --steps steps alternating --reps times in this one
    process; the median block, v over eps, and the C-ABI calls one eager step of each kind makes.
  * train: ms per train_step at the reference's training configuration (tools/ema_bench.py's), "eps": the plain MSE launch, "v":
    prediction="v" with compile(loss_weighting="min_snr"); blocks alternating likewise.
``--root TREE --kinds eps --parts step,train`` imports the package of another tree (a worktree of the parent commit) and times its
step and train_step with the same code: the parent's figures and call count, taken on the same box in the same visit.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="launch,step,train")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed block")
    ap.add_argument("--reps", type=int, default=5, help="timed blocks per kind")
    ap.add_argument("--kinds", default="eps,v")
    ap.add_argument("--root", default=ROOT, help="the tree whose package is imported")
    args = ap.parse_args()
    parts, kinds = args.parts.split(","), [k for k in args.kinds.split(",") if k]
    if set(parts) - {"launch", "step", "train"} or not kinds or set(kinds) - {"eps", "v"}:
        raise SystemExit("--parts takes launch, step, train; --kinds eps, v")
    sys.path.insert(0, os.path.abspath(args.root))
    import ctypes as C
    from types import SimpleNamespace
    import numpy as np
    import torch
    import dm3d_amd
    from dm3d_amd import _lib
    from dm3d_amd.networks import conditional_dm3d as cdm

    _lib.require_device()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    root = os.path.abspath(args.root)

    def blocks_us(launch, n=200):
        out = []
        for rep in range(args.reps + 1):                # rep 0 warms
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                launch()
            b.record()
            torch.cuda.synchronize()
            if rep:
                out.append(a.elapsed_time(b) / n * 1e3)
        return out

    def alternate(run):
        """ms per step of every kind: blocks of --steps calls of run[kind], kinds alternating, host clock around a synchronise."""
        blocks = {k: [] for k in run}
        for rep in range(args.reps + 1):                # rep 0 warms every kind
            for kind, fn in run.items():
                fn(True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    fn(False)
                torch.cuda.synchronize()
                if rep:
                    blocks[kind].append((time.perf_counter() - t0) / args.steps * 1e3)
        return blocks

    def report(part, config, blocks, unit="ms_per_step"):
        out = {"tool": "prediction_bench", "part": part, "config": dict(config, root=root, reps=args.reps)}
        med = {k: statistics.median(v) for k, v in blocks.items()}
        for k, v in blocks.items():
            out[f"{k}_{unit}"] = round(med[k], 4)
            out[f"{k}_{unit}_blocks"] = [round(x, 4) for x in v]
        if "eps" in med and "v" in med:
            out["v_over_eps"] = round(med["v"] / med["eps"], 5)
        return out

    if "launch" in parts:
        from dm3d_amd.diffusion import objective_rows, prediction_table
        B, per, T = args.batch, 32 ** 3 * 8, 1000
        g = torch.Generator(device=dev).manual_seed(0)
        pred, x = (torch.randn(B, per, generator=g, device=dev) for _ in range(2))
        tab = torch.from_numpy(prediction_table(dm3d_amd.Betas(T).alpha_bar, "v")).to(dev)
        t_idx = torch.full((B,), 517, dtype=torch.int32, device=dev)
        d = _lib.PredDesc()
        d.pred, d.x, d.table, d.t_idx = pred.data_ptr(), x.data_ptr(), tab.data_ptr(), t_idx.data_ptr()
        d.batch, d.per_sample, d.timesteps = B, per, T
        us = blocks_us(lambda: _lib.check(lib.dm3d_pred_to_eps(C.byref(d), st), "pred_to_eps"))
        out = {"tool": "prediction_bench", "part": "launch", "config": {"root": root, "reps": args.reps},
               "pred_to_eps": {"batch": B, "per_sample": per, "us": round(statistics.median(us), 2), "us_blocks": [round(v, 2) for v in us],
                               "TBps": round(12 * B * per / statistics.median(us) * 1e-6, 3)}}
        Bt, pt = 8, 8 ** 3 * 256
        p, z, c = (torch.randn(Bt, pt, generator=g, device=dev) for _ in range(3))
        dp = torch.empty_like(p)
        rows = torch.from_numpy(objective_rows(dm3d_amd.Betas(500).alpha_bar, np.arange(Bt) * 60, "v", "min_snr")).to(dev)
        partials = torch.empty(Bt * _lib.LOSS_PARTIAL_BLOCKS, dtype=torch.float64, device=dev)
        loss_rows, loss = torch.empty(Bt, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
        ld = _lib.LossDesc()
        ld.pred, ld.noise, ld.x0, ld.coef, ld.dpred = p.data_ptr(), z.data_ptr(), c.data_ptr(), rows.data_ptr(), dp.data_ptr()
        ld.partials, ld.loss_rows, ld.loss = partials.data_ptr(), loss_rows.data_ptr(), loss.data_ptr()
        ld.batch, ld.per_sample, ld.inv_divisor = Bt, pt, 1e-6
        us_o = blocks_us(lambda: _lib.check(lib.dm3d_objective_loss_grad(C.byref(ld), st), "objective_loss_grad"))
        us_m = blocks_us(lambda: _lib.check(lib.dm3d_mse_loss_grad(p.data_ptr(), z.data_ptr(), p.numel(), 1e-6, loss.data_ptr(), dp.data_ptr(), st), "mse"))
        out["loss"] = {"batch": Bt, "per_sample": pt, "objective_us": round(statistics.median(us_o), 2),
                       "mse_us": round(statistics.median(us_m), 2), "objective_us_blocks": [round(v, 2) for v in us_o],
                       "mse_us_blocks": [round(v, 2) for v in us_m]}
        print(json.dumps(out), flush=True)
        del pred, x, p, z, c, dp
        torch.cuda.empty_cache()

    def model(kind, S, Cc, B, T, W):
        kw = {} if kind == "eps" else dict(prediction="v")       # (the parent's constructor has no such keyword)
        return cdm.DiffusionModel(S, 1024, Cc, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B), weights=W, **kw)

    if "step" in parts:
        B, S, Cc, T, num = args.batch, 32, 8, 1000, 50
        W = dm3d_amd.synthetic_weights(dm3d_amd.UNetConfig(img_size=S, img_channels=Cc), seed=0)
        W = dict(W, **{k: W[k] * np.float32(0.1) for k in ("out.conv.kernel", "out.conv.bias")})
        shape = (B, S, S, S, Cc)
        x_T = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda()
        models = {k: model(k, S, Cc, B, T, W) for k in kinds}
        calls = {}
        for k, m in models.items():                     # the C-ABI calls of one eager step, counted through the bound handle
            count, saved = {}, {}
            for name in _lib.SIGNATURES:
                fn = getattr(lib, name)
                saved[name] = fn
                setattr(lib, name, lambda *a, _f=fn, _n=name: (count.__setitem__(_n, count.get(_n, 0) + 1), _f(*a))[1])
            try:
                smp = m.sampler(shape, context_value=1, seed=1234, kind="ddim", num_steps=num, use_graph=False)     # (binds its update entry)
                smp.reset(x_T)
                smp.step()
                count.clear()
                smp.step()
            finally:
                for name, fn in saved.items():
                    setattr(lib, name, fn)
            torch.cuda.synchronize()
            calls[k] = {"total": sum(v for n, v in count.items() if n not in ("dm3d_last_error",)),
                        "after_the_unet": {n: v for n, v in count.items() if n in ("dm3d_pred_to_eps", "dm3d_guide_update", "dm3d_x0_threshold",
                                                                                     "dm3d_ddim_update", "dm3d_edit_update", "dm3d_add_i32")}}
        smps = {}

        def step_fn(kind):
            def fn(first):
                if first:
                    smps[kind] = models[kind].sampler(shape, context_value=1, seed=1234, kind="ddim", num_steps=num).prepare()
                    smps[kind].reset(x_T)
                smps[kind].step()
            return fn

        if args.steps + 1 > num:
            raise SystemExit("--steps must stay under the 50-step chain")
        out = report("step", {"latent": f"{S}^3x{Cc}", "batch": B, "timesteps": T, "ddim_steps": num, "steps_per_block": args.steps},
                     alternate({k: step_fn(k) for k in kinds}))
        out["abi_calls_per_eager_step"] = calls
        print(json.dumps(out), flush=True)
        del models, smps
        torch.cuda.empty_cache()

    if "train" in parts:
        S, Cc, B, T = 8, 256, 8, 500
        W = dm3d_amd.synthetic_weights(dm3d_amd.UNetConfig(img_size=S, img_channels=Cc), 0)
        models = {k: model(k, S, Cc, B, T, W) for k in kinds}
        for k, m in models.items():
            m.compile(loss=None, optimizer=1e-4, **({} if k == "eps" else dict(loss_weighting="min_snr")))
        gen = torch.Generator().manual_seed(0)
        ctx = torch.randint(0, 2, (B, 1, 1), generator=gen)
        lat = torch.randn(B, S, S, S, Cc, generator=gen).to(dev)
        run = {k: (lambda first, m=m: m.train_step((None, None, ctx), latents=lat)) for k, m in models.items()}
        print(json.dumps(report("train", {"latent": f"{S}^3x{Cc}", "batch": B, "timesteps": T, "steps_per_block": args.steps},
                                alternate(run))), flush=True)


if __name__ == "__main__":
    main()
