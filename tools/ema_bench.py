#!/usr/bin/env python3
"""What the weight average costs: the fused dm3d_adam_ema launch against dm3d_adam, and train_step with the average off and on, at the
reference's training configuration (main_conditional_dm.py:141-147: latent 8^3 x 256ch, B = 8, T = 500; pre-encoded latents, seeded
weights as in tools/train_bench.py): one JSON line per part.

    python tools/ema_bench.py [--launches 200] [--steps 10] [--reps 5] [--kinds off,on] [--root TREE] [--skip-kernels]

  * us per launch of each entry over the flat buffers of the reference model (Trainer.total elements): blocks of --launches launches
    between two device events, dm3d_adam and dm3d_adam_ema blocks alternating --reps times (one warm-up pair first); the median block,
    and the bytes the algorithm moves (28 and 36 B per element) over it.  Back to back the buffers may stay in the Infinity Cache
    between launches, which a train step's launch does not enjoy (its buffers were last touched a whole step earlier), so each
    entry is also timed launch by launch after a pass over a 512 MiB buffer; both figures are reported.
  * ms per train_step of each kind in --kinds: blocks of --steps steps, kinds alternating --reps times in this one process on one
    model each, each block timed by the host clock around a device synchronise; the median block, and on over off.
``--root TREE --kinds off --skip-kernels`` imports the package of another tree (a worktree of the parent commit, tools/tree_ab.sh's
layout) and times its train_step with the same code: the parent's figure, taken on the same box in the same visit.
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
    ap.add_argument("--launches", type=int, default=200, help="optimizer launches per timed block")
    ap.add_argument("--steps", type=int, default=10, help="train steps per timed block")
    ap.add_argument("--reps", type=int, default=5, help="timed blocks per kind")
    ap.add_argument("--kinds", default="off,on", help="train_step kinds to time: off, on or off,on")
    ap.add_argument("--root", default=ROOT, help="the tree whose package is imported")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--decay", type=float, default=0.9999)
    args = ap.parse_args()
    kinds = [k for k in args.kinds.split(",") if k]
    if not kinds or set(kinds) - {"off", "on"}:
        raise SystemExit("--kinds takes off, on or off,on")
    sys.path.insert(0, os.path.abspath(args.root))
    from types import SimpleNamespace
    import torch
    import dm3d_amd
    from dm3d_amd import _lib
    from dm3d_amd.networks import conditional_dm3d as cdm

    _lib.require_device()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    S, C, B, T = 8, 256, 8, 500
    cfg = dm3d_amd.UNetConfig(img_size=S, img_channels=C)
    W = dm3d_amd.synthetic_weights(cfg, 0)
    config = {"latent": f"{S}^3x{C}", "batch": B, "timesteps": T, "root": os.path.abspath(args.root)}

    def model(kind):
        m = cdm.DiffusionModel(S, 1024, C, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B), weights=W)
        if kind == "on":
            m.compile(loss=None, optimizer=1e-4, ema_decay=args.decay)
        else:
            m.compile(loss=None, optimizer=1e-4)
        return m

    if not args.skip_kernels:
        from dm3d_amd.train import ADAM_BETA1, ADAM_BETA2, ADAM_EPS, Trainer
        n = Trainer(cfg, W, dev, forward_only=True).total
        g = torch.Generator(device=dev).manual_seed(0)
        w, grad, ema = (torch.randn(n, generator=g, device=dev) * s for s in (0.1, 1.0, 0.1))
        m_, v_ = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        flush = torch.empty(128 << 20, dtype=torch.float32, device=dev)             # 512 MiB: twice the Infinity Cache
        st = torch.cuda.current_stream().cuda_stream
        lib = _lib.lib()

        def launch(kind):
            if kind == "adam":
                _lib.check(lib.dm3d_adam(w.data_ptr(), grad.data_ptr(), m_.data_ptr(), v_.data_ptr(), n, 1e-6, ADAM_BETA1, ADAM_BETA2, ADAM_EPS, st), "adam")
            else:
                _lib.check(lib.dm3d_adam_ema(w.data_ptr(), grad.data_ptr(), m_.data_ptr(), v_.data_ptr(), ema.data_ptr(), n, 1e-6, ADAM_BETA1,
                                             ADAM_BETA2, ADAM_EPS, 1e-4, st), "adam_ema")

        warm = {k: [] for k in ("adam", "adam_ema")}
        cold = {k: [] for k in warm}
        for rep in range(args.reps + 1):                # rep 0 warms both entries
            for kind in warm:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.launches):
                    launch(kind)
                b.record()
                torch.cuda.synchronize()
                if rep:
                    warm[kind].append(a.elapsed_time(b) / args.launches * 1e3)
                # the same launch after a stream that evicts the buffers: one event pair per launch, a tenth as many of them
                us = []
                for _ in range(max(args.launches // 10, 1)):
                    flush.add_(1.0)
                    a.record()
                    launch(kind)
                    b.record()
                    torch.cuda.synchronize()
                    us.append(a.elapsed_time(b) * 1e3)
                if rep:
                    cold[kind].append(statistics.median(us))
        bytes_per = {"adam": 28, "adam_ema": 36}
        out = {"tool": "ema_bench", "part": "launch", "config": dict(config, elements=n, launches_per_block=args.launches, reps=args.reps)}
        for kind in warm:
            for name, blocks in (("cache_resident", warm[kind]), ("after_512MiB_stream", cold[kind])):
                us = statistics.median(blocks)
                out[f"{kind}_{name}_us"] = round(us, 2)
                out[f"{kind}_{name}_TBps"] = round(bytes_per[kind] * n / us * 1e-6, 3)
                out[f"{kind}_{name}_us_blocks"] = [round(v, 2) for v in blocks]
        print(json.dumps(out), flush=True)
        del w, grad, ema, m_, v_, flush
        torch.cuda.empty_cache()

    models = {k: model(k) for k in kinds}
    gen = torch.Generator().manual_seed(0)
    ctx = torch.randint(0, 2, (B, 1, 1), generator=gen)
    lat = torch.randn(B, S, S, S, C, generator=gen).to(dev)
    blocks = {k: [] for k in kinds}
    loss = {}
    for rep in range(args.reps + 1):                    # rep 0 warms every kind
        for kind in kinds:
            m = models[kind]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss[kind] = m.train_step((None, None, ctx), latents=lat)["loss"]
            torch.cuda.synchronize()
            if rep:
                blocks[kind].append((time.perf_counter() - t0) / args.steps * 1e3)
    ms = {k: statistics.median(v) for k, v in blocks.items()}
    out = {"tool": "ema_bench", "part": "train_step", "config": dict(config, steps_per_block=args.steps, reps=args.reps, decay=args.decay)}
    for k in kinds:
        out[f"ema_{k}_ms_per_step"] = round(ms[k], 3)
        out[f"ema_{k}_ms_per_step_blocks"] = [round(v, 3) for v in blocks[k]]
        out[f"ema_{k}_loss"] = loss[k]
    if len(kinds) == 2:
        out["on_over_off"] = round(ms["on"] / ms["off"], 4)
        out["on_minus_off_us"] = round((ms["on"] - ms["off"]) * 1e3, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
