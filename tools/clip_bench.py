#!/usr/bin/env python3
"""What global-norm clipping costs: dm3d_grad_scale and dm3d_adam_scaled against dm3d_adam_ema, and train_step with clipping off and on,
at the reference's training configuration (main_conditional_dm.py:141-147: latent 8^3 x 256ch, B = 8, T = 500; pre-encoded latents,
seeded weights as in tools/train_bench.py): one JSON line per part.  The procedure is tools/ema_bench.py's.

    python tools/clip_bench.py [--launches 200] [--steps 10] [--reps 5] [--kinds off,clip] [--root TREE] [--skip-kernels]

  * us per launch of each entry over the flat buffers of the reference model (Trainer.total elements): blocks of --launches launches
    between two device events, the entries' blocks alternating --reps times (one warm-up round first); the median block, and the bytes
    the algorithm moves over it (grad_scale 4 B per element, adam_ema and adam_scaled 36).  Each entry is also timed launch by launch
    after a pass over a 512 MiB buffer, which is what a train step's launch sees.  dm3d_grad_scale is two kernels behind one entry:
    ``grad_scale`` times both, ``grad_scale_fixed`` the entry at n = 4 — a one-block grad_sqnorm_kernel and the whole
    grad_scale_finalize_kernel, the part that does not grow with n — so grad_sqnorm_kernel at full size is their difference.
  * ms per train_step of each kind in --kinds (off: compile() as before, both with ema_decay; clip: global_clipnorm=1.0; accum2:
    grad_accum_steps=2, per call): blocks of --steps steps, kinds alternating --reps times in this one process on one model each, each
    block timed by the host clock around a device synchronise; the median block and every block, so the spread can be read off.
``--root TREE --kinds off --skip-kernels`` imports the package of another tree (a worktree of the parent commit) and times its
train_step with the same code.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"off": {}, "clip": dict(global_clipnorm=1.0), "accum2": dict(grad_accum_steps=2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200, help="launches per timed block")
    ap.add_argument("--steps", type=int, default=10, help="train steps per timed block")
    ap.add_argument("--reps", type=int, default=5, help="timed blocks per kind")
    ap.add_argument("--kinds", default="off,clip", help="train_step kinds to time, of off, clip, accum2")
    ap.add_argument("--root", default=ROOT, help="the tree whose package is imported")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--decay", type=float, default=0.9999)
    args = ap.parse_args()
    kinds = [k for k in args.kinds.split(",") if k]
    if not kinds or set(kinds) - set(KINDS):
        raise SystemExit(f"--kinds takes a comma-separated list of {', '.join(KINDS)}")
    sys.path.insert(0, os.path.abspath(args.root))
    import ctypes
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
    config = {"latent": f"{S}^3x{C}", "batch": B, "timesteps": T, "tree": os.path.relpath(os.path.abspath(args.root), ROOT)}      # "." is this tree

    def model(kind):
        m = cdm.DiffusionModel(S, 1024, C, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B), weights=W)
        m.compile(loss=None, optimizer=1e-4, ema_decay=args.decay, **KINDS[kind])
        return m

    if not args.skip_kernels:
        from dm3d_amd.train import ADAM_BETA1, ADAM_BETA2, ADAM_EPS, Trainer
        n = Trainer(cfg, W, dev, forward_only=True).total
        g = torch.Generator(device=dev).manual_seed(0)
        w, grad, ema = (torch.randn(n, generator=g, device=dev) * s for s in (0.1, 1.0, 0.1))
        m_, v_ = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        parts = torch.empty(_lib.GRADNORM_PARTIAL_BLOCKS, dtype=torch.float64, device=dev)
        state = torch.zeros(4, device=dev)
        flush = torch.empty(128 << 20, dtype=torch.float32, device=dev)             # 512 MiB: twice the Infinity Cache
        st = torch.cuda.current_stream().cuda_stream
        lib = _lib.lib()
        descs = {}
        for name, count in (("grad_scale", n), ("grad_scale_fixed", 4)):
            d = _lib.GradScaleDesc()
            d.g, d.n, d.partials, d.state, d.clip_norm, d.pre_scale = grad.data_ptr(), count, parts.data_ptr(), state.data_ptr(), 1.0, 1.0
            descs[name] = d
        ptrs = (w.data_ptr(), grad.data_ptr(), m_.data_ptr(), v_.data_ptr(), ema.data_ptr())

        def launch(kind):
            if kind in descs:
                _lib.check(lib.dm3d_grad_scale(ctypes.byref(descs[kind]), st), kind)
            elif kind == "adam_ema":
                _lib.check(lib.dm3d_adam_ema(*ptrs, n, 1e-6, ADAM_BETA1, ADAM_BETA2, ADAM_EPS, 1e-4, st), kind)
            else:
                _lib.check(lib.dm3d_adam_scaled(*ptrs, n, 1e-6, ADAM_BETA1, ADAM_BETA2, ADAM_EPS, 1e-4, state.data_ptr(), st), kind)

        launch("grad_scale")                            # adam_scaled reads a state a real gradient produced
        warm = {k: [] for k in ("grad_scale", "grad_scale_fixed", "adam_ema", "adam_scaled")}
        cold = {k: [] for k in warm}
        for rep in range(args.reps + 1):                # rep 0 warms every entry
            for kind in warm:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.launches):
                    launch(kind)
                b.record()
                torch.cuda.synchronize()
                if rep:
                    warm[kind].append(a.elapsed_time(b) / args.launches * 1e3)
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
            launch("grad_scale")
        bytes_per = {"grad_scale": 4, "adam_ema": 36, "adam_scaled": 36}
        out = {"tool": "clip_bench", "part": "launch", "config": dict(config, elements=n, launches_per_block=args.launches, reps=args.reps),
               "state": [float(x) for x in state.cpu()]}
        for kind in warm:
            for name, blocks in (("cache_resident", warm[kind]), ("after_512MiB_stream", cold[kind])):
                us = statistics.median(blocks)
                out[f"{kind}_{name}_us"] = round(us, 2)
                if kind in bytes_per:
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
    out = {"tool": "clip_bench", "part": "train_step", "config": dict(config, steps_per_block=args.steps, reps=args.reps, decay=args.decay)}
    for k in kinds:
        out[f"{k}_ms_per_step"] = round(ms[k], 3)
        out[f"{k}_ms_per_step_blocks"] = [round(v, 3) for v in blocks[k]]
        out[f"{k}_loss"] = loss[k]
        tr = models[k].trainer
        out[f"{k}_grad_norm"], out[f"{k}_skipped_steps"] = getattr(tr, "grad_norm", None), getattr(tr, "skipped_steps", None)
    for k in kinds:
        if k != "off" and "off" in ms:
            out[f"{k}_over_off"] = round(ms[k] / ms["off"], 4)
            out[f"{k}_minus_off_us"] = round((ms[k] - ms["off"]) * 1e3, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
