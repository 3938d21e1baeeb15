#!/usr/bin/env python3
"""What the update kernels' ``frame`` path costs and saves: one JSON line per part.

    python tools/ztsnr_bench.py [--parts launch,step] [--batch 32] [--steps 10] [--reps 5] [--parent-lib PATH]

  * launch: us per dm3d_ddim_update and dm3d_dpm_update launch at the step's shape (32^3 x 8ch, B = --batch), and per
    dm3d_ddim_update_frame / dm3d_dpm_update_frame launch with a v frame: blocks of 200 launches between two device events, the
    kinds alternating block by block, the median of --reps blocks after one warm block.  ``--parent-lib PATH`` (a libdm3d_hip.so built
    from the parent commit; the output records its file name) times the parent's kernels in the same process, its blocks alternating
    with this build's (the update descriptors are what they were).
  * step: ms per DDIM and DPM-Solver++ step (S = 50 of T = 1000, graph replay) of a v-model that converts to eps (plain schedule) and
    of a zero-terminal-SNR v-model that runs in its own frame, on the same weights (bench.py's seeded weights with the output conv
    scaled by 0.1, as tools/ddim_bench.py), blocks of --steps steps alternating --reps times in this one process; the median block, and
    the C-ABI calls one eager step of each makes.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="launch,step")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed block")
    ap.add_argument("--reps", type=int, default=5, help="timed blocks per kind")
    ap.add_argument("--parent-lib", default=None, help="a libdm3d_hip.so of the parent commit, for the launch part")
    args = ap.parse_args()
    parts = args.parts.split(",")
    if set(parts) - {"launch", "step"}:
        raise SystemExit("--parts takes launch, step")
    sys.path.insert(0, ROOT)
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

    def alternate_us(launches, n=200):
        """us per launch of every kind: blocks of n launches between two device events, kinds alternating."""
        blocks = {k: [] for k in launches}
        for rep in range(args.reps + 1):                # rep 0 warms every kind
            for kind, fn in launches.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(n):
                    fn()
                b.record()
                torch.cuda.synchronize()
                if rep:
                    blocks[kind].append(a.elapsed_time(b) / n * 1e3)
        return {k: {"us": round(statistics.median(v), 2), "us_blocks": [round(x, 2) for x in v]} for k, v in blocks.items()}

    if "launch" in parts:
        from dm3d_amd.diffusion import ddim_coefficients, dpm_coefficients, frame_table
        B, per, T = args.batch, 32 ** 3 * 8, 1000
        g = torch.Generator(device=dev).manual_seed(0)
        x, p, h, out, x0 = (torch.randn(B, per, generator=g, device=dev) for _ in range(5))
        ab = dm3d_amd.Betas(T).alpha_bar
        src, dst, prev = np.array([517]), np.array([497]), np.array([537])
        rows = np.zeros((2, 1, 8))
        rows[0, :, :5] = ddim_coefficients(ab, src, dst, 0.0)
        rows[1, :, :2], rows[1, :, 2:5] = rows[0, :, :2], dpm_coefficients(ab, src, dst, prev)
        rows[:, :, 5] = 1.0
        ddim_c, dpm_c = (torch.from_numpy(r.astype(np.float32)).to(dev) for r in rows)
        frame = torch.from_numpy(np.ascontiguousarray(frame_table(ab, "v")[src])).to(dev)
        tau = torch.tensor([517], dtype=torch.int32, device=dev)
        pos = torch.zeros(B, dtype=torch.int32, device=dev)

        def descs():
            d = _lib.DdimDesc()
            d.x, d.eps, d.out, d.coef, d.tau, d.pos = x.data_ptr(), p.data_ptr(), out.data_ptr(), ddim_c.data_ptr(), tau.data_ptr(), pos.data_ptr()
            d.batch, d.per_sample, d.rows, d.mode = B, per, 1, 0
            q = _lib.DpmDesc()
            q.x, q.eps, q.hist, q.out, q.x0_out, q.coef, q.pos = (x.data_ptr(), p.data_ptr(), h.data_ptr(), out.data_ptr(), x0.data_ptr(),
                                                                  dpm_c.data_ptr(), pos.data_ptr())
            q.batch, q.per_sample, q.rows, q.mode = B, per, 1, 0
            return d, q

        d0, q0 = descs()
        handles = {"this": lib}
        if args.parent_lib:
            handles["parent"] = C.CDLL(os.path.abspath(args.parent_lib))
            for name in ("dm3d_ddim_update", "dm3d_dpm_update"):
                getattr(handles["parent"], name).restype, getattr(handles["parent"], name).argtypes = _lib.SIGNATURES[name]
        launches = {}
        for who, hnd in handles.items():
            launches[f"ddim_null_{who}"] = lambda hnd=hnd: _lib.check(hnd.dm3d_ddim_update(C.byref(d0), st), "ddim_update")
            launches[f"dpm_null_{who}"] = lambda hnd=hnd: _lib.check(hnd.dm3d_dpm_update(C.byref(q0), st), "dpm_update")
        launches["ddim_frame_this"] = lambda: _lib.check(lib.dm3d_ddim_update_frame(C.byref(d0), frame.data_ptr(), st), "ddim_update_frame")
        launches["dpm_frame_this"] = lambda: _lib.check(lib.dm3d_dpm_update_frame(C.byref(q0), frame.data_ptr(), st), "dpm_update_frame")
        res = alternate_us(launches)
        print(json.dumps({"tool": "ztsnr_bench", "part": "launch", "config": {"batch": B, "per_sample": per, "reps": args.reps,
                                                                                "parent_lib": args.parent_lib and os.path.basename(args.parent_lib)},
                          **res}), flush=True)
        del x, p, h, out, x0
        torch.cuda.empty_cache()

    if "step" in parts:
        B, S, Cc, T, num = args.batch, 32, 8, 1000, 50
        W = dm3d_amd.synthetic_weights(dm3d_amd.UNetConfig(img_size=S, img_channels=Cc), seed=0)
        W = dict(W, **{k: W[k] * np.float32(0.1) for k in ("out.conv.kernel", "out.conv.bias")})
        shape = (B, S, S, S, Cc)
        x_T = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda()
        a = SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B)
        models = {"convert": cdm.DiffusionModel(S, 1024, Cc, None, a, weights=W, prediction="v"),
                  "native": cdm.DiffusionModel(S, 1024, Cc, None, a, weights=W, prediction="v", zero_terminal_snr=True)}
        if args.steps + 1 > num:
            raise SystemExit("--steps must stay under the 50-step chain")
        for solver in ("ddim", "dpmpp"):
            calls = {}
            for k, m in models.items():                 # the C-ABI calls of one eager step, counted through the bound handle
                count, saved = {}, {}
                for name in _lib.SIGNATURES:
                    fn = getattr(lib, name)
                    saved[name] = fn
                    setattr(lib, name, lambda *a_, _f=fn, _n=name: (count.__setitem__(_n, count.get(_n, 0) + 1), _f(*a_))[1])
                try:
                    smp = m.sampler(shape, context_value=1, seed=1234, kind=solver, num_steps=num, use_graph=False)
                    smp.reset(x_T)
                    smp.step()
                    count.clear()
                    smp.step()
                finally:
                    for name, fn in saved.items():
                        setattr(lib, name, fn)
                torch.cuda.synchronize()
                calls[k] = {"total": sum(v for n, v in count.items() if n != "dm3d_last_error"),
                            "after_the_unet": {n: v for n, v in count.items() if n in ("dm3d_pred_to_eps", "dm3d_ddim_update", "dm3d_dpm_update", "dm3d_ddim_update_frame", "dm3d_dpm_update_frame",
                                                                                         "dm3d_add_i32")}}
            smps, blocks = {}, {k: [] for k in models}
            for rep in range(args.reps + 1):            # rep 0 warms both
                for k, m in models.items():
                    smps[k] = m.sampler(shape, context_value=1, seed=1234, kind=solver, num_steps=num).prepare()
                    smps[k].reset(x_T)
                    smps[k].step()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        smps[k].step()
                    torch.cuda.synchronize()
                    if rep:
                        blocks[k].append((time.perf_counter() - t0) / args.steps * 1e3)
            med = {k: statistics.median(v) for k, v in blocks.items()}
            print(json.dumps({"tool": "ztsnr_bench", "part": "step", "solver": solver,
                              "config": {"latent": f"{S}^3x{Cc}", "batch": B, "timesteps": T, "chain_steps": num, "steps_per_block": args.steps,
                                         "reps": args.reps},
                              **{f"{k}_ms_per_step": round(v, 4) for k, v in med.items()},
                              **{f"{k}_ms_per_step_blocks": [round(x, 4) for x in v] for k, v in blocks.items()},
                              "native_minus_convert_us": round((med["native"] - med["convert"]) * 1e3, 1),
                              "abi_calls_per_eager_step": calls}), flush=True)


if __name__ == "__main__":
    main()
