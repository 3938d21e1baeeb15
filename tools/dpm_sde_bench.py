#!/usr/bin/env python3
"""What the stochastic DPM-Solver++(2M) update costs beside the kernels it is made of: one JSON line per part.

    python tools/dpm_sde_bench.py [--parts launch,step] [--batch 32] [--steps 10] [--reps 5] [--chain-steps 20] [--parent-lib PATH]

  * launch: us per launch at the step's shape (32^3 x 8ch, B = --batch, mode 0, a second-order row 517 -> 497 after 537, clip on) of
    dm3d_dpm_sde_update at eta = 1 (in-kernel Philox) and at eta = 0 (c_z = 0: dpm_kernel's work), of dm3d_dpm_update, and of
    dm3d_ddim_update at eta = 0 and eta = 1 (in-kernel Philox): blocks of 200 launches between two device events, the kinds
    alternating block by block, the median of --reps blocks after one warm block.  ``--parent-lib PATH`` (a libdm3d_hip.so built from
    the parent commit; the output records its file name) times the kernels of that library too in the same process, its blocks
    alternating with this build's.  The expectation the output states: dpm_sde (eta = 1) = dpm + (ddim eta 1 - ddim eta 0), the
    new kernel moving dpm_kernel's bytes and doing ddim_kernel's Philox work; ``margin_us`` is the largest block-to-block spread
    (max - min) of the kinds involved.
  * step: ms per step (graph replay) of an S = --chain-steps "dpmpp_sde" chain against the "dpmpp" chain of the same S on the same
    plan and weights (bench.py's seeded weights with the output conv scaled by 0.1, as tools/dpm_bench.py), blocks of --steps steps
    alternating --reps times in this one process; the median block.
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
    ap.add_argument("--chain-steps", type=int, default=20, help="S of both chains of the step part")
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
        return blocks

    if "launch" in parts:
        from dm3d_amd.diffusion import ddim_coefficients, dpm_coefficients, dpm_sde_coefficients
        B, per, T = args.batch, 32 ** 3 * 8, 1000
        g = torch.Generator(device=dev).manual_seed(0)
        x, p, h, out, x0 = (torch.randn(B, per, generator=g, device=dev) for _ in range(5))
        ab = dm3d_amd.Betas(T).alpha_bar
        src, dst, prev = np.array([517]), np.array([497]), np.array([537])
        rows = np.zeros((5, 1, 8))                       # ddim eta 0, ddim eta 1, dpm, dpm_sde eta 1, dpm_sde eta 0
        rows[0, :, :5], rows[1, :, :5] = ddim_coefficients(ab, src, dst, 0.0), ddim_coefficients(ab, src, dst, 1.0)
        rows[2:, :, :2] = rows[0, :, :2]
        rows[2, :, 2:5] = dpm_coefficients(ab, src, dst, prev)
        for r, eta in ((3, 1.0), (4, 0.0)):
            c = dpm_sde_coefficients(ab, src, dst, prev, 2, eta)
            rows[r, :, 2:5], rows[r, :, 6] = c[:, :3], c[:, 3]
        rows[:, :, 5] = 1.0
        assert rows[1, 0, 4] != 0 and rows[3, 0, 6] != 0 and rows[4, 0, 6] == 0 and rows[2, 0, 4] != 0
        ddim0_c, ddim1_c, dpm_c, sde1_c, sde0_c = (torch.from_numpy(r.astype(np.float32)).to(dev) for r in rows)
        tau = torch.tensor([517], dtype=torch.int32, device=dev)
        pos = torch.zeros(B, dtype=torch.int32, device=dev)

        def ddim_desc(coef):
            d = _lib.DdimDesc()
            d.x, d.eps, d.out, d.coef, d.tau, d.pos = x.data_ptr(), p.data_ptr(), out.data_ptr(), coef.data_ptr(), tau.data_ptr(), pos.data_ptr()
            d.batch, d.per_sample, d.rows, d.mode, d.seed = B, per, 1, 0, 1234
            return d

        def dpm_desc(cls, coef):
            q = cls()
            q.x, q.eps, q.hist, q.out, q.x0_out, q.coef, q.pos = (x.data_ptr(), p.data_ptr(), h.data_ptr(), out.data_ptr(), x0.data_ptr(),
                                                                  coef.data_ptr(), pos.data_ptr())
            q.batch, q.per_sample, q.rows, q.mode = B, per, 1, 0
            return q

        d0, d1, q0 = ddim_desc(ddim0_c), ddim_desc(ddim1_c), dpm_desc(_lib.DpmDesc, dpm_c)
        s1, s0 = dpm_desc(_lib.DpmSdeDesc, sde1_c), dpm_desc(_lib.DpmSdeDesc, sde0_c)
        for s in (s1, s0):
            s.tau, s.seed = tau.data_ptr(), 1234
        handles = {"this": lib}
        if args.parent_lib:
            handles["parent"] = C.CDLL(os.path.abspath(args.parent_lib))
            for name in ("dm3d_ddim_update", "dm3d_dpm_update", "dm3d_dpm_sde_update"):
                getattr(handles["parent"], name).restype, getattr(handles["parent"], name).argtypes = _lib.SIGNATURES[name]
        launches = {}
        for who, hnd in handles.items():
            launches[f"dpm_sde_eta1_{who}"] = lambda hnd=hnd: _lib.check(hnd.dm3d_dpm_sde_update(C.byref(s1), st), "dpm_sde_update")
            launches[f"dpm_sde_eta0_{who}"] = lambda hnd=hnd: _lib.check(hnd.dm3d_dpm_sde_update(C.byref(s0), st), "dpm_sde_update")
            launches[f"dpm_{who}"] = lambda hnd=hnd: _lib.check(hnd.dm3d_dpm_update(C.byref(q0), st), "dpm_update")
            launches[f"ddim_eta0_{who}"] = lambda hnd=hnd: _lib.check(hnd.dm3d_ddim_update(C.byref(d0), st), "ddim_update")
            launches[f"ddim_eta1_{who}"] = lambda hnd=hnd: _lib.check(hnd.dm3d_ddim_update(C.byref(d1), st), "ddim_update")
        blocks = alternate_us(launches)
        med = {k: statistics.median(v) for k, v in blocks.items()}
        who = "parent" if args.parent_lib else "this"      # the existing kernels: the parent's where its library was given
        used = ("dpm_sde_eta1_this", f"dpm_{who}", f"ddim_eta0_{who}", f"ddim_eta1_{who}")
        expected = med[f"dpm_{who}"] + med[f"ddim_eta1_{who}"] - med[f"ddim_eta0_{who}"]
        print(json.dumps({"tool": "dpm_sde_bench", "part": "launch",
                          "config": {"batch": B, "per_sample": per, "reps": args.reps, "launches_per_block": 200,
                                     "parent_lib": args.parent_lib and os.path.basename(args.parent_lib), "existing_kernels_from": who},
                          **{k: {"us": round(med[k], 2), "us_blocks": [round(v, 2) for v in blocks[k]]} for k in blocks},
                          "expected_dpm_sde_eta1_us": round(expected, 2),
                          "measured_minus_expected_us": round(med["dpm_sde_eta1_this"] - expected, 2),
                          "margin_us": round(max(max(blocks[k]) - min(blocks[k]) for k in used), 2)}), flush=True)
        del x, p, h, out, x0
        torch.cuda.empty_cache()

    if "step" in parts:
        B, S, Cc, T, num = args.batch, 32, 8, 1000, args.chain_steps
        if not 1 <= args.steps < num:
            raise SystemExit("--steps must lie in [1, --chain-steps)")
        W = dm3d_amd.synthetic_weights(dm3d_amd.UNetConfig(img_size=S, img_channels=Cc), seed=0)
        W = dict(W, **{k: W[k] * np.float32(0.1) for k in ("out.conv.kernel", "out.conv.bias")})
        shape = (B, S, S, S, Cc)
        x_T = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda()
        model = cdm.DiffusionModel(S, 1024, Cc, None, SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=B), weights=W)
        kinds = ("dpmpp", "dpmpp_sde")
        blocks = {k: [] for k in kinds}
        for rep in range(args.reps + 1):                # rep 0 warms both (and captures both graphs)
            for kind in kinds:
                smp = model.sampler(shape, context_value=1, seed=1234, kind=kind, num_steps=num).prepare()     # a new Sampler takes the plan over
                smp.reset(x_T)
                smp.step()                              # the first step of a chain is not timed (and is first order)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    smp.step()
                torch.cuda.synchronize()
                if rep:
                    blocks[kind].append((time.perf_counter() - t0) / args.steps * 1e3)
        med = {k: statistics.median(v) for k, v in blocks.items()}
        print(json.dumps({"tool": "dpm_sde_bench", "part": "step",
                          "config": {"latent": f"{S}^3x{Cc}", "batch": B, "timesteps": T, "chain_steps": num, "steps_per_block": args.steps,
                                     "reps": args.reps, "precision": model.network.precision, "weights": "seeded, output conv scaled by 0.1"},
                          **{f"{k}_ms_per_step": round(v, 4) for k, v in med.items()},
                          **{f"{k}_ms_per_step_blocks": [round(x, 4) for x in v] for k, v in blocks.items()},
                          "sde_minus_ode_us": round((med["dpmpp_sde"] - med["dpmpp"]) * 1e3, 1),
                          "sde_over_ode_step": round(med["dpmpp_sde"] / med["dpmpp"], 4)}), flush=True)


if __name__ == "__main__":
    main()
