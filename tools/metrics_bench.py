#!/usr/bin/env python3
"""What the reconstruction metrics cost at the reference's evaluation shape (B = 8 volumes of 128^3, one image channel read out of a
2-channel reconstruction): us per call of ops.pair_stats, ops.ssim and ops.psnr, and, on the same card in the same process, of the
equivalent composition of torch ops (min / max, the squared error, F.conv2d with the separable window over the four moment maps, the
formula, the means), which is what a user without these kernels would run.  One JSON line per part.  The procedure is
tools/clip_bench.py's: blocks of --launches calls between two device events, the parts' blocks alternating --reps times after one
warm-up round; the median block and every block, so the spread can be read off.

    python tools/metrics_bench.py [--batch 8] [--size 128] [--launches 20] [--reps 5]

Bytes: pair_stats reads x once and the lines of y that hold the compared channel (with cy = 2 all of y): 4 * (1 + cy) B per voxel;
ssim the same through its halos (each input element of a 42 x 42 halo per 32 x 32 tile: 1.72 x, most of it from L2)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--launches", type=int, default=20, help="calls per timed block")
    ap.add_argument("--reps", type=int, default=5, help="timed blocks per part")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    from dm3d_amd import _lib, ops

    _lib.require_device()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, S, S, S, 1, generator=g).to(dev)
    y = torch.rand(B, S, S, S, 2, generator=g).to(dev)
    y[..., :1] = x + 0.03 * torch.randn(B, S, S, S, 1, generator=g).to(dev)
    ch = dict(x_channels=(0, 1), y_channels=(0, 1))
    i = torch.arange(11, dtype=torch.float64)
    win = torch.exp(-(i - 5) ** 2 / 4.5)
    win = (win / win.sum()).float().to(dev)
    wrow, wcol = win.reshape(1, 1, 1, 11), win.reshape(1, 1, 11, 1)

    def torch_stats():
        yi = y[..., 0]
        return yi.amin(dim=(1, 2, 3)), yi.amax(dim=(1, 2, 3)), ((x[..., 0].double() - yi.double()) ** 2).sum(dim=(2, 3))

    def torch_ssim(L):
        xi, yi = x[..., 0].reshape(B * S, 1, S, S), y[..., 0].reshape(B * S, 1, S, S)
        filt = lambda v: F.conv2d(F.conv2d(v, wrow), wcol)
        mx, my, sxy, sq = filt(xi), filt(yi), filt(xi * yi), filt(xi * xi + yi * yi)
        Lb = L.repeat_interleave(S).reshape(-1, 1, 1, 1)
        c1, c2 = (0.01 * Lb) ** 2, (0.03 * Lb) ** 2
        n0, d0 = 2 * mx * my, mx * mx + my * my
        v = (n0 + c1) / (d0 + c1) * ((2 * sxy - n0 + c2) / (sq - d0 + c2))
        return v.double().mean(dim=(1, 2, 3)).float().reshape(B, S)

    def torch_psnr(sse, L):
        return 20 * torch.log10(L).reshape(B, 1) - 10 * torch.log10((sse / (S * S)).float())

    stats = ops.pair_stats(x, y, **ch)
    parts = {
        "pair_stats": lambda: ops.pair_stats(x, y, **ch),
        "ssim": lambda: ops.ssim(x, y, stats=stats, **ch),
        "psnr": lambda: ops.psnr(x, y, stats=stats, **ch),
        "torch_stats": torch_stats,
        "torch_ssim": lambda: torch_ssim(stats.y_range),
        "torch_psnr": lambda: torch_psnr(stats.sse, stats.y_range),
    }
    # the two paths agree (float32 filtering in another order: 1e-4 is far above either's error and far below a wrong formula's)
    err = float((parts["ssim"]() - parts["torch_ssim"]()).abs().max())
    assert err < 1e-4, err

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.launches

    times = {k: [] for k in parts}
    for rep in range(args.reps + 1):
        for k, fn in parts.items():
            t = block(fn)
            if rep:
                times[k].append(t)
    voxels = B * S ** 3
    moved = {"pair_stats": 12 * voxels, "ssim": 12 * voxels}
    config = {"batch": B, "size": S, "cx": 1, "cy": 2, "nc": 1, "launches": args.launches, "ssim_max_abs_diff_vs_torch": err}
    for k, ts in times.items():
        us = statistics.median(ts)
        row = {"part": k, "us_per_call": round(us, 2), "blocks_us": [round(t, 2) for t in ts], **config}
        if k in moved:
            row["gb_per_s_of_bytes_needed"] = round(moved[k] / us / 1e3, 1)
        print(json.dumps(row), flush=True)
    fused = sum(statistics.median(times[k]) for k in ("pair_stats", "ssim", "psnr"))
    comp = sum(statistics.median(times[k]) for k in ("torch_stats", "torch_ssim", "torch_psnr"))
    print(json.dumps({"part": "total", "fused_us": round(fused, 2), "torch_composition_us": round(comp, 2), "ratio": round(comp / fused, 2), **config}))


if __name__ == "__main__":
    main()
