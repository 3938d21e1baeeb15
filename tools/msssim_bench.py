#!/usr/bin/env python3
"""What the 3-D multi-scale SSIM costs: us per call of ops.ms_ssim at B = 8 pairs of 128^3 x 1 channel, 4 scales, 11 taps, and of
metrics.pairwise_ms_ssim over 10 volumes of 128^3 (45 pairs), and, on the same card in the same process, of the composition of torch ops
a user without these kernels would run (the separable window as three F.conv3d over each of the four moment maps, the formula, the
means, F.avg_pool3d between scales, the powers).  Also the per-launch times of the kernels behind ops.ms_ssim: the tile pass of each scale
(a call with that scale's volumes and one scale, so with its sum launch) and what the pooling launches add (a two-scale call minus the
two single-scale calls: two pooling launches less one sum launch), which bounds what pooling fused into the tile pass could save.  One
JSON line per part.  The procedure is tools/metrics_bench.py's: blocks of --launches calls between two device events, the parts' blocks
alternating --reps times after one warm-up round; the median block and every block, so the spread can be read off.

    python tools/msssim_bench.py [--batch 8] [--volumes 10] [--size 128] [--scales 4] [--launches 10] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--volumes", type=int, default=10)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--scales", type=int, default=4)
    ap.add_argument("--launches", type=int, default=10, help="calls per timed block")
    ap.add_argument("--reps", type=int, default=5, help="timed blocks per part")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    from dm3d_amd import _lib, metrics, ops

    _lib.require_device()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    B, N, S, M = args.batch, args.volumes, args.size, args.scales
    power = ops.MS_SSIM_POWER_FACTORS[:M]
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, S, S, S, 1, generator=g).to(dev)
    y = (x + 0.03 * torch.randn(B, S, S, S, 1, generator=g).to(dev)).contiguous()
    base = torch.rand(1, S, S, S, 1, generator=g)
    vols = (base + 0.05 * torch.randn(N, S, S, S, 1, generator=g)).to(dev).contiguous()
    L = 1.0
    i = torch.arange(11, dtype=torch.float64)
    win = torch.exp(-(i - 5) ** 2 / 4.5)
    win = (win / win.sum()).float().to(dev)
    ww, wh, wd = win.reshape(1, 1, 1, 1, 11), win.reshape(1, 1, 1, 11, 1), win.reshape(1, 1, 11, 1, 1)
    wp = torch.tensor(power, dtype=torch.float64, device=dev)

    def torch_ms_ssim(a, b):
        """a, b [P, 1, S, S, S] (one channel): [P] float32."""
        filt = lambda v: F.conv3d(F.conv3d(F.conv3d(v, ww), wh), wd)
        c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
        prod = torch.ones(a.shape[0], dtype=torch.float64, device=dev)
        for j in range(M):
            if j:
                a, b = F.avg_pool3d(a, 2), F.avg_pool3d(b, 2)
            mx, my, sxy, sq = filt(a), filt(b), filt(a * b), filt(a * a + b * b)
            n0, d0 = 2 * mx * my, mx * mx + my * my
            cs = (2 * sxy - n0 + c2) / (sq - d0 + c2)
            term = (cs * ((n0 + c1) / (d0 + c1)) if j == M - 1 else cs).double().mean(dim=(1, 2, 3, 4))
            prod = prod * term.clamp(min=0) ** wp[j]
        return prod.float()

    xt, yt = x.reshape(B, 1, S, S, S), y.reshape(B, 1, S, S, S)
    vt = vols.reshape(N, 1, S, S, S)
    pi = torch.triu_indices(N, N, 1, device=dev)
    kw = dict(power_factors=power, filter_size=11)
    # the volumes of every scale, for the per-launch parts
    xs, ys = [x], [y]
    for j in range(1, M):
        pool = lambda v: F.avg_pool3d(v.reshape(B, 1, *v.shape[1:4]), 2).reshape(B, v.shape[1] // 2, v.shape[2] // 2, v.shape[3] // 2, 1).contiguous()
        xs.append(pool(xs[-1])), ys.append(pool(ys[-1]))

    parts = {"ms_ssim": lambda: ops.ms_ssim(x, y, L, **kw),
             "torch_ms_ssim": lambda: torch_ms_ssim(xt, yt),
             "pairwise_ms_ssim": lambda: metrics.pairwise_ms_ssim(vols, L, **kw),
             "torch_pairwise_ms_ssim": lambda: torch_ms_ssim(vt[pi[0]], vt[pi[1]])}
    for j in range(M):
        parts[f"tile_scale{j}"] = lambda j=j: ops.ms_ssim(xs[j], ys[j], L, power_factors=(1.0,), filter_size=11)
    if M > 1:
        parts["tile_scale0+pool+tile_scale1"] = lambda: ops.ms_ssim(x, y, L, power_factors=power[:2], filter_size=11)
    # the two paths agree (float32 filtering in another order: 1e-4 is far above either's error and far below a wrong formula's)
    err = float((parts["ms_ssim"]() - parts["torch_ms_ssim"]()).abs().max())
    err_pw = float((parts["pairwise_ms_ssim"]() - parts["torch_pairwise_ms_ssim"]()).abs().max())
    assert err < 1e-4 and err_pw < 1e-4, (err, err_pw)

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
    config = {"batch": B, "volumes": N, "size": S, "scales": M, "filter_size": 11, "launches": args.launches,
              "max_abs_diff_vs_torch": err, "pairwise_max_abs_diff_vs_torch": err_pw}
    med = {k: statistics.median(ts) for k, ts in times.items()}
    for k, ts in times.items():
        print(json.dumps({"part": k, "us_per_call": round(med[k], 2), "blocks_us": [round(t, 2) for t in ts], **config}), flush=True)
    total = {"part": "total", "ms_ssim_ratio": round(med["torch_ms_ssim"] / med["ms_ssim"], 2),
             "pairwise_ratio": round(med["torch_pairwise_ms_ssim"] / med["pairwise_ms_ssim"], 2), **config}
    if M > 1:
        total["two_scale_minus_single_scale_calls_us"] = round(med["tile_scale0+pool+tile_scale1"] - med["tile_scale0"] - med["tile_scale1"], 2)
        total["its_share_of_ms_ssim"] = round(total["two_scale_minus_single_scale_calls_us"] / med["ms_ssim"], 4)
    print(json.dumps(total))


if __name__ == "__main__":
    main()
