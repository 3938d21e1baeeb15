#!/usr/bin/env python3
"""What the mask-channel scores cost: us per call of ops.mask_overlap, ops.distance_transform, ops.surface_distances and
metrics.mask_metrics at B = 8 volumes of 128^3 x 1 channel (a few ellipsoids against a perturbed copy of them).  Torch has no exact 3-D
distance transform, so there is no composition of torch ops to set beside them; each part is printed with the bytes its passes must move
(the float32 tensors read once, uint8 features written and read, the int32 map written by the w pass and read and written by the h and
d passes), so the time can be read against the memory traffic.  The procedure is tools/metrics_bench.py's: blocks of --launches calls
between two device events, the parts' blocks alternating --reps times after one warm-up round; the median block and every block, so the
spread can be read off.  One JSON line per part.

    python tools/mask_bench.py [--batch 8] [--size 128] [--launches 10] [--reps 5]"""
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
    ap.add_argument("--launches", type=int, default=10, help="calls per timed block")
    ap.add_argument("--reps", type=int, default=5, help="timed blocks per part")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from dm3d_amd import _lib, metrics, ops

    _lib.require_device()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    g = torch.Generator().manual_seed(0)
    ax = torch.arange(S, dtype=torch.float32)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")

    def blobs(shift):
        vols = []
        for _ in range(B):
            m = torch.zeros(S, S, S, dtype=torch.bool)
            for _ in range(3):
                c = torch.rand(3, generator=g) * (S - 1)
                r = (0.1 + 0.15 * torch.rand(1, generator=g)) * S
                m |= (z - c[0] - shift) ** 2 + (y - c[1]) ** 2 + (x - c[2] + shift) ** 2 <= r * r
            vols.append(m)
        return torch.stack(vols)[..., None]

    g.manual_seed(0)
    truth = blobs(0.0)
    g.manual_seed(0)
    other = blobs(2.5)
    noise = torch.rand(B, S, S, S, 1, generator=g)
    xt = (truth.float() * 0.6 + noise * 0.39).to(dev).contiguous()          # mask: above 0.6; background: below 0.39
    yt = (other.float() * 0.6 + noise * 0.39).to(dev).contiguous()

    parts = {"mask_overlap": lambda: ops.mask_overlap(xt, yt),
             "distance_transform": lambda: ops.distance_transform(xt),
             "surface_distances": lambda: ops.surface_distances(xt, yt),
             "mask_metrics": lambda: metrics.mask_metrics(xt, yt)}
    vox = B * S ** 3
    bins = 3 * (S - 1) ** 2 + 1
    edt_bytes = vox * (1 + 4) + 2 * vox * 8                                    # w pass: features in, map out; h and d: map in and out
    moved = {"mask_overlap": 2 * vox * 4,
             "distance_transform": vox * 4 + vox + edt_bytes,
             "surface_distances": 2 * vox * 4 + 2 * vox + 2 * (edt_bytes + vox * 5) + 3 * 2 * B * (bins + 1) * 4}
    moved["mask_metrics"] = moved["surface_distances"]
    m = parts["mask_metrics"]()
    torch.cuda.synchronize()
    scores = {k: [round(v, 4) for v in m[k].reshape(-1).tolist()] for k in ("dice", "hd_percentile", "assd")}

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
    config = {"batch": B, "size": S, "channels": 1, "launches": args.launches}
    for k, ts in times.items():
        med = statistics.median(ts)
        print(json.dumps({"part": k, "us_per_call": round(med, 2), "blocks_us": [round(t, 2) for t in ts], "bytes_moved": moved[k],
                          "gb_per_s": round(moved[k] / med / 1e3, 1), **config}), flush=True)
    print(json.dumps({"part": "scores", **scores, **config}))


if __name__ == "__main__":
    main()
