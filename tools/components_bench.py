#!/usr/bin/env python3
"""What connected components cost: us per call of ops.connected_components at each connectivity, of each filter of ops.component_filter
and of data.clean_mask, at B = 8 volumes of 128^3 x 1 channel, on two inputs: an ellipsoid with specks around it and cavities inside
it (what a predicted brain mask looks like), and a 30 % speckle (hundreds of thousands of components: the many-components case).  Torch
has no connected-component labelling, so there is no composition of torch ops to set beside them; each call is printed with the bytes
its passes must move (the float32 tensor read once, the int32 parent, size and root planes written and read by the passes that touch
them, the output written once), so the time can be read against the memory traffic.  Where scipy is installed, scipy.ndimage.label
and binary_fill_holes run on this machine's CPU over the same inputs, in this process, as the yardstick.  The procedure is
tools/mask_bench.py's: blocks of --launches calls between two device events, the parts' blocks alternating --reps times after one
warm-up round; the median block and every block.  One JSON line per part.

    python tools/components_bench.py [--batch 8] [--size 128] [--launches 5] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--launches", type=int, default=5, help="calls per timed block")
    ap.add_argument("--reps", type=int, default=5, help="timed blocks per part")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from dm3d_amd import _lib, data, ops

    _lib.require_device()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    g = torch.Generator().manual_seed(0)
    ax = torch.arange(S, dtype=torch.float32)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")

    def brain():
        vols = []
        for _ in range(B):
            c = (0.45 + 0.1 * torch.rand(3, generator=g)) * S
            r = (0.3 + 0.1 * torch.rand(3, generator=g)) * S
            m = ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0
            m ^= torch.rand(S, S, S, generator=g) < 0.002                      # specks outside, one-voxel cavities inside
            for _ in range(3):                                                  # larger cavities
                h = c + (torch.rand(3, generator=g) - 0.5) * 0.3 * S
                m &= (z - h[0]) ** 2 + (y - h[1]) ** 2 + (x - h[2]) ** 2 > (0.04 * S) ** 2
            vols.append(m)
        return torch.stack(vols)[..., None]

    inputs = {"brain": brain(), "speckle30": torch.rand(B, S, S, S, 1, generator=g) < 0.3}
    noise = torch.rand(B, S, S, S, 1, generator=g)
    tensors = {k: (m.float() * 0.6 + noise * 0.39).to(dev).contiguous() for k, m in inputs.items()}   # mask: above 0.6; background: below 0.39

    vox = B * S ** 3
    unions = vox * 4 + 2 * vox * 4 + 2 * vox * 4                               # x in, parent and size out; the seam pass reads parents; flatten reads parent, writes root
    labelled = unions + 2 * vox * 4 + 3 * vox * 4                              # count and rank read the roots; the label pass reads and writes labels, reads ranks
    filtered = unions + 2 * vox * 4                                            # the filter reads root, writes out (sizes are read where a voxel is kept)
    parts, moved = {}, {}
    for name, t in tensors.items():
        for conn in (6, 18, 26):
            parts[f"{name}/connected_components/{conn}"] = lambda t=t, conn=conn: ops.connected_components(t, connectivity=conn)
            moved[f"{name}/connected_components/{conn}"] = labelled
        parts[f"{name}/filter/largest"] = lambda t=t: ops.component_filter(t, keep="largest")
        parts[f"{name}/filter/min_size"] = lambda t=t: ops.component_filter(t, min_size=8)
        parts[f"{name}/filter/fill_holes"] = lambda t=t: ops.component_filter(t, fill_holes=True)
        parts[f"{name}/clean_mask"] = lambda t=t: data.clean_mask(t)
        moved[f"{name}/filter/largest"] = filtered + vox * 4
        moved[f"{name}/filter/min_size"] = moved[f"{name}/filter/fill_holes"] = filtered
        moved[f"{name}/clean_mask"] = 2 * filtered + vox * 4

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
    for name, t in tensors.items():
        comp = ops.connected_components(t)
        print(json.dumps({"part": f"{name}/result", "components": comp.count.reshape(-1).tolist(),
                          "largest_size": comp.largest[..., 1].reshape(-1).tolist(), **config}), flush=True)
    try:
        from scipy import ndimage as ndi
    except ImportError:
        print(json.dumps({"part": "scipy", "note": "scipy is not installed: no CPU yardstick", **config}))
        return
    for name, m in inputs.items():
        vols = m[..., 0].numpy()
        t0 = time.perf_counter()
        counts = [int(ndi.label(v)[1]) for v in vols]
        t1 = time.perf_counter()
        for v in vols:
            ndi.binary_fill_holes(v)
        t2 = time.perf_counter()
        print(json.dumps({"part": f"{name}/scipy_cpu", "label_us": round((t1 - t0) * 1e6, 0), "fill_holes_us": round((t2 - t1) * 1e6, 0),
                          "components": counts, **config}), flush=True)


if __name__ == "__main__":
    main()
