#!/usr/bin/env python3
"""What the device-side spatial augmentation costs: one and eight volumes of 128^3 and of 256^3 (NDHWC, one channel, with a mask).

Parts, us per call: ops.gaussian_filter (sigma 4, radius 16, mode "reflect"), ops.elastic_field (alpha 30, sigma 4: the draw, three
passes in place and the scaling), ops.warp at orders 1 and 3 (a field and a small rotation about the centre; order 3 with its
prefilter) and data.spatial_augment (the field, then image at order 1 and mask at order 0).  Beside them, in the same process, a torch
form: the Gaussian as three F.conv3d with 1-D kernels (zero padding, so only the interior is the same filter) and the trilinear warp as
F.grid_sample (align_corners=True, zeros padding) on a prebuilt grid that holds the same coordinates.  Where scipy imports, the CPU time
of scipy.ndimage.gaussian_filter and map_coordinates (order 1) for one volume (one run each, host clock).  The times are call times,
not kernel times: device events around a block of Python calls, so the wrappers' allocations, ctypes and launches are in them.  A block
holds as many calls as fill --window-ms (at least --launches), sized from a warm-up block; the parts' blocks alternate --reps times;
the median block and every block are printed.

    python tools/deform_bench.py [--sizes 128 256] [--batches 1 8] [--launches 3] [--window-ms 50] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA, ALPHA = 4.0, 30.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--launches", type=int, default=3, help="fewest calls per timed block")
    ap.add_argument("--window-ms", type=float, default=50.0, help="a timed block holds as many calls as fill this window")
    ap.add_argument("--reps", type=int, default=5, help="timed blocks per part")
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import torch.nn.functional as F
    from dm3d_amd import _lib, data, ops

    _lib.require_device()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")

    def block(fn, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches

    for n in args.sizes:
        shape = (n, n, n)
        matrix = data.affine_matrices(shape, 1, seed=1, rotate_range=0.05)[0]
        radii, table = ops._gauss_table(SIGMA, 4.0)
        taps = torch.from_numpy(np.concatenate([table[0, radii[0]:0:-1], table[0, :radii[0] + 1]])).float().to(dev)
        for B in args.batches:
            g = torch.Generator().manual_seed(0)
            images = torch.rand(B, *shape, 1, generator=g).to(dev)
            masks = (images > 0.5).float()
            planar = images.view(B, *shape)
            field = ops.elastic_field(shape, B, ALPHA, SIGMA, seed=1, device=dev)
            warped = ops.warp(planar, field, matrix, order=1)
            # torch's forms: the separable Gaussian as three conv3d, the warp as grid_sample at the same coordinates (normalised x, y, z)
            x5 = planar.unsqueeze(1)
            kernels = [taps.view(1, 1, -1, 1, 1), taps.view(1, 1, 1, -1, 1), taps.view(1, 1, 1, 1, -1)]
            pads = [(radii[0], 0, 0), (0, radii[0], 0), (0, 0, radii[0])]

            def torch_gauss():
                t = x5
                for k, p in zip(kernels, pads):
                    t = F.conv3d(t, k, padding=p)
                return t

            ours = ops.gaussian_filter(planar, SIGMA)
            r = radii[0]
            inner = (slice(None), slice(r, n - r), slice(r, n - r), slice(r, n - r))
            gauss_agree = float((torch_gauss()[:, 0][inner] - ours[inner]).abs().max())
            m64 = torch.from_numpy(matrix).to(dev)
            idx = torch.stack(torch.meshgrid(*(torch.arange(n, dtype=torch.float64, device=dev) for _ in range(3)), indexing="ij"))
            coords = torch.einsum("hk,kdyx->hdyx", m64[:3, :3], idx) + m64[:3, 3].view(3, 1, 1, 1) + field.double()          # [B, 3, n, n, n]
            grid = (coords * (2.0 / (n - 1)) - 1.0).flip(1).permute(0, 2, 3, 4, 1).float().contiguous()
            del coords, idx
            ref = F.grid_sample(x5, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
            both = (warped != 0) & (ref != 0)
            warp_agree = float(((ref - warped).abs() * both)[inner].max())              # away from the border, where the two rules differ
            del ref, both, ours

            parts = {"gaussian_filter": lambda: ops.gaussian_filter(planar, SIGMA),
                     "elastic_field": lambda: ops.elastic_field(shape, B, ALPHA, SIGMA, seed=1, device=dev),
                     "warp_order1": lambda: ops.warp(planar, field, matrix, order=1),
                     "warp_order3_with_prefilter": lambda: ops.warp(planar, field, matrix, order=3),
                     "spatial_augment": lambda: data.spatial_augment(images, masks, seed=1, rotate_range=0.05, elastic_alpha=ALPHA, elastic_sigma=SIGMA),
                     "torch_conv3d_gaussian": torch_gauss,
                     "torch_grid_sample": lambda: F.grid_sample(x5, grid, mode="bilinear", padding_mode="zeros", align_corners=True)}
            vox = B * n ** 3
            moved = {"gaussian_filter": vox * 4 * 6,                              # three passes, each read and written
                     "elastic_field": vox * 3 * 4 * 9,                            # written by the draw, three passes and the scaling read and write
                     "warp_order1": vox * 4 * (1 + 3 + 1),                        # the volume, the field, the output
                     "warp_order3_with_prefilter": vox * (4 + 8 + 2 * 16) + vox * (8 + 12 + 4),
                     "torch_conv3d_gaussian": vox * 4 * 6,
                     "torch_grid_sample": vox * 4 * (1 + 3 + 1)}
            moved["spatial_augment"] = moved["elastic_field"] + 2 * moved["warp_order1"]
            times, launches = {k: [] for k in parts}, {}
            for k, fn in parts.items():                                         # warm-up, and the size of a block
                block(fn, 1)
                launches[k] = min(5000, max(args.launches, int(args.window_ms * 1e3 / block(fn, 2)) + 1))
            for rep in range(args.reps):
                for k, fn in parts.items():
                    times[k].append(block(fn, launches[k]))
            config = {"batch": B, "shape": shape}
            for k, ts in times.items():
                med = statistics.median(ts)
                print(json.dumps({"part": k, "us_per_call": round(med, 1), "blocks_us": [round(t, 1) for t in ts], "calls_per_block": launches[k],
                                  "bytes_moved": moved[k], "call_gb_per_s": round(moved[k] / med / 1e3, 1), **config}), flush=True)
            print(json.dumps({"part": "torch_agreement", "gaussian_worst_abs_diff_interior": gauss_agree, "warp_worst_abs_diff_interior": warp_agree,
                              **config}), flush=True)
            del images, masks, planar, field, warped, x5, grid
            torch.cuda.empty_cache()

    if args.no_scipy:
        return
    try:
        import scipy.ndimage as ndi
    except ImportError:
        print(json.dumps({"part": "scipy_cpu", "note": "scipy does not import on this machine: not measured"}))
        return
    for n in args.sizes:
        v = np.random.default_rng(0).random((n, n, n), dtype=np.float32)
        t0 = time.perf_counter()
        u = np.stack([ndi.gaussian_filter(np.random.default_rng(h + 1).random((n, n, n), dtype=np.float32) * 2 - 1, SIGMA, mode="constant") for h in range(3)])
        t_field = time.perf_counter() - t0
        t0 = time.perf_counter()
        ndi.gaussian_filter(v, SIGMA)
        t_gauss = time.perf_counter() - t0
        grid = np.stack(np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij"))
        t0 = time.perf_counter()
        ndi.map_coordinates(v, grid + ALPHA * u, order=1, mode="constant")
        t_map = time.perf_counter() - t0
        print(json.dumps({"part": "scipy_cpu", "shape": (n, n, n), "gaussian_filter_s": round(t_gauss, 3), "elastic_field_s": round(t_field, 3),
                          "map_coordinates_order1_s": round(t_map, 3), "threads": 1}), flush=True)


if __name__ == "__main__":
    main()
