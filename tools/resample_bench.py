#!/usr/bin/env python3
"""What the device-side preprocessing costs at the reference's shape: one volume of 176 x 256 x 256 at 1 mm resampled into 256^3 (a small
rotation about the centre, the kind of near-axis-aligned matrix a scanner affine gives) and then by 2 into 128^3; B = 1 and B = 8.

Parts, us per call: the prefilter (ops.spline_filter), the resample kernel alone at order 1 (float32 data) and order 3 (float64
coefficients, through the raw entry so the prefilter is not in it), the reslice by 2 into 128^3, ops.volume_normalize and ops.augment at
128^3.  Beside them, in the same process: the same trilinear resample from torch.nn.functional.grid_sample (align_corners=True, zeros
padding; with its grid prebuilt, and with F.affine_grid inside the timed block), the only torch counterpart, torch has no cubic 3-D one; and,
where scipy imports, the CPU time of scipy.ndimage.affine_transform for one volume at orders 1 and 3 (one run each, host clock).  Each
part is printed with the bytes its kernels must move (inputs read once, outputs written once, the coefficient tensor read and written by
every pass).  The times are call times, not kernel times: device events around a block of Python calls, so the wrappers' allocations,
ctypes and launches are in them, and the small parts (normalize, augment, the reslice at B = 1) may be bound by the host; "call_gb_per_s"
is bytes over that call time, a lower bound of what the kernels reach.  Kernel times need a kernel trace in a run of its own, which
was not taken.  A block holds as many calls as fill --window-ms (at least --launches), sized from a warm-up block; the parts' blocks
alternate --reps times; the median block and every block are printed.

    python tools/resample_bench.py [--batches 1 8] [--launches 5] [--window-ms 50] [--reps 5]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_SHAPE, MID, FINAL = (176, 256, 256), (256, 256, 256), (128, 128, 128)


def rotation_about_centres():
    """(matrix [3, 3], offset [3]) mapping output voxels of MID to input voxels of IN_SHAPE: 0.05 rad about each axis, centre to centre."""
    import numpy as np
    a = 0.05
    c, s = np.cos(a), np.sin(a)
    m = np.array([[1, 0, 0], [0, c, -s], [0, s, c]]) @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    return m, (np.array(IN_SHAPE) - 1) / 2.0 - m @ ((np.array(MID) - 1) / 2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--launches", type=int, default=5, help="fewest calls per timed block")
    ap.add_argument("--window-ms", type=float, default=50.0, help="a timed block holds as many calls as fill this window")
    ap.add_argument("--reps", type=int, default=5, help="timed blocks per part")
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import torch.nn.functional as F
    from dm3d_amd import _lib, ops

    _lib.require_device()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    m, off = rotation_about_centres()
    vin, vmid, vfin = (int(np.prod(s)) for s in (IN_SHAPE, MID, FINAL))

    def block(fn, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches

    for B in args.batches:
        g = torch.Generator().manual_seed(0)
        x = torch.rand(B, *IN_SHAPE, generator=g).to(dev)
        coeff = ops.spline_filter(x)
        table = torch.from_numpy(np.tile(np.concatenate([m.reshape(9), off]), (B, 1))).to(dev)
        out3 = torch.empty(B, *MID, dtype=torch.float32, device=dev)
        mid = ops.affine_transform(x, m, off, MID, order=1)
        small = ops.affine_transform(mid, (2.0, 2.0, 2.0), output_shape=FINAL, order=1)
        images = ops.volume_normalize(small).out.unsqueeze(-1).contiguous()
        masks = (images > 0.5).float()

        def resample3():
            d = _lib.ResampleDesc()
            d.src, d.table, d.out, d.in_f64 = coeff.data_ptr(), table.data_ptr(), out3.data_ptr(), _lib.RESAMPLE_F64
            d.volumes, d.id, d.ih, d.iw = coeff.shape
            d.od, d.oh, d.ow = MID
            d.order, d.cval = 3, 0.0
            _lib.check(_lib.lib().dm3d_affine_resample(C.byref(d), torch.cuda.current_stream().cuda_stream), "affine_resample")

        # torch's counterpart: x_in = M o + offset in voxels, as normalised (x, y, z) coordinates with align_corners=True
        size_in, size_out = np.array(IN_SHAPE, np.float64) - 1, np.array(MID, np.float64) - 1
        lin = np.diag(2.0 / size_in) @ m @ np.diag(size_out / 2.0)
        trans = np.diag(2.0 / size_in) @ (m @ (size_out / 2.0) + off) - 1.0
        theta = np.concatenate([lin[::-1, ::-1], trans[::-1, None]], 1)      # grid_sample's axes run x, y, z
        theta = torch.from_numpy(np.ascontiguousarray(theta)).float().to(dev).expand(B, 3, 4).contiguous()
        x5 = x.unsqueeze(1)
        grid = F.affine_grid(theta, (B, 1) + MID, align_corners=True)
        ref = F.grid_sample(x5, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
        # the central 128^3 outputs, whose taps all lie inside the input: at the border the two differ by definition (zeros padding blends the
        # edge with zeros, scipy's rule gives cval from the first coordinate outside).  float32 coordinates against float64 ones: not a parity bar
        inner = (slice(None), slice(64, 192), slice(64, 192), slice(64, 192))
        agree = float((ref[inner] - mid[inner]).abs().max())
        del ref

        parts = {"spline_filter": lambda: ops.spline_filter(x),
                 "affine_resample_order1": lambda: ops.affine_transform(x, m, off, MID, order=1),
                 "affine_resample_order3": resample3,
                 "affine_transform_order3_with_prefilter": lambda: ops.affine_transform(x, m, off, MID, order=3),
                 "reslice_by_2_order1": lambda: ops.affine_transform(mid, (2.0, 2.0, 2.0), output_shape=FINAL, order=1),
                 "volume_normalize": lambda: ops.volume_normalize(small),
                 "augment": lambda: ops.augment(images, masks, seed=1),
                 "torch_grid_sample": lambda: F.grid_sample(x5, grid, mode="bilinear", padding_mode="zeros", align_corners=True),
                 "torch_affine_grid_and_grid_sample": lambda: F.grid_sample(x5, F.affine_grid(theta, (B, 1) + MID, align_corners=True), mode="bilinear",
                                                                            padding_mode="zeros", align_corners=True)}
        moved = {"spline_filter": B * vin * (4 + 8 + 2 * 16),                 # w: float32 in, float64 out; h, d: float64 in and out
                 "affine_resample_order1": B * (vin * 4 + vmid * 4),
                 "affine_resample_order3": B * (vin * 8 + vmid * 4),
                 "reslice_by_2_order1": B * (vmid * 4 + vfin * 4),
                 "volume_normalize": B * vfin * (4 + 4 + 4),                  # read for the extrema, read again, written
                 "augment": B * vfin * (4 + 4 + 4 + 4 + 4),                   # image read twice and written, mask read and written
                 "torch_grid_sample": B * (vin * 4 + vmid * 12 + vmid * 4),
                 "torch_affine_grid_and_grid_sample": B * (vin * 4 + 2 * vmid * 12 + vmid * 4)}
        moved["affine_transform_order3_with_prefilter"] = moved["spline_filter"] + moved["affine_resample_order3"]
        times, launches = {k: [] for k in parts}, {}
        for k, fn in parts.items():                                         # warm-up, and the size of a block
            block(fn, 1)
            launches[k] = min(5000, max(args.launches, int(args.window_ms * 1e3 / block(fn, 3)) + 1))
        for rep in range(args.reps):
            for k, fn in parts.items():
                times[k].append(block(fn, launches[k]))
        config = {"batch": B, "in_shape": IN_SHAPE}
        for k, ts in times.items():
            med = statistics.median(ts)
            print(json.dumps({"part": k, "us_per_call": round(med, 1), "blocks_us": [round(t, 1) for t in ts], "calls_per_block": launches[k],
                              "bytes_moved": moved[k], "call_gb_per_s": round(moved[k] / med / 1e3, 1), **config}), flush=True)
        print(json.dumps({"part": "grid_sample_agreement", "worst_abs_diff_interior": agree, **config}), flush=True)
        del x, coeff, out3, mid, small, images, masks, grid, x5
        torch.cuda.empty_cache()

    if args.no_scipy:
        return
    try:
        import scipy.ndimage as ndi
    except ImportError:
        print(json.dumps({"part": "scipy_cpu", "note": "scipy does not import on this machine: not measured"}))
        return
    v = np.random.default_rng(0).random(IN_SHAPE, dtype=np.float32)
    for order in (1, 3):
        t0 = time.perf_counter()
        ndi.affine_transform(v, m, off, MID, order=order, mode="constant")
        print(json.dumps({"part": f"scipy_cpu_affine_transform_order{order}", "seconds_one_volume": round(time.perf_counter() - t0, 3),
                          "threads": 1}), flush=True)


if __name__ == "__main__":
    main()
