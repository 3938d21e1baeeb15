#!/usr/bin/env python3
"""What the distribution metrics cost: us per call of ops.feature_moments, ops.knn_radius, ops.prdc_counts, ops.poly_mmd and
metrics.distribution_metrics on N = M rows of D float64 features (two overlapping Gaussian clouds), beside the same numbers from torch
float64 ops in the same process: torch.cov for the moments, |x|^2 + |y|^2 - 2 x.y by matmul with topk for the radii, the same with
comparisons and reductions for the PRDC counts, X @ Y.T for the kernel sums.  The torch route builds the N x M float64 matrices; the
kernels never store them, so the peak device memory of each route (torch.cuda.max_memory_allocated above what was held before the
call) is printed with the times.  The procedure is tools/mask_bench.py's: blocks of --launches calls between two device events, the parts' blocks alternating --reps times
after one warm-up round; the median block and every block.  One JSON line per part and size.

    python tools/distribution_bench.py [--rows 2048 8192] [--dim 256] [--k 5] [--launches 5] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[2048, 8192])
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--launches", type=int, default=5, help="calls per timed block")
    ap.add_argument("--reps", type=int, default=5, help="timed blocks per part")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from dm3d_amd import _lib, metrics, ops

    _lib.require_device()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    D, k = args.dim, args.k

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.launches

    for n in args.rows:
        g = torch.Generator().manual_seed(n)
        real = torch.randn(n, D, generator=g, dtype=torch.float64).to(dev)
        fake = (0.9 * torch.randn(n, D, generator=g, dtype=torch.float64) + 0.3 / D ** 0.5).to(dev)
        r_real, r_fake = ops.knn_radius(real, k), ops.knn_radius(fake, k)

        def torch_d2(x, y):                                                     # the matmul form: torch.cdist refuses 8192 x 8192 float64
            return ((x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * (x @ y.T)).clamp(min=0.0)

        def torch_radius(x):
            return torch_d2(x, x).topk(k + 1, dim=1, largest=False).values[:, k]

        def torch_counts():
            d2 = torch_d2(real, fake)
            return (d2 < r_real[:, None]).sum(0), (d2 < r_fake[None, :]).any(1), d2.min(1).values < r_real

        def torch_sums():
            out = []
            for a, b, within in ((real, real, True), (fake, fake, True), (real, fake, False)):
                kk = (a @ b.T / D + 1.0) ** 3
                out.append(kk.sum() - kk.diagonal().sum() if within else kk.sum())
            return torch.stack(out)

        parts = {"feature_moments": (lambda: ops.feature_moments(real), lambda: (real.mean(0), torch.cov(real.T))),
                 "knn_radius": (lambda: ops.knn_radius(real, k), lambda: torch_radius(real)),
                 "prdc_counts": (lambda: ops.prdc_counts(real, fake, r_real, r_fake), torch_counts),
                 "poly_mmd": (lambda: ops.poly_mmd(real, fake), torch_sums),
                 "distribution_metrics": (lambda: metrics.distribution_metrics(real, fake, nearest_k=k, num_subsets=100, subset_size=1000), None)}
        times, peaks = {}, {}
        for name, routes in parts.items():
            for route, fn in zip(("hip", "torch"), routes):
                if fn is None:
                    continue
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                fn()                                                            # warm-up, and the peak of one call
                torch.cuda.synchronize()
                peaks[name, route] = torch.cuda.max_memory_allocated() - before   # the first matmul's also holds the BLAS workspace
                times[name, route] = []
        for _ in range(args.reps):
            for key in times:
                times[key].append(block(parts[key[0]][0 if key[1] == "hip" else 1]))
        # the two routes agree (the torch route sums in another order and expands the square: to rounding, not to the bit)
        agree = {"radius_max_rel": float(((torch_radius(real) - r_real).abs() / r_real).max()),
                 "counts_equal_share": float((torch_counts()[0] == ops.prdc_counts(real, fake, r_real, r_fake).count_fake).double().mean()),
                 "sums_max_rel": float(((torch_sums() - ops.poly_mmd(real, fake)[0]).abs() / torch_sums().abs()).max())}
        config = {"rows": n, "dim": D, "k": k, "launches": args.launches}
        for (name, route), ts in times.items():
            print(json.dumps({"part": name, "route": route, "us_per_call": round(statistics.median(ts), 1), "blocks_us": [round(t, 1) for t in ts],
                              "peak_bytes": peaks[name, route], **config}), flush=True)
        print(json.dumps({"part": "agreement", **agree, **config}), flush=True)
        del real, fake, r_real, r_fake


if __name__ == "__main__":
    main()
