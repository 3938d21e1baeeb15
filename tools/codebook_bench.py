#!/usr/bin/env python3
"""What fitting the codebook costs: us per call of ops.code_stats, ops.code_usage, ops.codebook_ema and ops.codebook_replace at the
reference's VQ-VAE training shape (8 latents of 16^3: 32 768 rows; K = 512 codes of D = 256, sb_vqvae3d-monai.sbatch), beside
torch.bincount + a float64 index_add_ in the same process (atomics: fast, not in a fixed order).  Two assignments: uniform random
codes, and the adversarial case where one code owns every row, so that one wave per 64 features adds all 32 768 rows in order.  The
procedure is tools/distribution_bench.py's: blocks of --launches calls between two device events, the parts' blocks alternating --reps
times after one warm-up round; the median block and every block.  One JSON line per part and case.

    python tools/codebook_bench.py [--latents 8] [--edge 16] [--codes 512] [--dim 256] [--launches 10] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latents", type=int, default=8)
    ap.add_argument("--edge", type=int, default=16)
    ap.add_argument("--codes", type=int, default=512)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--launches", type=int, default=10, help="calls per timed block")
    ap.add_argument("--reps", type=int, default=5, help="timed blocks per part")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from dm3d_amd import _lib, ops

    _lib.require_device()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    rows, K, D = args.latents * args.edge ** 3, args.codes, args.dim

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.launches

    g = torch.Generator().manual_seed(rows)
    z = torch.randn(rows, D, generator=g).to(dev)
    cases = {"uniform": torch.randint(0, K, (rows,), generator=g, dtype=torch.int32).to(dev),
             "one_code": torch.full((rows,), K // 2, dtype=torch.int32, device=dev)}
    book = torch.randn(K, D, generator=g).to(dev)
    esq, size, ema_w = (book * book).sum(1), torch.ones(K, device=dev), book.clone()
    used = torch.zeros(K, dtype=torch.int32, device=dev)

    for case, idx in cases.items():
        idx64 = idx.long()
        stats = ops.code_stats(z, idx, K)

        def torch_stats():
            counts = torch.bincount(idx64, minlength=K)
            return counts, torch.zeros(K, D, dtype=torch.float64, device=dev).index_add_(0, idx64, z.double())

        def replace():
            used.copy_(stats.counts)                                             # the kernel zeroes it
            ops.codebook_replace(book, esq, used, 1, 1.0, seed=1, cluster_size=size, ema_w=ema_w)

        parts = {"code_stats": lambda: ops.code_stats(z, idx, K), "bincount+index_add_f64": torch_stats,
                 "code_usage": lambda: ops.code_usage(stats.counts, rows), "codebook_ema": lambda: ops.codebook_ema(book, esq, size, ema_w, stats.counts, stats.sums),
                 "codebook_replace": replace}
        times = {}
        for name, fn in parts.items():
            fn()                                                                 # warm-up
            torch.cuda.synchronize()
            times[name] = []
        for _ in range(args.reps):
            for name, fn in parts.items():
                times[name].append(block(fn))
        counts, sums = torch_stats()
        scale = torch.zeros(K, D, dtype=torch.float64, device=dev).index_add_(0, idx64, z.double().abs()).clamp(min=1e-300)
        agree = {"counts_equal": bool(torch.equal(counts.int(), stats.counts)), "sums_max_rel_of_abs_sum": float(((sums - stats.sums).abs() / scale).max())}
        config = {"case": case, "rows": rows, "codes": K, "dim": D, "launches": args.launches}
        for name, ts in times.items():
            print(json.dumps({"part": name, "us_per_call": round(statistics.median(ts), 1), "blocks_us": [round(t, 1) for t in ts], **config}), flush=True)
        print(json.dumps({"part": "agreement", **agree, **config}), flush=True)


if __name__ == "__main__":
    main()
