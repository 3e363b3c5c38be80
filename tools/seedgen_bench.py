#!/usr/bin/env python3
"""Seconds per subject of `seedgen.generate_seeds` at 256^3, max_subclasses 10, on a phantom subject.

    python tools/seedgen_bench.py [--size 256] [--max_subclasses 10] [--repeats 5]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/seedgen_bench.py --repeats 1     (per-kernel times)

One warm-up call, then `--repeats` timed calls (wall clock around a device synchronise).  Prints one JSON line: the
median / min / max seconds per subject, the voxel count per meta-label, and -- from HIP events around the three native
stages -- the seconds inside fusion + compaction, the EM batch and the assignment; the rest of a subject's time is host
work (k-means++ centres, tables) and launch gaps.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def phantom_subject(size, seed=0):
    """Nested ellipsoids labelled like a FeTA dseg, a textured T2w-like image, and non-brain signal around it."""
    rng = np.random.default_rng(seed)
    g = np.linspace(-1, 1, size, dtype=np.float32)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    r = np.sqrt((x / 0.8) ** 2 + (y / 0.7) ** 2 + (z / 0.75) ** 2)
    seg = np.zeros((size,) * 3, np.uint8)
    for lab, rad in ((1, 0.62), (2, 0.56), (3, 0.48), (4, 0.2), (5, 0.3), (6, 0.12), (7, 0.08)):
        seg[r < rad] = lab if lab != 5 else 3
    seg[(r < 0.3) & (r >= 0.2)] = 5
    base = np.array([0, 2000, 1200, 1700, 2100, 1500, 1100, 1300], np.float32)[seg]
    img = base + 80 * np.sin(9 * x) * np.cos(7 * y) + rng.normal(0, 60, seg.shape).astype(np.float32)
    img[(seg == 0) & (r >= 0.8)] = 0
    img[(seg == 0) & (r < 0.8)] = np.abs(rng.normal(500, 250, int(((seg == 0) & (r < 0.8)).sum()))).astype(np.float32) + 1
    return img.astype(np.float32), seg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--max_subclasses", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from fetalsyngen_amd import seedgen

    img, seg = phantom_subject(args.size)
    dev = "cuda:0"
    image, dseg = torch.from_numpy(img).to(dev), torch.from_numpy(seg).to(dev)
    seedgen.generate_seeds(image, dseg, args.max_subclasses, key=1)  # warm-up: library load, allocator, code objects
    torch.cuda.synchronize()
    times = []
    for r in range(args.repeats):
        t0 = time.perf_counter()
        seedgen.generate_seeds(image, dseg, args.max_subclasses, key=r)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)

    # stage times from events: the same calls `generate_seeds` makes, one after the other
    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return out, a.elapsed_time(b) / 1e3

    (meta, counts, px, pidx), t_fuse = timed(lambda: seedgen.meta_pack(image, dseg, "feta"))
    t0 = time.perf_counter()
    offs = np.concatenate([[0], np.cumsum(counts)])
    batch = seedgen._Batch(seedgen._lib.load())
    for m in range(1, 5):
        sample = px[torch.from_numpy(seedgen.subsample_index(counts[m - 1]) + offs[m - 1]).to(dev)].cpu().numpy()
        for k in range(2, args.max_subclasses + 1):
            for init in range(seedgen.N_INIT):
                batch.add(offs[m - 1], counts[m - 1], k, 100, 1, 1e-3, mu=seedgen.kmeanspp_means(sample, k, 0, m, init))
    t_host = time.perf_counter() - t0
    fit, t_em = timed(lambda: seedgen._Fit(px, batch))
    _params, _lb, status = fit.results()
    print(json.dumps({
        "size": args.size, "max_subclasses": args.max_subclasses, "voxels_per_meta_label": counts, "jobs": len(batch.rows),
        "seconds_per_subject_median": float(np.median(times)), "seconds_per_subject_min": min(times),
        "seconds_per_subject_max": max(times), "seconds_fusion_compaction": t_fuse, "seconds_em_batch": t_em,
        "seconds_host_init": t_host, "em_iterations_mean": float(status[:, 0].mean()), "em_iterations_max": int(status[:, 0].max()),
    }))


if __name__ == "__main__":
    main()
