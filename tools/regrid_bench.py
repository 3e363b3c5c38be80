#!/usr/bin/env python3
"""Microseconds per launch of `fsg_affine_resample` at 256^3 -> 256^3, float32 image + uint8 label in one launch.

    python tools/regrid_bench.py [--size 256] [--reps 20]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/regrid_bench.py --reps 5      (per-kernel times, a run of its own)

Transforms: the axis-aligned 2x up-sampling of a 1 mm -> 0.5 mm regrid, an axis-aligned half-voxel shift at unit scale, and
unit-scale rotations of 12 and 20 degrees about every axis (the angles the warp's figures in DESIGN.md section 4 are quoted
at), all about the centre of the volume.  Also the foreground box of the image.  Three warm-up launches, then `--reps`
launches between two HIP events.  One JSON line per case; GBps counts 5 bytes read and 5 written per voxel.
The yardstick is the fused warp on the same volumes: `python tools/kernel_bench.py --only warp_f32_u8_epi_ws --rot 0|12|20`.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def rotation(deg):
    r = np.deg2rad(deg)
    c, s = np.cos(r), np.sin(r)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, c, s], [0, -s, c]])   # -r about x
    Ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return Rz @ Rx @ Ry


def centred(A, n, shift=0.0):
    c = (n - 1) / 2.0
    return np.concatenate([A, (c - A @ np.full(3, c) + shift)[:, None]], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from fetalsyngen_amd import kernels as K
    from fetalsyngen_amd.phantom import make_seed_volumes

    n, dev = args.size, "cuda:0"
    seg, _seeds = make_seed_volumes((n, n, n))
    rng = np.random.default_rng(0)
    label = torch.from_numpy(seg.astype(np.uint8)).to(dev)
    image = torch.from_numpy((seg * 30 + rng.random(seg.shape) * 5).astype(np.float32)).to(dev)
    box = [0, n - 1] * 3
    cases = {"aligned_2x": centred(np.eye(3) * 0.5, n), "aligned_1x_half_voxel": centred(np.eye(3), n, 0.5),
             "oblique_12": centred(rotation(12), n), "oblique_20": centred(rotation(20), n)}

    def timeit(name, fn, nbytes):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.reps
        print(json.dumps({"case": name, "us": round(us, 2), "GBps": round(nbytes / us / 1e3, 1)}), flush=True)

    for name, M in cases.items():
        timeit(name, lambda M=M: K.affine_resample(image, label, M, box, (n, n, n)), 10 * n ** 3)
        timeit(name + "_image_only", lambda M=M: K.affine_resample(image, None, M, box, (n, n, n)), 8 * n ** 3)
    timeit("bbox_gt", lambda: K.bbox_gt(image), 4 * n ** 3)


if __name__ == "__main__":
    main()
