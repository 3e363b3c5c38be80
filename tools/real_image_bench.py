#!/usr/bin/env python3
"""Volumes/s and host microseconds per sample of real-image samples (the reference's `real_train` recipe: `load_image`,
with and without `image_as_intensity`) at 256^3, every gate on, phantom subjects.

    python tools/real_image_bench.py [--size 256] [--steps 40] [--warmup 8] [--subjects 4] [--batch 8]
    python tools/real_image_bench.py --warp-only --steps 10   under `rocprofv3 --kernel-trace --stats`, a run of its own:
        the dual-source warp launch against the two launches it replaces (per-kernel times from the trace)

Per configuration -- `image_as_intensity` (no seeds: the image is the prior) and `load_image` with seeds -- three legs in one
process: keyed single samples (each naming the next key), keyed `sample_batch` (two streams), and the stage-wise path
(`rng="device"`, what a real-image sample took before).  A leg is timed between two HIP events around `--steps` samples after
`--warmup`; host_us is the wall time of issuing them (no synchronisation inside).  One JSON line per leg.  On a build from
before the keyed image path (the other side of an A/B) a keyed single sample with an image falls back to the stage-wise path by
itself, and keyed `sample_batch` raises its "outside the fused keyed path" ValueError: only that one is reported as
{"skipped": reason}; any other exception is a failure and ends the run.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def generator(shape, dev, rng):
    from fetalsyngen_amd.generator.augmentation.synthseg import RandBiasField, RandGamma, RandNoise, RandResample
    from fetalsyngen_amd.generator.deformation.affine_nonrigid import SpatialDeformation
    from fetalsyngen_amd.generator.intensity.rand_gmm import ImageFromSeeds
    from fetalsyngen_amd.generator.model import FetalSynthGen

    labels = [0] + list(range(10, 50))
    classes = [0] + [10] * 10 + [20] * 10 + [30] * 10 + list(range(40, 50))
    return FetalSynthGen(
        shape=list(shape), resolution=[0.5, 0.5, 0.5], device=dev, intensity_generator=ImageFromSeeds(1, 6, labels, classes),
        spatial_deform=SpatialDeformation(20, 0.02, 0.1, list(shape), 1.0, True, 0.03, 0.06, 4, 0.5, dev),
        resampler=RandResample(1.0, 0.5, 1.5), bias_field=RandBiasField(1.0, 0.004, 0.02, 0.01, 0.3),
        noise=RandNoise(1.0, 5, 15), gamma=RandGamma(1.0, 0.1), rng=rng)


def timed(name, cfg, steps, warmup, run):
    try:
        run(warmup)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        n = run(steps)
        host = time.perf_counter() - t0
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        print(json.dumps({"config": cfg, "leg": name, "samples": n, "volumes_per_s": round(n / ms * 1e3, 1),
                          "gpu_us_per_sample": round(ms * 1e3 / n, 1), "host_us_per_sample": round(host * 1e6 / n, 1)}), flush=True)
    except ValueError as e:
        if "items outside the fused keyed path" not in str(e):
            raise
        print(json.dumps({"config": cfg, "leg": name, "skipped": f"{type(e).__name__}: {e}"[:160]}), flush=True)


def warp_only(n, dev, steps):
    from fetalsyngen_amd import kernels as K
    from fetalsyngen_amd import tables as T

    shape = (n, n, n)
    rs = np.random.RandomState(0)
    fs = (rs.randn(10, 10, 10, 3) * 2).astype(np.float32)
    ht, _new = T.zoom_tables(fs.shape[:3], np.array(shape) / np.array(fs.shape[:3]))
    r = np.deg2rad(12)
    A = np.array([[np.cos(r), -np.sin(r), 0], [np.sin(r), np.cos(r), 0], [0, 0, 1]], dtype=np.float32)
    c = (np.array(shape) - 1) / 2
    spec = K.DeformSpec(shape, A, c, c.astype(np.float32), False, torch.from_numpy(fs).to(dev), K.DeviceTables(ht, dev), device=dev)
    spec.prepare_rows()
    mm = K.coords_floormin(spec)
    a, b = torch.rand(shape, device=dev) * 255, torch.rand(shape, device=dev) * 255
    lab = torch.randint(0, 8, shape, dtype=torch.uint8, device=dev)
    for _ in range(steps):
        K.warp(spec, mm, src_lin=a, src_nn=lab, src_img=b, gamma=0.9, nn_out=torch.float32)   # one launch
        K.warp(spec, mm, src_lin=a, src_nn=lab, gamma=0.9, nn_out=torch.float32)              # the two it replaces
        K.warp(spec, mm, src_lin=b)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--subjects", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--warp-only", action="store_true")
    args = ap.parse_args()
    from fetalsyngen_amd import sharding
    from fetalsyngen_amd.data.datasets import SeedBank
    from fetalsyngen_amd.phantom import make_seed_volumes

    n, dev = args.size, "cuda:0"
    shape = (n, n, n)
    if args.warp_only:
        return warp_only(n, dev, args.steps)
    rng = np.random.default_rng(0)
    subj = []
    for v in range(args.subjects):
        seg, seeds = make_seed_volumes(shape, v)
        img = torch.from_numpy((seg * 30 + rng.random(seg.shape) * 5).astype(np.float32)).to(dev)
        subj.append((torch.from_numpy(seg).to(dev), SeedBank(seeds, dev), img))
    for cfg, with_seeds in (("image_as_intensity", False), ("load_image_with_seeds", True)):
        item = lambda i: (subj[i % len(subj)][2], subj[i % len(subj)][0], subj[i % len(subj)][1] if with_seeds else None)  # noqa: E731
        key = lambda i: sharding.sample_key(1, i)  # noqa: E731
        gk, gd = generator(shape, dev, "keyed"), generator(shape, dev, "device")

        def single(steps):
            for i in range(steps):
                im, sg, bank = item(i)
                gk._pipeline(im, sg, bank, {}, scale01=True, key=key(i), next_key=key(i + 1))
            return steps

        def batch(steps):
            done = 0
            while done < steps:
                b = min(args.batch, steps - done)
                gk.sample_batch([item(done + q) for q in range(b)], scale01=True, streams=2, keys=[key(done + q) for q in range(b)])
                done += b
            return done

        def stagewise(steps):
            for i in range(steps):
                im, sg, bank = item(i)
                gd._pipeline(im, sg, bank, {}, scale01=True)
            return steps

        timed("keyed_single", cfg, args.steps, args.warmup, single)
        timed("keyed_batch", cfg, args.steps, args.warmup, batch)
        timed("stagewise_device", cfg, args.steps, args.warmup, stagewise)


if __name__ == "__main__":
    main()
