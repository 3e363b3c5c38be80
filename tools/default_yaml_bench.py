#!/usr/bin/env python3
"""The reference's default generator configuration (tests/golden/generator_default.json, i.e. its
configs/dataset/generator/default.yaml: every SR-artifact stage configured, gates at the YAML's probabilities) at 256^3 on
phantom subjects: volumes/s, host microseconds per sample, and where the samples and the time go.

    python tools/default_yaml_bench.py [--rng keyed device] [--size 256] [--steps 64] [--warmup 8] [--subjects 4]

Two legs in one process.  `keyed`: a sample is `gen.sample(..., key=k)`.  `device`: the stage-wise path under the global
generators -- what this configuration ran before keyed mode took the stages, so it is the yardstick.  Per leg two passes over
the same keys / seeds:

  throughput   `--steps` samples after `--warmup` untimed ones (and after an untimed warm-up of every leg), between two HIP events, no synchronisation inside:
               volumes_per_s, host_us_per_sample (wall time of issuing; the stages synchronise by themselves);
  attribution  the same samples again with a synchronising timer around every stage and every sample: the share of samples
               in which each stage fired, each stage's share of the total time, and the mean time of a sample with and
               without SimulateMotion (its gate decides the mean).

The two legs draw different random numbers, so with 64 samples their gates fire a different number of times: compare the
per-class means (`ms_with_motion`, `ms_without_motion`, `ms_no_stage`), not only the totals.  One JSON line per leg."""
import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
STAGES = ("blur_cortex", "struct_noise", "simulate_motion", "boundaries")


def instantiate(node):
    """`hydra.utils.instantiate` for this file: a mapping with `_target_` -> the dotted class called with its kwargs."""
    if isinstance(node, dict):
        kw = {k: instantiate(v) for k, v in node.items() if k != "_target_"}
        if "_target_" in node:
            mod, _, name = node["_target_"].rpartition(".")
            return getattr(importlib.import_module(mod), name)(**kw)
        return kw
    if isinstance(node, list):
        return [instantiate(v) for v in node]
    return node


def fired(name, meta):
    if name == "blur_cortex":
        return meta.get("nblur") is not None
    if name == "boundaries":
        return not meta.get("no_mask_on")
    return bool(meta)


class Timed:
    """A stage with a synchronising wall-clock timer around it."""

    def __init__(self, stage):
        self.stage, self.ms = stage, 0.0

    def __call__(self, *a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = self.stage(*a, **k)
        torch.cuda.synchronize()
        self.ms += (time.perf_counter() - t0) * 1e3
        return out


def leg(mode, gen, shape, subjects, steps, warmup, warm_only=False):
    from fetalsyngen_amd import sharding

    def run(first, count):
        for i in range(first, first + count):
            seg, bank = subjects[i % len(subjects)]
            if mode == "keyed":
                gen.sample(None, seg, bank, key=sharding.sample_key(1, i))
            else:
                gen.sample(None, seg, bank)
        return count

    def seed():
        np.random.seed(1)
        torch.manual_seed(1)

    seed()
    run(0, warmup)
    if warm_only:
        return torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    seed()
    e0.record()
    t0 = time.perf_counter()
    run(warmup, steps)
    host = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    res = {"rng": mode, "size": shape[0], "samples": steps, "volumes_per_s": round(steps / ms * 1e3, 2),
           "ms_per_sample": round(ms / steps, 2), "host_us_per_sample": round(host * 1e6 / steps, 1)}

    # attribution: the same samples with a synchronising timer around every stage
    timers = {name: Timed(gen.artifacts[name]) for name in STAGES if gen.artifacts[name] is not None}
    gen.artifacts.update(timers)
    seed()
    count = {name: 0 for name in timers}
    per_sample, motion, any_stage = [], [], []
    for i in range(warmup, warmup + steps):
        seg, bank = subjects[i % len(subjects)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = gen.sample(None, seg, bank, key=sharding.sample_key(1, i)) if mode == "keyed" else gen.sample(None, seg, bank)
        torch.cuda.synchronize()
        per_sample.append((time.perf_counter() - t0) * 1e3)
        on = {name: fired(name, out[3]["artifacts"].get(name, {})) for name in timers}
        for name in timers:
            count[name] += on[name]
        motion.append(on.get("simulate_motion", False))
        any_stage.append(any(on.values()))
    per_sample, motion, any_stage = np.array(per_sample), np.array(motion), np.array(any_stage)
    total = float(per_sample.sum())
    mean = lambda a: round(float(a.mean()), 2) if a.size else None  # noqa: E731
    res.update({
        "share_of_samples": {name: round(count[name] / steps, 3) for name in timers},
        "share_of_time": {**{name: round(t.ms / total, 3) for name, t in timers.items()},
                          "hot_path": round(1.0 - sum(t.ms for t in timers.values()) / total, 3)},
        "ms_with_motion": mean(per_sample[motion]), "ms_without_motion": mean(per_sample[~motion]),
        "ms_no_stage": mean(per_sample[~any_stage]), "samples_no_stage": int((~any_stage).sum()),
        "ms_hot_path": round((total - sum(t.ms for t in timers.values())) / steps, 3),
    })
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rng", nargs="+", default=["keyed", "device"], choices=["keyed", "device"])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--subjects", type=int, default=4)
    args = ap.parse_args()
    from fetalsyngen_amd import compat
    from fetalsyngen_amd.data.datasets import SeedBank
    from fetalsyngen_amd.phantom import make_seed_volumes

    compat.install()
    cfg = json.loads((REPO / "tests" / "golden" / "generator_default.json").read_text())
    n, dev = args.size, cfg.get("device", "cuda:0")
    shape = (n, n, n)

    def resize(node):  # the YAML's 256^3 -> --size
        if isinstance(node, dict):
            return {k: ([n, n, n] if k in ("shape", "size") and isinstance(v, list) else resize(v)) for k, v in node.items()}
        return node

    cfg = resize(cfg)
    subjects = []
    for v in range(args.subjects):
        seg, seeds = make_seed_volumes(shape, v)
        subjects.append((torch.from_numpy(seg).to(dev), SeedBank(seeds, dev)))
    gens = {}
    for mode in args.rng:  # every leg is warmed before any is timed: the first one would pay for the allocator's growth alone
        gens[mode] = instantiate(cfg)
        gens[mode].rng = mode
        leg(mode, gens[mode], shape, subjects, args.steps, args.warmup, warm_only=True)
    for mode in args.rng:
        leg(mode, gens[mode], shape, subjects, args.steps, args.warmup)


if __name__ == "__main__":
    main()
