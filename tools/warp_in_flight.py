#!/usr/bin/env python3
"""The lean fused warp at 256^3 for rotations 0 / 12 / 20 degrees per axis and every barrier period (fsg_warp_set_variant
0 = the launch's own choice, 5 = none, 6 = every second step, 7 = every step), set up as tools/kernel_bench.py sets it up:
the form the bench step launches (warp_f32_u8tof32_epi_ws: uint8 labels in, float32 labels out, gamma + bias epilogue, per-row
workspace), the image-only and the label-only launch.  FSG_LIB=<another build of the library> runs the same on that build.

    python tools/warp_in_flight.py [--rounds 5] [--reps 20]        HIP-event timing, the periods interleaved; median and minimum
    rocprofv3 --pmc ... -- python tools/warp_in_flight.py --pmc    3 launches of the bench's form per rotation, nothing else
    python tools/warp_in_flight.py --summarise DIR                 table from the counter_collection CSVs of --pmc runs under DIR
"""
import argparse, csv, glob, json, statistics, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--rots", default="0,12,20")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--pmc", action="store_true")
ap.add_argument("--summarise", default=None)
args = ap.parse_args()
rots = [float(r) for r in args.rots.split(",")]
PMC_REPS = 3

if args.summarise:
    # the warp_lean_kernel dispatches of a --pmc run, in issue order, are PMC_REPS per rotation
    table = {}
    for f in sorted(glob.glob(args.summarise + "/**/*counter_collection.csv", recursive=True)):
        per = {}
        for r in csv.DictReader(open(f)):
            if "warp_lean_kernel" in r["Kernel_Name"]:
                per.setdefault(int(r["Dispatch_Id"]), {})[r["Counter_Name"]] = float(r["Counter_Value"])
        ids = sorted(per)
        if len(ids) != PMC_REPS * len(rots):
            print(f"{f}: {len(ids)} warp dispatches, expected {PMC_REPS * len(rots)}", file=sys.stderr)
            continue
        for n, rot in enumerate(rots):
            chunk = [per[i] for i in ids[n * PMC_REPS:(n + 1) * PMC_REPS]]
            cell = table.setdefault(f"rot{rot:g}", {})
            for c in chunk[0]:
                cell[c] = round(statistics.mean(d[c] for d in chunk), 1)
    print(json.dumps(table, indent=1, sort_keys=True))
    sys.exit(0)

import numpy as np, torch
from fetalsyngen_amd import kernels as K, tables as T, _lib
from fetalsyngen_amd.phantom import make_seed_volumes, combined_seed_labels
from fetalsyngen_amd.utils.generation import make_affine_matrix

dev = "cuda:0"
lib = _lib.load()
n = args.size
shape = (n, n, n)
rs = np.random.RandomState(0)
seg, seeds = make_seed_volumes(shape)
lab8 = torch.from_numpy(combined_seed_labels(seeds, {1: 3, 2: 4, 3: 2, 4: 5})).to(dev)
segf = torch.from_numpy(seg).to(dev)
seg8 = segf.to(torch.uint8)
mus = torch.from_numpy((25 + 200 * rs.rand(50)).astype(np.float32)).to(dev)
sig = torch.from_numpy((5 + 20 * rs.rand(50)).astype(np.float32)).to(dev)
img = K.gmm_sample(lab8, mus, sig, seed=1, stream_id=1)
fsz, bsz = max(1, round(0.05 * n)), max(1, round(0.012 * n))
fs = torch.from_numpy((rs.randn(fsz, fsz, fsz, 3) * 2.5).astype(np.float32)).to(dev)
ft, _ = T.zoom_tables((fsz,) * 3, np.array(shape) / fsz)
bias = torch.from_numpy((rs.randn(bsz, bsz, bsz) * 0.2).astype(np.float32)).to(dev)
bt, _ = T.zoom_tables((bsz,) * 3, np.array(shape) / bsz)
btabs = K.DeviceTables(bt, dev)
c = (np.array(shape) - 1) / 2
PACES = ((0, "default"), (5, "none"), (6, "every2"), (7, "every1"))

try:
    for rot in rots:
        r = np.deg2rad(rot)
        A = make_affine_matrix([r, -r, r], [0.01, -0.02, 0.015], [1.05, 0.95, 1.02]).astype(np.float32)
        spec = K.DeformSpec(shape, A, c, c.astype(np.float32), True, fs, K.DeviceTables(ft, dev), device=dev)
        spec.prepare_rows(bias, btabs)
        mm6 = K.coords_minmax(spec)
        kinds = {
            "warp_f32_u8tof32_epi_ws": lambda: K.warp(spec, mm6, src_lin=img, src_nn=seg8, gamma=1.1, bias=bias, bias_tabs=btabs,
                                                      nn_out=torch.float32),
            "warp_lin_only_ws": lambda: K.warp(spec, mm6, src_lin=img),
            "warp_nn_f32_only_ws": lambda: K.warp(spec, mm6, src_nn=segf),
        }
        if args.pmc:
            for _ in range(PMC_REPS):
                kinds["warp_f32_u8tof32_epi_ws"]()
            torch.cuda.synchronize()
            continue
        times = {}
        for _ in range(args.rounds):
            for kind, run in kinds.items():
                for pace, _name in PACES:
                    lib.fsg_warp_set_variant(pace)
                    run()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.reps):
                        run()
                    e1.record()
                    torch.cuda.synchronize()
                    times.setdefault((kind, pace), []).append(e0.elapsed_time(e1) * 1e3 / args.reps)
        for kind in kinds:
            row = {"kernel": kind, "rot": rot}
            for pace, name in PACES:
                v = times[(kind, pace)]
                row[name] = [round(statistics.median(v), 1), round(min(v), 1)]
            print(json.dumps(row), flush=True)
finally:
    lib.fsg_warp_set_variant(0)
