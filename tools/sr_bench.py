#!/usr/bin/env python3
"""Time the slice-acquisition kernels at BASELINE config 4 scale (384^3 volume at 0.5 mm, one stack of a
3 mm-thick, 0.8 mm in-plane acquisition) with HIP events on the launch stream.  Prints one JSON line.

    python tools/sr_bench.py [--size 384] [--slices 80] [--reps 5] [--deterministic] [--backward] [--adjoint-backward]

--deterministic adds a leg for the adjoint timings: the fixed-point accumulation (fsg_slice_acq_adjoint_det_f32) timed right
after the fp32-atomic entry on the same inputs (`*_det_ms`, the float figures are the yardstick), and its workspace size.
--backward adds the backward of the forward operator (fsg_slice_acq_backward_f32) at the same size: `backward_<mode>_<leg>_ms`
for grad_vol alone, grad_transforms alone and both, in both modes, beside the forward's and the float adjoint's times.
--backward --deterministic together add the fixed-point grad_vol (fsg_slice_acq_backward_det_f32) right after those float legs:
`backward_<mode>_<leg>_det_ms` for grad_vol alone and both, their ratios to the float legs, and the workspace size.
--adjoint-backward adds the backward of the adjoint (fsg_slice_acq_adjoint_backward_f32) on the same problem:
`adjoint_backward_<mode>[_eq]_<leg>_ms` for grad_slices alone, grad_transforms alone and both, in both modes, equalize off and
on (the pre-pass over the gradient included), and its ratios to forward_<mode>_ms and, with --backward, to
backward_<mode>_grad_transforms_ms of the same session.
--pose-chain runs INSTEAD of the legs above, on the same problem: the pose conversions of fsg_transform_convert.hip beside
`axisangle2mat_autograd`, alone and inside one iteration of a pose fit, at n = 80 and 250, by the host clock (pose_chain below).
--srr runs INSTEAD of the legs above, on the same problem: `svort.srr` (--srr-iters iterations) beside the same conjugate gradients
written in torch operations around slice_acquisition / slice_acquisition_adjoint, float and deterministic, and the three vector
launches of an iteration alone (srr_bench below).  --srr-lambda L > 0 adds the same solve with the first-order regulariser
(`srr_lam`; with --srr-huber-delta also `srr_lam_huber`, guided from round 0 on, --srr-outer rounds) to the alternated legs, and
`kernels.tk1_apply` alone against a streaming pass of the same bytes (tk1_bench below).
--svr runs INSTEAD of the legs above, on the same problem: a round of `svort.svr` beside a pose-fit iteration through autograd and
beside the forward plus the grad_transforms-only backward, at n = 80 and 250 (svr_bench below).
--robust runs INSTEAD of the legs above, on the same problem: one `svort.robust_weights` call (--robust-em EM iterations) beside
one CG iteration of `svort.srr`, and its three kernels alone, at n = 80 and 250 (robust_bench below).
--imatch runs INSTEAD of the legs above, on the same problem: one `svort.intensity_match` call at sigma = 16 and 4 pixels and
scale only beside one CG iteration of `svort.srr`, and its entries alone, at n = 80 and 250 (imatch_bench below).

--svr-groups runs INSTEAD of the legs above, on the same problem: a round of `svort.svr` with 3 groups beside today's per-slice
round, and the two launches the grouped round adds alone, at n = 80 and 250 (svr_groups_bench below).
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from fetalsyngen_amd import kernels as K  # noqa: E402
from fetalsyngen_amd.generator.artifacts.svort import get_PSF, random_stack  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def host_timed(fn, iters, warmup=20):
    """ms per call by the host clock around `iters` calls ended by a device synchronise, after a warm-up: for chains that are
    bound by host dispatch, where device events around single calls would time the wrong thing."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def pose_chain(a, dev, vs, ss, psf, vol, res):
    """--pose-chain: (n,6) poses on the device through the conversions and back, n = 80 and 250.
    (a) axisangle2mat_autograd(ax).backward(g)     the torch-operation route, the yardstick
    (b) transform_convert.axisangle2mat(ax).backward(g)
    (c) mat2axisangle(axisangle2mat(ax)).backward(g)
    (d), (e) one iteration of a pose fit on this bench's problem: poses -> matrices -> slice_acquisition (LINEAR, gradient of
    the transforms only) -> sum().backward(), with (a)'s and with (b)'s conversion.
    (a)/(b) and (d)/(e) are alternated three times; every repeat is reported."""
    from fetalsyngen_amd.generator.artifacts.svort import axisangle2mat_autograd, rigid, slice_acquisition
    from fetalsyngen_amd.generator.artifacts.svort import transform_convert as tc

    out = {"volume": vs, "psf": list(psf.shape), "iters": a.chain_iters, "clock": "host, synchronised at both ends"}
    rs = a.res_slice / res
    v5 = vol.reshape(1, 1, *vs)
    for n in (80, 250):
        np.random.seed(0)
        tr = random_stack(n, gap=a.size * res / n / res, max_angle=0.3)
        ax = rigid.mat2axisangle(tr).to(dev).requires_grad_()
        g12, g6 = torch.randn(n, 3, 4, device=dev), torch.randn(n, 6, device=dev)

        def conv(f, g):
            def run():
                ax.grad = None
                f(ax).backward(g)
            return run

        def fit(f):
            def run():
                ax.grad = None
                slice_acquisition(f(ax), v5, None, None, psf, (ss, ss), rs, False, False).sum().backward()
            return run

        legs = {"a_autograd": conv(axisangle2mat_autograd, g12), "b_kernel": conv(tc.axisangle2mat, g12),
                "c_roundtrip_kernel": conv(lambda x: tc.mat2axisangle(tc.axisangle2mat(x)), g6),
                "d_fit_autograd": fit(axisangle2mat_autograd), "e_fit_kernel": fit(tc.axisangle2mat)}
        row = {k: [] for k in legs}
        for _ in range(3):
            for k in ("a_autograd", "b_kernel"):
                row[k].append(round(host_timed(legs[k], a.chain_iters, warmup=200), 4))  # (20 calls left (b)'s first repeat 2.5x slow)
        row["c_roundtrip_kernel"].append(round(host_timed(legs["c_roundtrip_kernel"], a.chain_iters, warmup=200), 4))
        for _ in range(3):
            for k in ("d_fit_autograd", "e_fit_kernel"):
                row[k].append(round(host_timed(legs[k], a.chain_iters, warmup=5), 4))
        row["slices"] = [n, ss, ss]
        out[f"n{n}_ms"] = row
    return out


def torch_cg(tr, y, psf, vs, rs, n_iter, mu, deterministic, interp_psf=True):
    """The route without fsg_cg.hip: CG on (A^T P A + mu I) x = A^T P y from x = 0 in torch operations, alpha and beta as 0-dim
    tensors (no host synchronisation either), relu at the end.  What a user of the two operators writes."""
    from fetalsyngen_amd.generator.artifacts.svort import slice_acquisition, slice_acquisition_adjoint

    h, w = y.shape[-2:]

    def normal(v):
        s = slice_acquisition(tr, v, None, None, psf, (h, w), rs, False, interp_psf)
        return slice_acquisition_adjoint(tr, psf, s, None, None, vs, rs, interp_psf, False, deterministic=deterministic)

    r = slice_acquisition_adjoint(tr, psf, y, None, None, vs, rs, interp_psf, False, deterministic=deterministic)
    x = torch.zeros_like(r)
    p = r.clone()
    rr = (r * r).sum()
    for _ in range(n_iter):
        q = normal(p) + mu * p
        alpha = rr / (p * q).sum()
        x = x + alpha * p
        r = r - alpha * q
        rr_new = (r * r).sum()
        p = r + (rr_new / rr) * p
        rr = rr_new
    return torch.relu(x)


def tk1_bench(a, dev, vs):
    """kernels.tk1_apply alone (--srr with --srr-lambda > 0), by device events over --reps launches, alternated three times with a
    streaming pass of the same bytes (torch.mul by 1 into another tensor: 16-byte loads and stores, half the bytes read, half
    written).  Bytes from the shapes: p, t and out once each (the neighbours are re-reads of p that the caches serve), the guide
    once, the mask a quarter of a float volume."""
    n = int(np.prod(vs))
    g = lambda: torch.rand(vs, device=dev)  # noqa: E731
    p, t, guide, o = g(), g(), g(), torch.empty(vs, device=dev)
    mask = torch.rand(vs, device=dev) < 0.9
    lam, delta = a.srr_lambda, a.srr_huber_delta if a.srr_huber_delta is not None else 0.05
    legs = {"tk1": (12 * n, lambda: K.tk1_apply(p, t, vs, lam, out=o)),
            "tk1_mask": (13 * n, lambda: K.tk1_apply(p, t, vs, lam, mask=mask, out=o)),
            "tk1_mask_inplace": (13 * n, lambda: K.tk1_apply(p, t, vs, lam, mask=mask, out=t)),
            "tk1_mask_huber": (17 * n, lambda: K.tk1_apply(p, t, vs, lam, mask=mask, guide=guide, delta=delta, out=o))}
    out = {"tk1_clock": f"device events around {a.reps} launches, alternated three times with the copy of the same bytes"}
    for name, (nbytes, fn) in legs.items():
        half = nbytes // 8 * 4  # bytes read = bytes written
        src = torch.rand(half // 4, device=dev)
        dst = torch.empty_like(src)
        copy = lambda: torch.mul(src, 1.0, out=dst)  # noqa: E731
        rows = {"kernel": [], "copy": []}
        for _ in range(3):
            rows["kernel"].append(round(timed(fn, a.reps), 4))
            rows["copy"].append(round(timed(copy, a.reps), 4))
        out[f"{name}_ms"], out[f"{name}_copy_ms"], out[f"{name}_bytes"] = rows["kernel"], rows["copy"], nbytes
        out[f"{name}_GB_per_s"] = round(nbytes / min(rows["kernel"]) / 1e6, 1)
        out[f"{name}_copy_GB_per_s"] = round(2 * half / min(rows["copy"]) / 1e6, 1)
        del src, dst
    return out


def srr_bench(a, dev, vs, ss, psf, vol, tr, res):
    """--srr.  Per setting (float / deterministic adjoint): ms per iteration of svort.srr and of torch_cg, the legs alternated
    three times after a warm-up, host clock around one solve ended by a synchronise, divided by the iterations (the set-up,
    one adjoint, is in both).  Then the three vector launches of an iteration alone: a loop of `t = d * p` (torch, standing in
    for the operator: M = diag(d), d > 0, never converged, so no launch is a frozen one) + q + step + dir, minus the same loop
    with the multiplication only; their bytes come from the shapes: 12 volume-sized array passes per iteration (q: 2 reads + 1
    write, step: 4 + 2, dir: 2 + 1)."""
    from fetalsyngen_amd.generator.artifacts.svort import srr

    n_iter, mu, rs = a.srr_iters, 0.1, a.res_slice / res
    y = K.slice_acq_forward(tr, vol, None, None, psf, (ss, ss), rs, interp_psf=True)[:, None]
    out = {"volume": vs, "slices": [a.slices, ss, ss], "psf": list(psf.shape), "psf_taps": int((psf > 0).sum()), "iters": n_iter,
           "mu": mu, "interp_psf": True, "clock": "host, one solve per timing, synchronised at both ends"}

    def once(fn, iters=n_iter):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3 / iters, 3)

    lam, delta, outer = a.srr_lambda, a.srr_huber_delta, a.srr_outer
    for tag, det in (("float", False), ("det", True)):
        solve = lambda **kw: srr(tr, y, psf, vs, rs, interp_psf=True, mu=mu, n_iter=n_iter, deterministic=det, **kw)  # noqa: E731
        legs = {"srr": solve, "torch": lambda: torch_cg(tr, y, psf, vs, rs, n_iter, mu, det)}
        iters = {"srr": n_iter, "torch": n_iter}
        if lam > 0:  # the same solve with the first-order regulariser: unguided, and guided from round 0 on (by the truth)
            legs["srr_lam"], iters["srr_lam"] = (lambda: solve(lam=lam)), n_iter
            if delta is not None:
                legs["srr_lam_huber"] = lambda: solve(lam=lam, huber_delta=delta, n_outer=outer, guide=vol)
                iters["srr_lam_huber"] = n_iter * outer
        xs = {k: fn() for k, fn in legs.items()}  # warm-up, and the two routes solve the same problem
        out[f"{tag}_srr_vs_torch_max_abs_over_max"] = float((xs["srr"] - xs["torch"]).abs().max() / xs["torch"].abs().max())
        del xs
        row = {k: [] for k in legs}
        for _ in range(3):
            for k, fn in legs.items():
                row[k].append(once(fn, iters[k]))
        out[f"{tag}_ms_per_iter"] = row
        out[f"{tag}_torch_over_srr"] = round(min(row["torch"]) / min(row["srr"]), 3)
    if lam > 0:
        out.update(tk1_bench(a, dev, vs))
    # the vector launches alone
    n = int(np.prod(vs))
    g = lambda: torch.rand(vs, device=dev)  # noqa: E731
    d, b, t = g() + 0.5, g() - 0.5, g()
    r, p, x = torch.empty_like(b), torch.empty_like(b), torch.empty_like(b)
    ws = K.cg_workspace(n, n_iter, dev)

    def loop(vector):
        K.cg_init(ws, b, r, p, x)
        for k in range(1, n_iter + 1):
            torch.mul(d, p, out=t)
            if vector:
                K.cg_q(ws, k, p, t, mu=mu)
                K.cg_step(ws, k, p, t, x, r, relu=True)
                K.cg_dir(ws, k, r, p)

    loop(True), loop(False)
    with_v, without = [once(lambda: loop(True)) for _ in range(3)], [once(lambda: loop(False)) for _ in range(3)]
    loop(True)
    out["vector_loop_ms_per_iter"], out["mul_only_loop_ms_per_iter"] = with_v, without
    out["vector_frozen_at_end"] = int(ws.frozen[-1].item())
    vec = min(with_v) - min(without)
    nbytes = 12 * n * 4 - 2 * n * 4 / n_iter  # the last iteration stores no r and touches no p in dir: 9 passes
    out["vector_ms_per_iter"] = round(vec, 3)
    out["vector_bytes_per_iter"] = int(12 * n * 4)
    out["vector_GB_per_s"] = round(nbytes / vec / 1e6, 1)
    out["vector_share_of_float_iter"] = round(vec / min(out["float_ms_per_iter"]["srr"]), 4)
    out["vector_share_of_det_iter"] = round(vec / min(out["det_ms_per_iter"]["srr"]), 4)
    return out


def svr_bench(a, dev, vs, ss, psf, vol, res):
    """--svr, n = 80 and 250.  Per round of svort.svr (axisangle2mat, the Jacobian, fsg_svr_normal_f32, fsg_svr_update_f32):
    host clock around one solve of --svr-iters iterations ended by a synchronise, divided by its iters + 1 rounds.  Beside it,
    in the same session and alternated three times after a warm-up: (e) one pose-fit iteration through autograd as --pose-chain
    times it (conversion kernel, forward, backward of the transforms, conversion backward), by the host clock over
    --chain-iters iterations; and the forward (LINEAR) plus the grad_transforms-only backward, and fsg_svr_normal_f32 alone, by
    device events.  The launches of a round do not depend on the data (a frozen slice is still evaluated), so the poses need
    not converge for the timing to stand."""
    from fetalsyngen_amd.generator.artifacts.svort import rigid, slice_acquisition, svr
    from fetalsyngen_amd.generator.artifacts.svort import transform_convert as tc

    rs, n_iter = a.res_slice / res, a.svr_iters
    out = {"volume": vs, "psf": list(psf.shape), "psf_taps": int((psf > 0).sum()), "iters": n_iter, "rounds": n_iter + 1,
           "clock": "svr and fit: host, synchronised at both ends; forward/backward/normal: device events"}
    v5 = vol.reshape(1, 1, *vs)
    for n in (80, 250):
        np.random.seed(0)
        tr = random_stack(n, gap=a.size * res / n / res, max_angle=0.3)
        ax = rigid.mat2axisangle(tr).to(dev).float().contiguous()
        trd = K.axisangle2mat(ax)
        y = K.slice_acq_forward(trd, vol, None, None, psf, (ss, ss), rs)
        start = (ax + 0.01 * torch.randn_like(ax)).contiguous()
        axg = start.clone().requires_grad_()
        gs = torch.randn_like(y)
        onehot = torch.eye(12, device=dev).repeat(n, 1).view(12 * n, 3, 4)
        jac = K.axisangle2mat_backward(onehot, start.repeat_interleave(12, 0).contiguous()).view(n, 12, 6)

        def solve():
            return svr(start, y, vol, psf, rs, n_iter=n_iter)

        def once():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            solve()
            torch.cuda.synchronize()
            return round((time.perf_counter() - t0) * 1e3 / (n_iter + 1), 3)

        def fit():
            axg.grad = None
            slice_acquisition(tc.axisangle2mat(axg), v5, None, None, psf, (ss, ss), rs, False, False).sum().backward()

        legs = {
            "svr_round": once,
            "fit_iteration_autograd": lambda: round(host_timed(fit, a.chain_iters, warmup=5), 3),
            "forward_linear": lambda: round(timed(lambda: K.slice_acq_forward(trd, vol, None, None, psf, (ss, ss), rs), a.reps), 3),
            "backward_grad_transforms": lambda: round(timed(
                lambda: K.slice_acq_backward(trd, vol, None, None, psf, gs, rs, need_vol_grad=False), a.reps), 3),
            "svr_normal": lambda: round(timed(lambda: K.svr_normal(trd, jac, vol, psf, y, None, None, rs), a.reps), 3),
        }
        solve(), fit()  # warm-up
        row = {k: [] for k in legs}
        for _ in range(3):
            for k, fn in legs.items():
                row[k].append(fn())
        best = {k: min(v) for k, v in row.items()}
        row["slices"] = [n, ss, ss]
        row["svr_round_over_fit_iteration"] = round(best["svr_round"] / best["fit_iteration_autograd"], 3)
        row["svr_normal_over_backward"] = round(best["svr_normal"] / best["backward_grad_transforms"], 3)
        row["svr_normal_over_forward_plus_backward"] = round(
            best["svr_normal"] / (best["forward_linear"] + best["backward_grad_transforms"]), 3)
        p1, p2 = solve(), solve()
        row["poses_twice_equal"] = bool(torch.equal(p1, p2))
        out[f"n{n}_ms"] = row
    return out


def svr_groups_bench(a, dev, vs, ss, psf, vol, res):
    """--svr-groups, n = 80 and 250, 3 groups of consecutive slices.  A round of `svort.svr(groups=)` (axisangle2mat and its
    Jacobian on 3 rows, svr_compose, fsg_svr_normal_f32, svr_group_reduce, fsg_svr_update_f32 on 3 rows) beside a round of the
    per-slice `svort.svr` (the conversions and the update on n rows): device events around one solve of --svr-iters iterations,
    divided by its iters + 1 rounds, the two legs alternated three times after a warm-up.  Then fsg_svr_compose_f32 and
    fsg_svr_group_reduce_f64 alone, by device events over --reps launches.  The expectation: a grouped round is the per-slice
    round plus the two launches (the conversions and the update shrink from n rows to 3, which is below the clock's
    resolution either way); `grouped_minus_per_slice` against `compose_plus_reduce` and the legs' own spread says whether it
    holds."""
    from fetalsyngen_amd.generator.artifacts.svort import rigid, svr

    rs, n_iter, G = a.res_slice / res, a.svr_iters, 3
    out = {"volume": vs, "psf": list(psf.shape), "psf_taps": int((psf > 0).sum()), "iters": n_iter, "rounds": n_iter + 1, "groups": G,
           "clock": f"rounds: device events around one solve / rounds, legs alternated three times; launches: device events around {a.reps}"}
    for n in (80, 250):
        np.random.seed(0)
        tr = random_stack(n, gap=a.size * res / n / res, max_angle=0.3)
        ax = rigid.mat2axisangle(tr).to(dev).float().contiguous()
        y = K.slice_acq_forward(K.axisangle2mat(ax), vol, None, None, psf, (ss, ss), rs)
        start = (ax + 0.01 * torch.randn_like(ax)).contiguous()
        groups = (np.arange(n) * G // n).tolist()

        def solve(g):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            p = svr(start, y, vol, psf, rs, n_iter=n_iter, groups=g)
            e1.record()
            torch.cuda.synchronize()
            return p, round(e0.elapsed_time(e1) / (n_iter + 1), 4)

        solve(groups), solve(None)  # warm-up
        row = {"grouped_round": [], "per_slice_round": []}
        for _ in range(3):
            row["grouped_round"].append(solve(groups)[1])
            row["per_slice_round"].append(solve(None)[1])
        base = K.axisangle2mat(start)
        phi = 0.01 * torch.randn(G, 6, device=dev)
        onehot = torch.eye(12, device=dev).repeat(G, 1).view(12 * G, 3, 4)
        gm, gj = K.axisangle2mat(phi), K.axisangle2mat_backward(onehot, phi.repeat_interleave(12, 0).contiguous()).view(G, 12, 6)
        gd = torch.tensor(groups, dtype=torch.int32, device=dev)
        members = torch.arange(n, dtype=torch.int32, device=dev)
        offsets = torch.tensor(np.searchsorted(groups, np.arange(G + 1)), dtype=torch.int32, device=dev)
        buf = (torch.empty(n, 3, 4, device=dev), torch.empty(n, 12, 6, device=dev))
        stats, gstats = torch.rand(n, K.SVR_SLOTS, dtype=torch.float64, device=dev), torch.empty(G, K.SVR_SLOTS, dtype=torch.float64, device=dev)
        row["compose"] = [round(timed(lambda: K.svr_compose(gm, gj, base, gd, out=buf), a.reps), 4) for _ in range(3)]
        row["group_reduce"] = [round(timed(lambda: K.svr_group_reduce(stats, members, offsets, out=gstats), a.reps), 4) for _ in range(3)]
        best = {k: min(v) for k, v in row.items()}
        row["slices"] = [n, ss, ss]
        row["grouped_over_per_slice"] = round(best["grouped_round"] / best["per_slice_round"], 4)
        row["grouped_minus_per_slice"] = round(best["grouped_round"] - best["per_slice_round"], 4)
        row["compose_plus_reduce"] = round(best["compose"] + best["group_reduce"], 4)
        row["spread_of_the_rounds"] = round(max(max(row[k]) - min(row[k]) for k in ("grouped_round", "per_slice_round")), 4)
        p1, p2 = solve(groups)[0], solve(groups)[0]
        row["poses_twice_equal"] = bool(torch.equal(p1, p2))
        out[f"n{n}_ms"] = row
    return out


def robust_bench(a, dev, vs, ss, psf, vol, res):
    """--robust, n = 80 and 250.  One `svort.robust_weights` call (T = --robust-em: T + 1 pixel passes, T + 1 scalar passes, the
    weights) beside ONE iteration of the conjugate gradients of `svort.srr` (A, A^T in the float adjoint, q, step, dir), both by
    device events over --reps calls, the legs alternated three times after a warm-up.  Then the three kernels alone, with their
    bytes from the shapes: y, s and the forward's weight read once per pixel pass (12 bytes a pixel), the weights pass writes 4
    more.  No threshold is asserted: the figures are for DESIGN.md section 25."""
    from fetalsyngen_amd.generator.artifacts.svort import robust_weights

    rs, T = a.res_slice / res, a.robust_em
    out = {"volume": vs, "psf": list(psf.shape), "psf_taps": int((psf > 0).sum()), "n_em": T,
           "clock": f"device events around {a.reps} calls, legs alternated three times"}
    nvox = int(np.prod(vs))
    for n in (80, 250):
        np.random.seed(0)
        tr = random_stack(n, gap=a.size * res / n / res, max_angle=0.3).to(dev)
        y = K.slice_acq_forward(tr, vol, None, None, psf, (ss, ss), rs, interp_psf=True)
        y = y + 0.02 * torch.randn_like(y)
        y[n // 3] *= 0.2  # a slice to reject
        s, wgt = K.slice_acq_forward(tr, 0.95 * vol, None, None, psf, (ss, ss), rs, need_weight=True, interp_psf=True)
        ws = K.cg_workspace(nvox, 1, dev)
        b = torch.rand(vs, device=dev)
        r, p, x = torch.empty_like(b), torch.empty_like(b), torch.empty_like(b)

        def cg_iteration():
            K.cg_init(ws, b, r, p, x)
            t = K.slice_acq_forward(tr, p, None, None, psf, (ss, ss), rs, interp_psf=True)
            q = K.slice_acq_adjoint(tr, psf, t, None, None, vs, rs, interp_psf=True)
            K.cg_q(ws, 1, p, q)
            K.cg_step(ws, 1, p, q, x, r)
            K.cg_dir(ws, 1, r, p)

        st = K.robust_state(n, T, dev, (ss, ss))
        o = torch.empty_like(y)
        legs = {"robust_weights": lambda: robust_weights(y, s, sim_weight=wgt, n_em=T), "cg_iteration": cg_iteration,
                "cg_init_alone": lambda: K.cg_init(ws, b, r, p, x)}
        for fn in legs.values():
            fn()
        row = {k: [] for k in legs}
        for _ in range(3):
            for k, fn in legs.items():
                row[k].append(round(timed(fn, a.reps), 4))
        K.robust_estep(st, 0, y, s, None, wgt), K.robust_update(st, 0)
        alone = {"estep": lambda: K.robust_estep(st, 1, y, s, None, wgt), "update": lambda: K.robust_update(st, 1),
                 "weights_slice": lambda: K.robust_weights(st, y, s, None, wgt, out=o),
                 "weights_both": lambda: K.robust_weights(st, y, s, None, wgt, level="both", out=o)}
        for k, fn in alone.items():
            row[k] = [round(timed(fn, a.reps), 4) for _ in range(3)]
        npix = n * ss * ss
        row["estep_GB_per_s"] = round(12 * npix / min(row["estep"]) / 1e6, 1)
        row["weights_GB_per_s"] = round(16 * npix / min(row["weights_both"]) / 1e6, 1)
        it = min(row["cg_iteration"]) - min(row["cg_init_alone"])
        row["cg_iteration_without_init"] = round(it, 4)
        row["robust_over_cg_iteration"] = round(min(row["robust_weights"]) / it, 4)
        row["slices"] = [n, ss, ss]
        w1, i1 = robust_weights(y, s, sim_weight=wgt, n_em=T, return_info=True)
        w2 = robust_weights(y, s, sim_weight=wgt, n_em=T)
        row["weights_twice_equal"] = bool(torch.equal(w1, w2))
        row["rejected_slices"] = int((i1["ws"][-1] < 0.5).sum().item())
        out[f"n{n}_ms"] = row
        del y, s, wgt, o, st
    return out


def imatch_bench(a, dev, vs, ss, psf, vol, res):
    """--imatch, n = 80 and 250.  One `svort.intensity_match` call at sigma = 16 and 4 pixels and scale only, beside ONE iteration
    of the conjugate gradients of `svort.srr` (A, A^T in the float adjoint, q, step, dir; the operators as in robust_bench), by device events over
    --reps calls, the legs alternated three times after a warm-up.  Then the entries alone, with their bytes from the shapes
    (y, s and the forward's weight; no mask, robust weights or carried bias): sums reads 12 bytes a pixel; bias reads 12 and
    writes 12 in the row pass, reads 12 and writes 4 in the column pass (28 + 12 = 40); apply reads 8 and writes 8.  bias at
    sigma = 0.3 (radius 1) is the two passes with next to no taps: what remains of the other two is the taps' LDS work.  No
    threshold is asserted: the figures are for DESIGN.md section 28."""
    from fetalsyngen_amd.generator.artifacts.svort import intensity_match

    rs = a.res_slice / res
    out = {"volume": vs, "psf": list(psf.shape), "psf_taps": int((psf > 0).sum()),
           "clock": f"device events around {a.reps} calls, legs alternated three times"}
    nvox = int(np.prod(vs))
    for n in (80, 250):
        np.random.seed(0)
        tr = random_stack(n, gap=a.size * res / n / res, max_angle=0.3).to(dev)
        y = K.slice_acq_forward(tr, vol, None, None, psf, (ss, ss), rs, interp_psf=True)
        gain = torch.exp(0.25 * torch.randn(n, 1, 1, device=dev))
        y = y * gain + 0.02 * torch.randn_like(y)
        s, wgt = K.slice_acq_forward(tr, 0.95 * vol, None, None, psf, (ss, ss), rs, need_weight=True, interp_psf=True)
        ws = K.cg_workspace(nvox, 1, dev)
        b = torch.rand(vs, device=dev)
        r, p, x = torch.empty_like(b), torch.empty_like(b), torch.empty_like(b)

        def cg_iteration():
            K.cg_init(ws, b, r, p, x)
            t = K.slice_acq_forward(tr, p, None, None, psf, (ss, ss), rs, interp_psf=True)
            q = K.slice_acq_adjoint(tr, psf, t, None, None, vs, rs, interp_psf=True)
            K.cg_q(ws, 1, p, q)
            K.cg_step(ws, 1, p, q, x, r)
            K.cg_dir(ws, 1, r, p)

        legs = {"match_sigma16": lambda: intensity_match(y, s, sim_weight=wgt, bias_sigma=16.0),
                "match_sigma4": lambda: intensity_match(y, s, sim_weight=wgt, bias_sigma=4.0),
                "match_scale_only": lambda: intensity_match(y, s, sim_weight=wgt),
                "cg_iteration": cg_iteration, "cg_init_alone": lambda: K.cg_init(ws, b, r, p, x)}
        for fn in legs.values():
            fn()
        row = {k: [] for k in legs}
        for _ in range(3):
            for k, fn in legs.items():
                row[k].append(round(timed(fn, a.reps), 4))
        st = K.imatch_state(n, dev, (ss, ss))
        K.imatch_sums(st, y, s, None, wgt), K.imatch_scale(st)
        b1, cor = torch.empty_like(y), torch.empty_like(y)
        alone = {"sums": lambda: K.imatch_sums(st, y, s, None, wgt), "scale": lambda: K.imatch_scale(st),
                 "bias_sigma16": lambda: K.imatch_bias(st, y, s, 16.0, None, wgt, out=b1),
                 "bias_sigma4": lambda: K.imatch_bias(st, y, s, 4.0, None, wgt, out=b1),
                 "bias_sigma0.3": lambda: K.imatch_bias(st, y, s, 0.3, None, wgt, out=b1),
                 "apply_scale_only": lambda: K.imatch_apply(st, y, None, None, corrected=cor)}
        for k, fn in alone.items():
            fn()
            row[k] = [round(timed(fn, a.reps), 4) for _ in range(3)]
        npix = n * ss * ss
        row["sums_GB_per_s"] = round(12 * npix / min(row["sums"]) / 1e6, 1)
        row["apply_GB_per_s"] = round(12 * npix / min(row["apply_scale_only"]) / 1e6, 1)  # no bias read: y in, bias and corrected out
        for k in ("bias_sigma16", "bias_sigma4", "bias_sigma0.3"):
            row[k + "_GB_per_s"] = round(40 * npix / min(row[k]) / 1e6, 1)
        it = min(row["cg_iteration"]) - min(row["cg_init_alone"])
        row["cg_iteration_without_init"] = round(it, 4)
        for k in ("match_sigma16", "match_sigma4", "match_scale_only"):
            row[k + "_over_cg_iteration"] = round(min(row[k]) / it, 4)
        row["slices"] = [n, ss, ss]
        m1 = intensity_match(y, s, sim_weight=wgt, bias_sigma=4.0, return_info=True)
        m2 = intensity_match(y, s, sim_weight=wgt, bias_sigma=4.0)
        row["twice_equal"] = all(bool(torch.equal(u, v)) for u, v in zip(m1[:3], m2))
        row["frozen"] = int(m1[3]["frozen"].item())
        row["scale_against_gain_corr"] = round(float(torch.corrcoef(torch.stack([m1[1], 1 / gain.reshape(-1)]))[0, 1].item()), 4)
        out[f"n{n}_ms"] = row
        del y, s, wgt, st, b1, cor, m1, m2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--slices", type=int, default=80)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res-slice", type=float, default=0.8)
    ap.add_argument("--thick", type=float, default=3.0)
    ap.add_argument("--deterministic", action="store_true", help="also time the deterministic adjoint")
    ap.add_argument("--backward", action="store_true", help="also time the backward of the forward operator")
    ap.add_argument("--adjoint-backward", action="store_true", help="also time the backward of the adjoint")
    ap.add_argument("--pose-chain", action="store_true", help="time the pose conversions and a pose-fit iteration instead")
    ap.add_argument("--chain-iters", type=int, default=200, help="iterations per --pose-chain timing (host clock)")
    ap.add_argument("--srr", action="store_true", help="time svort.srr against the same CG in torch operations instead")
    ap.add_argument("--srr-iters", type=int, default=6, help="CG iterations per --srr solve")
    ap.add_argument("--srr-lambda", type=float, default=0.0, help="> 0: also time --srr with the first-order regulariser, and tk1_apply alone")
    ap.add_argument("--srr-huber-delta", type=float, default=None, help="with --srr-lambda: also the guided (Huber-weighted) solve")
    ap.add_argument("--srr-outer", type=int, default=1, help="rounds of the guided solve (n_outer)")
    ap.add_argument("--svr", action="store_true", help="time a round of svort.svr against a pose-fit iteration through autograd instead")
    ap.add_argument("--svr-iters", type=int, default=5, help="iterations per --svr solve (iters + 1 rounds)")
    ap.add_argument("--svr-groups", action="store_true", help="time a round of svort.svr with 3 groups beside the per-slice round instead")
    ap.add_argument("--robust", action="store_true", help="time svort.robust_weights beside one CG iteration instead")
    ap.add_argument("--robust-em", type=int, default=5, help="EM iterations per --robust call (n_em)")
    ap.add_argument("--imatch", action="store_true", help="time svort.intensity_match beside one CG iteration instead")
    a = ap.parse_args()
    dev, res = "cuda:0", 0.5
    vs = (a.size,) * 3
    ss = int(np.sqrt(3 * a.size**2 / 2.0) * res / a.res_slice)
    ss = int(np.ceil(ss / 32.0) * 32)
    psf = get_PSF(res_ratio=(a.res_slice / res, a.res_slice / res, a.thick / res)).to(dev)
    if a.pose_chain:
        print(json.dumps(pose_chain(a, dev, vs, ss, psf, torch.rand(vs, device=dev), res)))
        return
    if a.svr:
        print(json.dumps(svr_bench(a, dev, vs, ss, psf, torch.rand(vs, device=dev), res)))
        return
    if a.svr_groups:
        print(json.dumps(svr_groups_bench(a, dev, vs, ss, psf, torch.rand(vs, device=dev), res)))
        return
    if a.robust:
        print(json.dumps(robust_bench(a, dev, vs, ss, psf, torch.rand(vs, device=dev), res)))
        return
    if a.imatch:
        print(json.dumps(imatch_bench(a, dev, vs, ss, psf, torch.rand(vs, device=dev), res)))
        return
    delta = get_PSF(0).to(dev)
    np.random.seed(0)
    tr = random_stack(a.slices, gap=a.size * res / a.slices / res, max_angle=0.3).to(dev)
    vol = torch.rand(vs, device=dev)
    if a.srr:
        print(json.dumps(srr_bench(a, dev, vs, ss, psf, vol, tr, res)))
        return
    out = {"volume": vs, "slices": [a.slices, ss, ss], "psf": list(psf.shape), "psf_taps": int((psf > 0).sum())}
    rs = a.res_slice / res
    s = K.slice_acq_forward(tr, vol, None, None, psf, (ss, ss), rs)
    ntap = out["psf_taps"]
    npix = a.slices * ss * ss
    for name, fn in {
        "forward_linear_ms": lambda: K.slice_acq_forward(tr, vol, None, None, psf, (ss, ss), rs),
        "forward_delta_ms": lambda: K.slice_acq_forward(tr, vol, None, None, delta, (ss, ss), rs),
        "adjoint_nearest_psf_eq_ms": lambda: K.slice_acq_adjoint(tr, psf, s, None, None, vs, rs, interp_psf=True, equalize=True),
        "adjoint_linear_ms": lambda: K.slice_acq_adjoint(tr, psf, s, None, None, vs, rs, interp_psf=False),
        "forward_nearest_psf_ms": lambda: K.slice_acq_forward(tr, vol, None, None, psf, (ss, ss), rs, interp_psf=True),
        "forward_torch_ms": lambda: K.slice_acq_forward(tr, vol, None, None, psf, (ss, ss), rs, semantics="torch"),
    }.items():
        out[name] = round(timed(fn, a.reps), 3)
    # adjoint (interp_psf + equalize): direct atomics vs LDS pre-summation under a few shapes, and vs stack tilt
    from fetalsyngen_amd import _lib
    lib = _lib.load()
    adj = lambda t=tr: K.slice_acq_adjoint(t, psf, s, None, None, vs, rs, interp_psf=True, equalize=True)  # noqa: E731
    prev = lib.fsg_set_tuning(_lib.TUNE.SA_DIRECT)
    out["adjoint_direct_ms"] = round(timed(adj, a.reps), 3)
    lib.fsg_set_tuning(prev)
    if a.deterministic:
        det = lambda **kw: K.slice_acq_adjoint(tr, psf, s, None, None, vs, rs, deterministic=True, **kw)  # noqa: E731
        out["adjoint_nearest_psf_eq_det_ms"] = round(timed(lambda: det(interp_psf=True, equalize=True), a.reps), 3)
        out["adjoint_nearest_psf_eq_again_ms"] = round(timed(adj, a.reps), 3)  # the float leg once more: the session's spread
        out["adjoint_linear_det_ms"] = round(timed(lambda: det(interp_psf=False), a.reps), 3)
        prev = lib.fsg_set_tuning(_lib.TUNE.SA_DIRECT)
        out["adjoint_direct_det_ms"] = round(timed(lambda: det(interp_psf=True, equalize=True), a.reps), 3)
        lib.fsg_set_tuning(prev)
        out["det_workspace_bytes"] = int(lib.fsg_slice_acq_adjoint_det_ws_bytes(*vs, 1))
        a_f, a_d = adj(), det(interp_psf=True, equalize=True)
        out["det_vs_float_max_abs"] = float((a_f - a_d).abs().max())
        out["det_twice_equal"] = bool(torch.equal(a_d, det(interp_psf=True, equalize=True)))
    if a.backward:
        # backward of the forward (fsg_slice_acq_backward_f32) on the forward's own inputs, beside forward_*_ms and the float
        # adjoint's adjoint_*_ms above: each output alone and both, in both modes
        gs = torch.randn_like(s)
        for mode, ipsf in (("linear", False), ("nearest_psf", True)):
            for leg, kw in (("grad_vol", dict(need_transforms_grad=False)), ("grad_transforms", dict(need_vol_grad=False)),
                            ("both", {})):
                fn = lambda: K.slice_acq_backward(tr, vol, None, None, psf, gs, rs, interp_psf=ipsf, **kw)  # noqa: E731
                out[f"backward_{mode}_{leg}_ms"] = round(timed(fn, a.reps), 3)
        out["backward_workspace_bytes"] = int(lib.fsg_slice_acq_backward_ws_bytes(a.slices, ss, ss))
        t1, t2 = (K.slice_acq_backward(tr, vol, None, None, psf, gs, rs, need_vol_grad=False)[1] for _ in range(2))
        out["backward_grad_transforms_twice_equal"] = bool(torch.equal(t1, t2))
        if a.deterministic:
            # the fixed-point grad_vol (fsg_slice_acq_backward_det_f32) on the same inputs, right after the float legs above,
            # which are the yardstick: grad_vol alone and with grad_transforms, in both modes
            for mode, ipsf in (("linear", False), ("nearest_psf", True)):
                for leg, kw in (("grad_vol", dict(need_transforms_grad=False)), ("both", {})):
                    fn = lambda: K.slice_acq_backward(tr, vol, None, None, psf, gs, rs, interp_psf=ipsf, deterministic=True, **kw)  # noqa: E731
                    out[f"backward_{mode}_{leg}_det_ms"] = round(timed(fn, a.reps), 3)
                    out[f"backward_{mode}_{leg}_det_over_float"] = round(
                        out[f"backward_{mode}_{leg}_det_ms"] / out[f"backward_{mode}_{leg}_ms"], 2)
            out["backward_det_workspace_bytes"] = int(lib.fsg_slice_acq_backward_det_ws_bytes(*vs))
            bdet = lambda: K.slice_acq_backward(tr, vol, None, None, psf, gs, rs, need_transforms_grad=False, deterministic=True)[0]  # noqa: E731
            d1 = bdet()
            out["backward_det_twice_equal"] = bool(torch.equal(d1, bdet()))
            out["backward_det_vs_float_max_abs"] = float(
                (d1 - K.slice_acq_backward(tr, vol, None, None, psf, gs, rs, need_transforms_grad=False)[0]).abs().max())
    if a.adjoint_backward:
        # backward of the adjoint (fsg_slice_acq_adjoint_backward_f32): the slices of the forward, a random gradient on the
        # volume; with equalize, the volume and weight of the equalised adjoint of the same mode
        gv = torch.randn(vs, device=dev)
        for mode, ipsf in (("linear", False), ("nearest_psf", True)):
            ev, ew = K.slice_acq_adjoint(tr, psf, s, None, None, vs, rs, interp_psf=ipsf, equalize=True, return_weight=True)
            for eq, tag in ((False, ""), (True, "_eq")):
                st = dict(equalize=True, vol=ev, vol_weight=ew) if eq else {}
                for leg, kw in (("grad_slices", dict(need_transforms_grad=False)), ("grad_transforms", dict(need_slices_grad=False)),
                                ("both", {})):
                    fn = lambda: K.slice_acq_adjoint_backward(tr, gv, psf, s, None, None, rs, interp_psf=ipsf, **st, **kw)  # noqa: E731
                    out[f"adjoint_backward_{mode}{tag}_{leg}_ms"] = round(timed(fn, a.reps), 3)
            for leg in ("grad_slices", "grad_transforms", "both"):
                t = out[f"adjoint_backward_{mode}_{leg}_ms"]
                out[f"adjoint_backward_{mode}_{leg}_over_forward"] = round(t / out[f"forward_{mode}_ms"], 2)
            if a.backward:
                out[f"adjoint_backward_{mode}_grad_transforms_over_backward"] = round(
                    out[f"adjoint_backward_{mode}_grad_transforms_ms"] / out[f"backward_{mode}_grad_transforms_ms"], 2)
        out["adjoint_backward_workspace_bytes"] = int(lib.fsg_slice_acq_adjoint_backward_ws_bytes(*vs, a.slices, ss, ss, 1, 1))
        r1, r2 = (K.slice_acq_adjoint_backward(tr, gv, psf, s, None, None, rs, equalize=True, vol=ev, vol_weight=ew)
                  for _ in range(2))
        out["adjoint_backward_twice_equal"] = bool(torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1]))
    sweep = {}
    cfgs = ((4096, 0, 20), (3072, 0, 20), (6144, 0, 20), (4096, 3, 20), (4096, 2, 20), (6144, 1, 20), (4096, 0, 0), (4096, 0, 40))
    for ang in (0.3, 0.8, 1.5):
        np.random.seed(1)
        t2 = random_stack(a.slices, gap=a.size * res / a.slices / res, max_angle=ang).to(dev)
        row = {}
        prev = lib.fsg_set_tuning(_lib.TUNE.SA_DIRECT)
        row["direct"] = round(timed(lambda: adj(t2), a.reps), 2)
        lib.fsg_set_tuning(prev)
        for cap, zc, t16 in cfgs:
            lib.fsg_slice_acq_set_tuning(cap, zc, t16)
            row[f"{cap}/{zc}/{t16}"] = round(timed(lambda: adj(t2), a.reps), 2)
        sweep[f"tilt{ang}"] = row
    lib.fsg_slice_acq_set_tuning(3072, 0, 20)
    out["adjoint_sweep_ms"] = sweep
    out["pixel_taps"] = npix * ntap
    out["forward_linear_Gtaps_per_s"] = round(npix * ntap / out["forward_linear_ms"] / 1e6, 2)
    out["adjoint_Gtaps_per_s"] = round(npix * ntap / out["adjoint_nearest_psf_eq_ms"] / 1e6, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
