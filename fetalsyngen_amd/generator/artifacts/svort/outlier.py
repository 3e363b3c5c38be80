"""`robust_weights`: outlier rejection for `srr` and `svr` by the robust-statistics EM of the slice-to-volume family
(Kuklisova-Murgasova et al. 2012; DESIGN.md section 25, the rule in include/fsg_hip.h, fsg_robust_*).

Given the acquired slices y and the slices s = A x a reconstruction simulates, every pixel gets the posterior p of being an
inlier (Gaussian residual of a common sigma against a uniform outlier density over the intensity range) and every slice a
weight ws from a two-class mixture over its potential u = sqrt(mean (1 - p)^2).  The result is the per-pixel weight both
solves already take as `slices_weight`: ws ("slice") or ws * p ("both") on the pixels that take part, 0 elsewhere.

The loop is a fixed sequence of launches on torch's current stream, two per EM iteration and one for the weights; sigma, the
inlier fraction and the slice mixture live on the device (kernels.RobustState): nothing is read back.  No atomics and every
order of summation fixed: bit-identical from run to run and on any stream.  Not differentiable.
"""
from __future__ import annotations

import torch

from .... import kernels as K
from ._solver import check_options as _check_options, no_grad_inputs, prep

DEFAULTS = dict(min_weight=0.5, n_em=5, c0=0.9, sigma_floor=0.04, slice_floor=0.025, min_pixels=4, level="slice")


def check_options(opts):
    """the options of `robust_weights` as a complete dict; ValueError for an unknown name or a value the kernels refuse"""
    o = _check_options("robust", DEFAULTS, opts, ("min_weight", "sigma_floor", "slice_floor"))
    if not 0 < float(o["c0"]) <= 1:
        raise ValueError(f"c0 must be in (0, 1], got {o['c0']!r}")
    if not 1 <= int(o["n_em"]) <= K.ROBUST_MAX_EM:
        raise ValueError(f"n_em must be in 1..{K.ROBUST_MAX_EM}, got {o['n_em']!r}")
    if o["level"] not in K.ROBUST_LEVELS:
        raise ValueError(f"level must be one of {sorted(K.ROBUST_LEVELS)}, got {o['level']!r}")
    return o


def robust_weights(slices, simulated, *, slices_mask=None, sim_weight=None, min_weight=0.5, n_em=5, c0=0.9, sigma_floor=0.04,
                   slice_floor=0.025, min_pixels=4, level="slice", return_info=False):
    """slices, simulated (n,[1,]h,w) -> weights (n,h,w) fp32 on the device, for `slices_weight` of `srr` and `svr`.

    slices_mask (n,[1,]h,w) bool: pixels that take part.  sim_weight: the weight `slice_acquisition` computed for `simulated`
    (kernels.slice_acq_forward(need_weight=True)); a pixel takes part iff weight > 0 and weight >= min_weight (0.5 is the cut
    of `srr`'s adjoint).  A pixel whose residual is NaN or Inf takes no part.  n_em: EM iterations after the first estimate.
    c0: the inlier fraction the first iteration assumes.  sigma_floor: the inlier sigma is not allowed below this fraction of
    the intensity range max y - min y (a bare maximum-likelihood sigma switches off the pixels where a short regularised solve
    is still biased).  slice_floor: the same for the two sigmas of the slice mixture, in units of u.
    min_pixels: a slice with fewer pixels gets weight 0.  level: "slice" = the slice weight on every pixel of the slice, "both"
    = times the pixel posterior.  return_info: also the device histories sigma, c, mu1, mu2 (float64), frozen (int32), each
    n_em + 1 slots, ws (n_em + 1, n) and u (n)."""
    no_grad_inputs("robust_weights", slices=slices, simulated=simulated, sim_weight=sim_weight)
    o = check_options(dict(min_weight=min_weight, n_em=n_em, c0=c0, sigma_floor=sigma_floor, slice_floor=slice_floor,
                           min_pixels=min_pixels, level=level))
    K._need_gpu(slices, simulated)
    dev = slices.device
    h, w = (int(v) for v in slices.shape[-2:])
    n = int(slices.shape[0])

    y, s, wg = (prep(t, (n, h, w), dev) for t in (slices, simulated, sim_weight))
    sm = prep(slices_mask, (n, h, w), dev, torch.bool)
    st = K.robust_state(n, int(o["n_em"]), dev, (h, w))
    for t in range(st.n_em + 1):
        K.robust_estep(st, t, y, s, sm, wg, o["min_weight"])
        K.robust_update(st, t, c0=o["c0"], sigma_floor=o["sigma_floor"], slice_floor=o["slice_floor"],
                        min_pixels=o["min_pixels"])
    out = K.robust_weights(st, y, s, sm, wg, o["min_weight"], level=o["level"])
    return (out, st.info()) if return_info else out
