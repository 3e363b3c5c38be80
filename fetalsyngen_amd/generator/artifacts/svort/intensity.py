"""`intensity_match`: per-slice intensity matching for `srr`, the third part of the slice-to-volume method beside the solve and
the robust statistics (Kuklisova-Murgasova et al. 2012; DESIGN.md section 28, the rule in include/fsg_hip.h, fsg_imatch_*).

Given the acquired slices y and the slices s = A x a reconstruction simulates, every slice gets one multiplicative scale (the
least-squares gain of y against s, the scales gauged to mean 1) and, with `bias_sigma`, one smooth multiplicative bias field
exp(bias): the normalised Gaussian blur of log(scale y / s) over the pixels above a floor, its weighted mean per slice removed.
`corrected` = scale * exp(-bias) * y is what the next solve takes in place of y.

The call is a fixed sequence of launches on torch's current stream (sums, scale, with a bias field its three launches, apply);
the sums, the gauge and the freeze live on the device (kernels.ImatchState): nothing is read back.  No atomics and every order
of summation fixed: bit-identical from run to run and on any stream.  Not differentiable.
"""
from __future__ import annotations

import math

import torch

from .... import kernels as K
from ._solver import check_options as _check_options, no_grad_inputs, prep

DEFAULTS = dict(min_weight=0.5, bias_sigma=None, log_floor=0.01, min_pixels=4)


def check_options(opts):
    """the options of `intensity_match` as a complete dict; ValueError for an unknown name or a value the kernels refuse"""
    o = _check_options("match", DEFAULTS, opts, ("min_weight", "log_floor"))
    if o["bias_sigma"] is not None:
        v = float(o["bias_sigma"])
        if not (math.isfinite(v) and v >= 0 and 3 * v <= K.IMATCH_MAX_RADIUS):
            raise ValueError(f"bias_sigma must be in [0, {K.IMATCH_MAX_RADIUS / 3:g}] pixels (or None), got {o['bias_sigma']!r}")
    return o


def intensity_match(slices, simulated, *, weights=None, slices_mask=None, sim_weight=None, min_weight=0.5, bias0=None,
                    bias_sigma=None, log_floor=0.01, min_pixels=4, return_info=False):
    """slices, simulated (n,[1,]h,w) -> (corrected (n,h,w), scale (n,), bias (n,h,w)), fp32 on the device.

    weights: per-pixel weights of the fit, the robust weights of `robust_weights` (None: 1); a pixel whose weight is not > 0 takes
    no part.  slices_mask (n,[1,]h,w) bool: pixels that take part.  sim_weight: the weight `slice_acquisition` computed for
    `simulated`; a pixel takes part iff weight > 0 and weight >= min_weight.  A NaN or Inf pixel takes no part.  bias0: the
    log-bias of an earlier call (None: 0); it is removed before the scale is fitted and the new field is added to it.
    bias_sigma: the standard deviation of the bias field's Gaussian in PIXELS; 12 mm / res_slice is customary (15 for 0.8 mm
    slices).  None or 0: scale only, and `bias` is bias0 or zeros.  log_floor: pixels where the scaled slice or the simulation is
    not above this fraction of the intensity range max y - min y count for the scale and not for the bias (the logarithm of a
    ratio of two background values is noise).  min_pixels: a slice with fewer pixels keeps scale 1 and its bias as given.
    The scales have arithmetic mean 1 over the slices that got one, and the bias field of a slice a weighted mean of 0: a common
    gain is the volume's.  If the slices are flat or no slice qualifies the call freezes: scale 1, bias as given.
    return_info: also the device arrays scale, ok (n) int32, frozen (1) int32, raw (n) the gains before the gauge, rows (n,5)
    the sums N, A, B, min y, max y, mean (n) the removed means, consts (R, floor, g, the number of ok slices)."""
    no_grad_inputs("intensity_match", slices=slices, simulated=simulated, weights=weights, sim_weight=sim_weight, bias0=bias0)
    o = check_options(dict(min_weight=min_weight, bias_sigma=bias_sigma, log_floor=log_floor, min_pixels=min_pixels))
    K._need_gpu(slices, simulated)
    dev = slices.device
    h, w = (int(v) for v in slices.shape[-2:])
    n = int(slices.shape[0])
    sigma = float(o["bias_sigma"] or 0.0)

    y, s, wg, om, b0 = (prep(t, (n, h, w), dev) for t in (slices, simulated, sim_weight, weights, bias0))
    sm = prep(slices_mask, (n, h, w), dev, torch.bool)
    st = K.imatch_state(n, dev, (h, w))
    K.imatch_sums(st, y, s, sm, wg, o["min_weight"], om, b0)
    K.imatch_scale(st, o["log_floor"], o["min_pixels"])
    b1 = K.imatch_bias(st, y, s, sigma, sm, wg, o["min_weight"], om, b0) if sigma > 0 else None
    corrected, bias = K.imatch_apply(st, y, b1, b0)
    out = (corrected, st.scale, bias)
    return (*out, st.info()) if return_info else out
