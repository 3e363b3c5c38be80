"""What the drivers of the device solvers (`srr`, `svr`, `outlier.robust_weights`) share: none of them is differentiable, and
each brings its inputs to one device, dtype and shape before the first launch."""
from __future__ import annotations

import math

import torch


def no_grad_inputs(solver_name, **tensors):
    """NotImplementedError, naming the solver and the argument, when an input asks for a gradient the solve cannot give"""
    if not torch.is_grad_enabled():
        return
    for name, t in tensors.items():
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise NotImplementedError(f"{solver_name} is not differentiable: `{name}` requires grad.  Detach it, or call under "
                                      "torch.no_grad(); gradients through the solve are not implemented")


def prep(t, shape, device, dtype=torch.float32):
    """`t` detached, on `device`, as contiguous `dtype` of `shape`; None or an empty tensor (the reference's "absent") -> None"""
    if t is None or t.numel() == 0:
        return None
    return t.detach().to(device=device, dtype=dtype).reshape(shape).contiguous()


def check_options(kind, defaults, opts, nonneg):
    """`opts` over `defaults` as a complete dict; ValueError for an unknown name, for one of `nonneg` that is not finite and
    >= 0, and for min_pixels < 0.  What the options of `robust_weights` and `intensity_match` share."""
    unknown = set(opts) - set(defaults)
    if unknown:
        raise ValueError(f"unknown {kind} option(s) {sorted(unknown)}; known: {sorted(defaults)}")
    o = dict(defaults, **opts)
    for name in nonneg:
        v = float(o[name])
        if not (math.isfinite(v) and v >= 0):
            raise ValueError(f"{name} must be finite and >= 0, got {o[name]!r}")
    if int(o["min_pixels"]) < 0:
        raise ValueError(f"min_pixels must be >= 0, got {o['min_pixels']!r}")
    return o


def refinement(count_name, count, opts_name, opts, what, check):
    """A refinement of `srr` that runs `count` rounds with the options `opts` (None: the defaults) -> (count, the options the
    caller gave, checked by `check`)"""
    count = int(count)
    if count < 0:
        raise ValueError(f"{count_name} must be >= 0, got {count}")
    if opts is not None and count == 0:
        raise ValueError(f"{opts_name} sets the options of the {what}: it needs {count_name} > 0")
    full = check(dict(opts or {}))
    return count, {k: full[k] for k in opts or ()}
