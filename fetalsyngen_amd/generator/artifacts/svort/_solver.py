"""What the drivers of the device solvers (`srr`, `svr`, `outlier.robust_weights`) share: none of them is differentiable, and
each brings its inputs to one device, dtype and shape before the first launch."""
from __future__ import annotations

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
