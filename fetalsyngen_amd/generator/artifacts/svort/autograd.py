"""Differentiable counterpart of `rigid.axisangle2mat` for code that fits slice poses through `slice_acquisition`.

`rigid.axisangle2mat` and `RigidTransform` detach and work on the host by design (the generator never differentiates through a
pose, and relies on that).  A registration or reconstruction loop needs the opposite: the (n,6) parameters stay where they
are, on the GPU as a rule, and the (n,3,4) matrices keep their graph.  The formulas and their operation order are those of
`rigid.axisangle2mat`, so on the CPU the two agree bit for bit.
"""
from __future__ import annotations

import torch

from .rigid import EPS


def axisangle2mat_autograd(axisangle: torch.Tensor) -> torch.Tensor:
    """(n,6) [rotation vector | translation] -> (n,3,4) on the input's device and in its dtype, graph kept.  Rodrigues' formula
    for theta^2 > 1e-6, the first-order matrix I + [a]x below (transform_convert.py:24-85).  Both branches are evaluated
    for every row and selected with `where`; the square root sees 1 in place of a small theta^2, so neither branch puts a
    non-finite value, or a non-finite gradient, into the other."""
    if axisangle.dim() != 2 or axisangle.shape[1] != 6:
        raise ValueError(f"axisangle must be (n,6), got {tuple(axisangle.shape)}")
    ang, t = axisangle[:, :3], axisangle[:, 3:]
    th2 = (ang**2).sum(1)
    big = th2 > EPS
    th = torch.sqrt(torch.where(big, th2, torch.ones_like(th2)))
    u = ang / th[:, None]
    s, c = torch.sin(th), torch.cos(th)
    o = 1 - c
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    rows = [
        (c + x * x * o, x * y * o - z * s, y * s + x * z * o),
        (z * s + x * y * o, c + y * y * o, -x * s + y * z * o),
        (-y * s + x * z * o, x * s + y * z * o, c + z * z * o),
    ]
    one, ax, ay, az = torch.ones_like(th2), ang[:, 0], ang[:, 1], ang[:, 2]
    small = [(one, -az, ay), (az, one, -ax), (-ay, ax, one)]
    rot = torch.stack([torch.stack([torch.where(big, rows[i][j], small[i][j]) for j in range(3)], 1) for i in range(3)], 1)
    return torch.cat((rot, t[:, :, None]), 2)
