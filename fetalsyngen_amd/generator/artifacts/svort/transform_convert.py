"""Differentiable pose conversions on the device: mirror of the reference's transform_convert module
(svort/transform/transform_convert.py:164-209) and of the `RigidTransform` it carries (transform/transform.py:14-128), served
by the four kernels of fsg_transform_convert.hip.

`rigid.axisangle2mat`, `rigid.mat2axisangle` and `rigid.RigidTransform` detach and work on the host by design: the generator
never differentiates through a pose and relies on that.  A registration or reconstruction loop needs the opposite, and this
module is that opposite: the data stays on the CUDA device it was given on, in fp32, with its graph.

    axisangle2mat(ax), mat2axisangle(mat)   one launch forward, one backward, gradients as the reference's extension
    DeviceRigidTransform                    the methods of rigid.RigidTransform on such data; `to_host()` / `from_host()` cross over

There is no CPU path here: a CPU tensor raises the kernels' "MI355X only" RuntimeError.  `autograd.axisangle2mat_autograd` is
the CPU-capable differentiable form of the one direction it covers.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .... import kernels as K
from . import rigid


class Axisangle2MatFunction(torch.autograd.Function):
    """(n,6) -> (n,3,4) with the reference's backward (transform_convert.py:164-181)."""

    @staticmethod
    def forward(ctx, axisangle):
        ctx.save_for_backward(axisangle)
        return K.axisangle2mat(axisangle)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_mat):
        (axisangle,) = ctx.saved_tensors
        return K.axisangle2mat_backward(grad_mat.contiguous(), axisangle)


class Mat2AxisangleFunction(torch.autograd.Function):
    """(n,3,4) -> (n,6) with the reference's backward (transform_convert.py:184-201): the derivative with all 12 entries of a
    matrix free, except for rotations of 2e-3 rad or less, where it is the reference's floored rule."""

    @staticmethod
    def forward(ctx, mat):
        ctx.save_for_backward(mat)
        return K.mat2axisangle(mat)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_axisangle):
        (mat,) = ctx.saved_tensors
        return K.mat2axisangle_backward(mat, grad_axisangle.contiguous())


def _fp32(t):
    return t.to(torch.float32).contiguous()


def axisangle2mat(axisangle: torch.Tensor) -> torch.Tensor:
    """(n,6) [rotation vector | translation] -> (n,3,4) on the input's device, in fp32, graph kept.  With nothing requiring
    grad it is the plain forward launch."""
    a = _fp32(axisangle)
    if torch.is_grad_enabled() and a.requires_grad:
        return Axisangle2MatFunction.apply(a)
    return K.axisangle2mat(a)


def mat2axisangle(mat: torch.Tensor) -> torch.Tensor:
    """(n,3,4) -> (n,6) on the input's device, in fp32, graph kept.  With nothing requiring grad it is the plain forward
    launch."""
    m = _fp32(mat)
    if torch.is_grad_enabled() and m.requires_grad:
        return Mat2AxisangleFunction.apply(m)
    return K.mat2axisangle(m)


def _to_trans_first(mat):  # t' = R^T t
    R, t = mat[:, :, :3], mat[:, :, 3:]
    return torch.cat((R, R.transpose(-2, -1) @ t), -1)


def _to_trans_last(mat):  # t' = R t
    R, t = mat[:, :, :3], mat[:, :, 3:]
    return torch.cat((R, R @ t), -1)


class DeviceRigidTransform:
    """n rigid transforms, stored as given (axis-angle (n,6) or matrix (n,3,4)) with the reference's `trans_first` flag
    (transform.py:14-128), on the CUDA device they were given on, in fp32, graph kept.  The methods are those of
    `rigid.RigidTransform`; the two conversions are the kernels above, the rest ordinary torch operations in rigid.py's
    formulas, so every result stays differentiable in the data it was built from."""

    def __init__(self, data, trans_first=True, device=None):
        if device is not None:
            data = data.to(device)
        if not data.is_cuda:
            raise RuntimeError("DeviceRigidTransform holds device data (device='cuda:N'); rigid.RigidTransform is the host class")
        data = data.to(torch.float32)
        self.trans_first = trans_first
        self._axisangle = self._matrix = None
        if data.shape[1] == 6:
            self._axisangle = data
        elif data.shape[1] == 3:
            self._matrix = data
        else:
            raise Exception("Unknown format for rigid transform!")

    def _data(self):
        return self._axisangle if self._axisangle is not None else self._matrix

    def matrix(self, trans_first=True):
        mat = self._matrix if self._matrix is not None else axisangle2mat(self._axisangle)
        if self.trans_first and not trans_first:
            mat = _to_trans_last(mat)
        elif not self.trans_first and trans_first:
            mat = _to_trans_first(mat)
        return mat

    def axisangle(self, trans_first=True):
        ax = self._axisangle if self._axisangle is not None else mat2axisangle(self._matrix)
        if self.trans_first and not trans_first:
            ax = mat2axisangle(_to_trans_last(axisangle2mat(ax)))
        elif not self.trans_first and trans_first:
            ax = mat2axisangle(_to_trans_first(axisangle2mat(ax)))
        return ax

    def inv(self):
        m = self.matrix(True)
        R, t = m[:, :, :3], m[:, :, 3:]
        return DeviceRigidTransform(torch.cat((R.transpose(-2, -1), -(R @ t)), -1), True)

    def compose(self, other):
        a, b = self.matrix(True), other.matrix(True)
        R1, t1, R2, t2 = a[:, :, :3], a[:, :, 3:], b[:, :, :3], b[:, :, 3:]
        return DeviceRigidTransform(torch.cat((R1 @ R2, t2 + R2.transpose(-2, -1) @ t1), -1), True)

    def __getitem__(self, idx):
        d = self._data()[idx]
        if d.dim() < self._data().dim():
            d = d.unsqueeze(0)
        return DeviceRigidTransform(d, self.trans_first)

    def detach(self):
        return DeviceRigidTransform(self._data().detach(), self.trans_first)

    @property
    def device(self):
        return self._data().device

    def dtype(self):
        return self._data().dtype

    def __len__(self):
        return self._data().shape[0]

    @staticmethod
    def cat(transforms):
        return DeviceRigidTransform(torch.cat([t.matrix(True) for t in transforms], 0), True)

    def mean(self, trans_first=True, simple_mean=True):
        if not simple_mean:
            raise NotImplementedError("average_rotation (transform.py:301-336) is not on the generator's path")
        return DeviceRigidTransform(self.axisangle(trans_first).mean(0, keepdim=True), trans_first)

    def to_host(self) -> rigid.RigidTransform:
        """The same transforms as a detached host object."""
        return rigid.RigidTransform(self._data(), self.trans_first)

    @staticmethod
    def from_host(rt: rigid.RigidTransform, device) -> "DeviceRigidTransform":
        return DeviceRigidTransform(rt._data(), rt.trans_first, device=device)
