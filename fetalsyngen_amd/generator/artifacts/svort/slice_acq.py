"""`slice_acquisition` / `slice_acquisition_adjoint` with the reference's signatures
(svort/slice_acquisition/slice_acq.py:193-263), served by the gfx950 kernels of fsg_slice_acq.hip.

Tensor layouts are the reference's: vol (1,1,D,H,W), slices (n,1,h,w), masks bool of the same shapes,
transforms (n,3,4), psf (pd,ph,pw).  `semantics` selects which of the reference's two arithmetics is
followed: "cuda" (default; what the reference computes on a GPU) or "torch" (its CPU fallback, for
seed-matched comparison with a CPU run of the reference).  There is no CPU path here.

`slice_acquisition` is differentiable in `transforms` and `vol` under "cuda" semantics, as the reference's SliceAcqFunction
(fsg_slice_acq_bwd.hip); with `deterministic=True` (the default inside a keyed scope) its `vol` gradient
is summed in fixed point and is bit-identical from run to run as well.  `slice_acquisition_adjoint` is differentiable in `transforms` and `slices`, as
the reference's SliceAcqAdjointFunction (fsg_slice_acq_adjoint_bwd.hip), with or without `equalize`; both
of its gradients are bit-identical from run to run.  Neither has a backward under "torch" semantics, and the adjoint has none
for a `slice_ids` subset: those calls raise NotImplementedError when a gradient is asked for.
"""
from __future__ import annotations

import torch

from .... import kernels as K
from .... import rng as _rng

_SEMANTICS = "cuda"


def set_semantics(name: str) -> str:
    """Process-wide default for `semantics`; returns the previous value."""
    global _SEMANTICS
    if name not in ("cuda", "torch"):
        raise ValueError("semantics must be 'cuda' or 'torch'")
    prev, _SEMANTICS = _SEMANTICS, name
    return prev


def get_semantics() -> str:
    return _SEMANTICS


def _dev(t, device):
    return None if t is None else t.to(device).contiguous()


class SliceAcqFunction(torch.autograd.Function):
    """`slice_acquisition` with a backward, CUDA semantics (reference slice_acq.py:22-101): gradients with respect to
    `transforms` and `vol`; the masks, the PSF and the geometry get none, and the gradient that arrives for the weight
    output is ignored, as in the reference.  `deterministic` and `grad_scale` are kept for the backward and change nothing
    else: the forward is the same launch either way."""

    @staticmethod
    def forward(ctx, transforms, vol, vol_mask, slices_mask, psf, slice_shape, res_slice, need_weight, interp_psf,
                deterministic=False, grad_scale=1.0):
        out = K.slice_acq_forward(transforms, vol, vol_mask, slices_mask, psf, slice_shape, res_slice,
                                  need_weight=need_weight, interp_psf=interp_psf, semantics="cuda")
        ctx.save_for_backward(transforms, vol, vol_mask, slices_mask, psf)
        ctx.res_slice, ctx.interp_psf = res_slice, interp_psf
        ctx.deterministic, ctx.grad_scale = bool(deterministic), grad_scale
        return out

    @staticmethod
    def backward(ctx, grad_slices, *_grad_weight):
        transforms, vol, vol_mask, slices_mask, psf = ctx.saved_tensors
        # a call that did not ask for the fixed-point grad_vol is the call it always was
        det = dict(deterministic=True, grad_scale=ctx.grad_scale) if ctx.deterministic else {}
        grad_vol, grad_transforms = K.slice_acq_backward(
            transforms, vol, vol_mask, slices_mask, psf, grad_slices.contiguous(), ctx.res_slice, interp_psf=ctx.interp_psf,
            need_vol_grad=ctx.needs_input_grad[1], need_transforms_grad=ctx.needs_input_grad[0], **det)
        return grad_transforms, grad_vol, None, None, None, None, None, None, None, None, None


def slice_acquisition(transforms, vol, vol_mask, slices_mask, psf, slice_shape, res_slice, need_weight, interp_psf,
                      semantics=None, deterministic=None, grad_scale=1.0):
    """Differentiable in `transforms` and `vol` under `semantics="cuda"`: when either requires grad the call goes through
    SliceAcqFunction (kernels.slice_acq_backward); otherwise it is the plain forward launch.

    deterministic: how the backward sums the gradient of `vol` -- None = in fixed point inside a keyed scope
    (`rng.in_keyed_scope()`) under "cuda" semantics, as the adjoint's own rule; True / False force the fixed-point or the
    fp32-atomic accumulation.  It changes the backward only.  True with `semantics="torch"` raises ValueError.  grad_scale: a
    power of two in [2^-20, 2^20] the contributions are divided by before they are quantised (kernels.slice_acq_backward)."""
    sem = semantics or _SEMANTICS
    if deterministic and sem == "torch":
        raise ValueError("the deterministic grad_vol follows the CUDA semantics only (semantics='cuda')")
    if deterministic is None:
        deterministic = _rng.in_keyed_scope() and sem == "cuda"
    dev = vol.device
    if torch.is_grad_enabled() and (transforms.requires_grad or vol.requires_grad):
        if sem != "cuda":
            raise NotImplementedError("slice_acquisition is differentiable under semantics='cuda' only: the reference's CPU "
                                      "fallback (semantics='torch') is a sparse-matrix product with no backward kernel here")
        n, (h, w) = transforms.shape[0], slice_shape
        v = vol.reshape(vol.shape[-3:]).contiguous()
        vm = None if vol_mask is None or vol_mask.numel() == 0 else _dev(vol_mask, dev).reshape(v.shape)
        sm = None if slices_mask is None or slices_mask.numel() == 0 else _dev(slices_mask, dev).reshape(n, h, w)
        out = SliceAcqFunction.apply(_dev(transforms.float(), dev), v, vm, sm, _dev(psf.float(), dev), (h, w), res_slice,
                                     need_weight, interp_psf, bool(deterministic), grad_scale)
        if need_weight:
            return out[0].view(n, 1, h, w), out[1].view(n, 1, h, w)
        return out.view(n, 1, h, w)
    v = vol.reshape(vol.shape[-3:]).contiguous()
    n, (h, w) = transforms.shape[0], slice_shape
    vm = None if vol_mask is None or vol_mask.numel() == 0 else _dev(vol_mask, dev).reshape(v.shape)
    sm = None if slices_mask is None or slices_mask.numel() == 0 else _dev(slices_mask, dev).reshape(n, h, w)
    out = K.slice_acq_forward(_dev(transforms.float(), dev), v, vm, sm, _dev(psf.float(), dev), (h, w), res_slice,
                              need_weight=need_weight, interp_psf=interp_psf, semantics=sem)
    if need_weight:
        return out[0].view(n, 1, h, w), out[1].view(n, 1, h, w)
    return out.view(n, 1, h, w)


class SliceAcqAdjointFunction(torch.autograd.Function):
    """`slice_acquisition_adjoint` with a backward, CUDA semantics (reference slice_acq.py:104-190): gradients with respect
    to `transforms` and `slices`; the masks, the PSF and the geometry get none.  With `equalize` the equalised volume and its
    weight are saved for the backward, as in the reference; the gradient that arrives is read, never written."""

    @staticmethod
    def forward(ctx, transforms, psf, slices, slices_mask, vol_mask, vol_shape, res_slice, interp_psf, equalize, deterministic):
        out = K.slice_acq_adjoint(transforms, psf, slices, slices_mask, vol_mask, vol_shape, res_slice, interp_psf=interp_psf,
                                  equalize=equalize, semantics="cuda", return_weight=equalize, deterministic=deterministic)
        if equalize:
            vol, vol_weight = out
            ctx.save_for_backward(transforms, psf, slices, slices_mask, vol_mask, vol, vol_weight)
        else:
            vol = out
            ctx.save_for_backward(transforms, psf, slices, slices_mask, vol_mask)
        ctx.res_slice, ctx.interp_psf, ctx.equalize = res_slice, interp_psf, equalize
        return vol

    @staticmethod
    def backward(ctx, grad_vol):
        transforms, psf, slices, slices_mask, vol_mask, *eq = ctx.saved_tensors
        vol, vol_weight = eq if ctx.equalize else (None, None)
        grad_slices, grad_transforms = K.slice_acq_adjoint_backward(
            transforms, grad_vol.contiguous(), psf, slices, slices_mask, vol_mask, ctx.res_slice, interp_psf=ctx.interp_psf,
            equalize=ctx.equalize, vol=vol, vol_weight=vol_weight, need_slices_grad=ctx.needs_input_grad[2],
            need_transforms_grad=ctx.needs_input_grad[0])
        return grad_transforms, None, grad_slices, None, None, None, None, None, None, None


def slice_acquisition_adjoint(transforms, psf, slices, slices_mask, vol_mask, vol_shape, res_slice, interp_psf,
                              equalize, semantics=None, slice_ids=None, deterministic=None):
    """deterministic: None = inside a keyed scope (`rng.in_keyed_scope()`), where a sample is a function of its key; True /
    False force the fixed-point or the fp32-atomic accumulation (kernels.slice_acq_adjoint).

    Differentiable in `transforms` and `slices` under `semantics="cuda"`: when either requires grad the call goes through
    SliceAcqAdjointFunction (kernels.slice_acq_adjoint_backward); otherwise it is the plain adjoint launch."""
    sem = semantics or _SEMANTICS
    if deterministic is None:
        deterministic = _rng.in_keyed_scope() and sem == "cuda"
    if torch.is_grad_enabled() and (transforms.requires_grad or slices.requires_grad):
        if sem != "cuda":
            raise NotImplementedError("slice_acquisition_adjoint is differentiable under semantics='cuda' only: the reference's "
                                      "CPU fallback (semantics='torch') is a sparse-matrix product with no backward kernel here")
        if slice_ids is not None:
            raise NotImplementedError("slice_acquisition_adjoint has no backward for a slice_ids subset: pass the slices and "
                                      "transforms of the subset themselves")
        dev = slices.device
        h, w = slices.shape[-2:]
        D, H, W = (int(v) for v in vol_shape)
        n = transforms.shape[0]
        vm = None if vol_mask is None or vol_mask.numel() == 0 else _dev(vol_mask, dev).reshape(D, H, W)
        sm = None if slices_mask is None or slices_mask.numel() == 0 else _dev(slices_mask, dev).reshape(n, h, w)
        vol = SliceAcqAdjointFunction.apply(_dev(transforms.float(), dev), _dev(psf.float(), dev),
                                            slices.reshape(-1, h, w).contiguous(), sm, vm, (D, H, W), res_slice, interp_psf,
                                            bool(equalize), bool(deterministic))
        return vol.view(1, 1, D, H, W)
    dev = slices.device
    h, w = slices.shape[-2:]
    s = slices.reshape(-1, h, w).contiguous()
    D, H, W = (int(v) for v in vol_shape)
    n = transforms.shape[0]
    vm = None if vol_mask is None or vol_mask.numel() == 0 else _dev(vol_mask, dev).reshape(D, H, W)
    sm = None if slices_mask is None or slices_mask.numel() == 0 else _dev(slices_mask, dev).reshape(n, h, w)
    vol = K.slice_acq_adjoint(_dev(transforms.float(), dev), _dev(psf.float(), dev), s, sm, vm, (D, H, W), res_slice,
                              interp_psf=interp_psf, equalize=equalize, semantics=sem, slice_ids=slice_ids,
                              deterministic=bool(deterministic))
    return vol.view(1, 1, D, H, W)
