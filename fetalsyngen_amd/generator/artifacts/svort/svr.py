"""`svr`: per-slice slice-to-volume registration by Gauss-Newton with Levenberg-Marquardt damping.

Each slice has its own 6 pose parameters theta = [rotation vector | translation] (the rows of `transform_convert`) and its own
least-squares problem

    min over theta of  sum over the pixels P of  w (A(theta) vol - y)^2

with A = `slice_acquisition` in the CUDA semantics, LINEAR geometry, P the pixels inside `slices_mask` whose PSF weight inside
the volume is at least `min_weight`, and w = `slices_weight`.  One kernel pass over the PSF taps gives the simulated pixel, its
derivative with respect to the pose and the pixel's share of the 6x6 normal matrix H, of the gradient g and of the cost
(kernels.svr_normal); a second kernel takes the damped step delta = -(H + lambda diag H)^-1 g, accepts the trial when the cost
fell and adapts lambda (kernels.svr_update).  It is the pose half of the motion-correction pair whose volume half is `srr`.

The loop is a fixed sequence of launches on torch's current stream, n_iter + 1 rounds of

    axisangle2mat(theta_trial);  axisangle2mat_backward (the Jacobian of the 12 transform entries);  svr_normal;  svr_update

All decisions live on the device (kernels.SVRState): nothing is read back, so the call never synchronises with the host, and
the result is a pure function of its inputs: bit-identical from run to run, on any stream, for any order of the slices, and
for a slice solved alone or in a batch.  Not differentiable.
"""
from __future__ import annotations

import torch

from .... import kernels as K
from ._solver import no_grad_inputs, prep


def svr(poses, slices, vol, psf, res_slice, *, slices_mask=None, slices_weight=None, n_iter=10, lambda0=1e-3, factor=10.0,
        lambda_min=1e-9, lambda_max=1e10, min_weight=0.5, min_overlap=0.5, tol=0.0, return_info=False):
    """poses (n,6) [rotation vector | translation], slices (n,1,h,w) or (n,h,w), vol (..,D,H,W), psf (pd,ph,pw) -> (n,6) poses
    after `n_iter` damped Gauss-Newton steps per slice.

    slices_mask (n,[1,]h,w) bool: pixels that take part.  slices_weight: non-negative per-pixel weights; to reject outliers
    (signal voids, slices that do not fit the volume) pass `outlier.robust_weights(slices, simulated, sim_weight=...)`, with
    `simulated` and its weight from `kernels.slice_acq_forward(..., need_weight=True)` at the poses the call starts from
    (DESIGN.md section 25).  lambda0, factor,
    lambda_min, lambda_max: the damping starts at lambda0, is divided by `factor` after an accepted step (not below lambda_min)
    and multiplied after a rejected one; a slice whose lambda passes lambda_max stops.  min_weight: a pixel takes part when the
    PSF weight it finds inside the volume is at least this.  min_overlap: a trial that keeps fewer than min_overlap times the
    starting number of pixels is rejected.  tol: a slice stops once an accepted step lowers its cost by no more than tol times
    the cost.  A slice with no pixel, no weight or non-finite sums keeps the pose it came with, bit for bit.
    return_info: also a dict of the device histories cost, lambda (float64), accepted, frozen (int32), each
    (n_iter + 1, n), row k for round k."""
    no_grad_inputs("svr", poses=poses, slices=slices, vol=vol, psf=psf, slices_weight=slices_weight)
    n_iter = int(n_iter)
    dev = slices.device
    h, w = (int(v) for v in slices.shape[-2:])
    D, H, W = (int(v) for v in vol.shape[-3:])
    n = int(poses.shape[0])

    theta = prep(poses, (n, 6), dev).clone()  # the trial; overwritten by every update
    ps = prep(psf, tuple(psf.shape), dev)
    y = prep(slices, (n, h, w), dev)
    x = prep(vol, (D, H, W), dev)
    sm = prep(slices_mask, (n, h, w), dev, torch.bool)
    wt = prep(slices_weight, (n, h, w), dev)

    # everything the loop needs, made before it
    state = K.svr_state(n, n_iter, dev)
    onehot = torch.eye(12, dtype=torch.float32, device=dev).repeat(n, 1).view(12 * n, 3, 4)  # grad_mat of entry k, per slice
    rep = torch.empty((n, 12, 6), dtype=torch.float32, device=dev)  # every pose 12 times
    stats = torch.empty((n, K.SVR_SLOTS), dtype=torch.float64, device=dev)
    ws = torch.empty(K.svr_ws_bytes(n, h, w) // 8, dtype=torch.int64, device=dev)
    for k in range(n_iter + 1):
        tr = K.axisangle2mat(theta)
        rep.copy_(theta.view(n, 1, 6).expand(n, 12, 6))
        jac = K.axisangle2mat_backward(onehot, rep.view(12 * n, 6)).view(n, 12, 6)  # row k: d entry k / d pose
        K.svr_normal(tr, jac, x, ps, y, sm, wt, res_slice, min_weight, out=stats, ws=ws)
        K.svr_update(state, k, stats, theta, lambda0=lambda0, factor=factor, lambda_min=lambda_min, lambda_max=lambda_max,
                     min_overlap=min_overlap, tol=tol)
    out = state.theta_cur.clone()
    return (out, state.info()) if return_info else out


class SVR:
    """`svr` for callers that hold `RigidTransform`-style (n,3,4) matrices: in and out through `mat2axisangle` /
    `axisangle2mat` on the device."""

    def __init__(self, n_iter=10, **options):
        self.n_iter, self.options = n_iter, options

    def __call__(self, transforms, slices, volume, psf, res_slice, slices_mask=None, slices_weight=None):
        no_grad_inputs("svr", transforms=transforms)
        mat = transforms.detach().to(device=slices.device, dtype=torch.float32).reshape(-1, 3, 4).contiguous()
        poses = svr(K.mat2axisangle(mat), slices, volume, psf, res_slice, slices_mask=slices_mask, slices_weight=slices_weight,
                    n_iter=self.n_iter, **self.options)
        return K.axisangle2mat(poses)
