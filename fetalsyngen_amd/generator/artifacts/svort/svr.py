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

With `groups` several slices share ONE increment: a group (a stack, a package of slices) moves as a rigid
body of the volume frame about the volume centre, x' = Q x + d with [Q | d] = axisangle2mat(phi), phi the group's 6 parameters
starting at 0.  The per-slice kernel is the same; around it kernels.svr_compose turns the group's [Q | d] and its Jacobian into
every member's transform and the derivative of that transform with respect to phi, and kernels.svr_group_reduce adds the
members' normal equations.  The rounds are

    axisangle2mat(phi_trial);  axisangle2mat_backward over 12 G rows;  svr_compose;  svr_normal;  svr_group_reduce;
    svr_update on a state of G rows

and one svr_compose at the accepted phi after the loop.  With `groups=None` nothing of this is launched.
"""
from __future__ import annotations

import numpy as np
import torch

from .... import kernels as K
from ._solver import no_grad_inputs, prep


def parse_groups(groups, n, what="groups"):
    """HOST data (a sequence, a numpy array or a CPU integer tensor of length n; -1 = fixed, any other value >= 0 a group id) ->
    (ids, group, members, offsets): the ids in increasing order, the slices' relabelled ids 0..G-1 (or -1), each group's members
    in increasing slice index, and the G + 1 offsets into them, as int32 numpy arrays.  A device tensor raises TypeError:
    reading it would synchronise."""
    if isinstance(groups, torch.Tensor):
        if groups.device.type != "cpu":
            raise TypeError(f"{what} is host data: got a tensor on {groups.device}, and reading it would synchronise")
        if groups.dtype.is_floating_point or groups.dtype == torch.bool:
            raise TypeError(f"{what} must hold integers, got {groups.dtype}")
        groups = groups.numpy()
    g = np.asarray(groups)
    if g.dtype.kind not in "iu":
        raise TypeError(f"{what} must hold integers, got {g.dtype}")
    if g.shape != (n,):
        raise ValueError(f"{what} must have one entry per slice, ({n},), got {g.shape}")
    g = g.astype(np.int64)
    if (g < -1).any():
        raise ValueError(f"{what} holds -1 (fixed) or a group id >= 0, got {int(g.min())}")
    ids = np.unique(g[g >= 0])
    if ids.size == 0:
        raise ValueError(f"{what} names no group: every slice is fixed")
    group = np.where(g >= 0, np.searchsorted(ids, g), -1).astype(np.int32)
    members = np.concatenate([np.flatnonzero(group == j) for j in range(ids.size)]).astype(np.int32)
    offsets = np.concatenate(([0], np.cumsum(np.bincount(group[group >= 0], minlength=ids.size)))).astype(np.int32)
    return ids, group, members, offsets


def operands(n, slices, vol, psf, slices_mask, slices_weight):
    """the operands of a registration of n slices, prepared on the device of `slices`: (psf, slices (n,h,w), vol (D,H,W) or
    None when none is given yet, slices_mask, slices_weight)"""
    dev = slices.device
    nhw = (n, *(int(v) for v in slices.shape[-2:]))
    x = None if vol is None else prep(vol, tuple(int(v) for v in vol.shape[-3:]), dev)
    return (prep(psf, tuple(psf.shape), dev), prep(slices, nhw, dev), x, prep(slices_mask, nhw, dev, torch.bool),
            prep(slices_weight, nhw, dev))


def lm_rounds(par, stats_of, *, n_iter=10, lambda0=1e-3, factor=10.0, lambda_min=1e-9, lambda_max=1e10, min_overlap=0.5, tol=0.0):
    """The n_iter + 1 rounds of both solves on par (rows,6), the trial that every update overwrites: axisangle2mat(par), the
    Jacobian of its 12 entries, stats_of(mat, jac) -> the (rows, SVR_SLOTS) sums at the trial, svr_update.  -> (the state of
    `rows` rows, the Jacobian of the last round)"""
    rows, dev = int(par.shape[0]), par.device
    # everything the loop needs, made before it
    state = K.svr_state(rows, int(n_iter), dev)
    onehot = torch.eye(12, dtype=torch.float32, device=dev).repeat(rows, 1).view(12 * rows, 3, 4)  # grad_mat of entry k, per row
    rep = torch.empty((rows, 12, 6), dtype=torch.float32, device=dev)  # every row of par 12 times
    for k in range(state.n_iter + 1):
        mat = K.axisangle2mat(par)
        rep.copy_(par.view(rows, 1, 6).expand(rows, 12, 6))
        jac = K.axisangle2mat_backward(onehot, rep.view(12 * rows, 6)).view(rows, 12, 6)  # row k: d entry k / d parameter
        K.svr_update(state, k, stats_of(mat, jac), par, lambda0=lambda0, factor=factor, lambda_min=lambda_min, lambda_max=lambda_max,
                     min_overlap=min_overlap, tol=tol)
    return state, jac


def solve_groups(base, groups, y, x, ps, sm, wt, res_slice, *, min_weight=0.5, **lm):
    """The grouped solve on prepared device operands: base (n,3,4) -> (the composed transforms (n,3,4), the state of G rows, the
    host ids, the slices' relabelled ids on the device).  lm: the keywords of `lm_rounds`."""
    dev = y.device
    n, h, w = (int(v) for v in y.shape)
    ids, group, members, offsets = parse_groups(groups, n)
    G = int(ids.size)

    # the two index arrays and the slices' ids are uploaded once, before the first launch
    group_d = torch.from_numpy(group).to(dev)
    members_d, offsets_d = torch.from_numpy(members).to(dev), torch.from_numpy(offsets).to(dev)
    out = (torch.empty((n, 3, 4), dtype=torch.float32, device=dev), torch.empty((n, 12, 6), dtype=torch.float32, device=dev))
    stats = torch.empty((n, K.SVR_SLOTS), dtype=torch.float64, device=dev)
    gstats = torch.empty((G, K.SVR_SLOTS), dtype=torch.float64, device=dev)
    ws = torch.empty(K.svr_ws_bytes(n, h, w) // 8, dtype=torch.int64, device=dev)

    def stats_of(gm, gj):
        tr, jac = K.svr_compose(gm, gj, base, group_d, out=out)
        K.svr_normal(tr, jac, x, ps, y, sm, wt, res_slice, min_weight, out=stats, ws=ws)
        return K.svr_group_reduce(stats, members_d, offsets_d, out=gstats)

    state, gj = lm_rounds(torch.zeros((G, 6), dtype=torch.float32, device=dev), stats_of, **lm)
    # the accepted increments; the Jacobian of the last round is only a valid operand here, the jac it gives is not used
    tr, _ = K.svr_compose(K.axisangle2mat(state.theta_cur), gj, base, group_d, out=out)
    return tr, state, ids, group_d


def _group_info(state, ids):
    return dict(state.info(), group_poses=state.theta_cur.clone(), group_ids=[int(v) for v in ids])


def svr(poses, slices, vol, psf, res_slice, *, slices_mask=None, slices_weight=None, n_iter=10, lambda0=1e-3, factor=10.0,
        lambda_min=1e-9, lambda_max=1e10, min_weight=0.5, min_overlap=0.5, tol=0.0, return_info=False, groups=None):
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
    (n_iter + 1, n), row k for round k.

    groups: HOST data of length n (a sequence, a numpy array or a CPU integer tensor; a device tensor raises TypeError), -1 for
    a slice that stays where it is or the id of the group it moves with.  The ids need not be contiguous: they are relabelled
    in increasing order, and a group's members are taken in increasing slice index.  Every group gets ONE 6-parameter rigid
    motion of the volume frame, fitted to all its members' pixels together; `min_overlap` and `tol` act on the group's sums; a
    group with no pixel freezes at slot 0 and its slices keep their poses.  The poses of member slices come back through
    `mat2axisangle` of the moved matrices (a group that did not move, and every fixed slice: the input row bit for bit).  The
    histories are then (n_iter + 1, G), and the info dict gains `group_poses` (G,6), the groups' increments, and `group_ids`, the
    host list of the ids in row order.
    Walking the hierarchy of Kuklisova-Murgasova et al. 2012 is three kinds of call, each against a volume reconstructed
    WITHOUT the slices being moved (`align_stacks` does the first): `groups` = the stack of every slice, then `groups` = its
    package (the slices acquired in one sweep of an interleaved stack), then `groups=None` for single slices once the volume
    is sharp enough to hold them.  No driver is shipped for the walk."""
    no_grad_inputs("svr", poses=poses, slices=slices, vol=vol, psf=psf, slices_weight=slices_weight)
    n = int(poses.shape[0])
    lm = dict(n_iter=n_iter, lambda0=lambda0, factor=factor, lambda_min=lambda_min, lambda_max=lambda_max, min_overlap=min_overlap,
              tol=tol)
    theta = prep(poses, (n, 6), slices.device).clone()  # the trial; overwritten by every update
    ps, y, x, sm, wt = operands(n, slices, vol, psf, slices_mask, slices_weight)

    if groups is not None:
        tr, state, ids, group_d = solve_groups(K.axisangle2mat(theta), groups, y, x, ps, sm, wt, res_slice, min_weight=min_weight, **lm)
        # a slice moved iff its group's accepted increment is not 0 (selected on the device: nothing is read back)
        moved = (state.theta_cur != 0).any(dim=1)[group_d.clamp(min=0).long()] & (group_d >= 0)
        out = torch.where(moved[:, None], K.mat2axisangle(tr), theta)
        return (out, _group_info(state, ids)) if return_info else out

    h, w = (int(v) for v in slices.shape[-2:])
    stats = torch.empty((n, K.SVR_SLOTS), dtype=torch.float64, device=slices.device)
    ws = torch.empty(K.svr_ws_bytes(n, h, w) // 8, dtype=torch.int64, device=slices.device)

    def stats_of(tr, jac):
        return K.svr_normal(tr, jac, x, ps, y, sm, wt, res_slice, min_weight, out=stats, ws=ws)

    state, _ = lm_rounds(theta, stats_of, **lm)
    out = state.theta_cur.clone()
    return (out, state.info()) if return_info else out


class SVR:
    """`svr` for callers that hold `RigidTransform`-style (n,3,4) matrices: in and out through `mat2axisangle` /
    `axisangle2mat` on the device.  With `groups` (here or in the call; see `svr`) the matrices are moved directly, with no
    round trip through poses: a fixed slice and a group that did not move come back bit for bit."""

    def __init__(self, n_iter=10, groups=None, **options):
        self.n_iter, self.groups, self.options = n_iter, groups, options

    def __call__(self, transforms, slices, volume, psf, res_slice, slices_mask=None, slices_weight=None, groups=None,
                 return_info=False):
        no_grad_inputs("svr", transforms=transforms)
        mat = transforms.detach().to(device=slices.device, dtype=torch.float32).reshape(-1, 3, 4).contiguous()
        groups = self.groups if groups is None else groups
        if groups is None:
            poses = svr(K.mat2axisangle(mat), slices, volume, psf, res_slice, slices_mask=slices_mask, slices_weight=slices_weight,
                        n_iter=self.n_iter, return_info=return_info, **self.options)
            return (K.axisangle2mat(poses[0]), poses[1]) if return_info else K.axisangle2mat(poses)
        no_grad_inputs("svr", slices=slices, vol=volume, psf=psf, slices_weight=slices_weight)
        ps, y, x, sm, wt = operands(int(mat.shape[0]), slices, volume, psf, slices_mask, slices_weight)
        tr, state, ids, _ = solve_groups(mat, groups, y, x, ps, sm, wt, res_slice, n_iter=self.n_iter, **self.options)
        return (tr, _group_info(state, ids)) if return_info else tr
