"""`align_stacks`: rigid alignment of whole stacks, the first level of the motion-correction hierarchy.

Every stack but the template moves as ONE rigid body (`svr` with `groups`), and each is registered against a volume that does
NOT contain it: reconstructed from the very slices being registered, a volume absorbs their misalignment and every slice then
registers to its own displaced image.  Leaving the moving stack out of the target is what makes the
alternation of `srr` and `svr` lower the pose error.

    round 0     target = srr of the template stack alone; every other stack is registered to it, all in one batch
    round r>=1  for every stack g but the template: target = srr of all stacks but g at the poses the round started from
                (the left-out slices are excluded through `slices_mask`); g is registered to it.  The update is Jacobi-style:
                all stacks move at the end of the round.

A fixed sequence of launches on torch's current stream; nothing is read back.  Not differentiable.
"""
from __future__ import annotations

import torch

from ._solver import no_grad_inputs, prep
from .srr import srr as _srr
from .svr import operands, parse_groups, solve_groups


def align_stacks(transforms, slices, stack_ids, psf, vol_shape, res_slice, *, template=None, n_rounds=3,
                 srr=dict(lam=0.03, n_iter=12), svr=dict(n_iter=10), slices_mask=None, slices_weight=None, return_info=False):
    """transforms (n,3,4), slices (n,1,h,w) or (n,h,w), stack_ids (n) -> (n,3,4) transforms after `n_rounds` rounds.

    stack_ids: HOST data as `svr`'s `groups` (a sequence, a numpy array or a CPU integer tensor; a device tensor raises
    TypeError), the stack of every slice, ids >= 0.  template: the id of the stack that never moves (default: the stack of the
    first slice); its transforms are returned bit for bit.  srr: the options of the target reconstructions (`srr`'s keywords;
    the regulariser `lam` keeps a target from few stacks well posed).  svr: the options of the grouped registrations (`svr`'s
    keywords n_iter, lambda0, ..., tol).  slices_mask, slices_weight: as `srr` and `svr` take them; both see them.
    Inside a keyed scope the reconstructions are deterministic, as `srr` is, and so is the result.
    return_info: also a dict: "rounds", per round the list of (stack ids, the `svr` info dict of that registration), and
    "template"."""
    no_grad_inputs("align_stacks", transforms=transforms, slices=slices, psf=psf, slices_weight=slices_weight)
    n_rounds = int(n_rounds)
    if n_rounds < 1:
        raise ValueError(f"n_rounds must be >= 1, got {n_rounds}")
    sopts, ropts = dict(srr), dict(svr)
    for name, opts, taken in (("srr", sopts, ("slices_mask", "slices_weight", "return_info", "x0")),
                              ("svr", ropts, ("slices_mask", "slices_weight", "return_info", "groups"))):
        bad = [k for k in taken if k in opts]
        if bad:
            raise ValueError(f"align_stacks sets {bad} of {name} itself")
    dev = slices.device
    h, w = (int(v) for v in slices.shape[-2:])
    D, H, W = (int(v) for v in vol_shape)
    n = int(transforms.shape[0])
    ids, stack, _, _ = parse_groups(stack_ids, n, "stack_ids")
    if (stack < 0).any():
        raise ValueError("stack_ids must name the stack of every slice: -1 is not a stack")
    first = int(ids[stack[0]])
    template = first if template is None else int(template)
    if template not in ids.tolist():
        raise ValueError(f"template {template} is not one of the stacks {ids.tolist()}")
    if ids.size < 2:
        raise ValueError("align_stacks needs the template and at least one stack to move")
    t = ids.tolist().index(template)
    moving = [g for g in range(ids.size) if g != t]

    tr = prep(transforms, (n, 3, 4), dev)
    ps, y, _, sm, wt = operands(n, slices, None, psf, slices_mask, slices_weight)  # the targets are reconstructed below

    # the index sets and the leave-out masks, made on the host and uploaded before the first launch
    stack_t = torch.from_numpy(stack.astype("int64"))

    def rows(keep):
        return torch.nonzero(keep).view(-1).to(dev)

    def mask(keep):
        m = keep.view(n, 1, 1).expand(n, h, w).to(dev)
        return (m if sm is None else m & sm).contiguous()

    sel = {g: rows(stack_t == g) for g in moving}
    sel_all = rows(stack_t != t)
    mask_template = mask(stack_t == t)
    mask_without = {g: mask(stack_t != g) for g in moving}
    groups_all = stack[stack != t]

    def sub(a, idx):
        return None if a is None else a.index_select(0, idx)

    def register(cur, idx, groups, target):
        moved, state, gids, _ = solve_groups(cur.index_select(0, idx), groups, sub(y, idx), target.view(D, H, W), ps, sub(sm, idx),
                                             sub(wt, idx), res_slice, **ropts)
        return moved, dict(state.info(), group_poses=state.theta_cur.clone())

    rounds = []
    for r in range(n_rounds):
        nxt = tr.clone()
        if r == 0:
            target = _srr(tr, y, ps, (D, H, W), res_slice, slices_mask=mask_template, slices_weight=wt, **sopts)
            moved, info = register(tr, sel_all, groups_all, target)
            nxt.index_copy_(0, sel_all, moved)
            rounds.append([([int(ids[g]) for g in moving], info)])
        else:
            done = []
            for g in moving:
                target = _srr(tr, y, ps, (D, H, W), res_slice, slices_mask=mask_without[g], slices_weight=wt, **sopts)
                moved, info = register(tr, sel[g], [0] * int(sel[g].numel()), target)
                nxt.index_copy_(0, sel[g], moved)
                done.append(([int(ids[g])], info))
            rounds.append(done)
        tr = nxt
    return (tr, dict(rounds=rounds, template=template)) if return_info else tr
