"""`srr`: slice-to-volume reconstruction by conjugate gradients on the normal equations

    (A^T P W A + mu I) x = A^T P W y + mu z        restricted to the voxels of `vol_mask`

with A = `slice_acquisition` and A^T = `slice_acquisition_adjoint` (not equalised) in the CUDA semantics, P the pixels the
adjoint keeps (PSF weight inside the volume >= 0.5) and W = diag(slices_weight).  The reference's svort/ was vendored without
this solve; it is the volume update of the SVoRT / NeSVoR family.

The loop is a fixed sequence of launches on torch's current stream: per iteration the forward, (the weight,) the adjoint and
the three vector kernels of fsg_cg.hip.  alpha, beta, the dot products and the stopping decision live on the device
(kernels.CGWorkspace): nothing is read back, so the call never synchronises with the host.  With
`deterministic=True` (the default inside a keyed scope) the adjoint is the fixed-point one and the whole solve is a pure
function of its inputs: bit-identical from run to run, on any stream and for any order of the slices.

`vol_mask` is NOT passed to the operators (their per-pixel weights treat masked voxels differently: the forward leaves them
out of its weight, the adjoint does not, and A^T would stop being the transpose of A); it is applied around them as the 0/1
projection V by the vector kernels.  Not differentiable.

With `lam > 0` the operator gains the first-order regulariser of DESIGN.md section 24: M + lam L, L the graph Laplacian of the
6-neighbour grid inside V (kernels.tk1_apply, one launch after every application of A^T P W A; the cg kernels are untouched).
`huber_delta` and `n_outer` make it edge preserving by reweighting: `n_outer` complete solves, each guided by the x of the one
before, whose edges steeper than `huber_delta` are weighted down by Huber's rule.  With `lam == 0`, the default, the launch
sequence is the one above and tk1_apply is never called.

With `n_robust > 0` the solve rejects outliers: after the complete solve the slices are simulated from
its x, `outlier.robust_weights` turns the residual into per-pixel weights, they multiply the caller's `slices_weight`, the
right-hand side is rebuilt and the whole solve runs again from `x0` as given, `n_robust` times.  With `n_robust == 0`, the
default, none of this is launched.

With `n_match > 0` the solve matches the slices' intensities: after a complete solve
`intensity.intensity_match` fits one scale and, with `bias_sigma`, one smooth bias field per slice against the slices simulated
from its x, and the next solve takes the corrected slices in place of y.  The refinement loop runs max(n_robust, n_match) rounds;
a round first takes the robust weights, then the match under them.  With `n_match == 0`, the default, none of it is launched.
"""
from __future__ import annotations

import math

import torch

from .... import kernels as K
from .... import rng as _rng
from ._solver import no_grad_inputs, prep, refinement
from .intensity import check_options as _match_options, intensity_match
from .outlier import check_options as _robust_options, robust_weights


def srr(transforms, slices, psf, vol_shape, res_slice, *, interp_psf=False, slices_mask=None, vol_mask=None,
        slices_weight=None, x0=None, mu=0.0, z=None, n_iter=10, tol=0.0, output_relu=True, deterministic=None,
        value_scale=1.0, return_info=False, lam=0.0, huber_delta=None, n_outer=1, guide=None,
        n_robust=0, robust=None, n_match=0, match=None):
    """transforms (n,3,4), slices (n,1,h,w) or (n,h,w), psf (pd,ph,pw) -> volume (1,1,D,H,W) after `n_iter` CG iterations.

    slices_mask (n,[1,]h,w) bool: pixels that take part.  vol_mask (D,H,W)-shaped bool: the voxels solved for, the rest is 0.
    slices_weight: non-negative per-pixel weights.  x0: the start (default 0), z / mu: the Tikhonov term mu |x - z|^2.
    tol: the solve stops changing x once <r,r> <= tol (on the device; the launches still run and do nothing).
    output_relu: x = max(x, 0) at the end.  deterministic: None = inside a keyed scope; value_scale: as
    kernels.slice_acq_adjoint.  return_info: also a dict of the device histories rr, pq (float64), alpha, beta (float32) and
    frozen (int32), n_iter + 1 slots each, slot k for iteration k; with lam > 0 they are the last round's and "rounds" lists every round's dict.
    lam: the weight of the first-order regulariser lam * sum over the grid edges inside vol_mask of c |x_i - x_j|^2 (0 = none).
    huber_delta: with a guide, c = min(1, huber_delta / |g_i - g_j|) instead of 1.  n_outer: that many complete solves of
    `n_iter` iterations; round 0 is guided by `guide` (None: c = 1), every later round starts from the x of the round before
    and is guided by it.  The relu is applied in the last round only.
    n_robust: that many outlier-rejection rounds: weights from `robust_weights(slices, A x, ...)` times `slices_weight`, then
    the complete solve (all `n_outer` rounds) again from `x0`; the relu is applied in the very last solve only.  robust: a
    dict of `robust_weights`' options (n_em, c0, sigma_floor, slice_floor, min_pixels, level, min_weight).  With n_robust > 0
    the info dict gains "robust": the list of the EM histories, one dict per rejection round.
    n_match: that many intensity-matching rounds, run beside the rejection rounds (max(n_robust, n_match) refinement rounds in
    all): round r < n_match calls `intensity_match(slices, A x, weights=<the weights the next solve takes>, bias0=<the bias of
    the round before>)` on the slices AS GIVEN, and the next solve (and the next round's `robust_weights`) takes its `corrected`
    in place of `slices`.  match: a dict of `intensity_match`'s options (bias_sigma, log_floor, min_pixels, min_weight).  With
    n_match > 0 the info dict gains "match": per round a dict of the device arrays scale, ok, frozen; and "match_bias", the bias
    (n,h,w) of the last round."""
    no_grad_inputs("srr", transforms=transforms, slices=slices, psf=psf, slices_weight=slices_weight, x0=x0, z=z, guide=guide)
    lam, n_outer = float(lam), int(n_outer)
    if not (math.isfinite(lam) and lam >= 0):
        raise ValueError(f"lam must be finite and >= 0, got {lam}")
    if huber_delta is not None:
        huber_delta = float(huber_delta)
        if not lam > 0:
            raise ValueError("huber_delta weights the regulariser: it needs lam > 0")
        if not (math.isfinite(huber_delta) and huber_delta > 0):
            raise ValueError(f"huber_delta must be finite and > 0, got {huber_delta}")
    if n_outer < 1:
        raise ValueError(f"n_outer must be >= 1, got {n_outer}")
    if huber_delta is None and (n_outer > 1 or guide is not None):
        raise ValueError("n_outer > 1 and guide reweight the edges by huber_delta: give it")
    n_robust, ropts = refinement("n_robust", n_robust, "robust", robust, "outlier rejection", _robust_options)
    n_match, mopts = refinement("n_match", n_match, "match", match, "intensity matching", _match_options)
    n_refine = max(n_robust, n_match)
    if deterministic is None:
        deterministic = _rng.in_keyed_scope()
    det = bool(deterministic)
    n_iter = int(n_iter)
    dev = slices.device
    h, w = (int(v) for v in slices.shape[-2:])
    D, H, W = (int(v) for v in vol_shape)
    n = int(transforms.shape[0])
    nvox = D * H * W

    tr = prep(transforms, (n, 3, 4), dev)
    ps = prep(psf, tuple(psf.shape), dev)
    y = prep(slices, (n, h, w), dev)
    sm = prep(slices_mask, (n, h, w), dev, torch.bool)
    vm = prep(vol_mask, (D, H, W), dev, torch.bool)
    wt = wt_given = prep(slices_weight, (n, h, w), dev)
    zz = prep(z, (D, H, W), dev)
    xs = prep(x0, (D, H, W), dev)
    gd = prep(guide, (D, H, W), dev)

    def normal(v):
        """A^T P W A v"""
        s = K.slice_acq_forward(tr, v, None, sm, ps, (h, w), res_slice, interp_psf=interp_psf, semantics="cuda")
        if wt is not None:
            s = K.mul(s, wt)
        return K.slice_acq_adjoint(tr, ps, s, sm, None, (D, H, W), res_slice, interp_psf=interp_psf, semantics="cuda",
                                   deterministic=det, value_scale=value_scale)

    def apply(v, g):
        """(A^T P W A + lam L_g) v"""
        t = normal(v)
        if lam > 0:
            K.tk1_apply(v, t, (D, H, W), lam, mask=vm, guide=g, delta=None if g is None else huber_delta, out=t)
        return t

    robust_info, match_info = [], []
    xs0, gd0 = xs, gd
    y_given, bias = y, None
    for rb in range(n_refine + 1):
        xs, gd = xs0, gd0  # every robust round solves from x0 as given: a warm start keeps the outliers' imprint
        rounds = []
        for o in range(n_outer):
            ws = K.cg_workspace(nvox, n_iter, dev)
            if o == 0:
                b = K.slice_acq_adjoint(tr, ps, y if wt is None else K.mul(y, wt), sm, None, (D, H, W), res_slice,
                                        interp_psf=interp_psf, semantics="cuda", deterministic=det, value_scale=value_scale)
                if rb == 0 and xs is not None and vm is not None:
                    xs = xs0 = torch.where(vm, xs, torch.zeros((), dtype=xs.dtype, device=dev))  # A sees V x0
            else:
                xs = gd = x  # the round before: already inside V
            t0 = None if xs is None else apply(xs, gd)
            r, p, x = (torch.empty((D, H, W), dtype=torch.float32, device=dev) for _ in range(3))
            K.cg_init(ws, b, r, p, x, mask=vm, mu=mu, z=zz, x0=xs, t0=t0)
            relu = bool(output_relu) and o == n_outer - 1 and rb == n_refine
            for k in range(1, n_iter + 1):
                q = apply(p, gd)
                K.cg_q(ws, k, p, q, mask=vm, mu=mu, tol=tol)
                K.cg_step(ws, k, p, q, x, r, relu=relu)
                K.cg_dir(ws, k, r, p, tol=tol)
            rounds.append(ws.info())
        if rb < n_refine:
            s, wgt = K.slice_acq_forward(tr, x, None, sm, ps, (h, w), res_slice, need_weight=True, interp_psf=interp_psf,
                                         semantics="cuda")
        if rb < n_robust:
            rw = robust_weights(y, s, slices_mask=sm, sim_weight=wgt, return_info=True, **ropts)
            robust_info.append(rw[1])
            wt = rw[0] if wt_given is None else K.mul(rw[0], wt_given)
        if rb < n_match:
            y, _, bias, mi = intensity_match(y_given, s, weights=wt, slices_mask=sm, sim_weight=wgt, bias0=bias, return_info=True,
                                             **mopts)
            match_info.append({k: mi[k] for k in ("scale", "ok", "frozen")})
    out = x.view(1, 1, D, H, W)
    if not return_info:
        return out
    info = dict(rounds[-1], rounds=rounds) if lam > 0 else rounds[-1]  # lam == 0: the dict it has always been
    if n_robust > 0:
        info = dict(info, robust=robust_info)
    return out, (dict(info, match=match_info, match_bias=bias) if n_match > 0 else info)


class SRR:
    """`srr` behind the call shape of `PSFreconstruction`: `params` carries psf, interp_psf, res_s, res_r, s_thick and
    volume_shape."""

    def __init__(self, n_iter=10, tol=0.0, output_relu=True, lam=0.0, huber_delta=None, n_outer=1, n_robust=0, robust=None, n_match=0,
                 match=None):
        self.n_iter, self.tol, self.output_relu = n_iter, tol, output_relu
        # the regulariser, the outlier rejection and the intensity matching of `srr`, handed on only when set
        self.reg = {k: v for k, v, unset in (("lam", lam, 0.0), ("huber_delta", huber_delta, None), ("n_outer", n_outer, 1),
                                             ("n_robust", n_robust, 0), ("robust", robust, None),
                                             ("n_match", n_match, 0), ("match", match, None))
                    if v != unset}

    def __call__(self, transforms, slices, volume, params, p=None, mu=0, z=None, vol_mask=None, slices_mask=None):
        vol_shape = params["volume_shape"] if volume is None else volume.shape[-3:]
        return srr(transforms, slices, params["psf"], vol_shape, params["res_s"] / params["res_r"],
                   interp_psf=params.get("interp_psf", False), slices_mask=slices_mask, vol_mask=vol_mask, slices_weight=p,
                   x0=volume, mu=mu, z=z, n_iter=self.n_iter, tol=self.tol, output_relu=self.output_relu, **self.reg)
