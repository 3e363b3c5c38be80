"""CPU restatement of the conjugate-gradient slice-to-volume reconstruction `svort.srr` (the rule of the
vector kernels is in include/fsg_hip.h, fsg_cg_*).  Test infrastructure, numpy only; `ft` is the type every operation is done
in, as in tests/util_sa_adjoint_backward64.adjoint64.

    forward(...)       A, the slice acquisition in the CUDA semantics WITHOUT vol_mask, written beside adjoint64: the same
                       geometry object and tap walk, a gather where the adjoint scatters.  Held to
                       oracle.fsg_oracle_sr.slice_acq_forward_cuda by the CPU tests.
    adjoint(...)       A^T P: adjoint64's arithmetic without its rounding of the slices to fp32 (a float64 iterate stays float64)
                       and with the 0.5 cut of P as a parameter (`cut`, for the mutant that leaves P out).  Held to adjoint64.
    Operator           M p = V (A^T (P w A (V p)) + mu p) for one geometry.  P lives in the adjoint leg alone: it is a 0/1
                       diagonal, so (PA)^T W (PA) = A^T P W A, and a forward leg with or without it gives the same M.
    dot32(a, b)        <a,b> of two float32 arrays in the kernels' order (below): the bits of the device.
    cg(...)            the solve with the freeze rule; ft = float64: every operation in float64, dot products by math.fsum;
                       ft = float32: element-wise operations in float32 one rounding each, dot32, alpha and beta rounded to float32
                       from the double quotient: what the device computes, operator apart.
    init32 / q32 / step32 / dir32   one launch each on a dict of the scalar block, for the bit-equality tests.

Dot-product order (fsg_hip.h): B = clamp(ceil(n/1024), 1, 1024) workgroups of 256 threads, T = 256 B.  Group g = e // 4 belongs
to thread g % T; a thread adds the exact double products of its elements in increasing e from +0.0; the 64 lanes of a wave fold
by v[i] = v[i] + v[i ^ o], o = 32..1; the 4 waves add as ((w0 + w1) + w2) + w3; the B partials add in index order from +0.0.

Freeze rule: frozen[0] = rr[0] <= tol; iteration k: frozen[k-1] -> nothing; pq[k] = <p, M p>; !(pq[k] > 0) -> frozen, x untouched;
alpha = rr[k-1] / pq[k]; x += alpha p; r -= alpha q; rr[k] = <r,r>; rr[k] <= tol -> frozen, p untouched; beta = rr[k] / rr[k-1];
p = r + beta p.  relu is applied once to the x that is returned.

The capability case (`capability_case`): section 18's smooth phantom (util_sa_backward_cases.fit_case) seen by three orthogonal
stacks of 7 slices of 13 x 11 pixels at res 1.5 under its 1 x 3 x 3 PSF, x0 = the equalised PSF reconstruction.  Run here in
float64 (LINEAR, relu on): data residual |P(y - A x)|^2 = 4.5643 at x0 and 0.021086 after 6 iterations: far more than halved.

E_CPU: max |cg(float32) - cg(float64)| / max |cg(float64)| of x over the two general cases (psf335, psf223_vm as V) with x0 = None,
w = None, per (interp_psf, n_iter, mu); the operator in float32 sums its scatter in float64 and rounds once.  E_CPU_RR and
E_CPU_ALPHA: the same for the histories, max over the slots of the relative difference.  Measured on the CPU
(python -m tests.util_srr64 prints them), written below rounded up in the third digit with the measured value beside each.
"""
import math

import numpy as np

from tests.util_sa_adjoint_backward64 import _Geometry, _fac, _psf_value
from tests.util_sa_backward64 import CORNERS
from tests import util_sa_backward_cases as BC

F32, F64 = np.float32, np.float64


# ---- the operators ---------------------------------------------------------------------------------------------------------
def _walk(G, interp_psf, live=None):
    """Per PSF tap: (list of (flat voxel index, geometric coefficient, accepted), tap value or PSF value at the voxel).
    LINEAR: 8 corners with their trilinear weights, tap value pv (scalar); NEAREST_PSF: the rounded voxel with coefficient 1
    and the re-interpolated PSF value there (array)."""
    one = G.ft(1)
    for fx, fy, fz, pv in G.taps():
        x, y, z, acc = G.position(fx, fy, fz)
        if live is not None:
            acc = acc & live
        if interp_psf:
            xr, yr, zr, iv = G.rounded(x, y, z, acc)
            _, accp, wf, q = G.psf_cell(xr, yr, zr, acc)
            yield [(np.where(accp, iv, 0), None, accp)], _psf_value(G, wf, q), accp
        else:
            (wx, wy, wz), iv = G.cell(x, y, z, acc)
            cs = [(G.corner_index(iv, c, acc), _fac(wx, c[0], one) * _fac(wy, c[1], one) * _fac(wz, c[2], one), acc) for c in CORNERS]
            yield cs, pv, acc


def forward(transforms, vol, psf, slices_mask, slice_shape, res_slice, interp_psf, ft=F64):
    """slices = sum(coef * vol) / sum(coef) where the sum of coefficients is > 0 and inside slices_mask, else 0.  Returns
    slices and weight (n,h,w) in ft.  `vol` is taken in ft as it is (a float64 iterate is not rounded to fp32)."""
    v = np.asarray(vol).astype(ft)
    n = np.asarray(transforms).reshape(-1, 3, 4).shape[0]
    h, w = slice_shape
    G = _Geometry(transforms, psf, (n, h, w), v.shape, res_slice, ft)
    flat = v.reshape(-1)
    val, wgt = np.zeros((n, h, w), ft), np.zeros((n, h, w), ft)
    old = np.seterr(invalid="ignore", over="ignore", divide="ignore")
    try:
        for cells, pv, _ in _walk(G, interp_psf):
            for idx, coef, ok in cells:
                pw = pv if coef is None else (coef * pv).astype(ft)
                val = np.where(ok, (val + (pw * flat[idx]).astype(ft)).astype(ft), val)
                wgt = np.where(ok, (wgt + pw).astype(ft), wgt)
        sm = np.ones((n, h, w), bool) if slices_mask is None else np.asarray(slices_mask, bool).reshape(n, h, w)
        good = (wgt > 0) & sm
        out = np.where(good, val / np.where(good, wgt, 1), 0).astype(ft)
    finally:
        np.seterr(**old)
    return out, np.where(good, wgt, 0).astype(ft)


def adjoint(transforms, psf, slices, slices_mask, vol_shape, res_slice, interp_psf, ft=F64, cut=0.5):
    """A^T P without vol_mask and without equalisation: pass 1 the pixel's weight, pixels with weight < cut dropped (cut = 0:
    weight > 0 kept, the forward's own rule), pass 2 the contributions divided by the weight, summed in float64 and rounded to
    ft once.  Returns vol (D,H,W) in ft and the pixel weight."""
    sl = np.asarray(slices).astype(ft)
    n, h, w = sl.shape
    G = _Geometry(transforms, psf, (n, h, w), vol_shape, res_slice, ft)
    D, H, W = G.D, G.H, G.W
    sm = np.ones((n, h, w), bool) if slices_mask is None else np.asarray(slices_mask, bool).reshape(n, h, w)
    old = np.seterr(invalid="ignore", over="ignore", divide="ignore")
    try:
        weight = np.zeros((n, h, w), ft)
        for _, pv, ok in _walk(G, interp_psf):
            weight = np.where(ok, weight + pv, weight).astype(ft)
        live = sm & (~(weight < cut) if cut > 0 else (weight > 0))
        wsafe = np.where(live, weight, 1)
        vol = np.zeros(D * H * W, F64)
        for cells, pv, _ in _walk(G, interp_psf, live):
            pn = (pv / wsafe).astype(ft)
            for idx, coef, ok in cells:
                cw = pn if coef is None else (coef * pn).astype(ft)
                np.add.at(vol, idx[ok], (cw * sl)[ok].astype(F64))
    finally:
        np.seterr(**old)
    return vol.astype(ft).reshape(D, H, W), weight


class Operator:
    """M for one geometry.  mutant: None, "no_P" (the 0.5 cut left out: pixels with weight in (0, 0.5) stay) or "no_V_on_q"
    (V left off the result)."""

    def __init__(self, tr, psf, vol_shape, slice_shape, res, interp_psf, sm=None, V=None, w=None, mu=0.0, ft=F64, mutant=None):
        self.tr, self.psf, self.vs, self.ss, self.res, self.interp_psf = tr, psf, tuple(vol_shape), tuple(slice_shape), res, interp_psf
        self.sm, self.ft, self.mutant = sm, ft, mutant
        self.V = None if V is None else np.asarray(V, bool).reshape(self.vs)
        self.w = None if w is None else np.asarray(w).astype(ft)
        self.mu = ft(mu)
        self.cut = 0.0 if mutant == "no_P" else 0.5

    def mask(self, v):
        return v if self.V is None else np.where(self.V, v, self.ft(0))

    def A(self, v):
        return forward(self.tr, v, self.psf, self.sm, self.ss, self.res, self.interp_psf, self.ft)[0]

    def At(self, s):
        return adjoint(self.tr, self.psf, s, self.sm, self.vs, self.res, self.interp_psf, self.ft, self.cut)[0]

    def normal(self, v):
        """A^T P W A v (v already inside V)"""
        s = self.A(v)
        if self.w is not None:
            s = (s * self.w).astype(self.ft)
        return self.At(s)

    def rhs_raw(self, y):
        y = np.asarray(y).astype(self.ft)
        return self.At(y if self.w is None else (y * self.w).astype(self.ft))

    def __call__(self, p):
        p = np.asarray(p).astype(self.ft)
        t = (self.normal(self.mask(p)) + self.mu * p).astype(self.ft)
        return t if self.mutant == "no_V_on_q" else self.mask(t)

    def P(self):
        """the pixels the adjoint keeps"""
        n = np.asarray(self.tr).reshape(-1, 3, 4).shape[0]
        _, wgt = adjoint(self.tr, self.psf, np.zeros((n, *self.ss)), self.sm, self.vs, self.res, self.interp_psf, F64, self.cut)
        sm = np.ones(wgt.shape, bool) if self.sm is None else np.asarray(self.sm, bool)
        return sm & ~(wgt < 0.5)


# ---- the dot product in the kernels' order ------------------------------------------------------------------------------------
def cg_blocks(n):
    return min(max((n + 1023) // 1024, 1), 1024)


def dot32_partials(a, b):
    """the B doubles the launch stores"""
    a, b = np.asarray(a, F32).reshape(-1), np.asarray(b, F32).reshape(-1)
    n = a.size
    B = cg_blocks(n)
    T = 256 * B
    ng = (n + 3) // 4
    trips = max((ng + T - 1) // T, 1)
    prod = np.zeros(trips * T * 4, F64)
    prod[:n] = a.astype(F64) * b.astype(F64)  # exact; padding adds +0.0, which changes no sum that started from +0.0
    prod = prod.reshape(trips, T, 4)
    acc = np.zeros(T, F64)
    for t in range(trips):
        for j in range(4):
            acc = acc + prod[t, :, j]
    v = acc.reshape(B, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    wv = v[:, :, 0]
    return ((wv[:, 0] + wv[:, 1]) + wv[:, 2]) + wv[:, 3]


def fold(partials):
    s = F64(0.0)
    for x in partials:
        s = s + x
    return s


def dot32(a, b):
    return fold(dot32_partials(a, b))


def dot64(a, b):
    return math.fsum((np.asarray(a, F64).reshape(-1) * np.asarray(b, F64).reshape(-1)).tolist())


# ---- one launch each, float32 ---------------------------------------------------------------------------------------------------
def new_ws(n_iter, st=F32):
    s = n_iter + 1
    return dict(rr=np.zeros(s, F64), pq=np.zeros(s, F64), alpha=np.zeros(s, st), beta=np.zeros(s, st), frozen=np.zeros(s, np.int32),
                part_rr=None, part_pq=None, n_iter=n_iter)


def _keep(mask, v):
    return v if mask is None else np.where(np.asarray(mask, bool).reshape(v.shape), v, F32(0))


def init32(ws, b, mask=None, mu=0.0, z=None, x0=None, t0=None):
    """-> r, p, x"""
    mu = F32(mu)
    b = np.asarray(b, F32)
    a = b if z is None else (b + (mu * np.asarray(z, F32)).astype(F32)).astype(F32)
    a = _keep(mask, a)
    if x0 is not None:
        x0 = np.asarray(x0, F32)
        c = _keep(mask, (np.asarray(t0, F32) + (mu * x0).astype(F32)).astype(F32))
        a = (a - c).astype(F32)
        x = _keep(mask, x0).copy()
    else:
        x = np.zeros_like(b)
    ws["part_rr"] = dot32_partials(a, a)
    return a.copy(), a.copy(), x


def q32(ws, k, p, t, mask=None, mu=0.0, tol=0.0):
    """-> q (t itself when the launch is frozen: nothing is written)"""
    if k == 1:
        ws["rr"][0] = fold(ws["part_rr"])
        ws["frozen"][0] = ws["rr"][0] <= tol
    if ws["frozen"][k - 1]:
        return np.asarray(t, F32).copy()
    p = np.asarray(p, F32)
    q = _keep(mask, (np.asarray(t, F32) + (F32(mu) * p).astype(F32)).astype(F32))
    ws["part_pq"] = dot32_partials(p, q)
    return q


def step32(ws, k, p, q, x, r, relu=False):
    """-> x, r"""
    K = ws["n_iter"]
    last = k == K
    x, r = np.asarray(x, F32).copy(), np.asarray(r, F32).copy()
    frozen = bool(ws["frozen"][k - 1])
    pq = F64(0.0)
    if not frozen:
        pq = fold(ws["part_pq"])
        frozen = not (pq > 0)
    with np.errstate(all="ignore"):
        alpha = F32(0) if frozen else F32(ws["rr"][k - 1] / pq)
    ws["pq"][k], ws["alpha"][k] = pq, alpha
    if frozen:
        if last and relu:
            x = np.where(x > 0, x, F32(0))
        return x, r
    xn = (x + (alpha * np.asarray(p, F32)).astype(F32)).astype(F32)
    if last and relu:
        xn = np.where(xn > 0, xn, F32(0))
    rn = (r - (alpha * np.asarray(q, F32)).astype(F32)).astype(F32)
    ws["part_rr"] = dot32_partials(rn, rn)
    return xn, (r if last else rn)


def dir32(ws, k, r, p, tol=0.0):
    """-> p"""
    K = ws["n_iter"]
    p = np.asarray(p, F32).copy()
    rr_old = ws["rr"][k - 1]
    frozen = bool(ws["frozen"][k - 1]) or not (ws["pq"][k] > 0)
    rr, beta = rr_old, F32(0)
    if not frozen:
        rr = fold(ws["part_rr"])
        with np.errstate(all="ignore"):
            beta = F32(rr / rr_old)
        frozen = bool(rr <= tol)
    ws["rr"][k], ws["beta"][k], ws["frozen"][k] = rr, beta, frozen
    if frozen or k == K:
        return p
    return (np.asarray(r, F32) + (beta * p).astype(F32)).astype(F32)


# ---- the solve ------------------------------------------------------------------------------------------------------------------
def cg(op, y, n_iter, x0=None, z=None, tol=0.0, relu=False, ft=F64, mutant=None, b=None):
    """n_iter iterations of CG on M x = V(b + mu z), b = A^T P W y (or given).  mutant "beta_swapped": beta = rr[k-1] / rr[k].
    Returns x (ft) and the histories (dict as new_ws)."""
    assert op.ft is ft and (mutant is None or ft is F64)  # the mutants run in float64
    shape = op.vs
    b = op.rhs_raw(y) if b is None else np.asarray(b).astype(ft)
    if ft is F32:
        ws = new_ws(n_iter)
        t0 = None if x0 is None else op.normal(op.mask(np.asarray(x0, F32)))
        r, p, x = init32(ws, b, op.V, op.mu, z, x0, t0)
        for k in range(1, n_iter + 1):
            t = op.normal(p) if not (k > 1 and ws["frozen"][k - 1]) else np.zeros(shape, F32)
            q = q32(ws, k, p, t, op.V, op.mu, tol)
            x, r = step32(ws, k, p, q, x, r, relu)
            p = dir32(ws, k, r, p, tol)
        return x, ws
    ws = new_ws(n_iter, F64)
    mu = F64(op.mu)
    rhs = op.mask(b if z is None else b + mu * np.asarray(z, F64))
    if x0 is not None:
        x = op.mask(np.asarray(x0, F64))
        r = rhs - op.mask(op.normal(x) + mu * np.asarray(x0, F64))
    else:
        x, r = np.zeros(shape, F64), rhs
    p = r.copy()
    ws["rr"][0] = dot64(r, r)
    ws["frozen"][0] = ws["rr"][0] <= tol
    for k in range(1, n_iter + 1):
        ws["rr"][k], ws["frozen"][k] = ws["rr"][k - 1], 1
        if ws["frozen"][k - 1]:
            continue
        q = op(p)
        ws["pq"][k] = pq = dot64(p, q)
        if not (pq > 0):
            continue
        ws["alpha"][k] = alpha = ws["rr"][k - 1] / pq
        x = x + alpha * p
        r = r - alpha * q
        ws["rr"][k] = rr = dot64(r, r)
        beta = (ws["rr"][k - 1] / rr) if mutant == "beta_swapped" else (rr / ws["rr"][k - 1])
        ws["beta"][k] = beta
        ws["frozen"][k] = rr <= tol
        if ws["frozen"][k]:
            continue
        p = r + beta * p
    return (np.maximum(x, 0) if relu else x), ws


# ---- cases ----------------------------------------------------------------------------------------------------------------------
MIN_KEPT = 0.30
_CASES = {}


def solver_case(name, interp_psf):
    """A general case of util_sa_backward_cases with slices y = A(vol) (float64, rounded to fp32), and ONE slices_mask for the whole solve: the
    case's own (every decision distance > 2e-3) minus the pixels whose float64 weight is within 1e-3 of the 0.5 cut.  The `vm` of
    psf223_vm is the solver's outer V only."""
    key = (name, interp_psf)
    if key not in _CASES:
        c = BC.general_case(name, interp_psf)
        ss = c["g"].shape[1:]
        _, wgt = adjoint(c["tr"], c["psf"], np.zeros_like(c["g"]), None, BC.VS, c["res"], interp_psf, F64)
        sm = c["sm"] & ~(np.abs(wgt - 0.5) <= 1e-3)
        y = forward(c["tr"], c["vol"], c["psf"], sm, ss, c["res"], interp_psf, F64)[0].astype(F32)
        _CASES[key] = dict(tr=c["tr"], psf=c["psf"], res=c["res"], ss=ss, sm=sm, sm_own=c["sm"], V=c["vm"], y=y, vol=c["vol"],
                           kept=float(sm.mean()), kept_before=float(c["sm"].mean()))
    return _CASES[key]


def case_operator(case, interp_psf, mu=0.0, ft=F64, w=None, use_V=True, mutant=None):
    return Operator(case["tr"], case["psf"], BC.VS, case["ss"], case["res"], interp_psf, sm=case["sm"],
                    V=case["V"] if use_V else None, w=w, mu=mu, ft=ft, mutant=mutant)


SOLVER_CASES = ("psf335", "psf223_vm")
N_ITERS, MUS = (1, 3, 6), (0.0, 0.5)

# (interp_psf, n_iter, mu): bound, measured beside it
E_CPU = {
    (False, 1, 0.0): 2.12e-06,  # 2.112e-06
    (False, 3, 0.0): 3.34e-06,  # 3.332e-06
    (False, 6, 0.0): 2.01e-06,  # 2.002e-06
    (False, 1, 0.5): 2.38e-06,  # 2.371e-06
    (False, 3, 0.5): 2.88e-06,  # 2.877e-06
    (False, 6, 0.5): 2.85e-06,  # 2.846e-06
    (True, 1, 0.0): 2.40e-07,  # 2.396e-07
    (True, 3, 0.0): 5.44e-07,  # 5.434e-07
    (True, 6, 0.0): 5.69e-07,  # 5.686e-07
    (True, 1, 0.5): 2.84e-07,  # 2.839e-07
    (True, 3, 0.5): 4.30e-07,  # 4.294e-07
    (True, 6, 0.5): 4.83e-07,  # 4.826e-07
}
E_CPU_RR = {
    (False, 1, 0.0): 5.36e-07,  # 5.360e-07
    (False, 3, 0.0): 5.36e-07,  # 5.360e-07
    (False, 6, 0.0): 5.36e-07,  # 5.360e-07
    (False, 1, 0.5): 5.36e-07,  # 5.360e-07
    (False, 3, 0.5): 5.36e-07,  # 5.360e-07
    (False, 6, 0.5): 5.36e-07,  # 5.360e-07
    (True, 1, 0.0): 2.39e-08,  # 2.389e-08
    (True, 3, 0.0): 2.39e-08,  # 2.389e-08
    (True, 6, 0.0): 2.39e-08,  # 2.389e-08
    (True, 1, 0.5): 2.39e-08,  # 2.389e-08
    (True, 3, 0.5): 2.39e-08,  # 2.389e-08
    (True, 6, 0.5): 2.39e-08,  # 2.389e-08
}
E_CPU_ALPHA = {
    (False, 1, 0.0): 7.55e-07,  # 7.540e-07
    (False, 3, 0.0): 7.30e-07,  # 7.292e-07
    (False, 6, 0.0): 9.49e-07,  # 9.482e-07
    (False, 1, 0.5): 2.70e-07,  # 2.695e-07
    (False, 3, 0.5): 2.70e-07,  # 2.695e-07
    (False, 6, 0.5): 2.47e-07,  # 2.464e-07
    (True, 1, 0.0): 3.64e-08,  # 3.636e-08
    (True, 3, 0.0): 5.68e-08,  # 5.680e-08
    (True, 6, 0.0): 1.09e-07,  # 1.082e-07
    (True, 1, 0.5): 2.56e-08,  # 2.558e-08
    (True, 3, 0.5): 5.43e-08,  # 5.424e-08
    (True, 6, 0.5): 9.96e-08,  # 9.954e-08
}


def measure_e_cpu():
    out = {}
    for interp_psf in (False, True):
        for mu in MUS:
            worst = {k: [0.0, 0.0, 0.0] for k in N_ITERS}
            for name in SOLVER_CASES:
                c = solver_case(name, interp_psf)
                o64, o32 = case_operator(c, interp_psf, mu, F64), case_operator(c, interp_psf, mu, F32)
                for k in N_ITERS:
                    x64, h64 = cg(o64, c["y"], k, ft=F64)
                    x32, h32 = cg(o32, c["y"], k, ft=F32)
                    e = np.abs(x32.astype(F64) - x64).max() / np.abs(x64).max()
                    err = np.abs(h32["rr"] - h64["rr"]).max() / np.abs(h64["rr"]).max()
                    ea = np.abs(h32["alpha"][1:].astype(F64) - h64["alpha"][1:].astype(F64)).max() / np.abs(h64["alpha"][1:]).max()
                    worst[k] = [max(a, b) for a, b in zip(worst[k], (e, err, ea))]
            for k in N_ITERS:
                out[(interp_psf, k, mu)] = worst[k]
    return out


def capability_case():
    """fit_case's phantom under three orthogonal 7-slice stacks (axial, coronal, sagittal), the slices y = A(phantom) in float64
    rounded to fp32, and x0 = the equalised PSF reconstruction of them."""
    f = BC.fit_case()
    n, ss, res = 7, f["ss"], f["res"]
    rots = (np.eye(3), np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]]), np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]]))
    tr = np.zeros((3 * n, 3, 4), F32)
    for s, R in enumerate(rots):
        for i in range(n):
            tr[s * n + i, :, :3] = R
            tr[s * n + i, :, 3] = (0.0, 0.0, (i - (n - 1) / 2) * 2.5)
    y = forward(tr, f["vol"], f["psf"], None, ss, res, False, F64)[0].astype(F32)
    return dict(tr=tr, psf=f["psf"], res=res, ss=ss, y=y, vol=f["vol"])


def equalised_x0(case, interp_psf=False):
    from tests.util_sa_adjoint_backward64 import adjoint64

    return adjoint64(case["tr"], case["psf"], case["y"], None, None, BC.VS, case["res"], interp_psf, True)["vol"]


def data_residual(op, y, x):
    d = np.where(op.P(), np.asarray(y, F64) - op.A(np.asarray(x, F64)), 0.0)
    return float((d * d).sum())


if __name__ == "__main__":
    for key, (e, err, ea) in measure_e_cpu().items():
        print(key, f"x {e:.3e}  rr {err:.3e}  alpha {ea:.3e}")
    for name in SOLVER_CASES:
        for ip in (False, True):
            c = solver_case(name, ip)
            print(name, ip, "kept", c["kept"], "before the 0.5 band", c["kept_before"])
    cap = capability_case()
    op = Operator(cap["tr"], cap["psf"], BC.VS, cap["ss"], cap["res"], False)
    x0 = equalised_x0(cap)
    x6, _ = cg(op, cap["y"], 6, x0=x0, relu=True)
    print("capability: residual x0", data_residual(op, cap["y"], x0), "after 6", data_residual(op, cap["y"], x6))
