"""CPU restatement of the first-order regulariser of `svort.srr` (the rule is in include/fsg_hip.h,
fsg_tk1_apply_f32).  Test infrastructure, numpy only; `ft` is the type every operation is done in, as in tests/util_srr64.

    apply(p, t, lam, ...)   out = t + lam * L p, vectorised, in the header's operation order.  ft = float32 is what the device
                            computes, bit for bit: only + - * /, abs and a comparison, one rounding each.
    apply_loop(...)         the same rule as a literal triple loop over the voxels, written independently of `apply`.
    dense(shape, ...)       L as a matrix, from one application per voxel.
    edges(shape, mask)      the participating edges (i, j), i < j, as flat indices.
    RegOperator             util_srr64.Operator with M + lam L: `normal` is followed by `apply`, as svort.srr follows
                            A^T P W A by kernels.tk1_apply.
    srr(...)                the outer loop of svort.srr around util_srr64.cg: n_outer complete solves, round o > 0 started from
                            and guided by the x of the round before, the relu in the last round only.

Which edges take part: both ends inside the volume and inside the mask.  Weight: 1, or with a guide g and delta
a = |fl(g_i - g_j)|, c = 1 if a <= delta else fl(delta / a).  Per voxel: acc = +0; over x-, x+, y-, y+, z-, z+ (x the last axis)
for the neighbours that take part d = fl(p_i - p_j), d = fl(c * d) when guided, acc = fl(acc + d); out = fl(t + fl(lam * acc)),
and out = t outside the mask.

Mutants (`mutant=`), each caught by a stated check of tests/test_tk1_64_reference.py:
    "mask_one_end"   the mask tested at the voxel's own end of an edge only      -> L is not symmetric
    "guide_one_end"  a = |g_i| in place of |g_i - g_j|                          -> L is not symmetric
    "wrap_x"         the x neighbours taken from the flat array, across row ends -> differs from the literal loop on (1,2,3)

E_CPU_TK1: max |srr(float32) - srr(float64)| / max |srr(float64)| of x over the two general cases of util_srr64 (x0 = None, mu = 0,
relu on, N_ITER iterations per round, LAM) per (interp_psf, huber): huber False = plain TK1, True = HUBER_DELTA with N_OUTER
rounds.  CAP_*: the float64 RMS errors of the two capability cases against their phantoms.  All measured on the CPU
(python -m tests.util_tk1_64 prints them), written below rounded up in the third digit with the measured value beside each.
"""
import numpy as np

from tests import util_sa_backward_cases as BC
from tests import util_srr64 as U

F32, F64 = np.float32, np.float64
DIRECTIONS = ((2, -1), (2, 1), (1, -1), (1, 1), (0, -1), (0, 1))  # x-, x+, y-, y+, z-, z+ as (axis, step)


def _shift(a, axis, step, fill):
    """b[i] = a[i + step along axis] where that is inside, else fill"""
    out = np.full(a.shape, fill, a.dtype)
    src, dst = [slice(None)] * 3, [slice(None)] * 3
    src[axis], dst[axis] = (slice(None, -1), slice(1, None)) if step < 0 else (slice(1, None), slice(None, -1))
    out[tuple(dst)] = a[tuple(src)]
    return out


def _wrapped(a, step, fill):
    """the mutant's x neighbour: element i + step of the flat array"""
    flat = np.full(a.size, fill, a.dtype)
    if step < 0:
        flat[1:] = a.reshape(-1)[:-1]
    else:
        flat[:-1] = a.reshape(-1)[1:]
    return flat.reshape(a.shape)


def apply(p, t, lam, mask=None, guide=None, delta=None, ft=F64, mutant=None):
    p, t = np.asarray(p).astype(ft), np.asarray(t).astype(ft)
    assert p.ndim == 3 and t.shape == p.shape
    V = np.ones(p.shape, bool) if mask is None else np.asarray(mask, bool).reshape(p.shape)
    g = None if guide is None else np.asarray(guide).astype(ft)
    lam = ft(lam)
    acc = np.zeros(p.shape, ft)
    old = np.seterr(all="ignore")
    try:
        for axis, step in DIRECTIONS:
            nb = (lambda a, fill: _wrapped(a, step, fill)) if mutant == "wrap_x" and axis == 2 else (lambda a, fill: _shift(a, axis, step, fill))
            on = nb(np.ones(p.shape, bool), False) & V
            if mutant != "mask_one_end":
                on = on & nb(V, False)
            d = (p - nb(p, ft(0))).astype(ft)
            if g is not None:
                a = np.abs(g if mutant == "guide_one_end" else (g - nb(g, ft(0))).astype(ft))
                c = np.where(a <= ft(delta), ft(1), (ft(delta) / np.where(a <= ft(delta), ft(1), a)).astype(ft))
                d = (c * d).astype(ft)
            acc = np.where(on, (acc + d).astype(ft), acc)
        out = (t + (lam * acc).astype(ft)).astype(ft)
    finally:
        np.seterr(**old)
    return np.where(V, out, t)


def apply_loop(p, t, lam, mask=None, guide=None, delta=None, ft=F64):
    p, t = np.asarray(p).astype(ft), np.asarray(t).astype(ft)
    D, H, W = p.shape
    out = t.copy()
    for z in range(D):
        for y in range(H):
            for x in range(W):
                if mask is not None and not mask[z][y][x]:
                    continue
                acc = ft(0)
                for zz, yy, xx in ((z, y, x - 1), (z, y, x + 1), (z, y - 1, x), (z, y + 1, x), (z - 1, y, x), (z + 1, y, x)):
                    if not (0 <= zz < D and 0 <= yy < H and 0 <= xx < W):
                        continue
                    if mask is not None and not mask[zz][yy][xx]:
                        continue
                    d = ft(p[z, y, x] - p[zz, yy, xx])
                    if guide is not None:
                        a = abs(ft(ft(guide[z][y][x]) - ft(guide[zz][yy][xx])))
                        if not a <= ft(delta):
                            d = ft(ft(ft(delta) / a) * d)
                    acc = ft(acc + d)
                out[z, y, x] = ft(t[z, y, x] + ft(ft(lam) * acc))
    return out


def dense(shape, mask=None, guide=None, delta=None, ft=F64, mutant=None):
    """L (lam = 1, t = 0), column j from the application to the j-th unit vector"""
    n = int(np.prod(shape))
    L = np.zeros((n, n), ft)
    zero = np.zeros(shape, ft)
    for j in range(n):
        e = np.zeros(n, ft)
        e[j] = 1
        L[:, j] = apply(e.reshape(shape), zero, 1.0, mask, guide, delta, ft, mutant).reshape(-1)
    return L


def edges(shape, mask=None):
    D, H, W = shape
    V = np.ones(shape, bool) if mask is None else np.asarray(mask, bool).reshape(shape)
    idx = np.arange(D * H * W).reshape(shape)
    out = []
    for axis in (2, 1, 0):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(None, -1), slice(1, None)
        ok = V[tuple(a)] & V[tuple(b)]
        out += list(zip(idx[tuple(a)][ok].tolist(), idx[tuple(b)][ok].tolist()))
    return out


class RegOperator(U.Operator):
    """M + lam L_g: util_srr64.Operator whose `normal` is followed by `apply` (lam == 0: nothing is added, not even a zero)"""

    def __init__(self, *args, lam=0.0, guide=None, delta=None, **kw):
        super().__init__(*args, **kw)
        self.lam, self.guide, self.delta = lam, guide, delta

    def normal(self, v):
        t = super().normal(v)
        if self.lam > 0:
            t = apply(np.asarray(v).astype(self.ft), t, self.lam, self.V, self.guide, self.delta, self.ft)
        return t


def srr(make_op, y, n_iter, huber_delta=None, n_outer=1, guide=None, x0=None, z=None, relu=True, ft=F64):
    """make_op(guide, delta) -> the round's RegOperator.  Returns x and the list of the rounds' histories."""
    assert n_outer >= 1 and (huber_delta is not None or (n_outer == 1 and guide is None))
    x, g, hist = x0, guide, []
    for o in range(n_outer):
        op = make_op(g, None if g is None else huber_delta)
        x, h = U.cg(op, y, n_iter, x0=x, z=z, relu=relu and o == n_outer - 1, ft=ft)
        hist.append(h)
        g = x
    return x, hist


# ---- the solver cases and their constants ---------------------------------------------------------------------------------------
LAM, HUBER_DELTA, N_OUTER, N_ITER = 0.1, 0.05, 2, 3


def case_maker(c, interp_psf, ft, lam=LAM):
    return lambda g, delta: RegOperator(c["tr"], c["psf"], BC.VS, c["ss"], c["res"], interp_psf, sm=c["sm"], V=c["V"], ft=ft,
                                        lam=lam, guide=g, delta=delta)


def solve_case(name, interp_psf, huber, ft):
    c = U.solver_case(name, interp_psf)
    kw = dict(huber_delta=HUBER_DELTA, n_outer=N_OUTER) if huber else {}
    return srr(case_maker(c, interp_psf, ft), c["y"], N_ITER, ft=ft, **kw)[0]


# (interp_psf, huber): bound, measured beside it
E_CPU_TK1 = {
    (False, False): 2.22e-06,  # 2.215e-06
    (False, True): 1.96e-06,  # 1.955e-06
    (True, False): 3.12e-07,  # 3.111e-07
    (True, True): 3.49e-07,  # 3.487e-07
}


def measure_e_cpu():
    out = {}
    for interp_psf in (False, True):
        for huber in (False, True):
            worst = 0.0
            for name in U.SOLVER_CASES:
                x64, x32 = solve_case(name, interp_psf, huber, F64), solve_case(name, interp_psf, huber, F32)
                worst = max(worst, float(np.abs(x32.astype(F64) - x64).max() / np.abs(x64).max()))
            out[(interp_psf, huber)] = worst
    return out


# ---- the capability cases -----------------------------------------------------------------------------------------------------------
def piecewise_phantom():
    """1.0 inside the ellipsoid r2 < 1, + 0.8 where r2 < 0.35, - 0.6 in an off-centre box; voxel index coordinates of BC.VS"""
    s = np.array(BC.VS, F64)
    c = (s - 1) / 2
    z, y, x = np.meshgrid(*(np.arange(int(n), dtype=F64) for n in s), indexing="ij")
    r2 = ((z - c[0]) / (0.38 * s[0])) ** 2 + ((y - c[1]) / (0.38 * s[1])) ** 2 + ((x - c[2]) / (0.38 * s[2])) ** 2
    vol = np.where(r2 < 1, 1.0, 0.0) + np.where(r2 < 0.35, 0.8, 0.0)
    box = (np.abs(z - c[0] - 2) < 2.5) & (np.abs(y - c[1] + 2) < 3) & (np.abs(x - c[2]) < 2.5)
    return (vol - np.where(box, 0.6, 0.0)).astype(F32)


_CAP = {}


def capability_cases():
    """case 1: util_srr64.capability_case() (the smooth phantom); case 2: the same geometry seeing piecewise_phantom()"""
    if not _CAP:
        smooth = U.capability_case()
        vol = piecewise_phantom()
        y = U.forward(smooth["tr"], vol, smooth["psf"], None, smooth["ss"], smooth["res"], False, F64)[0].astype(F32)
        _CAP.update(smooth=smooth, piecewise=dict(smooth, vol=vol, y=y))
    return _CAP


def cap_maker(c, lam, ft=F64):
    return lambda g, delta: RegOperator(c["tr"], c["psf"], BC.VS, c["ss"], c["res"], False, ft=ft, lam=lam, guide=g, delta=delta)


def rms(x, vol):
    d = np.asarray(x, F64).reshape(-1) - np.asarray(vol, F64).reshape(-1)
    return float(np.sqrt((d * d).mean()))


# the solves of the capability test: name -> (case, lam, n_iter, huber_delta, n_outer)
CAP_RUNS = {
    "smooth_tk1": ("smooth", 0.1, 6, None, 1),
    "piecewise_none": ("piecewise", 0.0, 24, None, 1),
    "piecewise_tk1": ("piecewise", 0.1, 24, None, 1),
    "piecewise_huber": ("piecewise", 0.1, 6, 0.05, 4),
}
# float64 RMS error against the phantom: rounded up in the third digit, measured beside it
CAP_RMS = {
    "smooth_tk1": 0.0404,  # 0.040371
    "piecewise_none": 0.2034,  # 0.203361
    "piecewise_tk1": 0.1675,  # 0.167463
    "piecewise_huber": 0.0942,  # 0.094176
}


def cap_run(name, ft=F64):
    case, lam, n_iter, delta, n_outer = CAP_RUNS[name]
    c = capability_cases()[case]
    x, _ = srr(cap_maker(c, lam, ft), c["y"], n_iter, huber_delta=delta, n_outer=n_outer, relu=True, ft=ft)
    return rms(x, c["vol"])


if __name__ == "__main__":
    for key, e in measure_e_cpu().items():
        print(key, f"{e:.3e}")
    for name in CAP_RUNS:
        print(name, f"{cap_run(name):.4f}")
