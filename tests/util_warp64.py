"""References of the warp family (csrc/fsg_warp_lean.hip, csrc/fsg_deform.hip: K2, K3, K4, K5) for the tests (not a test module):
plain numpy restatements of the kernels' operations.  Every reference comes twice: `*32` in the kernels' float32 operation order
(numpy's float32 arithmetic is IEEE, the library is built without FMA contraction: a BIT-FOR-BIT reference), `*64` from the same
float32 inputs with all arithmetic in float64.

  Spec                   host description of one deformation: what kernels.DeformSpec uploads
  positions32 / 64       fsg_position: (i - cen) + the coarse field interpolated x, then y, then z through the table entries (each
                         step  w_lo * a + w_hi * b, two rounded products and a rounded sum: util_zoom64.zoom32 on the three
                         channels), the affine rows ((A0*px + A1*py) + A2*pz) + c2, the clamps to [0, n-1] (x < 0 -> 0: -0.0 stays)
  position_bound         elementwise bound on |positions32 - positions64|: (sum of the magnitudes of every term) x (roundings on
                         the longest chain) x 2^-24 x 1.01, like util_resample64.error_bound
  minmax32, margins      the six extrema as order keys (fsg_f2key: -0.0 < +0.0); floor(min) and 1 + ceil(max)
  rows32                 the per-(i, j) coarse rows of fsg_deform_rows_f32: x blend then y blend, 3 * f2 displacement values
                         (channel-major) and b2 bias values
  linear32 / 64          sample_linear at positions from which the margin is already subtracted: valid iff every coordinate is in
                         (0, n-1] (STRICT > 0), upper neighbour clamped onto the base, blend x, then y, then z, flip = reversed
                         axis-0 index.  The source is NOT cropped by the margin (the reference implementation's behaviour).
  linear32(lean=True)    the lean kernel's reading of the same operation: no index is clamped, the source is flat memory in which
                         an element outside the volume reads +0.0; z on the last column reads the pair one to the left with
                         weights (0, 1).  Equal in value to linear32 for finite sources; the sign of a zero can differ, and only
                         at outputs with a coordinate exactly on the last plane, row or column (on_upper_limit).
  nearest                round half to even, index clamp, flip
  epilogue64             300 * (v / 300) ** gamma when gamma > 0, then * exp(zoomed bias), in float64
"""
from collections import namedtuple

import numpy as np

from tests import util_zoom64 as Z
from tests.util_resample64 import U32

F = np.float32
Spec = namedtuple("Spec", "shape A cen c2 field tabs")


def make_spec(shape, A, cen, c2, field=None, tabs=None):
    """Everything as the float32 values the library receives."""
    shape = tuple(int(v) for v in shape)
    A = np.asarray(A, dtype=F).reshape(3, 3)
    if field is not None:
        field = np.ascontiguousarray(field, dtype=F)
        assert field.ndim == 4 and field.shape[3] == 3 and tuple(len(t) for t in tabs) == shape
    return Spec(shape, A, np.asarray(cen, dtype=F), np.asarray(c2, dtype=F), field, tabs)


def _grid(shape, dt):
    return [np.arange(n, dtype=dt).reshape([-1 if a == b else 1 for b in range(3)]) for a, n in enumerate(shape)]


def _clamp(t, n):
    t = np.where(t < 0, t.dtype.type(0), t)  # -0.0 < 0 is false: it stays
    return np.where(t > n - 1, t.dtype.type(n - 1), t)


def positions32(spec):
    g = _grid(spec.shape, F)
    p = [np.broadcast_to(g[a] - spec.cen[a], spec.shape) for a in range(3)]
    if spec.field is not None:
        d = Z.zoom32(spec.field, spec.tabs)
        p = [p[a] + d[..., a] for a in range(3)]
    out = []
    for r in range(3):
        A = spec.A[r]
        t = A[0] * p[0] + A[1] * p[1] + A[2] * p[2] + spec.c2[r]
        assert t.dtype == F
        out.append(_clamp(t, spec.shape[r]))
    return out


def positions64(spec):
    g = _grid(spec.shape, np.float64)
    p = [np.broadcast_to(g[a] - np.float64(spec.cen[a]), spec.shape) for a in range(3)]
    if spec.field is not None:
        d = Z.zoom64(spec.field, spec.tabs)
        p = [p[a] + d[..., a] for a in range(3)]
    out = []
    for r in range(3):
        A = spec.A[r].astype(np.float64)
        t = A[0] * p[0] + A[1] * p[1] + A[2] * p[2] + np.float64(spec.c2[r])
        out.append(_clamp(t, spec.shape[r]))
    return out


def position_roundings(spec):
    """Roundings on the longest chain of one coordinate: i - cen (1), the product with A (1), three sums (3); with a field its three
    two-term blends (2 each, as util_resample64.error_bound counts them) and its addition (1)."""
    return 5 + (7 if spec.field is not None else 0)


def position_bound(spec):
    """[bx, by, bz]: |positions32 - positions64| <= bound.  The clamps are 1-Lipschitz and exact, so the bound of the unclamped
    coordinate holds for the clamped one."""
    g = _grid(spec.shape, np.float64)
    mag = [np.broadcast_to(np.abs(g[a]) + abs(np.float64(spec.cen[a])), spec.shape) for a in range(3)]
    if spec.field is not None:
        d = Z.zoom64(np.abs(spec.field), spec.tabs)
        mag = [mag[a] + d[..., a] for a in range(3)]
    out = []
    for r in range(3):
        A = np.abs(spec.A[r].astype(np.float64))
        m = A[0] * mag[0] + A[1] * mag[1] + A[2] * mag[2] + abs(np.float64(spec.c2[r]))
        out.append(1.01 * position_roundings(spec) * U32 * m)
    return out


def minmax32(pos):
    """Six order keys: min x, y, z, max x, y, z."""
    k = [Z.f2key(p) for p in pos]
    return [int(v.min()) for v in k] + [int(v.max()) for v in k]


def margins(keys):
    v = Z.key2f(np.asarray(keys, dtype=np.int32))
    return [int(np.floor(t)) for t in v[:3]] + [int(1 + np.ceil(t)) for t in v[3:]]


def subtract_margins(pos, keys):
    """pos - floor(min) per axis as load_margins has it: the floor of the minimum's key, so a minimum of -0.0 subtracts -0.0 (and
    turns a coordinate of -0.0 into +0.0)."""
    lo = np.floor(Z.key2f(np.asarray(keys[:3], dtype=np.int32)))
    return [p - p.dtype.type(lo[a]) for a, p in enumerate(pos)]


def rows32(spec, bias=None, bias_tabs=None):
    """(n0, n1, need): need = 3 * f2 (+ b2)."""
    parts = []
    if spec.field is not None:
        y = Z._lerp_axis32(Z._lerp_axis32(spec.field, 0, spec.tabs[0]), 1, spec.tabs[1])  # (n0, n1, f2, 3)
        parts.append(np.moveaxis(y, 3, 2).reshape(y.shape[0], y.shape[1], -1))            # channel-major
    if bias is not None:
        parts.append(Z._lerp_axis32(Z._lerp_axis32(np.asarray(bias, dtype=F), 0, bias_tabs[0]), 1, bias_tabs[1]))
    r = np.concatenate(parts, axis=2)
    assert r.dtype == F
    return r


def on_upper_limit(shape, pos):
    """Outputs with a coordinate exactly on the last plane, row or column of the source."""
    return (pos[0] == shape[0] - 1) | (pos[1] == shape[1] - 1) | (pos[2] == shape[2] - 1)


def _linear(src, pos, flip, dt, lean):
    n = src.shape
    x = [np.asarray(p) for p in pos]
    ok = np.ones(x[0].shape, bool)
    for a in range(3):
        ok &= (x[a] > 0) & (x[a] <= n[a] - 1)
    f = [np.floor(p) for p in x]
    if lean:
        assert n[2] >= 2
        f[2] = np.minimum(f[2], x[2].dtype.type(n[2] - 2))
    b = [(x[a] - f[a]).astype(dt) for a in range(3)]
    w = [dt(1) - t for t in b]
    i0 = [np.clip(f[a].astype(np.int64), 0, n[a] - 1) for a in range(3)]
    flat = np.concatenate([src.ravel().astype(dt), np.zeros(1, dt)])  # [nvox]: what an out-of-range read returns
    nvox, sy, sx = src.size, n[2], n[1] * n[2]
    sxs, base = (-sx, (n[0] - 1) * sx) if flip else (sx, 0)

    def corner(dx, dy, dz):
        if lean:
            e = base + (i0[0] + dx) * sxs + (i0[1] + dy) * sy + i0[2] + dz
            return flat[np.where((e >= 0) & (e < nvox), e, nvox)]
        xi, yi, zi = (np.minimum(i0[a] + d, n[a] - 1) for a, d in enumerate((dx, dy, dz)))
        return flat[base + xi * sxs + yi * sy + zi]

    with np.errstate(all="ignore"):
        c00 = corner(0, 0, 0) * w[0] + corner(1, 0, 0) * b[0]
        c01 = corner(0, 0, 1) * w[0] + corner(1, 0, 1) * b[0]
        c10 = corner(0, 1, 0) * w[0] + corner(1, 1, 0) * b[0]
        c11 = corner(0, 1, 1) * w[0] + corner(1, 1, 1) * b[0]
        c0 = c00 * w[1] + c10 * b[1]
        c1 = c01 * w[1] + c11 * b[1]
        v = c0 * w[2] + c1 * b[2]
    assert v.dtype == dt
    return np.where(ok, v, dt(0))


def linear32(src, pos, flip, lean=False):
    assert src.dtype == F and all(p.dtype == F for p in pos)
    return _linear(src, pos, flip, F, lean)


def linear64(src, pos, flip):
    return _linear(src, pos, flip, np.float64, False)


def linear_magnitude(src, pos, flip):
    """The blend of |src| in float64: the magnitude every rounding of the blend is relative to."""
    return _linear(np.abs(src), pos, flip, np.float64, False)


LINEAR_ROUNDINGS = 10  # 1 - b (1), then three levels of two rounded products and a rounded sum (3 each)


def nearest(src, pos, flip):
    n = src.shape
    i = [np.clip(np.rint(p).astype(np.int64), 0, n[a] - 1) for a, p in enumerate(pos)]  # rint: round half to even
    if flip:
        i[0] = n[0] - 1 - i[0]
    return src[i[0], i[1], i[2]]


def near_tie_or_zero(pos64, bound, pos32):
    """Where a float32 position within `bound` of the float64 one may round to another voxel, or fall on the other side of the
    strict > 0 rule: within the bound of k + 0.5 on any axis, or within the bound of 0 unless both positions are the exact 0 the
    lower clamp writes."""
    out = np.zeros(pos64[0].shape, bool)
    for p, b, q in zip(pos64, bound, pos32):
        frac = p - np.floor(p)
        out |= (np.abs(frac - 0.5) <= b) | ((p <= b) & ((p > 0) | (q > 0)))
    return out


def epilogue64(v, gamma=None, bias=None, bias_tabs=None):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        if gamma is not None and F(gamma) > 0:
            v = 300.0 * (v / 300.0) ** np.float64(F(gamma))
        if bias is not None:
            v = v * np.exp(Z.zoom64(np.asarray(bias, dtype=F), bias_tabs))
    return v
