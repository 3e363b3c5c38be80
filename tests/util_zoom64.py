"""References of the zoom family (csrc/fsg_zoom.hip: K5b, K7, K9a, K9b, K10) for the tests (not a test module): plain numpy
restatements of what include/fsg_hip.h promises for fsg_zoom3d_f32, fsg_zoom3d_minmax*_f32 and fsg_zoom3d_normalise*_f32.

  zoom32       the operation in float32 in the promised order: x, then y, then z, each step  w_lo * a + w_hi * b  with a
               separately rounded product and a separately rounded sum; an output with lo < 0 on any axis is +0.0.  numpy's
               float32 arithmetic is IEEE and the library is built with -ffp-contract=off, so this is a BIT-FOR-BIT reference.
               The zoom is separable and every step is elementwise, so blending whole axes in turn performs, per output, exactly
               the operations of fsg_tab_interp: the x blend of the four corners, then the two y blends, then z.
  zoom64       the same in float64 (util_resample64.lerp_axis64 per axis); a float32 result lies within
               util_resample64.error_bound(x, (None,) * 3, tabs) of it: the 6-term rounding bound of three two-term lerps.
  minmax32     min and max of a float32 array as the order keys of fsg_f2key (-0.0 orders below +0.0); NaN is ignored, an
               all-NaN (or empty) input gives the identities {key(+inf), key(-inf)} (what fsg_minmax_init writes).
  normalise32  t = y / mx; mode 0: t; mode 1: q = mn / mx, t * 0 when q == 1, else (t - q) / (1 - q) -- float32, IEEE division.
               The kernels' `den == 1` shortcut is not part of it: x / 1.0f == x exactly.
"""
import numpy as np

from tests.util_resample64 import error_bound, lerp_axis64

F = np.float32
KEY_MIN_IDENTITY = 0x7F800000       # key(+inf)
KEY_MAX_IDENTITY = -2139095041      # key(-inf) = 0xFF800000 ^ 0x7FFFFFFF as int32


def _lerp_axis32(y, axis, tab):
    lo = tab["lo"].astype(np.int64)
    hi = tab["hi"].astype(np.int64)
    ok = lo >= 0
    shape = [1] * y.ndim
    shape[axis] = len(tab)
    wl = tab["w_lo"].astype(F).reshape(shape)
    wh = tab["w_hi"].astype(F).reshape(shape)
    a = np.take(y, np.where(ok, lo, 0), axis=axis)
    b = np.take(y, np.where(ok, hi, 0), axis=axis)
    p, q = wl * a, wh * b  # two float32 products, each rounded
    assert p.dtype == F and q.dtype == F
    return p + q           # one float32 sum


def outside_mask(tabs, ndim=3):
    """True where an output is "outside": lo < 0 on any axis (broadcast over the channels of a 4-D volume)."""
    out = np.zeros([len(t) for t in tabs] + [1] * (ndim - 3), dtype=bool)
    for a, t in enumerate(tabs):
        shape = [1] * ndim
        shape[a] = len(t)
        out = out | (t["lo"] < 0).reshape(shape)
    return out


def zoom32(x, tabs):
    x = np.asarray(x)
    assert x.dtype == F and x.ndim in (3, 4) and (x.ndim == 3 or x.shape[3] in (1, 3))
    y = x
    with np.errstate(all="ignore"):
        for a in range(3):
            y = _lerp_axis32(y, a, tabs[a])
    y = np.where(outside_mask(tabs, x.ndim), F(0.0), y)
    assert y.dtype == F
    return y


def zoom64(x, tabs):
    y = np.asarray(x, dtype=np.float64)
    for a in range(3):
        y = lerp_axis64(y, a, tabs[a])
    return y


def zoom_bound(x, tabs):
    """Elementwise bound on |float32 zoom - zoom64|: the existing rounding bound without a blur (2 terms per axis)."""
    return error_bound(x, (None,) * 3, tabs)


def f2key(v):
    """fsg_f2key: the int32 whose integer order is the float order (-0.0 < +0.0)."""
    b = np.asarray(v, dtype=F).view(np.int32)
    return np.where(b >= 0, b, b ^ np.int32(0x7FFFFFFF))


def key2f(k):
    k = np.asarray(k, dtype=np.int32)
    return np.where(k >= 0, k, k ^ np.int32(0x7FFFFFFF)).astype(np.int32).view(F)


def minmax32(y):
    y = np.asarray(y)
    assert y.dtype == F
    k = f2key(y[~np.isnan(y)])
    if k.size == 0:
        return KEY_MIN_IDENTITY, KEY_MAX_IDENTITY
    return int(k.min()), int(k.max())


def normalise32(y, mn, mx, mode):
    y = np.asarray(y)
    assert y.dtype == F and mode in (0, 1)
    mn, mx = F(mn), F(mx)
    with np.errstate(all="ignore"):
        t = y / mx
        if mode == 0:
            return t
        q = mn / mx
        if q == F(1.0):
            return t * F(0.0)
        r = (t - q) / (F(1.0) - q)
    assert r.dtype == F
    return r
