"""Float64 reference of K6 + K7 + K8 (blur, axis-aligned down-sampling, low-resolution noise) for the tests (not a test
module).  Plain numpy, any per-axis tap set and any packed table (tables.TAP_DTYPE).

Semantics (csrc/fsg_blur_rs.hip header, tables.position_table):
  * blur along x, then y, then z: B[i] = sum_t k[t] * x[i + t - R], R = len(k) // 2, zero padded, not renormalised;
  * per-axis lerp from the packed table: out[j] = w_lo[j] * B[lo[j]] + w_hi[j] * B[hi[j]]; an output with lo < 0 is 0;
  * optional noise: + std * z with z a given field, then negatives clamped to 0.

`error_bound` is the float32 rounding bound of any kernel computing the same operation: each axis is a sum of at most
len(k) products (blur) and a two-term lerp, with non-negative coefficients, so a computed result differs from the exact one
by at most  u * (sum over axes of (len(k_a) + 2)) * (the same operator applied to |x|)  (first order in u = 2^-24, in any
summation order, with or without fused multiply-adds), plus 2u of the noise term for the add and its product.
"""
import numpy as np

U32 = 2.0 ** -24  # unit roundoff of float32


def blur_axis64(x, axis: int, taps) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    k = np.asarray(taps, dtype=np.float64)
    if k.ndim != 1 or len(k) % 2 == 0:
        raise ValueError("odd number of taps expected")
    R = len(k) // 2
    n = x.shape[axis]
    pad = [(0, 0)] * x.ndim
    pad[axis] = (R, R)
    xp = np.pad(x, pad)
    out = np.zeros_like(x)
    for t in range(len(k)):
        out += k[t] * np.take(xp, np.arange(t, t + n), axis=axis)
    return out


def lerp_axis64(b, axis: int, tab) -> np.ndarray:
    b = np.asarray(b, dtype=np.float64)
    lo = tab["lo"].astype(np.int64)
    hi = tab["hi"].astype(np.int64)
    ok = lo >= 0
    shape = [1] * b.ndim
    shape[axis] = len(tab)
    wl = np.where(ok, tab["w_lo"].astype(np.float64), 0.0).reshape(shape)
    wh = np.where(ok, tab["w_hi"].astype(np.float64), 0.0).reshape(shape)
    a = np.take(b, np.where(ok, lo, 0), axis=axis)
    c = np.take(b, np.where(ok, hi, 0), axis=axis)
    return np.where(ok.reshape(shape), wl * a + wh * c, 0.0)


def blur_resample64(x, taps, tabs, noise_std=None, z=None) -> np.ndarray:
    """K6 (taps[a] None: no blur on axis a) + K7 (tabs[a] None: axis kept) + K8 (z given: + noise_std * z, clamp)."""
    y = np.asarray(x, dtype=np.float64)
    for a in range(3):
        if taps[a] is not None:
            y = blur_axis64(y, a, taps[a])
    for a in range(3):
        if tabs[a] is not None:
            y = lerp_axis64(y, a, tabs[a])
    if z is not None:
        y = y + np.float64(np.float32(noise_std)) * np.asarray(z, dtype=np.float64)
        y = np.maximum(y, 0.0)
    return y


def error_bound(x, taps, tabs, noise_std=None, z=None) -> np.ndarray:
    """Elementwise bound on |float32 result - blur_resample64(...)| (module docstring); exactly 0 wherever every input
    the output depends on is 0."""
    terms = sum(len(k) for k in taps if k is not None) + 2 * sum(t is not None for t in tabs)
    mag = blur_resample64(np.abs(np.asarray(x, dtype=np.float64)), taps, tabs)
    bound = terms * U32 * mag
    if z is not None:
        nz = np.abs(np.float64(np.float32(noise_std)) * np.asarray(z, dtype=np.float64))
        bound = bound + 2 * U32 * (mag + nz)
    return 1.01 * bound  # second-order terms
