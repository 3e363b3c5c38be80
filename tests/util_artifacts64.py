"""Float64 reference of the kernels in csrc/fsg_artifacts.hip and csrc/fsg_reduce.hip for the tests (not a test module).

Plain numpy: float64 arithmetic on the float32 inputs the kernels read (integers as int64), one short function per
operation, each citing the lines of the reference it restates (paths relative to the reference's `fetalsyngen/`; the
kernel sources name the same lines).  Nothing here imports the product.

For every operation that rounds, `*_bound(...)` returns the per-element float32 rounding bound of the operation as the
kernel is allowed to evaluate it: (rounded operations on the path) x u x (the magnitude that flows through them), u = 2^-24,
first order, times 1.01 for the second-order terms (the style of util_resample64.error_bound).  Transcendentals:
  * `expf`, `sqrtf` of the device library: <= 1 ulp = 2u relative (ROCm device-libs, OCML accuracy table);
  * `v_exp_f32`: 1 ulp (AMD CDNA3/CDNA4 ISA guide, V_EXP_F32 "1 ULP accuracy"), results below the smallest normal may be
    flushed to zero: 2^-126 absolute per evaluation.
"""
import math

import numpy as np

from oracle.fsg_keyed_draws import philox4x32_10

U32 = 2.0 ** -24       # unit roundoff of float32
ULP1 = 2.0 * U32       # one ulp, relative
TINY = 2.0 ** -126     # smallest normal float32
SECOND = 1.01          # second-order terms
DIST_BIG = 1e9         # "no set voxel in the window" of the distance passes


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- mixture of Gaussians (generator/artifacts/utils.py:125-160 `mog_3d_tensor`) ----------------------------------------
def _mog_terms(shape, centers, sigmas):
    """d[g] = ((x-x0)/sx)^2 + ((y-y0)/sy)^2 + ((z-z0)/sz)^2 on the (D,H,W) grid, x the LAST axis (:151-156)."""
    D, H, W = shape
    c = f64(np.asarray(centers, np.float32)).reshape(-1, 3)
    s = f64(np.asarray(sigmas, np.float32)).reshape(-1, 3)
    z, y, x = np.meshgrid(np.arange(D, dtype=np.float64), np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64),
                          indexing="ij")
    return np.stack([((x - c[g, 0]) / s[g, 0]) ** 2 + ((y - c[g, 1]) / s[g, 1]) ** 2 + ((z - c[g, 2]) / s[g, 2]) ** 2
                     for g in range(len(c))])


def mog64(shape, centers, sigmas):
    """clamp(sum_g exp(-d_g / 2), 0, 1) (:157-160)."""
    return np.clip(np.exp(-_mog_terms(shape, centers, sigmas) / 2).sum(0), 0.0, 1.0)


def mog_bound(shape, centers, sigmas):
    """Per blob: each squared term carries 5u (subtract, divide, both squared by one product), the two adds 2u, the scaling
    of the exponent and its constant 2u: 9u relative on the exponent d/2, so exp(-d/2) moves by exp(-d/2) 9u d/2; the
    exponential itself 1 ulp (+ the flush of a sub-normal result, which also covers a blob skipped because its value is
    below 2^-126); k adds of partial sums <= the whole sum.  The clamp does not increase an error."""
    d = _mog_terms(shape, centers, sigmas)
    e = np.exp(-d / 2)
    per = e * (9 * U32 * d / 2 + ULP1 + U32) + TINY
    return SECOND * (per.sum(0) + len(d) * U32 * e.sum(0))


# ---- Perlin noise (generator/artifacts/utils.py:224-388) --------------------------------------------------------------------
def _perlin_parts(shape, res, grad, lins):
    """Corner dot products, their magnitudes, fades: the pieces of one octave (utils.py:255-327)."""
    g = f64(grad)
    lin = [f64(np.asarray(v, np.float32)) for v in lins]
    cell = [np.floor(v) for v in lin]
    loc = [v - c for v, c in zip(lin, cell)]
    idx = [[np.minimum(c.astype(np.int64) + d, r) for d in (0, 1)] for c, r in zip(cell, res)]
    L = np.meshgrid(*loc, indexing="ij")
    dots, mags = {}, {}
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                gi = g[idx[0][dx][:, None, None], idx[1][dy][None, :, None], idx[2][dz][None, None, :]]
                off = [L[0] - dx, L[1] - dy, L[2] - dz]
                dots[dx, dy, dz] = sum(gi[..., a] * off[a] for a in range(3))
                mags[dx, dy, dz] = sum(np.abs(gi[..., a] * off[a]) for a in range(3))
    fade = [t * t * t * (t * (t * 6 - 15) + 10) for t in L]
    # fade error: the cubic 3u relative, the bracket 46u absolute (its terms reach 15), their product u
    dfade = [t ** 3 * ((4 * np.abs(t * (t * 6 - 15) + 10) + 46) * U32) for t in L]
    return dots, mags, fade, dfade


def _lerp(a, b, t):
    return a * (1 - t) + t * b


def perlin_octave64(shape, res, grad, lins):
    """One octave: gradient dot offset at the 8 corners (corner index clamped to r), quintic fade, lerp along axis 0, then 1,
    then 2 (utils.py:255-327).  lins: the three float32 linspace(0, r_a, n_a) tables the kernel is handed."""
    d, _m, t, _dt = _perlin_parts(shape, res, grad, lins)
    n00, n10 = _lerp(d[0, 0, 0], d[1, 0, 0], t[0]), _lerp(d[0, 1, 0], d[1, 1, 0], t[0])
    n01, n11 = _lerp(d[0, 0, 1], d[1, 0, 1], t[0]), _lerp(d[0, 1, 1], d[1, 1, 1], t[0])
    return _lerp(_lerp(n00, n10, t[1]), _lerp(n01, n11, t[1]), t[2])


def perlin_octave_bound(shape, res, grad, lins):
    """A corner: offset, product, two adds = 4u of sum |g_a off_a|.  A lerp a (1-t) + t b: 1 - t, two products, one add = 3u of
    |a| (1-t) + t |b| plus u |a| (the rounding of 1 - t is absolute), plus |b - a| times the fade's own error, plus the
    errors of a and b carried through with the same weights."""
    d, m, t, dt = _perlin_parts(shape, res, grad, lins)
    err = {k: 4 * U32 * m[k] for k in d}

    def lerp_e(a, ea, b, eb, ax):
        v = _lerp(a, b, t[ax])
        e = ea * (1 - t[ax]) + t[ax] * eb + np.abs(b - a) * dt[ax] + U32 * (3 * (np.abs(a) * (1 - t[ax]) + t[ax] * np.abs(b))
                                                                             + np.abs(a))
        return v, e

    n00, e00 = lerp_e(d[0, 0, 0], err[0, 0, 0], d[1, 0, 0], err[1, 0, 0], 0)
    n10, e10 = lerp_e(d[0, 1, 0], err[0, 1, 0], d[1, 1, 0], err[1, 1, 0], 0)
    n01, e01 = lerp_e(d[0, 0, 1], err[0, 0, 1], d[1, 0, 1], err[1, 0, 1], 0)
    n11, e11 = lerp_e(d[0, 1, 1], err[0, 1, 1], d[1, 1, 1], err[1, 1, 1], 0)
    m0, f0 = lerp_e(n00, e00, n10, e10, 1)
    m1, f1 = lerp_e(n01, e01, n11, e11, 1)
    return SECOND * lerp_e(m0, f0, m1, f1, 2)[1]


def perlin_fractal64(shape, octaves):
    """sum_q amp_q * octave_q and its min / max (utils.py:375-384).  octaves: [(grad, [lin0, lin1, lin2], (r0,r1,r2), amp)]."""
    v = sum(float(np.float32(amp)) * perlin_octave64(shape, r, g, lins) for g, lins, r, amp in octaves)
    return v, float(v.min()), float(v.max())


def perlin_fractal_bound(shape, octaves):
    """Per octave its own bound and the product with the amplitude (u); each accumulation u of the partial sums."""
    tot, mag = 0.0, 0.0
    for g, lins, r, amp in octaves:
        a = abs(float(np.float32(amp)))
        o = np.abs(perlin_octave64(shape, r, g, lins))
        tot = tot + a * (perlin_octave_bound(shape, r, g, lins) + U32 * o)
        mag = mag + a * o
    return SECOND * (tot + len(octaves) * U32 * mag)


def perlin_normalise64(noise, increase):
    """clamp((noise + increase - min) / (max - min), 0, 1) (utils.py:386-387)."""
    noise = f64(noise)
    return np.clip((noise + float(np.float32(increase)) - noise.min()) / (noise.max() - noise.min()), 0.0, 1.0)


# ---- weighted blend (simulate_reco.py:704, augmentation/artifacts.py:125, :322-337) ------------------------------------------
def _blend_parts(a, b, w, w_mm, increase, seg, noise_std, b_mm, a_mm):
    w = f64(w)
    dw = np.zeros_like(w)
    if w_mm is not None:  # raw Perlin noise normalised on the fly (utils.py:386-387)
        mn, mx = float(w_mm[0]), float(w_mm[1])
        inc = float(np.float32(increase))
        raw = (w + inc - mn) / (mx - mn)
        # w + inc, - mn: u each of their results; max - min and the quotient: 2u of the quotient
        dw = U32 * (np.abs(w + inc) + np.abs(w + inc - mn)) / abs(mx - mn) + 2 * U32 * np.abs(raw)
        w = np.clip(raw, 0.0, 1.0)
    if seg is not None:  # w *= (seg > 0): exact
        keep = f64(seg) > 0
        w, dw = w * keep, dw * keep
    if a is None:
        return w, dw, None, None, None, None
    a, b = f64(a), f64(b)
    db = np.zeros_like(b)
    if noise_std is not None:  # structured noise: b' = clamp(a + std * b / max|b|, 0, 2 max a) (artifacts.py:322-327)
        sc = max(abs(float(b_mm[0])), abs(float(b_mm[1])))
        t = float(np.float32(noise_std)) * (b / sc)
        db = U32 * (2 * np.abs(t) + np.abs(a + t))  # quotient, product, sum
        b = np.clip(a + t, 0.0, 2 * float(a_mm[1]))
    return w, dw, a, b, db, (1 - w) * a + w * b


def blend64(a, b, w, w_mm=None, increase=0.0, seg=None, noise_std=None, b_mm=None, a_mm=None):
    """(out, weight used); out None when a is None.  *_mm: (min, max) as floats."""
    w, _dw, _a, _b, _db, out = _blend_parts(a, b, w, w_mm, increase, seg, noise_std, b_mm, a_mm)
    return out, w


def blend_bound(a, b, w, w_mm=None, increase=0.0, seg=None, noise_std=None, b_mm=None, a_mm=None):
    """(bound of out, bound of the weight).  out = (1-w) a + w b: 1 - w (u, absolute, times |a|), two products and the sum
    (3u of |(1-w) a| + |w b|), |b - a| times the weight's error, w times b's error."""
    w, dw, a, b, db, _out = _blend_parts(a, b, w, w_mm, increase, seg, noise_std, b_mm, a_mm)
    if a is None:
        return None, SECOND * dw
    e = np.abs(b - a) * dw + w * db + U32 * np.abs(a) + 3 * U32 * (np.abs((1 - w) * a) + np.abs(w * b))
    return SECOND * e, SECOND * dw


# ---- scanner corruptions (generator/artifacts/simulate_reco.py:236-298, :409) --------------------------------------------------
def rician64(s, thr, sigma, z1, z2):
    """s = sqrt((s + sigma z1)^2 + (sigma z2)^2) where s > thr, strictly (simulate_reco.py:247-255)."""
    s, sg = f64(s), float(np.float32(sigma))
    m = s > float(np.float32(thr))
    return np.where(m, np.sqrt((s + f64(z1) * sg) ** 2 + (f64(z2) * sg) ** 2), s)


def rician_bound(s, thr, sigma, z1, z2):
    """p = s + sigma z1: 2 ops; q = sigma z2: 1; r = sqrt(p p + q q): three ops under the root (1.5u of r) and the root (1 ulp)."""
    s, sg = f64(s), float(np.float32(sigma))
    m = s > float(np.float32(thr))
    p, q = s + f64(z1) * sg, f64(z2) * sg
    dp, dq = U32 * (np.abs(f64(z1) * sg) + np.abs(p)), U32 * np.abs(q)
    r = np.sqrt(p * p + q * q)
    e = np.where(r > 0, (np.abs(p) * dp + np.abs(q) * dq) / np.where(r > 0, r, 1.0), dp + dq) + (1.5 * U32 + ULP1) * r
    return np.where(m, SECOND * e, 0.0)


def _void_parts(h_lin, w_lin, par):
    yc, xc, c, sn, A, sx, sy = (float(v) for v in np.asarray(par, np.float32))
    y, x = f64(np.asarray(h_lin, np.float32))[:, None] - yc, f64(np.asarray(w_lin, np.float32))[None, :] - xc
    xr, yr = c * x - sn * y, sn * x + c * y
    mag = np.abs(c * x) + np.abs(sn * y), np.abs(sn * x) + np.abs(c * y)
    E = sx * xr * xr + sy * yr * yr
    return xr, yr, mag, E, A, sx, sy


def void64(slices, ids, params, ylin, xlin):
    """slice ids[t] *= 1 - A exp(sx x'^2 + sy y'^2), (x', y') rotated about (xc, yc) (simulate_reco.py:258-298);
    params[t] = {yc, xc, cos, sin, A, sx, sy}.  ids distinct."""
    out = f64(slices).copy()
    for t, i in enumerate(ids):
        _xr, _yr, _mag, E, A, _sx, _sy = _void_parts(ylin, xlin, params[t])
        out[i] *= 1 - A * np.exp(E)
    return out


def void_bound(slices, ids, params, ylin, xlin):
    """x, y: u; a rotated coordinate: 3u of |c x| + |s y| (incl. x, y); its square: twice that relative + u; each scaled
    square + the sum: 2u of the exponent's terms; expf 1 ulp; A exp: u; 1 - : u; the product with the pixel: u."""
    s = f64(slices)
    out = np.zeros_like(s)
    for t, i in enumerate(ids):
        xr, yr, (mx, my), E, A, sx, sy = _void_parts(ylin, xlin, params[t])
        dE = abs(sx) * (2 * np.abs(xr) * 3 * U32 * mx + U32 * xr * xr) + abs(sy) * (2 * np.abs(yr) * 3 * U32 * my + U32 * yr * yr) \
            + 2 * U32 * (np.abs(sx * xr * xr) + np.abs(sy * yr * yr))
        ex = np.exp(E)
        dm = abs(A) * ex * (dE + ULP1 + U32) + U32 * np.abs(1 - A * ex)
        out[i] = SECOND * (np.abs(s[i]) * (dm + U32 * np.abs(1 - A * ex)))
    return out


def slice_sums64(slices):
    """Per-slice sum (simulate_reco.py:409), exactly rounded (math.fsum)."""
    s = f64(slices).reshape(len(slices), -1)
    return np.array([math.fsum(r.tolist()) for r in s])


def slice_sums_bound(slices):
    """Accumulated in float64 (hw additions of at most sum |x|, 2^-53 each), rounded once to float32."""
    s = f64(slices).reshape(len(slices), -1)
    return SECOND * (U32 * np.abs(slice_sums64(slices)) + s.shape[1] * 2.0 ** -53 * np.abs(s).sum(1))


# ---- voxel sets (augmentation/artifacts.py:78-80 boolean-mask gather; torch.where(mask)[...][randperm]) -------------------------
def pred64(v, op, value):
    """The predicate on (float)v; NaN != 0 is true, -0.0 != 0 is false (IEEE, as torch)."""
    f = np.asarray(v).astype(np.float32)
    value = np.float32(value)
    with np.errstate(invalid="ignore"):
        return {">": f > value, "==": f == value, "!=": f != value}[op]


def rank_coords64(v, op, value, ranks):
    """Coordinates of the ranks-th voxels satisfying the predicate, raster order (np.argwhere)."""
    return np.argwhere(pred64(v, op, value)).astype(np.int64)[np.asarray(ranks, dtype=np.int64)]


def rank_flat64(v, op, value, ranks):
    return np.flatnonzero(pred64(v, op, value)).astype(np.int64)[np.asarray(ranks, dtype=np.int64)]


def compact64(values, pred, op, value):
    return np.asarray(values)[pred64(pred, op, value)]


def scatter64(shape, flat_idx):
    """Zeros with ones at the flat indices inside [0, n); the others are ignored."""
    out = np.zeros(int(np.prod(shape)), np.float32)
    i = np.asarray(flat_idx, dtype=np.int64)
    out[i[(i >= 0) & (i < out.size)]] = 1.0
    return out.reshape(shape)


EWISE = ("add", "gt", "eq", "mul", "mul_gt", "max", "sub_gt", "le")


def ewise64(op, a, b=None, value=0.0):
    """The eight element-wise helpers.  One float32 operation each: the float64 result of two float32 operands is exact for
    + - *, so rounding it once to float32 is the float32 operation."""
    a = f64(a)
    b = None if b is None else f64(b)
    v = float(np.float32(value))
    r = {"add": lambda: a + b, "gt": lambda: a > v, "eq": lambda: a == v, "mul": lambda: a * b,
         "mul_gt": lambda: a * (b > v), "max": lambda: np.maximum(a, b),
         "sub_gt": lambda: f64((a - b).astype(np.float32)) > v, "le": lambda: a <= v}[op]()
    return np.asarray(r, dtype=np.float64).astype(np.float32)


# ---- binary morphology (generator/artifacts/utils.py:163-210, augmentation/artifacts.py:484-499, :587-589) ---------------------
def distance_brute64(mask, radius, metric):
    """min over the set voxels of the squared Euclidean ("euclid2") / city-block ("l1") distance, by direct minimisation
    (no separable form); DIST_BIG where it exceeds radius^2 / radius or the mask is empty."""
    m = np.asarray(mask) > 0
    pts = np.argwhere(m).astype(np.int64)
    cap = radius * radius if metric == "euclid2" else radius
    out = np.full(m.shape, np.iinfo(np.int64).max, dtype=np.int64)
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.int64) for n in m.shape], indexing="ij"), -1)
    for p in pts:
        d = grid - p
        d = (d * d).sum(-1) if metric == "euclid2" else np.abs(d).sum(-1)
        np.minimum(out, d, out=out)
    return np.where(out <= cap, out.astype(np.float64), DIST_BIG)


def distance_separable64(mask, radius, metric):
    """The same capped distance by three windowed axis passes in int64 (for volumes too large for the brute force)."""
    m = np.asarray(mask) > 0
    big = np.int64(10 ** 9)
    d = np.where(m, np.int64(0), big)
    for axis in (2, 1, 0):
        n = d.shape[axis]
        best = d.copy()
        for t in range(1, min(radius, n - 1) + 1):
            c = np.int64(t * t if metric == "euclid2" else t)
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, n - t), slice(t, n)
            lo, hi = tuple(lo), tuple(hi)
            np.minimum(best[lo], d[hi] + c, out=best[lo])
            np.minimum(best[hi], d[lo] + c, out=best[hi])
        d = best
    cap = radius * radius if metric == "euclid2" else radius
    return np.where(d <= cap, d.astype(np.float64), DIST_BIG)


def ball_dilate64(mask, r):
    """Zero-padded convolution with the (2r+1)^3 ball x^2 + y^2 + z^2 <= r^2, > 0 (artifacts.py:484-499)."""
    m = np.asarray(mask) > 0
    p = np.pad(m, r)
    out = np.zeros_like(m)
    for dx in range(-r, r + 1):
        for dy in range(-r, r + 1):
            for dz in range(-r, r + 1):
                if dx * dx + dy * dy + dz * dz <= r * r:
                    out |= p[r + dx:r + dx + m.shape[0], r + dy:r + dy + m.shape[1], r + dz:r + dz + m.shape[2]]
    return out


def cross_dilate64(mask, r):
    """r successive dilations with the 3x3x3 cross ball(1) (artifacts.py:587-589)."""
    m = np.asarray(mask) > 0
    for _ in range(r):
        p = np.pad(m, 1)
        m = (p[1:-1, 1:-1, 1:-1] | p[:-2, 1:-1, 1:-1] | p[2:, 1:-1, 1:-1] | p[1:-1, :-2, 1:-1] | p[1:-1, 2:, 1:-1]
             | p[1:-1, 1:-1, :-2] | p[1:-1, 1:-1, 2:])
    return m


def box_sum64(v, k):
    """Zero-padded k x k x k box sum (conv3d with a ones kernel, padding k // 2: utils.py:163-210), int64."""
    v = np.asarray(v).astype(np.int64)
    r = k // 2
    for axis in range(3):
        pad = [(0, 0)] * 3
        pad[axis] = (r, r)
        p = np.pad(v, pad)
        v = sum(np.take(p, np.arange(t, t + v.shape[axis]), axis=axis) for t in range(k))
    return v


NEAR_TIE = 2.0 ** -22


def boundary64(image, mask, mask_modif, mog, dist, n_dilate):
    """SimulatedBoundaries, fuzzy branch (artifacts.py:565-602): k = max(rint(p n - 1), 0) (ties to even), p = mog on the
    voxels mask_modif added to mask and 0 elsewhere; m = mask_modif * (dist <= max(k - 1, 0)); out = image * m.
    Returns (out or None, m, near): near marks the voxels whose p n - 1 lies within NEAR_TIE of a half-integer."""
    mm = f64(mask_modif)
    p = np.where((mm - f64(mask)) > 0, f64(mog), 0.0)
    x = p * n_dilate - 1
    k = np.maximum(np.rint(x), 0.0)
    m = mm * (f64(dist) <= np.maximum(k - 1, 0.0))
    near = np.abs(x - np.floor(x) - 0.5) < NEAR_TIE
    return (None if image is None else f64(image) * m), m, near


def bernoulli64(a, p, seed, stream_id):
    """a * (u < p): element e takes word e % 4 of Philox block e // 4 (counter = (block lo, block hi, stream lo, stream hi),
    key = (seed lo, seed hi)), u = top 24 bits * 2^-24; zeros stay zero (stand-in for artifacts.py:515-518)."""
    a = np.asarray(a, np.float32).reshape(-1)
    e = np.arange(a.size, dtype=np.uint64)
    blk = e >> np.uint64(2)
    words = np.stack(philox4x32_10(blk & np.uint64(0xFFFFFFFF), blk >> np.uint64(32), stream_id & 0xFFFFFFFF, stream_id >> 32,
                                   seed & 0xFFFFFFFF, seed >> 32), -1)
    w = words[np.arange(a.size), (e & np.uint64(3)).astype(np.int64)]
    u = (w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return np.where((a != 0) & (u < np.float32(p)), a, np.float32(0)).astype(np.float32)


# ---- reductions and scalings (augmentation/synthseg.py:112, data/datasets.py:40, :311, generator/model.py:138) -------------------
def minmax64(x):
    """(min, max), NaN ignored (fminf / fmaxf); all NaN or empty: the identities (+inf, -inf)."""
    x = f64(x).reshape(-1)
    x = x[~np.isnan(x)]
    return (float(x.min()), float(x.max())) if x.size else (math.inf, -math.inf)


def scale64(x, mn, mx, mode):
    """0: x / max; 1: (x - min) / (max - min), all zeros when flat; 2: (x - min) / (max - min) * 255."""
    x = f64(x)
    if mode == 0:
        return x / mx
    if mode == 1 and mn == mx:
        return x * 0.0
    with np.errstate(invalid="ignore"):  # mode 2 on a flat input is 0 / 0, as in the reference
        return (x - mn) / (mx - mn) * (255.0 if mode == 2 else 1.0)


def scale_bound(x, mn, mx, mode):
    """mode 0: one division; 1: x - min, max - min, the division (3u of the result, none when flat); 2: one product more."""
    r = np.abs(scale64(x, mn, mx, mode))
    return SECOND * U32 * r * (1 if mode == 0 else (3 if mode == 1 else 4))


def cast_f16_64(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16)
