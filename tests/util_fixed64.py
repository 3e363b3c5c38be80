"""numpy restatement of the deterministic slice-acquisition adjoint (fsg_slice_acq_adjoint_det_f32, include/fsg_hip.h).

Two layers:
  * the accumulation rule alone: `quantise` (one rounding, half to even, to a multiple of 2^-F, carried as two int64 limbs
    hi * 2^L + lo), integer sums of each limb, `finalise` (the exact integer -> float32 with one rounding, then an exact
    power of two); `quantise_exact` states the same rounding in rational arithmetic;
  * `adjoint_nearest_psf`: the whole FSG_SA_NEAREST_PSF adjoint in np.float32 operations in the kernel's order (the
    library is built without FMA contraction, so every kernel operation is one IEEE operation and can be restated).
    The GPU test compares it bit for bit for slices aligned with the volume axes.
"""
import math
from fractions import Fraction

import numpy as np

F = 72  # FSG_SA_DET_FRAC_BITS
L = 40  # FSG_SA_DET_LIMB_BITS
WF = 32  # the per-pixel weight is summed in one limb of 2^-32
f32, f64 = np.float32, np.float64


def check_value_scale(value_scale):
    """The refusal rule of the entry point: a power of two in [2^-20, 2^20]."""
    v = float(value_scale)
    if not (v > 0) or math.isinf(v):
        raise ValueError(f"value_scale {value_scale!r}")
    m, e = math.frexp(v)
    if m != 0.5 or not -20 <= e - 1 <= 20:
        raise ValueError(f"value_scale {value_scale!r} is not a power of two in [2^-20, 2^20]")
    return f32(v)


def quantise(c, value_scale=1.0):
    """float32 contribution(s) -> (hi, lo) int64 with hi * 2^L + lo = rint_half_even(c * 2^F / value_scale), the way the
    kernel forms the limbs: d = c * 2^(F-L) / value_scale is exact in float64, hi = rint(d), lo = rint((d - hi) * 2^L)."""
    c = np.asarray(c)
    assert c.dtype == f32
    d = c.astype(f64) * (f64(2.0 ** (F - L)) / f64(check_value_scale(value_scale)))
    hi = np.rint(d)  # np.rint: half to even
    return hi.astype(np.int64), np.rint((d - hi) * f64(2.0 ** L)).astype(np.int64)


def quantise_exact(c, value_scale=1.0):
    """The same integers Q in rational arithmetic (Python's round() of a Fraction goes half to even)."""
    k = Fraction(2) ** F / Fraction(float(check_value_scale(value_scale)))
    return [round(Fraction(float(v)) * k) for v in np.asarray(c, f32).reshape(-1)]


def total(hi, lo):
    """Limb sums -> the exact integers (Python ints)."""
    return [(int(h) << L) + int(l) for h, l in zip(np.asarray(hi).reshape(-1).tolist(), np.asarray(lo).reshape(-1).tolist())]


def int_to_f32(values):
    """Integers of any size -> float32 with ONE rounding to nearest even, in integer arithmetic."""
    out = np.empty(len(values), f32)
    for i, a in enumerate(values):
        m, neg = abs(int(a)), a < 0
        shift = max(m.bit_length() - 24, 0)
        if shift:
            q, r = m >> shift, m & ((1 << shift) - 1)
            half = 1 << (shift - 1)
            q += int(r > half or (r == half and (q & 1)))
            m = q << shift  # at most 25 significant bits with trailing zeros: exact in float32
        out[i] = f32(float(-m if neg else m))
    return out


def finalise(hi, lo, value_scale=1.0):
    """Limb sums -> float32: the exact integer rounded once, then * 2^-F * value_scale (exact).  0 -> +0.0."""
    return int_to_f32(total(hi, lo)) * f32(2.0 ** -F * float(check_value_scale(value_scale)))


def pixel_weight(wq):
    """The per-pixel weight from its 2^-32 integer sum: int64 -> float32 (numpy's cast is the C cast: one rounding to
    nearest even, pinned against int_to_f32 in the CPU test), then * 2^-32."""
    return np.asarray(wq, np.int64).astype(f32) * f32(2.0 ** -WF)


def quantise_weight_tap(pv):
    return np.rint(np.asarray(pv, f32).astype(f64) * f64(2.0 ** WF)).astype(np.int64)


def _round_pos(x):
    return np.floor(x + f32(0.49999997))


def _psf_at(psf, T, dx, dy, dz):
    """sa_psf_at_fast: the PSF re-interpolated at a snapped voxel; (valid, value)."""
    pd, ph, pw = psf.shape
    xp = ((T[0] * dx + T[4] * dy) + T[8] * dz) + f32(pw - 1) * f32(0.5)
    yp = ((T[1] * dx + T[5] * dy) + T[9] * dz) + f32(ph - 1) * f32(0.5)
    zp = ((T[2] * dx + T[6] * dy) + T[10] * dz) + f32(pd - 1) * f32(0.5)
    xf, yf, zf = np.floor(xp), np.floor(yp), np.floor(zp)
    jx, jy, jz = xf.astype(np.int64), yf.astype(np.int64), zf.astype(np.int64)
    ok = (jx >= 0) & (jx < pw - 1) & (jy >= 0) & (jy < ph - 1) & (jz >= 0) & (jz < pd - 1)
    jx, jy, jz = np.where(ok, jx, 0), np.where(ok, jy, 0), np.where(ok, jz, 0)
    if pw < 2 or ph < 2 or pd < 2:
        return ok, np.zeros_like(xp)
    wx, wy, wz = xp - xf, yp - yf, zp - zf

    def q(oz, oy, ox):
        return psf[jz + oz, jy + oy, jx + ox]

    a00 = q(0, 0, 0) + wx * (q(0, 0, 1) - q(0, 0, 0))
    a10 = q(0, 1, 0) + wx * (q(0, 1, 1) - q(0, 1, 0))
    a01 = q(1, 0, 0) + wx * (q(1, 0, 1) - q(1, 0, 0))
    a11 = q(1, 1, 0) + wx * (q(1, 1, 1) - q(1, 1, 0))
    b0 = a00 + wy * (a10 - a00)
    b1 = a01 + wy * (a11 - a01)
    return ok, b0 + wz * (b1 - b0)


def adjoint_nearest_psf(transforms, psf, slices, vol_shape, res_slice, slices_mask=None, vol_mask=None, value_scale=1.0,
                        slice_ids=None):
    """(value, weight) float32 volumes of the deterministic FSG_SA_NEAREST_PSF adjoint, not equalised."""
    D, H, W = vol_shape
    psf = np.asarray(psf, f32)
    pd, ph, pw = psf.shape
    slices = np.asarray(slices, f32)
    h, w = slices.shape[1:]
    res = f32(res_slice)
    acc = np.zeros((4, D * H * W), np.int64)  # value hi, value lo, weight hi, weight lo
    hx, hy, hz = f32(W - 1), f32(H - 1), f32(D - 1)
    iy, ix = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    taps = [(kz, ky, kx) for kz in range(pd) for ky in range(ph) for kx in range(pw) if psf[kz, ky, kx] != 0]
    for z, T34 in enumerate(np.asarray(transforms, f32)):
        T = T34.reshape(12)
        sid = z if slice_ids is None else int(slice_ids[z])
        s = slices[sid]
        live = np.ones((h, w), bool) if slices_mask is None else np.asarray(slices_mask[sid], bool)
        # sa_centre: the pixel offset in double, the rotation in fp32, the volume centre added in double
        _x = ((ix.astype(f64) - (w - 1) / 2.0) * f64(res) + f64(T[3])).astype(f32)
        _y = ((iy.astype(f64) - (h - 1) / 2.0) * f64(res) + f64(T[7])).astype(f32)
        _z = T[11]
        xc = ((T[0] * _x + T[1] * _y) + T[2] * _z)
        yc = ((T[4] * _x + T[5] * _y) + T[6] * _z)
        zc = ((T[8] * _x + T[9] * _y) + T[10] * _z)
        xc = (xc.astype(f64) + (W - 1) / 2.0).astype(f32)
        yc = (yc.astype(f64) + (H - 1) / 2.0).astype(f32)
        zc = (zc.astype(f64) + (D - 1) / 2.0).astype(f32)
        tx = [[T[a * 4 + 0] * f32(i - pw // 2) for i in range(pw)] for a in range(3)]
        ty = [[T[a * 4 + 1] * f32(i - ph // 2) for i in range(ph)] for a in range(3)]
        tz = [[T[a * 4 + 2] * f32(i - pd // 2) for i in range(pd)] for a in range(3)]

        def tap(kz, ky, kx):
            x = ((xc + tx[0][kx]) + ty[0][ky]) + tz[0][kz]
            y = ((yc + tx[1][kx]) + ty[1][ky]) + tz[1][kz]
            zz = ((zc + tx[2][kx]) + ty[2][ky]) + tz[2][kz]
            ok = ~((x < 0) | (y < 0) | (zz < 0) | (x >= hx) | (y >= hy) | (zz >= hz))
            xr, yr, zr = _round_pos(x), _round_pos(y), _round_pos(zz)
            inpsf, pv = _psf_at(psf, T, xr - xc, yr - yc, zr - zc)
            iv = (zr.astype(np.int64) * H + yr.astype(np.int64)) * W + xr.astype(np.int64)
            return ok & inpsf & live, pv.astype(f32), iv

        wq = np.zeros((h, w), np.int64)  # pass 1: the pixel weight in fixed point
        for t in taps:
            ok, pv, _ = tap(*t)
            wq += np.where(ok, quantise_weight_tap(pv), 0)
        wsum = pixel_weight(wq)
        live = live & ~(wsum < f32(0.5))
        with np.errstate(divide="ignore"):
            inv = np.where(live, f32(1.0) / wsum, f32(0))
        for t in taps:  # pass 2
            ok, pv, iv = tap(*t)
            ok = ok & live
            if vol_mask is not None:
                ok = ok & np.asarray(vol_mask, bool).reshape(-1)[np.where(ok, iv, 0)]
            pv = (pv * inv).astype(f32)
            for j, q in enumerate(quantise((pv * s).astype(f32), value_scale) + quantise(pv)):
                np.add.at(acc[j], iv[ok], q[ok])
    return finalise(acc[0], acc[1], value_scale).reshape(D, H, W), finalise(acc[2], acc[3]).reshape(D, H, W)
