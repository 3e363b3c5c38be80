"""numpy restatement of the deterministic grad_vol of the slice-acquisition backward (fsg_slice_acq_backward_det_f32; the rule
is in include/fsg_hip.h and DESIGN.md section 20).  Test infrastructure, numpy only.

    contributions(...)   every float32 value the kernel hands to its accumulator, with the voxel it goes to: the formula of
                         util_sa_backward64.backward32 with every operation in np.float32 in the kernel's order (the library
                         is built without FMA contraction, so every kernel operation is one IEEE operation), slice by slice,
                         tap by tap, corner by corner.  The per-pixel weight is one thread's sum in tap order.
    accumulate(...)      each contribution quantised once (util_fixed64.quantise), the integers summed per voxel as Python
                         integers, every voxel finalised with one rounding (util_fixed64.finalise).
    backward_det(...)    the two together: grad_vol (D,H,W) float32 and k_vol, the number of contributions per voxel.
"""
import numpy as np

from tests import util_fixed64 as X
from tests.util_sa_backward64 import CORNERS, _round_away

f32, f64 = np.float32, np.float64


def contributions(transforms, vol_shape, vol_mask, psf, grad_slices, slices_mask, res_slice, interp_psf):
    """-> (voxel index int64 [m], contribution float32 [m]) in the order slice, tap, corner, pixel."""
    D, H, W = vol_shape
    psf = np.asarray(psf, f32)
    pd, ph, pw = psf.shape
    g = np.asarray(grad_slices, f32)
    n, h, w = g.shape
    vm = None if vol_mask is None else np.asarray(vol_mask, bool).reshape(-1)
    sm = np.ones((n, h, w), bool) if slices_mask is None else np.asarray(slices_mask, bool).reshape(n, h, w)
    res = f64(f32(res_slice))
    hx, hy, hz = f32(W - 1), f32(H - 1), f32(D - 1)
    qx, qy, qz = f32(pw - 1), f32(ph - 1), f32(pd - 1)
    one = f32(1)
    iy, ix = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    taps = [(kz, ky, kx) for kz in range(pd) for ky in range(ph) for kx in range(pw) if psf[kz, ky, kx] != 0]
    pp = np.pad(psf, ((0, 1), (0, 1), (0, 1)))  # (a rejected PSF cell is read at index 0 and never used)
    out_i, out_c = [], []
    old = np.seterr(invalid="ignore", over="ignore", divide="ignore")
    try:
        for z, T34 in enumerate(np.asarray(transforms, f32).reshape(-1, 3, 4)):
            T = T34.reshape(12)
            # sa_pixel / sa_centre: the pixel offset in double, the rotation in fp32, the volume centre added in double
            _x = ((ix.astype(f64) - (w - 1) / 2.0) * res + f64(T[3])).astype(f32)
            _y = ((iy.astype(f64) - (h - 1) / 2.0) * res + f64(T[7])).astype(f32)
            _z = T[11]
            xc = (((T[0] * _x + T[1] * _y) + T[2] * _z).astype(f64) + (W - 1) / 2.0).astype(f32)
            yc = (((T[4] * _x + T[5] * _y) + T[6] * _z).astype(f64) + (H - 1) / 2.0).astype(f32)
            zc = (((T[8] * _x + T[9] * _y) + T[10] * _z).astype(f64) + (D - 1) / 2.0).astype(f32)
            tx = [[T[a * 4 + 0] * f32(i - pw // 2) for i in range(pw)] for a in range(3)]
            ty = [[T[a * 4 + 1] * f32(i - ph // 2) for i in range(ph)] for a in range(3)]
            tz = [[T[a * 4 + 2] * f32(i - pd // 2) for i in range(pd)] for a in range(3)]

            def fac(wv, bit):
                return wv if bit else (one - wv)

            def tap(kz, ky, kx):
                """-> accepted, the tap's value in the weight (raw or re-interpolated), and what pass 2 needs"""
                x = ((xc + tx[0][kx]) + ty[0][ky]) + tz[0][kz]
                y = ((yc + tx[1][kx]) + ty[1][ky]) + tz[1][kz]
                zz = ((zc + tx[2][kx]) + ty[2][ky]) + tz[2][kz]
                ok = (x >= 0) & (y >= 0) & (zz >= 0) & (x < hx) & (y < hy) & (zz < hz)
                x, y, zz = (np.where(ok, v, 0).astype(f32) for v in (x, y, zz))
                if not interp_psf:
                    return ok, np.full((h, w), psf[kz, ky, kx], f32), (x, y, zz)
                xr, yr, zr = _round_away(x), _round_away(y), _round_away(zz)
                ex, ey, ez = xr - xc, yr - yc, zr - zc
                xp = (((T[0] * ex + T[4] * ey) + T[8] * ez).astype(f64) + (pw - 1) / 2.0).astype(f32)
                yp = (((T[1] * ex + T[5] * ey) + T[9] * ez).astype(f64) + (ph - 1) / 2.0).astype(f32)
                zp = (((T[2] * ex + T[6] * ey) + T[10] * ez).astype(f64) + (pd - 1) / 2.0).astype(f32)
                ok = ok & (xp >= 0) & (yp >= 0) & (zp >= 0) & (xp < qx) & (yp < qy) & (zp < qz)
                xp, yp, zp = (np.where(ok, v, 0).astype(f32) for v in (xp, yp, zp))
                xf, yf, zf = np.floor(xp), np.floor(yp), np.floor(zp)
                wx, wy, wz = xp - xf, yp - yf, zp - zf
                jx, jy, jz = xf.astype(np.int64), yf.astype(np.int64), zf.astype(np.int64)
                val = np.zeros((h, w), f32)  # sa_tri8: eight terms added to 0 in the corner list's order
                for c in CORNERS:
                    val = val + ((fac(wx, c[0]) * fac(wy, c[1])) * fac(wz, c[2])) * pp[jz + c[2], jy + c[1], jx + c[0]]
                return ok, val, (xr, yr, zr)

            # ---- pass 1: the pixel's weight, one thread's sum in tap order (vol_mask not consulted) ----
            weight = np.zeros((h, w), f32)
            for t in taps:
                ok, pv, _ = tap(*t)
                weight = np.where(ok, weight + pv, weight).astype(f32)
            live = sm[z] & (g[z] != 0) & (weight != 0)
            gs = np.where(live, g[z] / np.where(live, weight, one), 0).astype(f32)

            # ---- pass 2 ----
            for t in taps:
                ok, pv, (x, y, zz) = tap(*t)
                ok = ok & live
                if interp_psf:
                    iv = (zz.astype(np.int64) * H + y.astype(np.int64)) * W + x.astype(np.int64)
                    iv = np.where(ok, iv, 0)
                    if vm is not None:
                        ok = ok & vm[iv]
                    out_i.append(iv[ok])
                    out_c.append((pv * gs).astype(f32)[ok])
                else:
                    xf, yf, zf = np.floor(x), np.floor(y), np.floor(zz)
                    wx, wy, wz = x - xf, y - yf, zz - zf
                    iv = (zf.astype(np.int64) * H + yf.astype(np.int64)) * W + xf.astype(np.int64)
                    pg = (pv * gs).astype(f32)
                    for c in CORNERS:
                        ic = np.where(ok, iv + (c[2] * H + c[1]) * W + c[0], 0)
                        okc = ok if vm is None else (ok & vm[ic])
                        out_i.append(ic[okc])
                        out_c.append(((((fac(wx, c[0]) * fac(wy, c[1])) * fac(wz, c[2])) * pg).astype(f32))[okc])
    finally:
        np.seterr(**old)
    if not out_i:
        return np.zeros(0, np.int64), np.zeros(0, f32)
    idx, c = np.concatenate(out_i), np.concatenate(out_c)
    assert c.dtype == f32
    return idx, c


def accumulate(idx, c, nvox, grad_scale=1.0):
    """Contributions -> float32 [nvox]: quantised once each, summed per voxel as Python integers, finalised once."""
    hi, lo = X.quantise(np.asarray(c, f32), grad_scale)
    acc = np.zeros(nvox, object)  # Python integers: no width to overflow
    q = np.empty(len(idx), object)
    q[:] = X.total(hi, lo)
    np.add.at(acc, idx, q)
    return X.finalise(np.zeros(nvox, object), acc, grad_scale)  # (the whole integer in the low limb's place: any split will do)


def backward_det(transforms, vol_shape, vol_mask, psf, grad_slices, slices_mask, res_slice, interp_psf, grad_scale=1.0):
    D, H, W = vol_shape
    idx, c = contributions(transforms, vol_shape, vol_mask, psf, grad_slices, slices_mask, res_slice, interp_psf)
    k = np.zeros(D * H * W, np.int64)
    np.add.at(k, idx, 1)
    return {"grad_vol": accumulate(idx, c, D * H * W, grad_scale).reshape(D, H, W), "k_vol": k.reshape(D, H, W)}


def of_case(case, interp_psf, grad_scale=1.0):
    """backward_det of a case of tests/util_sa_backward_cases.py"""
    return backward_det(case["tr"], case["vol"].shape, case["vm"], case["psf"], case["g"], case["sm"], case["res"], interp_psf,
                        grad_scale)
