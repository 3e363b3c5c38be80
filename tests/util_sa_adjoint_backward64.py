"""CPU restatements of the slice-acquisition ADJOINT (CUDA semantics) and of its backward (include/fsg_hip.h,
fsg_slice_acq_adjoint_backward_f32).  Test infrastructure, numpy only.

    adjoint64(...)            the adjoint forward, every operation in float64 from the fp32 inputs: vol, vol_weight and the
                              per-pixel weight.  Pinned to oracle/fsg_oracle_sr.py by the CPU tests.
    adjoint_backward64(...)   the backward, every operation in float64 from the fp32 inputs: the yardstick.
    adjoint_backward32(...)   the same formula with every operation in np.float32 in the kernel's operation order, the per-pixel
                              sums over the taps (val, weight, the 12 transform sums) included: what one thread of the kernel
                              computes.  Only the sum over the pixels of a slice, which the kernel reduces in a tree, is carried
                              in float64.  The difference to adjoint_backward64 is what fp32 costs the formula itself.

The rule of the backward, restated (quirks of the reference named):
  * equalize: g' = grad_vol / (w < 1e-3 ? 1e-3 : w) where w = vol_weight > 0, grad_vol elsewhere (QUIRK: the 1e-3 floor; the
    forward divides by w itself).  grad_vol is not modified.  Otherwise g' = grad_vol;
  * a pixel outside slices_mask gives nothing.  ONE pass over the non-zero taps with 0 <= p < size-1 on every axis:
      LINEAR       val_ = sum over unmasked corners of corner weight * g'; val += psf * val_; weight += psf, whatever vol_mask
                   says; transforms from s = (equalize ? slice - vol[corner] : slice) * g'[corner] per unmasked corner;
      NEAREST_PSF  a masked rounded voxel skips the tap BEFORE the weight (QUIRK: the forward's weight counts it), then taps whose
                   PSF coordinate is outside [0, psf_size-1) are skipped; val += psf' * g'[voxel]; weight += psf';
  * QUIRK: weight > 0 keeps the pixel (the forward drops weight < 0.5): grad_slices = val / weight, the 12 sums / weight;
  * QUIRK: the weight is held constant in grad_transforms.
Every range test is in accepting form (`x >= 0 and x < hi`): a NaN or Inf coordinate fails it and the tap is skipped.

The backward functions return a dict:
    grad_slices (n,h,w) f64, grad_transforms (n,12) f64
    k_sl, s_sl / k_tr, s_tr       number of finest-grain terms summed into each output element and the sum of their
                                  magnitudes (a term: one corner's product, divided by the pixel's weight, before cancellation)
    dist                          smallest distance, over the pixels inside slices_mask, of a tap coordinate to a decision point:
                                  'bounds', 'grid', 'psf_bounds', 'psf_grid' as tests/util_sa_backward64.py
    pixel_margin (n,h,w)          the same minimum per pixel over all four kinds, for EVERY pixel (inf where it has no tap)
    pixel_weight (n,h,w)          the backward's own per-pixel weight
"""
import numpy as np

from tests.util_sa_backward64 import CORNERS, _round_away

FLOOR = 1e-3


class _Geometry:
    def __init__(self, transforms, psf, nhw, vol_shape, res_slice, ft):
        f64 = np.float64
        self.ft = ft
        self.T = np.asarray(transforms, np.float32).reshape(-1, 3, 4).astype(ft)
        self.psf = np.asarray(psf, np.float32).astype(ft)
        self.D, self.H, self.W = (int(v) for v in vol_shape)
        self.pd, self.ph, self.pw = self.psf.shape
        n, h, w = self.nhw = tuple(int(v) for v in nhw)
        res = f64(np.float32(res_slice))
        T, D, H, W = self.T, self.D, self.H, self.W
        r = self.r
        ixs = np.arange(w, dtype=f64)[None, None, :]
        iys = np.arange(h, dtype=f64)[None, :, None]
        t64 = T.astype(f64)
        # pixel in slice axes (formed in double, kept in ft), centre in voxel coordinates
        self._x = np.broadcast_to(((ixs - (w - 1) / 2.0) * res + t64[:, 0, 3, None, None]).astype(ft), (n, h, w))
        self._y = np.broadcast_to(((iys - (h - 1) / 2.0) * res + t64[:, 1, 3, None, None]).astype(ft), (n, h, w))
        self._z = np.broadcast_to(T[:, 2, 3, None, None], (n, h, w))
        _x, _y, _z = self._x, self._y, self._z
        self.xc = ((r(0, 0) * _x + r(0, 1) * _y + r(0, 2) * _z).astype(f64) + (W - 1) / 2.0).astype(ft)
        self.yc = ((r(1, 0) * _x + r(1, 1) * _y + r(1, 2) * _z).astype(f64) + (H - 1) / 2.0).astype(ft)
        self.zc = ((r(2, 0) * _x + r(2, 1) * _y + r(2, 2) * _z).astype(f64) + (D - 1) / 2.0).astype(ft)

    def r(self, i, j):
        return self.T[:, i, j][:, None, None]

    def taps(self):
        ft, pd, ph, pw = self.ft, self.pd, self.ph, self.pw
        for kz in range(pd):
            for ky in range(ph):
                for kx in range(pw):
                    pv = self.psf[kz, ky, kx]
                    if pv != 0:
                        yield ft(kx - pw // 2), ft(ky - ph // 2), ft(kz - pd // 2), pv

    def position(self, fx, fy, fz):
        r = self.r
        x = self.xc + r(0, 0) * fx + r(0, 1) * fy + r(0, 2) * fz
        y = self.yc + r(1, 0) * fx + r(1, 1) * fy + r(1, 2) * fz
        z = self.zc + r(2, 0) * fx + r(2, 1) * fy + r(2, 2) * fz
        acc = (x >= 0) & (y >= 0) & (z >= 0) & (x < self.W - 1) & (y < self.H - 1) & (z < self.D - 1)
        return x, y, z, acc

    def rounded(self, x, y, z, acc):
        xr, yr, zr = (np.where(acc, _round_away(np.where(acc, v, 0)), 0).astype(self.ft) for v in (x, y, z))
        iv = zr.astype(np.int64) * (self.H * self.W) + yr.astype(np.int64) * self.W + xr.astype(np.int64)
        return xr, yr, zr, iv

    def psf_cell(self, xr, yr, zr, acc):
        """NEAREST_PSF: PSF coordinate of the rounded voxel -> coordinates, accepted, fractions, the 8 PSF values (kernel order)"""
        f64, ft, r, pd, ph, pw = np.float64, self.ft, self.r, self.pd, self.ph, self.pw
        ex, ey, ez = xr - self.xc, yr - self.yc, zr - self.zc
        xp = ((r(0, 0) * ex + r(1, 0) * ey + r(2, 0) * ez).astype(f64) + (pw - 1) / 2.0).astype(ft)
        yp = ((r(0, 1) * ex + r(1, 1) * ey + r(2, 1) * ez).astype(f64) + (ph - 1) / 2.0).astype(ft)
        zp = ((r(0, 2) * ex + r(1, 2) * ey + r(2, 2) * ez).astype(f64) + (pd - 1) / 2.0).astype(ft)
        accp = acc & (xp >= 0) & (yp >= 0) & (zp >= 0) & (xp < pw - 1) & (yp < ph - 1) & (zp < pd - 1)
        xf, yf, zf = (np.where(accp, np.floor(v), 0) for v in (xp, yp, zp))
        wx, wy, wz = (np.where(accp, a - b, 0).astype(ft) for a, b in ((xp, xf), (yp, yf), (zp, zf)))
        xi, yi, zi = xf.astype(np.int64), yf.astype(np.int64), zf.astype(np.int64)
        pp = np.pad(self.psf, ((0, 1), (0, 1), (0, 1)))
        q = [pp[zi + c[2], yi + c[1], xi + c[0]] for c in CORNERS]
        return (xp, yp, zp), accp, (wx, wy, wz), q

    def cell(self, x, y, z, acc):
        """LINEAR: fractions and the flat index of the cell's first corner"""
        xf, yf, zf = (np.where(acc, np.floor(v), 0) for v in (x, y, z))
        wx, wy, wz = (np.where(acc, a - b, 0).astype(self.ft) for a, b in ((x, xf), (y, yf), (z, zf)))
        iv = zf.astype(np.int64) * (self.H * self.W) + yf.astype(np.int64) * self.W + xf.astype(np.int64)
        return (wx, wy, wz), iv

    def corner_index(self, iv, c, acc):
        return np.where(acc, iv + c[2] * (self.H * self.W) + c[1] * self.W + c[0], 0)


def _fac(wv, bit, one):
    return wv if bit else (one - wv)


def _psf_value(G, wf, q):
    one = G.ft(1)
    wx, wy, wz = wf
    val = np.zeros(G.nhw, G.ft)
    for c, qc in zip(CORNERS, q):
        val = val + _fac(wx, c[0], one) * _fac(wy, c[1], one) * _fac(wz, c[2], one) * qc
    return val


def adjoint64(transforms, psf, slices, slices_mask, vol_mask, vol_shape, res_slice, interp_psf, equalize, ft=np.float64):
    """The adjoint forward, CUDA semantics (slice_acq_cuda_kernel.cu:472-693): pass 1 the pixel's weight (vol_mask not
    consulted), pixels with weight < 0.5 dropped, pass 2 the contributions divided by the weight; equalize divides by the
    accumulated weight where it is > 0.  Returns vol, vol_weight (D,H,W) and pixel_weight (n,h,w)."""
    sl = np.asarray(slices, np.float32).astype(ft)
    n, h, w = sl.shape
    G = _Geometry(transforms, psf, (n, h, w), vol_shape, res_slice, ft)
    D, H, W = G.D, G.H, G.W
    vm = None if vol_mask is None else np.asarray(vol_mask, bool).reshape(-1)
    sm = np.ones((n, h, w), bool) if slices_mask is None else np.asarray(slices_mask, bool).reshape(n, h, w)
    one = ft(1)
    old = np.seterr(invalid="ignore", over="ignore", divide="ignore")
    try:
        weight = np.zeros((n, h, w), ft)
        for fx, fy, fz, pv in G.taps():
            x, y, z, acc = G.position(fx, fy, fz)
            if interp_psf:
                xr, yr, zr, _ = G.rounded(x, y, z, acc)
                _, accp, wf, q = G.psf_cell(xr, yr, zr, acc)
                weight = np.where(accp, weight + _psf_value(G, wf, q), weight)
            else:
                weight = np.where(acc, weight + pv, weight)
        live = sm & ~(weight < 0.5)
        wsafe = np.where(live, weight, 1)
        vol, vw = np.zeros(D * H * W, np.float64), np.zeros(D * H * W, np.float64)
        for fx, fy, fz, pv in G.taps():
            x, y, z, acc = G.position(fx, fy, fz)
            acc = acc & live
            if interp_psf:
                xr, yr, zr, iv = G.rounded(x, y, z, acc)
                _, accp, wf, q = G.psf_cell(xr, yr, zr, acc)
                pn = (_psf_value(G, wf, q) / wsafe).astype(ft)
                ok = accp if vm is None else (accp & vm[iv])
                np.add.at(vol, iv[ok], (pn * sl)[ok].astype(np.float64))
                np.add.at(vw, iv[ok], pn[ok].astype(np.float64))
            else:
                (wx, wy, wz), iv = G.cell(x, y, z, acc)
                pn = (pv / wsafe).astype(ft)
                for c in CORNERS:
                    ic = G.corner_index(iv, c, acc)
                    ok = acc if vm is None else (acc & vm[ic])
                    cw = (_fac(wx, c[0], one) * _fac(wy, c[1], one) * _fac(wz, c[2], one) * pn).astype(ft)
                    np.add.at(vol, ic[ok], (cw * sl)[ok].astype(np.float64))
                    np.add.at(vw, ic[ok], cw[ok].astype(np.float64))
        vol, vw = vol.astype(ft), vw.astype(ft)
        if equalize:
            m = vw > 0
            vol[m] = vol[m] / vw[m]
    finally:
        np.seterr(**old)
    return {"vol": vol.reshape(D, H, W), "vol_weight": vw.reshape(D, H, W), "pixel_weight": weight}


def equalized_grad(grad_vol, vol_weight, ft, state64=False):
    """g' of the rule; a new array, grad_vol is not modified.  In fp32 the comparison with and the division by 1e-3 are done in
    double (the reference's literal promotes), the division by the weight in fp32."""
    g = np.asarray(grad_vol, np.float32).astype(ft)
    w = np.asarray(vol_weight, np.float64 if state64 else np.float32).astype(ft)
    pos = w > 0
    low = pos & (w.astype(np.float64) < FLOOR)
    old = np.seterr(invalid="ignore", over="ignore", divide="ignore")
    try:
        out = np.where(low, (g.astype(np.float64) / FLOOR).astype(ft), np.where(pos, g / np.where(pos, w, 1), g))
    finally:
        np.seterr(**old)
    return out.astype(ft)


def _adjoint_backward(transforms, grad_vol, psf, slices, slices_mask, vol_mask, res_slice, interp_psf, equalize, vol,
                      vol_weight, ft, state64=False):
    f64 = np.float64
    sl = np.asarray(slices, np.float32).astype(ft)
    n, h, w = sl.shape
    gin = np.asarray(grad_vol, np.float32)
    G = _Geometry(transforms, psf, (n, h, w), gin.shape, res_slice, ft)
    D, H, W = G.D, G.H, G.W
    r = G.r
    vm = None if vol_mask is None else np.asarray(vol_mask, bool).reshape(-1)
    sm = np.ones((n, h, w), bool) if slices_mask is None else np.asarray(slices_mask, bool).reshape(n, h, w)
    if equalize:
        if vol is None or vol_weight is None:
            raise ValueError("equalize needs vol and vol_weight")
        gp = equalized_grad(gin, vol_weight, ft, state64).reshape(-1)
        vv = np.asarray(vol, np.float64 if state64 else np.float32).astype(ft).reshape(-1)
    else:
        gp = gin.astype(ft).reshape(-1)
        vv = None
    one = ft(1)
    INF = np.inf
    kinds = {k: np.full((n, h, w), INF) for k in ("bounds", "grid", "psf_bounds", "psf_grid")}

    def note(kind, d, where):
        kinds[kind] = np.minimum(kinds[kind], np.where(where & np.isfinite(d), d, INF))

    def sval(ic, ok):
        """s of the rule at flat voxel index ic: (slice - vol) * g' under equalize, slice * g' otherwise; 0 where not ok"""
        a = (sl - vv[ic]) if equalize else sl
        return np.where(ok, a * gp[ic], 0).astype(ft)

    old = np.seterr(invalid="ignore", over="ignore", divide="ignore")
    try:
        val, weight = np.zeros((n, h, w), ft), np.zeros((n, h, w), ft)
        mval, kval = np.zeros((n, h, w), f64), np.zeros((n, h, w), np.int64)
        g = [np.zeros((n, h, w), ft) for _ in range(12)]
        mg = [np.zeros((n, h, w), f64) for _ in range(12)]
        kg = [np.zeros((n, h, w), np.int64) for _ in range(12)]

        def add_g(k, term, mag, count, where):
            g[k] = np.where(where, g[k] + term, g[k]).astype(ft)
            mg[k] += np.where(where, mag, 0)
            kg[k] += np.where(where, count, 0)

        for fx, fy, fz, pv in G.taps():
            x, y, z, acc0 = G.position(fx, fy, fz)
            for v, hi in ((x, W - 1), (y, H - 1), (z, D - 1)):
                v64 = v.astype(f64)
                note("bounds", np.minimum(np.abs(v64), np.abs(v64 - hi)), np.ones_like(acc0))
                frac = v64 - np.floor(v64)
                note("grid", np.abs(frac - 0.5) if interp_psf else np.minimum(frac, 1 - frac), acc0)
            acc = acc0 & sm
            if interp_psf:
                xr, yr, zr, iv = G.rounded(x, y, z, acc0)
                pc, accp0, _, _ = G.psf_cell(xr, yr, zr, acc0)
                for v, hi in zip(pc, (G.pw - 1, G.ph - 1, G.pd - 1)):
                    v64 = v.astype(f64)
                    note("psf_bounds", np.minimum(np.abs(v64), np.abs(v64 - hi)), acc0)
                    frac = v64 - np.floor(v64)
                    note("psf_grid", np.minimum(frac, 1 - frac), accp0)
                if vm is not None:
                    acc = acc & vm[iv]  # QUIRK: before the weight
                _, ok, (wx, wy, wz), q = G.psf_cell(xr, yr, zr, acc)
                pp = _psf_value(G, (wx, wy, wz), q)
                gv = np.where(ok, gp[np.where(ok, iv, 0)], 0).astype(ft)
                val = np.where(ok, val + pp * gv, val).astype(ft)
                weight = np.where(ok, weight + pp, weight).astype(ft)
                mc = np.zeros((n, h, w), f64)
                for c, qc in zip(CORNERS, q):
                    mc = mc + np.abs((_fac(wx, c[0], one) * _fac(wy, c[1], one) * _fac(wz, c[2], one) * qc).astype(f64))
                mval += np.where(ok, mc * np.abs(gv.astype(f64)), 0)
                kval += ok * 8
                dx, dy, dz = (np.zeros((n, h, w), ft) for _ in range(3))
                mx, my, mz = (np.zeros((n, h, w), f64) for _ in range(3))
                for c, qc in zip(CORNERS, q):
                    ax = _fac(wy, c[1], one) * _fac(wz, c[2], one) * qc
                    ay = _fac(wx, c[0], one) * _fac(wz, c[2], one) * qc
                    az = _fac(wx, c[0], one) * _fac(wy, c[1], one) * qc
                    dx = dx + ax if c[0] else dx - ax
                    dy = dy + ay if c[1] else dy - ay
                    dz = dz + az if c[2] else dz - az
                    mx, my, mz = mx + np.abs(ax), my + np.abs(ay), mz + np.abs(az)
                t = ((((sl - vv[np.where(ok, iv, 0)]) if equalize else sl) * gv)).astype(ft)
                t = np.where(ok, t, 0).astype(ft)
                dx, dy, dz = dx * t, dy * t, dz * t
                mx, my, mz = (m * np.abs(t.astype(f64)) for m in (mx, my, mz))
                lev = (xr - ft((W - 1) * 0.5), yr - ft((H - 1) * 0.5), zr - ft((D - 1) * 0.5))
                cnt = ok.astype(np.int64) * 8
                for a in range(3):
                    for b, (d, m) in enumerate(((dx, mx), (dy, my), (dz, mz))):
                        add_g(4 * a + b, d * lev[a], m * np.abs(lev[a].astype(f64)), cnt, ok)
                for b, (d, m) in enumerate(((dx, mx), (dy, my), (dz, mz))):
                    add_g(4 * b + 3, -d, m, cnt, ok)
            else:
                (wx, wy, wz), iv = G.cell(x, y, z, acc)
                val_ = np.zeros((n, h, w), ft)
                mv_ = np.zeros((n, h, w), f64)
                dx, dy, dz = (np.zeros((n, h, w), ft) for _ in range(3))
                mx, my, mz = (np.zeros((n, h, w), f64) for _ in range(3))
                cnt = np.zeros((n, h, w), np.int64)
                for c in CORNERS:
                    ic = G.corner_index(iv, c, acc)
                    ok = acc if vm is None else (acc & vm[ic])
                    term = _fac(wx, c[0], one) * _fac(wy, c[1], one) * _fac(wz, c[2], one) * gp[ic]
                    val_ = np.where(ok, val_ + term, val_).astype(ft)
                    mv_ += np.where(ok, np.abs(term.astype(f64)), 0)
                    t = sval(ic, ok)
                    ax = _fac(wy, c[1], one) * _fac(wz, c[2], one) * t
                    ay = _fac(wx, c[0], one) * _fac(wz, c[2], one) * t
                    az = _fac(wx, c[0], one) * _fac(wy, c[1], one) * t
                    dx = dx + ax if c[0] else dx - ax
                    dy = dy + ay if c[1] else dy - ay
                    dz = dz + az if c[2] else dz - az
                    mx, my, mz = mx + np.abs(ax), my + np.abs(ay), mz + np.abs(az)
                    cnt += ok
                val = np.where(acc, val + pv * val_, val).astype(ft)
                weight = np.where(acc, weight + pv, weight).astype(ft)
                mval += np.where(acc, abs(f64(pv)) * mv_, 0)
                kval += cnt
                dx, dy, dz = dx * pv, dy * pv, dz * pv
                mx, my, mz = (m.astype(f64) * abs(f64(pv)) for m in (mx, my, mz))
                lev = (G._x + fx, G._y + fy, G._z + fz)
                for a, (d, m) in enumerate(((dx, mx), (dy, my), (dz, mz))):
                    for b in range(3):
                        add_g(4 * a + b, d * lev[b], m * np.abs(lev[b].astype(f64)), cnt, acc)
                for b in range(3):
                    term = dx * r(0, b) + dy * r(1, b) + dz * r(2, b)
                    mag = mx * np.abs(r(0, b).astype(f64)) + my * np.abs(r(1, b).astype(f64)) + mz * np.abs(r(2, b).astype(f64))
                    add_g(4 * b + 3, term, mag, 3 * cnt, acc)

        kept = sm & (weight > 0)  # QUIRK: > 0, the forward drops < 0.5
        wsafe = np.where(kept, weight, 1)
        aw = np.abs(wsafe.astype(f64))
        gsl = np.where(kept, val / wsafe, 0).astype(f64)
        s_sl = np.where(kept, mval / aw, 0)
        k_sl = np.where(kept, kval, 0)
        gtr, s_tr, k_tr = np.zeros((n, 12), f64), np.zeros((n, 12), f64), np.zeros((n, 12), np.int64)
        for k in range(12):
            gtr[:, k] = np.where(kept, (g[k] / wsafe).astype(ft), 0).astype(f64).sum((1, 2))
            s_tr[:, k] = np.where(kept, mg[k] / aw, 0).sum((1, 2))
            k_tr[:, k] = np.where(kept, kg[k], 0).sum((1, 2))
        margin = np.full((n, h, w), INF)
        for kname in kinds:
            margin = np.minimum(margin, kinds[kname])
    finally:
        np.seterr(**old)
    dist = {k: float(np.where(sm, v, np.inf).min()) if sm.any() else float("inf") for k, v in kinds.items()}
    return {"grad_slices": gsl, "grad_transforms": gtr, "k_sl": k_sl, "s_sl": s_sl, "k_tr": k_tr, "s_tr": s_tr, "dist": dist,
            "pixel_margin": margin, "pixel_weight": weight.astype(f64)}


def adjoint_backward64(transforms, grad_vol, psf, slices, slices_mask, vol_mask, res_slice, interp_psf, equalize=False, vol=None,
                       vol_weight=None, state64=False):
    """state64: take `vol` and `vol_weight` as float64 (the float64 adjoint's own state) instead of rounding them to fp32, which
    is what a kernel is handed: for comparisons with differences of the float64 adjoint."""
    return _adjoint_backward(transforms, grad_vol, psf, slices, slices_mask, vol_mask, res_slice, interp_psf, equalize, vol,
                             vol_weight, np.float64, state64)


def adjoint_backward32(transforms, grad_vol, psf, slices, slices_mask, vol_mask, res_slice, interp_psf, equalize=False, vol=None,
                       vol_weight=None):
    return _adjoint_backward(transforms, grad_vol, psf, slices, slices_mask, vol_mask, res_slice, interp_psf, equalize, vol,
                             vol_weight, np.float32)
