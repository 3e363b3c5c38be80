"""Two CPU restatements of the backward of the slice-acquisition forward operator (include/fsg_hip.h,
fsg_slice_acq_backward_f32).  Test infrastructure, numpy only.

    backward64(...)   every operation in float64 from the fp32 inputs: the yardstick.
    backward32(...)   the same formula with every operation in np.float32, in the kernel's operation order (the per-pixel
                      weight and the per-tap derivative sums included); only the sums over taps and pixels that the kernel
                      reduces or scatters (grad_vol cells, the 12 transform sums) are carried in float64.  The difference
                      to backward64 is what fp32 costs the formula itself, whatever the summation order.

The rule, restated (quirks of the reference named):
  * a pixel outside slices_mask or with grad_slices == 0 contributes nothing;
  * pass 1: weight = sum over the taps with 0 <= p < size-1 on every axis of the PSF value -- raw (LINEAR) or re-interpolated
    at the rounded voxel, taps whose PSF coordinate is outside [0, psf_size-1) skipped (NEAREST_PSF).  QUIRK: vol_mask is not
    consulted, although the forward's weight leaves masked voxels out;
  * QUIRK: weight == 0 ends the pixel (the forward tests weight > 0, so a negative weight goes on here);
    gs = grad_slices / weight;
  * pass 2: grad_vol and the 12 transform sums over the unmasked terms, the weight held constant.
Every range test is in accepting form (`x >= 0 and x < hi`): a NaN or Inf coordinate fails it and the tap is skipped.

Both return a dict:
    grad_vol (D,H,W) f64, grad_transforms (n,12) f64
    k_vol, s_vol / k_tr, s_tr     number of finest-grain terms summed into each output element and the sum of their
                                  magnitudes (a term: one corner's product, before any cancellation)
    dist                          smallest distance, over the pixels that contribute, of a tap coordinate to a decision point:
                                  'bounds' (0 and size-1, every tap), 'grid' (an integer in LINEAR, a half-integer in
                                  NEAREST_PSF, accepted taps), 'psf_bounds' / 'psf_grid' (NEAREST_PSF: the PSF coordinate
                                  against 0 / psf_size-1 and against an integer)
    pixel_margin (n,h,w)          the same minimum per pixel over all four kinds, for EVERY pixel (inf where it has no tap)
"""
import numpy as np

CORNERS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))  # (a,b,c) on x,y,z; kernel order


def _round_away(x):
    """round half away from zero for x >= 0, exact in any float type"""
    f = np.floor(x)
    return f + ((x - f) >= 0.5).astype(x.dtype)


def _backward(transforms, vol, vol_mask, psf, grad_slices, slices_mask, res_slice, interp_psf, ft):
    f64 = np.float64
    tr32 = np.asarray(transforms, np.float32).reshape(-1, 3, 4)
    T = tr32.astype(ft)
    vol = np.asarray(vol, np.float32).astype(ft)
    psf = np.asarray(psf, np.float32).astype(ft)
    gsl = np.asarray(grad_slices, np.float32).astype(ft)
    res = f64(np.float32(res_slice))
    D, H, W = vol.shape
    pd, ph, pw = psf.shape
    n, h, w = gsl.shape
    vm = None if vol_mask is None else np.asarray(vol_mask, bool)
    sm = np.ones((n, h, w), bool) if slices_mask is None else np.asarray(slices_mask, bool).reshape(n, h, w)
    r = lambda i, j: T[:, i, j][:, None, None]  # noqa: E731
    old = np.seterr(invalid="ignore", over="ignore", divide="ignore")
    try:
        # pixel in slice axes (formed in double, kept in ft), centre in voxel coordinates
        ixs = np.arange(w, dtype=f64)[None, None, :]
        iys = np.arange(h, dtype=f64)[None, :, None]
        t64 = T.astype(f64)
        _x = np.broadcast_to(((ixs - (w - 1) / 2.0) * res + t64[:, 0, 3, None, None]).astype(ft), (n, h, w))
        _y = np.broadcast_to(((iys - (h - 1) / 2.0) * res + t64[:, 1, 3, None, None]).astype(ft), (n, h, w))
        _z = np.broadcast_to(T[:, 2, 3, None, None], (n, h, w))
        xc = ((r(0, 0) * _x + r(0, 1) * _y + r(0, 2) * _z).astype(f64) + (W - 1) / 2.0).astype(ft)
        yc = ((r(1, 0) * _x + r(1, 1) * _y + r(1, 2) * _z).astype(f64) + (H - 1) / 2.0).astype(ft)
        zc = ((r(2, 0) * _x + r(2, 1) * _y + r(2, 2) * _z).astype(f64) + (D - 1) / 2.0).astype(ft)
        one = ft(1)

        def taps():
            for kz in range(pd):
                for ky in range(ph):
                    for kx in range(pw):
                        pv = psf[kz, ky, kx]
                        if pv != 0:
                            yield ft(kx - pw // 2), ft(ky - ph // 2), ft(kz - pd // 2), pv

        def position(fx, fy, fz):
            x = xc + r(0, 0) * fx + r(0, 1) * fy + r(0, 2) * fz
            y = yc + r(1, 0) * fx + r(1, 1) * fy + r(1, 2) * fz
            z = zc + r(2, 0) * fx + r(2, 1) * fy + r(2, 2) * fz
            acc = (x >= 0) & (y >= 0) & (z >= 0) & (x < W - 1) & (y < H - 1) & (z < D - 1)
            return x, y, z, acc

        def psf_cell(xr, yr, zr, acc):
            """NEAREST_PSF: PSF coordinate of the rounded voxel -> accepted, fractions, the 8 PSF values (kernel order)"""
            ex, ey, ez = xr - xc, yr - yc, zr - zc
            xp = ((r(0, 0) * ex + r(1, 0) * ey + r(2, 0) * ez).astype(f64) + (pw - 1) / 2.0).astype(ft)
            yp = ((r(0, 1) * ex + r(1, 1) * ey + r(2, 1) * ez).astype(f64) + (ph - 1) / 2.0).astype(ft)
            zp = ((r(0, 2) * ex + r(1, 2) * ey + r(2, 2) * ez).astype(f64) + (pd - 1) / 2.0).astype(ft)
            accp = acc & (xp >= 0) & (yp >= 0) & (zp >= 0) & (xp < pw - 1) & (yp < ph - 1) & (zp < pd - 1)
            xf, yf, zf = (np.where(accp, np.floor(v), 0) for v in (xp, yp, zp))
            wx, wy, wz = (np.where(accp, a - b, 0).astype(ft) for a, b in ((xp, xf), (yp, yf), (zp, zf)))
            xi, yi, zi = xf.astype(np.int64), yf.astype(np.int64), zf.astype(np.int64)
            pp = np.pad(psf, ((0, 1), (0, 1), (0, 1)))
            q = [pp[zi + c[2], yi + c[1], xi + c[0]] for c in CORNERS]
            return (xp, yp, zp), accp, (wx, wy, wz), q

        def fac(wv, bit):
            return wv if bit else (one - wv)

        # ---- decision distances ----
        INF = np.inf
        margin = np.full((n, h, w), INF)
        kinds = {"bounds": np.full((n, h, w), INF), "grid": np.full((n, h, w), INF),
                 "psf_bounds": np.full((n, h, w), INF), "psf_grid": np.full((n, h, w), INF)}

        def note(kind, d, where):
            d = np.where(where & np.isfinite(d), d, INF)
            kinds[kind] = np.minimum(kinds[kind], d)

        # ---- pass 1 ----
        weight = np.zeros((n, h, w), ft)
        for fx, fy, fz, pv in taps():
            x, y, z, acc = position(fx, fy, fz)
            for v, hi in ((x, W - 1), (y, H - 1), (z, D - 1)):
                v64 = v.astype(f64)
                note("bounds", np.minimum(np.abs(v64), np.abs(v64 - hi)), np.ones_like(acc))
                frac = v64 - np.floor(v64)
                note("grid", np.abs(frac - 0.5) if interp_psf else np.minimum(frac, 1 - frac), acc)
            if interp_psf:
                xr, yr, zr = (np.where(acc, _round_away(np.where(acc, v, 0)), 0).astype(ft) for v in (x, y, z))
                pc, accp, (wx, wy, wz), q = psf_cell(xr, yr, zr, acc)
                for v, hi in zip(pc, (pw - 1, ph - 1, pd - 1)):
                    v64 = v.astype(f64)
                    note("psf_bounds", np.minimum(np.abs(v64), np.abs(v64 - hi)), acc)
                    frac = v64 - np.floor(v64)
                    note("psf_grid", np.minimum(frac, 1 - frac), accp)
                val = np.zeros((n, h, w), ft)
                for c, qc in zip(CORNERS, q):
                    val = val + fac(wx, c[0]) * fac(wy, c[1]) * fac(wz, c[2]) * qc
                weight = np.where(accp, weight + val, weight)
            else:
                weight = np.where(acc, weight + pv, weight)
        for kname in kinds:
            margin = np.minimum(margin, kinds[kname])

        active = sm & (gsl != 0)
        live = active & (weight != 0)
        gs = np.where(live, gsl / np.where(live, weight, 1), 0).astype(ft)

        # ---- pass 2 ----
        gvol, kvol, svol = np.zeros(D * H * W, f64), np.zeros(D * H * W, np.int64), np.zeros(D * H * W, f64)
        gtr, ktr, s_tr = np.zeros((n, 12), f64), np.zeros((n, 12), np.int64), np.zeros((n, 12), f64)

        def scatter(idx, ok, contrib):
            np.add.at(gvol, idx[ok], contrib[ok].astype(f64))
            np.add.at(kvol, idx[ok], 1)
            np.add.at(svol, idx[ok], np.abs(contrib[ok].astype(f64)))

        def add_tr(k, term, mag, count):
            """term (n,h,w) ft: what the kernel adds to sum k for this tap; mag: sum of the magnitudes of its finest terms"""
            gtr[:, k] += term.astype(f64).sum((1, 2))
            s_tr[:, k] += mag.astype(f64).sum((1, 2))
            ktr[:, k] += count.sum((1, 2))

        for fx, fy, fz, pv in taps():
            x, y, z, acc = position(fx, fy, fz)
            acc = acc & live
            if interp_psf:
                xr, yr, zr = (np.where(acc, _round_away(np.where(acc, v, 0)), 0).astype(ft) for v in (x, y, z))
                _pc, accp, (wx, wy, wz), q = psf_cell(xr, yr, zr, acc)
                iv = zr.astype(np.int64) * (H * W) + yr.astype(np.int64) * W + xr.astype(np.int64)
                ok = accp if vm is None else (accp & vm.reshape(-1)[iv])
                val = np.zeros((n, h, w), ft)
                for c, qc in zip(CORNERS, q):
                    val = val + fac(wx, c[0]) * fac(wy, c[1]) * fac(wz, c[2]) * qc
                scatter(iv, ok, val * gs)
                dx, dy, dz = (np.zeros((n, h, w), ft) for _ in range(3))
                mx, my, mz = (np.zeros((n, h, w), f64) for _ in range(3))
                for c, qc in zip(CORNERS, q):
                    ax, ay, az = fac(wy, c[1]) * fac(wz, c[2]) * qc, fac(wx, c[0]) * fac(wz, c[2]) * qc, fac(wx, c[0]) * fac(wy, c[1]) * qc
                    dx = dx + ax if c[0] else dx - ax
                    dy = dy + ay if c[1] else dy - ay
                    dz = dz + az if c[2] else dz - az
                    mx, my, mz = mx + np.abs(ax), my + np.abs(ay), mz + np.abs(az)
                t = np.where(ok, gs * vol.reshape(-1)[iv], 0).astype(ft)
                dx, dy, dz = dx * t, dy * t, dz * t
                mx, my, mz = (m * np.abs(t.astype(f64)) for m in (mx, my, mz))
                lev = (xr - ft((W - 1) * 0.5), yr - ft((H - 1) * 0.5), zr - ft((D - 1) * 0.5))
                cnt = ok.astype(np.int64) * 8
                for a in range(3):
                    for b, (d, m) in enumerate(((dx, mx), (dy, my), (dz, mz))):
                        add_tr(4 * a + b, np.where(ok, d * lev[a], 0), np.where(ok, m * np.abs(lev[a].astype(f64)), 0), cnt)
                for b, (d, m) in enumerate(((dx, mx), (dy, my), (dz, mz))):
                    add_tr(4 * b + 3, np.where(ok, -d, 0), np.where(ok, m, 0), cnt)
            else:
                xf, yf, zf = (np.where(acc, np.floor(v), 0) for v in (x, y, z))
                wx, wy, wz = (np.where(acc, a - b, 0).astype(ft) for a, b in ((x, xf), (y, yf), (z, zf)))
                iv = zf.astype(np.int64) * (H * W) + yf.astype(np.int64) * W + xf.astype(np.int64)
                pg = (pv * gs).astype(ft)
                dx, dy, dz = (np.zeros((n, h, w), ft) for _ in range(3))
                mx, my, mz = (np.zeros((n, h, w), f64) for _ in range(3))
                cnt = np.zeros((n, h, w), np.int64)
                for c in CORNERS:
                    ic = iv + c[2] * (H * W) + c[1] * W + c[0]
                    ic = np.where(acc, ic, 0)
                    ok = acc if vm is None else (acc & vm.reshape(-1)[ic])
                    scatter(ic, ok, fac(wx, c[0]) * fac(wy, c[1]) * fac(wz, c[2]) * pg)
                    t = np.where(ok, pg * vol.reshape(-1)[ic], 0).astype(ft)
                    ax, ay, az = fac(wy, c[1]) * fac(wz, c[2]) * t, fac(wx, c[0]) * fac(wz, c[2]) * t, fac(wx, c[0]) * fac(wy, c[1]) * t
                    dx = dx + ax if c[0] else dx - ax
                    dy = dy + ay if c[1] else dy - ay
                    dz = dz + az if c[2] else dz - az
                    mx, my, mz = mx + np.abs(ax), my + np.abs(ay), mz + np.abs(az)
                    cnt += ok
                lev = (_x + fx, _y + fy, _z + fz)
                for a, (d, m) in enumerate(((dx, mx), (dy, my), (dz, mz))):
                    for b in range(3):
                        add_tr(4 * a + b, np.where(acc, d * lev[b], 0), np.where(acc, m * np.abs(lev[b].astype(f64)), 0), cnt)
                for b in range(3):
                    term = dx * r(0, b) + dy * r(1, b) + dz * r(2, b)
                    mag = mx * np.abs(r(0, b).astype(f64)) + my * np.abs(r(1, b).astype(f64)) + mz * np.abs(r(2, b).astype(f64))
                    add_tr(4 * b + 3, np.where(acc, term, 0), np.where(acc, mag, 0), 3 * cnt)
    finally:
        np.seterr(**old)
    dist = {k: float(np.where(active, v, np.inf).min()) if active.any() else float("inf") for k, v in kinds.items()}
    return {"grad_vol": gvol.reshape(D, H, W), "grad_transforms": gtr, "k_vol": kvol.reshape(D, H, W),
            "s_vol": svol.reshape(D, H, W), "k_tr": ktr, "s_tr": s_tr, "dist": dist, "pixel_margin": margin}


def backward64(transforms, vol, vol_mask, psf, grad_slices, slices_mask, res_slice, interp_psf):
    return _backward(transforms, vol, vol_mask, psf, grad_slices, slices_mask, res_slice, interp_psf, np.float64)


def backward32(transforms, vol, vol_mask, psf, grad_slices, slices_mask, res_slice, interp_psf):
    return _backward(transforms, vol, vol_mask, psf, grad_slices, slices_mask, res_slice, interp_psf, np.float32)
