"""CPU restatement of the per-slice Levenberg-Marquardt registration `svort.svr` (the rule of the two
kernels is in include/fsg_hip.h, fsg_svr_*).  Test infrastructure, numpy only; `ft` is the type every per-pixel operation is
done in, as in tests/util_srr64.

    pixels(...)            per pixel: weight, whether it takes part, s, e, J12 (the twelve sums of the backward for gs = 1 / weight),
                           J6 = J12 projected through jac, the 30 terms, and for the exact-geometry bound the number of
                           finest-grain terms and the sum of their magnitudes behind s and behind every J6.
    stats64(terms)         the 32 slots per slice, the pixels added in float64 (any order: the yardstick).
    stats_device(terms32)  the 32 slots in the kernel's order: per 16x16 tile the 64 lanes of a wave folded by v[i] += v[i + o],
                           o = 32..1, in float32; the four waves added in wave order in float32; the tiles of a slice added in
                           float64 in tile-index order (tile = tile_y * tiles_x + tile_x) from +0.0.
    update(...)            one call of fsg_svr_update_f32 on a dict of the state, float64 scalars, + - * / only (the
                           factorisation is A = L D L^T in the header's operation order).  theta_dtype float32 is the device;
                           float64 keeps the poses unrounded for the float64 solver.
    solve(...)             the whole loop: axisangle2mat, the Jacobian by axisangle2mat_backward of the 12 one-hot matrices,
                           pixels + stats, update.  mutant: "delta_sign", "lambda_swapped", "identity_damping".

Capability case (`capability_case`): util_sa_backward_cases.fit_case's phantom and PSF, five 9 x 9 slices at res_slice 1.0 at
the case's true poses, starts perturbed by default_rng(5).uniform(-0.03, 0.03, (5,3)) rad and .uniform(-0.75, 0.75, (5,3)) voxels.
Every footprint stays inside the volume, so the pixel set does not change with the pose.  The figures measured on the CPU with
n_iter = 12 (python -m tests.util_svr64 prints them) are beside the CAP_* constants below.
"""
import numpy as np

from tests import util_sa_backward_cases as BC
from tests import util_transform_convert64 as TC
from tests.util_sa_adjoint_backward64 import _Geometry
from tests.util_sa_backward64 import CORNERS

F32, F64 = np.float32, np.float64
SLOTS, TERMS, TILE = 32, 30, 16
PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]  # slot order of H's upper triangle
GROUPS = {"H": slice(0, 21), "g": slice(21, 27), "cost": slice(27, 29)}


def _fac(wv, bit, one):
    return wv if bit else (one - wv)


def pixels(tr, jac, vol, psf, y, sm, sw, res, min_weight, ft=F64):
    tr = np.asarray(tr, F32).reshape(-1, 3, 4)
    n = tr.shape[0]
    vol = np.asarray(vol, F32).astype(ft)
    y = np.asarray(y, F32).astype(ft)
    _, h, w = y.shape
    jac = np.asarray(jac).reshape(n, 12, 6).astype(ft)  # (a float64 jac stays float64 under ft = float64)
    G = _Geometry(tr, psf, (n, h, w), vol.shape, res, ft)
    flat = vol.reshape(-1)
    one, zero = ft(1), ft(0)
    sm = np.ones((n, h, w), bool) if sm is None else np.asarray(sm, bool).reshape(n, h, w)
    wgt = np.ones((n, h, w), ft) if sw is None else np.asarray(sw, F32).astype(ft).reshape(n, h, w)
    old = np.seterr(invalid="ignore", over="ignore", divide="ignore")
    try:
        weight = np.zeros((n, h, w), ft)
        for fx, fy, fz, pv in G.taps():
            _, _, _, acc = G.position(fx, fy, fz)
            weight = np.where(acc, weight + pv, weight).astype(ft)
        part = sm & (weight > 0) & (weight >= ft(F32(min_weight)))
        wsafe = np.where(part, weight, one)
        gs = (one / wsafe).astype(ft)
        val = np.zeros((n, h, w), ft)
        g = [np.zeros((n, h, w), ft) for _ in range(12)]
        mag_v, cnt_v = np.zeros((n, h, w), F64), np.zeros((n, h, w), np.int64)
        mag = [np.zeros((n, h, w), F64) for _ in range(12)]
        cnt = [np.zeros((n, h, w), np.int64) for _ in range(12)]
        r = G.r
        for fx, fy, fz, pv in G.taps():
            x, yy, z, acc = G.position(fx, fy, fz)
            acc = acc & part
            (wx, wy, wz), iv = G.cell(x, yy, z, acc)
            pg = (pv * gs).astype(ft)
            tri = np.zeros((n, h, w), ft)
            dx, dy, dz = (np.zeros((n, h, w), ft) for _ in range(3))
            mx, my, mz = (np.zeros((n, h, w), F64) for _ in range(3))
            mt = np.zeros((n, h, w), F64)
            for c in CORNERS:
                cv = np.where(acc, flat[G.corner_index(iv, c, acc)], zero).astype(ft)
                fxw, fyw, fzw = _fac(wx, c[0], one), _fac(wy, c[1], one), _fac(wz, c[2], one)
                term = fxw * fyw * fzw * cv
                tri = tri + term
                mt = mt + np.abs(term.astype(F64))
                t = pg * cv
                ax, ay, az = fyw * fzw * t, fxw * fzw * t, fxw * fyw * t
                dx = dx + ax if c[0] else dx - ax
                dy = dy + ay if c[1] else dy - ay
                dz = dz + az if c[2] else dz - az
                mx, my, mz = mx + np.abs(ax.astype(F64)), my + np.abs(ay.astype(F64)), mz + np.abs(az.astype(F64))
            val = np.where(acc, val + pv * tri, val).astype(ft)
            mag_v = mag_v + np.where(acc, abs(float(pv)) * mt, 0)
            cnt_v = cnt_v + 8 * acc
            lev = (G._x + fx, G._y + fy, G._z + fz)
            for a, (d, m) in enumerate(((dx, mx), (dy, my), (dz, mz))):
                for b in range(3):
                    g[4 * a + b] = np.where(acc, g[4 * a + b] + d * lev[b], g[4 * a + b]).astype(ft)
                    mag[4 * a + b] = mag[4 * a + b] + np.where(acc, m * np.abs(lev[b].astype(F64)), 0)
                    cnt[4 * a + b] = cnt[4 * a + b] + 8 * acc
            for b in range(3):
                term = dx * r(0, b) + dy * r(1, b) + dz * r(2, b)
                g[4 * b + 3] = np.where(acc, g[4 * b + 3] + term, g[4 * b + 3]).astype(ft)
                mg = mx * np.abs(r(0, b).astype(F64)) + my * np.abs(r(1, b).astype(F64)) + mz * np.abs(r(2, b).astype(F64))
                mag[4 * b + 3] = mag[4 * b + 3] + np.where(acc, mg, 0)
                cnt[4 * b + 3] = cnt[4 * b + 3] + 24 * acc
        s = np.where(part, val / wsafe, zero).astype(ft)
        e = np.where(part, s - y, zero).astype(ft)
        we = (wgt * e).astype(ft)
        J6, M6, K6 = [], [], []
        for a in range(6):
            acc6, m6, k6 = np.zeros((n, h, w), ft), np.zeros((n, h, w), F64), np.zeros((n, h, w), np.int64)
            for k in range(12):
                ja = jac[:, k, a][:, None, None]
                acc6 = acc6 + ja * g[k]
                m6 = m6 + np.abs(ja.astype(F64)) * mag[k]
                k6 = k6 + (ja != 0) * cnt[k]
            J6.append(acc6.astype(ft)), M6.append(m6), K6.append(k6)
        terms = np.zeros((n, h, w, TERMS), ft)
        for o, (a, b) in enumerate(PAIRS):
            terms[..., o] = (wgt * J6[a]).astype(ft) * J6[b]
        for a in range(6):
            terms[..., 21 + a] = we * J6[a]
        terms[..., 27] = we * e
        terms[..., 28] = wgt
        terms[..., 29] = one
        terms = np.where(part[..., None], terms, zero).astype(ft)
    finally:
        np.seterr(**old)
    m_e = mag_v / wsafe.astype(F64) + np.abs(y.astype(F64))  # magnitude behind e = s - y
    return dict(weight=weight, part=part, s=s, e=e, J12=np.stack(g, -1), J6=np.stack(J6, -1), terms=terms, w=wgt,
                M6=np.stack(M6, -1), K6=np.stack(K6, -1), M_e=m_e, K_e=cnt_v + 2)


def stats64(terms):
    n = terms.shape[0]
    out = np.zeros((n, SLOTS), F64)
    out[:, :TERMS] = terms.astype(F64).reshape(n, -1, TERMS).sum(1)
    return out


def stats_device(terms32):
    t = np.asarray(terms32, F32)
    n, h, w, _ = t.shape
    ty, tx = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
    pad = np.zeros((n, ty * TILE, tx * TILE, TERMS), F32)
    pad[:, :h, :w] = t
    out = np.zeros((n, SLOTS), F64)
    for j in range(ty):  # tile = j * tx + i: increasing in this loop nest
        for i in range(tx):
            v = pad[:, j * TILE:(j + 1) * TILE, i * TILE:(i + 1) * TILE].reshape(n, 4, 64, TERMS)  # thread = y * 16 + x
            for o in (32, 16, 8, 4, 2, 1):
                v = v[:, :, :o] + v[:, :, o:2 * o]
            v = v[:, :, 0]
            part = ((v[:, 0] + v[:, 1]) + v[:, 2]) + v[:, 3]
            out[:, :TERMS] = out[:, :TERMS] + part.astype(F64)
    return out


def bounds(p):
    """(K, S) per slice and slot for the exact-geometry bound (K + 16) * 2^-24 * S.  A term of slot H_ab is w * J6[a] * J6[b]:
    each factor is a sum of K6 finest-grain products (jac entry * corner derivative * lever) of total magnitude M6, formed
    with at most 8 roundings per product; the two factors multiply (2 roundings) and the m pixels add.  So K = the largest
    K6[a] + K6[b] over the pixels + m + 4 and S = sum over the pixels of w M6[a] M6[b].  g_a: e = s - y has K_e terms of
    magnitude M_e.  sum w e^2 likewise; sum w and m are sums of exact values."""
    part, wv = p["part"], p["w"].astype(F64)
    n = part.shape[0]
    m = part.reshape(n, -1).sum(1)
    K6 = np.where(part[..., None], p["K6"], 0).reshape(n, -1, 6).max(1)
    Ke = np.where(part, p["K_e"], 0).reshape(n, -1).max(1)
    M6 = np.where(part[..., None], p["M6"], 0)
    Me = np.where(part, p["M_e"], 0)
    K, S = np.zeros((n, SLOTS)), np.zeros((n, SLOTS))
    for o, (a, b) in enumerate(PAIRS):
        K[:, o] = K6[:, a] + K6[:, b] + m + 4
        S[:, o] = (wv * M6[..., a] * M6[..., b]).reshape(n, -1).sum(1)
    for a in range(6):
        K[:, 21 + a] = Ke + K6[:, a] + m + 4
        S[:, 21 + a] = (wv * Me * M6[..., a]).reshape(n, -1).sum(1)
    K[:, 27], S[:, 27] = 2 * Ke + m + 4, (wv * Me * Me).reshape(n, -1).sum(1)
    K[:, 28], S[:, 28] = m, np.where(part, wv, 0).reshape(n, -1).sum(1)
    K[:, 29], S[:, 29] = m, m
    return K, S


# ---- the update ---------------------------------------------------------------------------------------------------------------
OPTS = dict(lambda0=1e-3, factor=10.0, lambda_min=1e-9, lambda_max=1e10, min_overlap=0.5, tol=0.0)


def new_state(n, n_iter, theta_dtype=F32):
    s = n_iter + 1
    return dict(n=n, n_iter=n_iter, stats_cur=np.zeros((n, SLOTS)), lam=np.zeros(n), m0=np.zeros(n), theta_cur=np.zeros((n, 6), theta_dtype),
                frozen_now=np.zeros(n, np.int32), cost=np.zeros((s, n)), lambda_hist=np.zeros((s, n)),
                accepted=np.zeros((s, n), np.int32), frozen=np.zeros((s, n), np.int32))


def step(cur, lam, mutant=None):
    """delta and whether a pivot failed, from one slice's 32 sums: A = H + lam diag(H), L D L^T, delta = -A^-1 g."""
    A = np.zeros((6, 6))
    for o, (a, b) in enumerate(PAIRS):
        A[a, b] = A[b, a] = cur[o]
    b = np.array(cur[21:27], F64)
    for a in range(6):
        live = A[a, a] != 0.0
        damped = A[a, a] + lam * (F64(1.0) if mutant == "identity_damping" else A[a, a])
        if not live:
            A[a, :] = 0.0
            A[:, a] = 0.0
            b[a] = 0.0
        A[a, a] = damped if live else 1.0
    bad = False
    with np.errstate(all="ignore"):
        for j in range(6):
            dj = A[j, j]
            for p in range(j):
                dj = dj - A[j, p] * A[j, p] * A[p, p]
            bad = bad or not (dj > 0.0)
            A[j, j] = dj
            for r in range(j + 1, 6):
                v = A[r, j]
                for p in range(j):
                    v = v - A[r, p] * A[j, p] * A[p, p]
                A[r, j] = v / dj
        z = np.zeros(6)
        for r in range(6):
            v = b[r]
            for p in range(r):
                v = v - A[r, p] * z[p]
            z[r] = v
        for r in range(6):
            z[r] = z[r] / A[r, r]
        d = np.zeros(6)
        for r in range(5, -1, -1):
            v = z[r]
            for p in range(r + 1, 6):
                v = v - A[p, r] * d[p]
            d[r] = v
    return (d if mutant == "delta_sign" else -d), bad


def update(st, k, stats_trial, theta_trial, mutant=None, **opts):
    """One call for slot k; theta_trial is overwritten (and returned)."""
    o = dict(OPTS, **opts)
    K = st["n_iter"]
    tdt = st["theta_cur"].dtype.type
    stats_trial = np.asarray(stats_trial, F64)
    with np.errstate(all="ignore"):
        for i in range(st["n"]):
            tr, cur = stats_trial[i], st["stats_cur"][i]
            fin = bool(np.all(np.isfinite(tr[:TERMS])))
            cost_t, m_t = tr[27] / tr[28], tr[29]
            accepted = 0
            if k == 0:
                cur[:] = tr
                st["theta_cur"][i] = theta_trial[i]
                st["m0"][i] = m_t
                lam = F64(o["lambda0"])
                frozen = (not m_t >= 1.0) or (not tr[28] > 0.0) or not fin
            else:
                frozen, lam = bool(st["frozen_now"][i]), st["lam"][i]
                if not frozen:
                    cost_old = cur[27] / cur[28]
                    if fin and m_t >= o["min_overlap"] * st["m0"][i] and cost_t < cost_old:
                        accepted = 1
                        cur[:] = tr
                        st["theta_cur"][i] = theta_trial[i]
                        lam = (lam * o["factor"]) if mutant == "lambda_swapped" else max(lam / o["factor"], F64(o["lambda_min"]))
                        if cost_old - cost_t <= o["tol"] * cost_old:
                            frozen = True
                    else:
                        lam = max(lam / o["factor"], F64(o["lambda_min"])) if mutant == "lambda_swapped" else lam * o["factor"]
                        if lam > o["lambda_max"]:
                            frozen = True
            d, bad = step(cur, lam, mutant)
            if not frozen and k < K and bad:
                frozen = True
            if not frozen and k < K:
                theta_trial[i] = (st["theta_cur"][i].astype(F64) + d).astype(tdt)
            else:
                theta_trial[i] = st["theta_cur"][i]
            st["lam"][i], st["frozen_now"][i] = lam, frozen
            st["cost"][k, i], st["lambda_hist"][k, i] = cur[27] / cur[28], lam
            st["accepted"][k, i], st["frozen"][k, i] = accepted, frozen
    return theta_trial


# ---- the solve ------------------------------------------------------------------------------------------------------------------
ONEHOT = np.eye(12).reshape(12, 3, 4)


def jacobian(theta, dtype=F64):
    """(n,12,6): row k = d (transform entry k) / d pose, by axisangle2mat_backward of the 12 one-hot matrices"""
    th = np.asarray(theta).astype(dtype)
    n = th.shape[0]
    return TC.axisangle2mat_backward(np.tile(ONEHOT, (n, 1, 1)), np.repeat(th, 12, axis=0), dtype).reshape(n, 12, 6)


def normal(theta, vol, psf, y, sm, sw, res, min_weight=0.5, ft=F64, device_order=False):
    """stats at the poses theta.  ft float64: theta as it is (transforms and jac are NOT rounded to fp32 on the way in)."""
    tr = TC.axisangle2mat(theta, ft)
    jac = jacobian(theta, ft)
    if ft is F64:
        return stats64(_pixels_raw(tr, jac, vol, psf, y, sm, sw, res, min_weight)["terms"])
    p = pixels(tr, jac, vol, psf, y, sm, sw, res, min_weight, F32)
    return stats_device(p["terms"]) if device_order else stats64(p["terms"])


def _pixels_raw(tr64, jac64, vol, psf, y, sm, sw, res, min_weight):
    """pixels() in float64 on float64 transforms and jac (pixels() itself takes them as the fp32 values the device gets)"""
    n = np.asarray(tr64).reshape(-1, 3, 4).shape[0]
    return _pixels64(np.asarray(tr64, F64).reshape(n, 3, 4), np.asarray(jac64, F64), vol, psf, y, sm, sw, res, min_weight)


def _pixels64(T, jac, vol, psf, y, sm, sw, res, min_weight):
    """The same rule as pixels(ft=float64), written directly on float64 transforms: s, e, J6 and the 30 terms only."""
    vol = np.asarray(vol, F64)
    y = np.asarray(y, F64)
    psf = np.asarray(psf, F64)
    n, h, w = y.shape
    D, H, W = vol.shape
    pd, ph, pw = psf.shape
    flat = vol.reshape(-1)
    r = lambda i, j: T[:, i, j][:, None, None]  # noqa: E731
    ixs, iys = np.arange(w, dtype=F64)[None, None, :], np.arange(h, dtype=F64)[None, :, None]
    _x = np.broadcast_to((ixs - (w - 1) / 2.0) * F64(F32(res)) + r(0, 3), (n, h, w))
    _y = np.broadcast_to((iys - (h - 1) / 2.0) * F64(F32(res)) + r(1, 3), (n, h, w))
    _z = np.broadcast_to(r(2, 3), (n, h, w))
    xc = r(0, 0) * _x + r(0, 1) * _y + r(0, 2) * _z + (W - 1) / 2.0
    yc = r(1, 0) * _x + r(1, 1) * _y + r(1, 2) * _z + (H - 1) / 2.0
    zc = r(2, 0) * _x + r(2, 1) * _y + r(2, 2) * _z + (D - 1) / 2.0
    sm = np.ones((n, h, w), bool) if sm is None else np.asarray(sm, bool).reshape(n, h, w)
    wgt = np.ones((n, h, w)) if sw is None else np.asarray(sw, F64).reshape(n, h, w)
    taps = [(kx - pw // 2, ky - ph // 2, kz - pd // 2, psf[kz, ky, kx]) for kz in range(pd) for ky in range(ph) for kx in range(pw)
            if psf[kz, ky, kx] != 0]

    def pos(fx, fy, fz):
        x = xc + r(0, 0) * fx + r(0, 1) * fy + r(0, 2) * fz
        yy = yc + r(1, 0) * fx + r(1, 1) * fy + r(1, 2) * fz
        z = zc + r(2, 0) * fx + r(2, 1) * fy + r(2, 2) * fz
        return x, yy, z, (x >= 0) & (yy >= 0) & (z >= 0) & (x < W - 1) & (yy < H - 1) & (z < D - 1)

    with np.errstate(all="ignore"):
        weight = np.zeros((n, h, w))
        for fx, fy, fz, pv in taps:
            weight = np.where(pos(fx, fy, fz)[3], weight + pv, weight)
        part = sm & (weight > 0) & (weight >= F64(F32(min_weight)))
        wsafe = np.where(part, weight, 1.0)
        val, g = np.zeros((n, h, w)), [np.zeros((n, h, w)) for _ in range(12)]
        for fx, fy, fz, pv in taps:
            x, yy, z, acc = pos(fx, fy, fz)
            acc = acc & part
            xf, yf, zf = (np.where(acc, np.floor(v), 0) for v in (x, yy, z))
            wx, wy, wz = (np.where(acc, a - b, 0) for a, b in ((x, xf), (yy, yf), (z, zf)))
            iv = zf.astype(np.int64) * (H * W) + yf.astype(np.int64) * W + xf.astype(np.int64)
            pg = pv / wsafe
            tri, dx, dy, dz = (np.zeros((n, h, w)) for _ in range(4))
            for c in CORNERS:
                cv = np.where(acc, flat[np.where(acc, iv + c[2] * H * W + c[1] * W + c[0], 0)], 0.0)
                fxw, fyw, fzw = _fac(wx, c[0], 1.0), _fac(wy, c[1], 1.0), _fac(wz, c[2], 1.0)
                tri = tri + fxw * fyw * fzw * cv
                t = pg * cv
                dx = dx + (1 if c[0] else -1) * fyw * fzw * t
                dy = dy + (1 if c[1] else -1) * fxw * fzw * t
                dz = dz + (1 if c[2] else -1) * fxw * fyw * t
            val = val + np.where(acc, pv * tri, 0)
            lev = (_x + fx, _y + fy, _z + fz)
            for a, d in enumerate((dx, dy, dz)):
                for b in range(3):
                    g[4 * a + b] = g[4 * a + b] + np.where(acc, d * lev[b], 0)
            for b in range(3):
                g[4 * b + 3] = g[4 * b + 3] + np.where(acc, dx * r(0, b) + dy * r(1, b) + dz * r(2, b), 0)
        s = np.where(part, val / wsafe, 0.0)
        e = np.where(part, s - y, 0.0)
        J6 = np.stack([sum(jac[:, k, a][:, None, None] * g[k] for k in range(12)) for a in range(6)], -1)
        terms = np.zeros((n, h, w, TERMS))
        for o, (a, b) in enumerate(PAIRS):
            terms[..., o] = wgt * J6[..., a] * J6[..., b]
        for a in range(6):
            terms[..., 21 + a] = wgt * e * J6[..., a]
        terms[..., 27], terms[..., 28], terms[..., 29] = wgt * e * e, wgt, 1.0
        terms = np.where(part[..., None], terms, 0.0)
    return dict(part=part, s=s, e=e, J6=J6, terms=terms, weight=weight)


def solve(theta0, vol, psf, y, res, n_iter, sm=None, sw=None, min_weight=0.5, ft=F64, mutant=None, device_order=False, **opts):
    """-> (theta, state).  ft float64: poses, transforms and Jacobian in float64 throughout; ft float32: what the device
    computes (poses float32, conversions and per-pixel arithmetic in float32 operations, the update in float64)."""
    tdt = F64 if ft is F64 else F32
    theta = np.array(theta0, tdt)
    st = new_state(theta.shape[0], n_iter, tdt)
    for k in range(n_iter + 1):
        stats = normal(theta, vol, psf, y, sm, sw, res, min_weight, ft, device_order)
        theta = update(st, k, stats, theta, mutant, **opts)
    return st["theta_cur"].copy(), st


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def forward_at(theta, vol, psf, ss, res):
    """float64 slices at float64 poses (every pixel that has weight > 0)"""
    n = np.asarray(theta).shape[0]
    p = _pixels64(TC.axisangle2mat(theta, F64).reshape(n, 3, 4), np.zeros((n, 12, 6)), vol, psf, np.zeros((n, *ss)), None, None, res, 0.0)
    return p["s"], p["weight"]


CAP_N_ITER = 12


def capability_case():
    f = BC.fit_case()
    true = f["true"].astype(F64)
    ss, res = (9, 9), 1.0
    y, wgt = forward_at(true, f["vol"], f["psf"], ss, res)
    rng = np.random.default_rng(5)
    start = true.copy()
    start[:, :3] += rng.uniform(-0.03, 0.03, (BC.N, 3))
    start[:, 3:] += rng.uniform(-0.75, 0.75, (BC.N, 3))
    return dict(vol=f["vol"], psf=f["psf"], res=res, ss=ss, y=y.astype(F32), y64=y, true=true, start=start.astype(F32), weight=wgt)


def pose_errors(theta, true):
    """largest |component| of the rotation-vector error (rad) and of the translation error (voxels)"""
    d = np.abs(np.asarray(theta, F64) - np.asarray(true, F64))
    return float(d[:, :3].max()), float(d[:, 3:].max())


# The capability case in CAP_N_ITER = 12 rounds, measured on the CPU.  Start: cost 2.9e-4 .. 2.8e-2 per slice, errors up to
# 0.0300 rad / 0.722 voxel.
#   float64, slices not rounded (y64):     cost 3.9e-33 .. 1.5e-31, errors 2.2e-15 rad / 5.8e-15 voxel, 7-8 accepted steps.
#   float64, slices rounded to fp32 (y):   cost 3.4e-17 .. 2.4e-15, errors 2.8e-7 / 5.2e-7: the floor the fp32 slices set.
#   fp32 operations, device order (y):     cost 6.3e-16 .. 1.9e-14, 5-8 accepted steps; the three figures below.
# The GPU test asserts a tenth of the factor and four times each error.
CAP32_COST_FACTOR = 4.58e11  # smallest cost[0] / cost[12] over the slices; measured 4.582e11
CAP32_ROT_ERR = 8.54e-7      # measured 8.531e-7
CAP32_TRANS_ERR = 2.63e-6    # measured 2.623e-6

# max |fp32-operation stats - float64 stats| / max |float64 stats| per group over the two general cases, measured on the CPU
# (python -m tests.util_svr64 prints them), rounded up in the third digit with the measured value beside each
E_CPU = {"H": 8.34e-07,  # 8.3348e-07
         "g": 1.81e-06,  # 1.8090e-06
         "cost": 4.87e-08}  # 4.8652e-08
MIN_KEPT = 0.30
_CASES = {}


def general_case(name):
    """util_sa_backward_cases.general_case(name, interp_psf=False) as a registration problem: y = the case's random slices,
    jac random, slices_weight random in [0.5, 1.5], and ONE slices_mask: the case's margin mask (every floor and range decision
    further than 2e-3 from its threshold) minus the pixels whose float64 weight is within 1e-3 of min_weight."""
    if name not in _CASES:
        c = BC.general_case(name, False)
        rng = np.random.default_rng(sum(map(ord, name)))
        n = c["tr"].shape[0]
        jac = rng.standard_normal((n, 12, 6)).astype(F32)
        sw = rng.uniform(0.5, 1.5, c["g"].shape).astype(F32)
        min_weight = 0.5 * float(np.asarray(c["psf"], F64).sum())  # half the PSF inside the volume
        p = pixels(c["tr"], jac, c["vol"], c["psf"], c["g"], None, None, c["res"], 0.0, F64)
        sm = c["sm"] & ~(np.abs(p["weight"] - F64(F32(min_weight))) <= 1e-3)
        _CASES[name] = dict(tr=c["tr"], jac=jac, vol=c["vol"], psf=c["psf"], y=c["g"], sm=sm, sw=sw, res=c["res"],
                            min_weight=min_weight, kept=float(sm.mean()))
    return _CASES[name]


GENERAL = ("psf335", "psf223_vm")


def case_pixels(c, ft, sw=True):
    return pixels(c["tr"], c["jac"], c["vol"], c["psf"], c["y"], c["sm"], c["sw"] if sw else None, c["res"], c["min_weight"], ft)


def measure_e_cpu():
    worst = {k: 0.0 for k in GROUPS}
    for name in GENERAL:
        c = general_case(name)
        s64, s32 = stats64(case_pixels(c, F64)["terms"]), stats64(case_pixels(c, F32)["terms"])
        for key, sl in GROUPS.items():
            worst[key] = max(worst[key], float(np.abs(s32[:, sl] - s64[:, sl]).max() / np.abs(s64[:, sl]).max()))
    return worst


def measure_capability(ft=F32, mutant=None, n_iter=CAP_N_ITER, unrounded=False):
    """unrounded: the float64 slices as they are (float64 runs only); otherwise the fp32 slices the device gets"""
    c = capability_case()
    y = c["y64"] if unrounded else c["y"]
    theta, st = solve(c["start"], c["vol"], c["psf"], y, c["res"], n_iter, ft=ft, mutant=mutant, device_order=ft is F32)
    rot, trans = pose_errors(theta, c["true"])
    return dict(theta=theta, st=st, cost0=st["cost"][0], cost=st["cost"][-1], rot=rot, trans=trans,
                factor=float((st["cost"][0] / st["cost"][-1]).min()), accepted=st["accepted"].sum(0))


if __name__ == "__main__":
    print("E_CPU", {k: f"{v:.4e}" for k, v in measure_e_cpu().items()})
    for name in GENERAL:
        print(name, "kept", general_case(name)["kept"])
    c = capability_case()
    print("start errors", pose_errors(c["start"], c["true"]), "weights", c["weight"].min(), c["weight"].max())
    runs = [(F64, m, True) for m in (None, "delta_sign", "lambda_swapped", "identity_damping")] + [(F64, None, False), (F32, None, False)]
    for ft, mutant, unrounded in runs:
        r = measure_capability(ft, mutant, unrounded=unrounded)
        print(ft.__name__, mutant, "slices float64" if unrounded else "slices fp32", "cost0", r["cost0"], "cost", r["cost"], "factor",
              r["factor"], "rot", r["rot"], "trans", r["trans"], "accepted", r["accepted"])
