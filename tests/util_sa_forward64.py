"""CPU restatement of the slice-acquisition FORWARD operator in the CUDA semantics (include/fsg_hip.h, fsg_slice_acq_forward_f32;
DESIGN.md section 26), with vol_mask.  Test infrastructure, numpy only; written beside tests/util_srr64.forward (which stays as it
is: other tests hold it) on the same geometry object and tap walk.  For the adjoint the yardstick is
util_sa_adjoint_backward64.adjoint64 as it is; `adjoint32` below states the float kernels' own sums.

    forward(transforms, vol, vol_mask, psf, slices_mask, slice_shape, res_slice, interp_psf, ft, form, mutant) -> dict
        slices, weight (n,h,w) in ft   slices = sum(coef * vol) / sum(coef) where the sum of coefficients is > 0 and the pixel is
                                       inside slices_mask, else 0; weight = that sum of coefficients, else 0
        k (n,h,w) int                  number of accepted finest-grain terms (LINEAR: corners, NEAREST_PSF: taps)
        bounds_dist (n,h,w) f64        smallest distance of any tap coordinate of the pixel (accepted or not) to 0 or size-1
                                       (inf for a PSF without a non-zero tap)

The rule, restated:
  * taps with a PSF value of 0 are skipped; a tap at position p is accepted when 0 <= p < size-1 on every axis;
  * LINEAR: the 8 corners of the cell, coefficient = trilinear weight * PSF value; a corner outside vol_mask leaves BOTH the
    value and the weight sum;
  * NEAREST_PSF: the voxel round-half-away(p); a voxel outside vol_mask is skipped; then the PSF re-interpolated at the voxel's
    PSF coordinate, skipped when that lies outside [0, psf_size-1) on an axis; coefficient = that PSF value.

ft and form:
  ft = float64                 every operation in float64 from the fp32 inputs: the yardstick (either form: they differ by 1e-16);
  ft = float32, "weights"      the operation order of the generic kernel (the reference's source), one rounding per operation:
                               pw = ((fx * fy) * fz) * pv;  val += pw * vol[corner];  weight += pw    in the corner order;
  ft = float32, "lerp"         LINEAR without vol_mask only: the formula of the two fast kernels as their comment block states
                               it -- the 2x2x2 blend as lerps on the x-pairs, then along y, then along z
                                   a_yz = v_0yz + wx (v_1yz - v_0yz);  b_z = a_0z + wy (a_1z - a_0z);  c = b_0 + wz (b_1 - b_0)
                                   val += pv * c;  weight += pv     (the eight trilinear weights of a tap add up to pv)
                               one rounding per operation, the taps summed in raster order.

mutant (a wrong operator on purpose; the CPU tests show that every bound of the GPU tests would catch each of them):
    "drop_last_tap"     the last non-zero tap is left out
    "dup_plane_start"   the first non-zero tap at or after the start of PSF plane min(1, pd-1) is counted twice (a plane start of
                        the compacted tap list that is one too low); the last tap when none follows that start
    "swap_xy_corner"    the weights of the corners (1,0,0) and (0,1,0) are exchanged (NEAREST_PSF: in the PSF's own cell)
    "weight_all_taps"   the weight also sums the PSF value of the taps that fail the bounds test
"""
import numpy as np

from tests.util_sa_adjoint_backward64 import _Geometry, _fac
from tests.util_sa_backward64 import CORNERS
from tests.util_srr64 import _walk

F32, F64 = np.float32, np.float64
MUTANTS = ("drop_last_tap", "dup_plane_start", "swap_xy_corner", "weight_all_taps")


class _Taps(_Geometry):
    """_Geometry whose tap list a mutant may alter; everything else (positions, cells, PSF cells) is the shared geometry."""

    mutant = None

    def taps(self):
        ft, pd, ph, pw = self.ft, self.pd, self.ph, self.pw
        nz = [(kz, ky, kx) for kz in range(pd) for ky in range(ph) for kx in range(pw) if self.psf[kz, ky, kx] != 0]
        if nz and self.mutant == "drop_last_tap":
            nz = nz[:-1]
        elif nz and self.mutant == "dup_plane_start":
            plane = min(1, pd - 1)
            at = next((i for i, t in enumerate(nz) if t[0] >= plane), len(nz) - 1)
            nz = nz[:at + 1] + nz[at:]
        for kz, ky, kx in nz:
            yield ft(kx - pw // 2), ft(ky - ph // 2), ft(kz - pd // 2), self.psf[kz, ky, kx]


def _psf_value_swapped(G, wf, q):
    """_psf_value with the weights of the corners (1,0,0) and (0,1,0) exchanged"""
    one = G.ft(1)
    wx, wy, wz = wf
    order = list(CORNERS)
    order[1], order[2] = order[2], order[1]
    val = np.zeros(G.nhw, G.ft)
    for c, qc in zip(order, q):
        val = val + _fac(wx, c[0], one) * _fac(wy, c[1], one) * _fac(wz, c[2], one) * qc
    return val


def forward(transforms, vol, vol_mask, psf, slices_mask, slice_shape, res_slice, interp_psf, ft=F64, form="weights", mutant=None):
    if form not in ("weights", "lerp") or mutant not in (None,) + MUTANTS:
        raise ValueError((form, mutant))
    if form == "lerp" and (interp_psf or vol_mask is not None):
        raise ValueError("the lerp form is the LINEAR forward without vol_mask")
    v = np.asarray(vol).astype(ft)
    n = np.asarray(transforms).reshape(-1, 3, 4).shape[0]
    h, w = (int(s) for s in slice_shape)
    G = _Taps(transforms, psf, (n, h, w), v.shape, res_slice, ft)
    G.mutant = mutant
    flat = v.reshape(-1)
    vm = None if vol_mask is None else np.asarray(vol_mask, bool).reshape(-1)
    val, wgt = np.zeros((n, h, w), ft), np.zeros((n, h, w), ft)
    k = np.zeros((n, h, w), np.int64)
    dist = np.full((n, h, w), np.inf)
    swap = mutant == "swap_xy_corner"
    old = np.seterr(invalid="ignore", over="ignore", divide="ignore")
    try:
        for (fx, fy, fz, raw), (cells, pv, acc) in zip(G.taps(), _walk(G, interp_psf)):
            x, y, z, acc0 = G.position(fx, fy, fz)
            for c, hi in ((x, G.W - 1), (y, G.H - 1), (z, G.D - 1)):
                c64 = c.astype(F64)
                d = np.minimum(np.abs(c64), np.abs(c64 - hi))
                dist = np.minimum(dist, np.where(np.isfinite(d), d, np.inf))
            if mutant == "weight_all_taps":
                wgt = np.where(~acc0, (wgt + raw).astype(ft), wgt)
            if interp_psf:
                (idx, _, ok), = cells
                if swap:
                    xr, yr, zr, _ = G.rounded(x, y, z, acc0)
                    _, _, wf, q = G.psf_cell(xr, yr, zr, acc0)
                    pv = _psf_value_swapped(G, wf, q)
                if vm is not None:
                    ok = ok & vm[idx]
                val = np.where(ok, (val + (pv * flat[idx]).astype(ft)).astype(ft), val)
                wgt = np.where(ok, (wgt + pv).astype(ft), wgt)
                k += ok
            elif form == "lerp":
                (wx, wy, wz), iv = G.cell(x, y, z, acc0)
                q = {c: flat[G.corner_index(iv, c, acc0)] for c in CORNERS}
                if swap:
                    q[(1, 0, 0)], q[(0, 1, 0)] = q[(0, 1, 0)], q[(1, 0, 0)]
                a = {(b, c): (q[0, b, c] + (wx * (q[1, b, c] - q[0, b, c]).astype(ft)).astype(ft)).astype(ft) for b in (0, 1) for c in (0, 1)}
                bz = [(a[0, c] + (wy * (a[1, c] - a[0, c]).astype(ft)).astype(ft)).astype(ft) for c in (0, 1)]
                blend = (bz[0] + (wz * (bz[1] - bz[0]).astype(ft)).astype(ft)).astype(ft)
                val = np.where(acc0, (val + (pv * blend).astype(ft)).astype(ft), val)
                wgt = np.where(acc0, (wgt + pv).astype(ft), wgt)
                k += acc0 * 8
            else:
                coefs = [c[1] for c in cells]
                if swap:
                    coefs[1], coefs[2] = coefs[2], coefs[1]
                for (idx, _, ok), coef in zip(cells, coefs):
                    if vm is not None:
                        ok = ok & vm[idx]
                    pw = (coef * pv).astype(ft)
                    val = np.where(ok, (val + (pw * flat[idx]).astype(ft)).astype(ft), val)
                    wgt = np.where(ok, (wgt + pw).astype(ft), wgt)
                    k += ok
        sm = np.ones((n, h, w), bool) if slices_mask is None else np.asarray(slices_mask, bool).reshape(n, h, w)
        good = (wgt > 0) & sm
        out = np.where(good, val / np.where(good, wgt, 1), 0).astype(ft)
    finally:
        np.seterr(**old)
    return {"slices": out, "weight": np.where(good, wgt, 0).astype(ft), "k": np.where(sm, k, 0), "bounds_dist": dist}


def adjoint32(transforms, psf, slices, slices_mask, vol_mask, vol_shape, res_slice, interp_psf, order="raster"):
    """The float adjoint (fsg_slice_acq_adjoint_f32) with the sums the kernels form: every contribution by adjoint64's float32
    operations (pass 1 the pixel weight, pixels below 0.5 dropped, pn = pv / weight, LINEAR ((fx * fy) * fz) * pn per corner), and
    the scatter as ONE FLOAT32 ADDITION PER CONTRIBUTION -- the kernels' fp32 atomics -- here in the order taps (raster) x corners x
    pixels (raster) for order = "raster", in exactly the opposite order for "reverse", and shuffled by
    np.random.default_rng(order) for an integer.  The order of the atomics is not fixed, and what a float32 sum loses depends on
    it (small inexact terms added before or after the large exact ones): a bound that is to hold for the kernels is measured
    over several orders and the largest value taken.  adjoint64(ft=float32) carries these sums in float64 and rounds once; a voxel of an exact-geometry stack
    receives hundreds of contributions, many of them the same number (interior pixels share one weight), and the roundings of
    such a sum do not average out: they grow with the number of terms.  Returns vol, vol_weight (D,H,W) and pixel_weight as
    adjoint64 without equalisation."""
    ft = F32
    sl = np.asarray(slices, F32)
    n, h, w = sl.shape
    G = _Geometry(transforms, psf, (n, h, w), vol_shape, res_slice, ft)
    vm = None if vol_mask is None else np.asarray(vol_mask, bool).reshape(-1)
    sm = np.ones((n, h, w), bool) if slices_mask is None else np.asarray(slices_mask, bool).reshape(n, h, w)
    old = np.seterr(invalid="ignore", over="ignore", divide="ignore")
    try:
        weight = np.zeros((n, h, w), ft)
        for _, pv, ok in _walk(G, interp_psf):
            weight = np.where(ok, weight + pv, weight).astype(ft)
        live = sm & ~(weight < 0.5)
        wsafe = np.where(live, weight, 1).astype(ft)
        vol, vw = np.zeros(G.D * G.H * G.W, ft), np.zeros(G.D * G.H * G.W, ft)
        terms = []
        for cells, pv, _ in _walk(G, interp_psf, live):
            pn = (pv / wsafe).astype(ft)
            for idx, coef, ok in cells:
                if vm is not None:
                    ok = ok & vm[idx]
                cw = pn if coef is None else (coef * pn).astype(ft)
                terms.append((idx[ok], (cw * sl)[ok].astype(ft), cw[ok].astype(ft)))
        idx, tv, tw = (np.concatenate([t[j] for t in terms]) if terms else np.zeros(0, t0) for j, t0 in enumerate((np.int64, ft, ft)))
        if order == "reverse":
            idx, tv, tw = idx[::-1], tv[::-1], tw[::-1]
        elif order != "raster":
            perm = np.random.default_rng(int(order)).permutation(idx.size)
            idx, tv, tw = idx[perm], tv[perm], tw[perm]
        np.add.at(vol, idx, tv)  # unbuffered: one float32 addition per element, in order
        np.add.at(vw, idx, tw)
    finally:
        np.seterr(**old)
    return {"vol": vol.reshape(G.D, G.H, G.W), "vol_weight": vw.reshape(G.D, G.H, G.W), "pixel_weight": weight}


def equalized(adj, ft=F64):
    """adjoint64's own equalisation applied to its un-equalised result (vol / vol_weight where the weight is > 0), so that one
    run of adjoint64 serves both settings.  Held to adjoint64(..., equalize=True) by the CPU tests."""
    vol, vw = adj["vol"].astype(ft).copy(), adj["vol_weight"].astype(ft)
    m = vw > 0
    vol[m] = vol[m] / vw[m]
    return vol
