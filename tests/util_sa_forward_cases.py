"""Inputs of tests/test_sa_forward_edges_gpu.py and tests/test_sa_forward64_reference.py, built on the host with numpy in the style
of tests/util_sa_backward_cases.py (whose PERMS, rotation, exact_case and general_case are reused), the host replica of the
forward's route selection (`census`), and the measured fp32 cost of the formulas (`E_CPU_FWD`, `E_CPU_ADJ`).  DESIGN.md section 26.

Exact geometry (`kind == "exact"`): signed-permutation rotations, translations multiples of 1/8, PSF values multiples of 1/32 with
some zero taps, res_slice 0.75 or 1.5, volumes randn.  Every coordinate and every weight is exact in fp32, so fp32 and float64 take
the same decisions.  Some slices of every stack reach past a face.  The shapes are the smallest at which a route exists:

    name                       PSF          volume     slices             route of the LINEAR unmasked forward it is there for
    the five BC.EXACT          as there     20x18x22   5 x (13,11)/(37,29) one chunk; delta: direct gathers only; both selections
    multi_chunk                (8,9,9)      40x36x44   6 x (21,19) 1.5    2 and more chunks per tile
    tall                       (12,7,7)     40x36x44   6 x (21,19) 1.5    1-2 chunks of many planes
    wide                       (2,30,30)    20x44x48   6 x (21,19) 0.75   planes that do not fit: direct gathers inside the plate kernel
    plate_limit / direct_only  (4,22,22) / (5,20,20)  20x44x48  6 x (21,19)  either side of lds_p > 64000
    generic_big                (1,63,64)    20x72x72   3 x (13,11)        more than 4000 PSF elements: the generic kernel
    sparse / sparse_zero       (3,5,7)      20x18x22   5 x (13,11)        ~30 % zero taps, plane 1 all zero: two compaction rounds,
                                                                          an empty plane / no tap at all (nt == 0)
    counts_n{1,8,9,17}_{hxw}   (2,2,3)      20x18x22   n x (13,11)/(37,29) XCD slice mapping, `groups` rounding
    shapes_{hxw}               (2,2,3)      20x18x22   2 x (1,1) (1,40) (16,16) (17,4)   tile edges of 16 and of 4
    shapes_faces               (2,2,3)      20x18x22   6 x (13,11)        one stack wholly beyond each face by 1.5 voxels and more (the
                                                                          PSF reaches 1): exact zeros, also in weight

General rotations:
    lin_psf335 / lin_psf899    (3,3,5) 0.75 / (8,9,9) 1.5, volume 40x36x44, 6 x (13,11), rotation(rng, 1.0), translations in +-2:
                               LINEAR interior stacks, no mask; the seeds are chosen so that bounds_dist.min() > 1e-3 (asserted):
                               LINEAR is continuous across grid crossings, only the bounds test could flip, and then it cannot.
    gen_psf335 / gen_psf223_vm the two GENERAL cases of util_sa_backward_cases with their margin mask (every decision distance
                               > 2e-3), per interp_psf: NEAREST_PSF, and LINEAR with vol_mask.

A case is a dict: tr, vol, vm (never None: the modes decide whether it is passed), psf, sm (or None), g (slices for the adjoint),
res, ss, vs, kind, and `small`: whether the modes without routes of their own (LINEAR with vol_mask, NEAREST_PSF: one generic kernel
each) run on it -- the cases that exist for a threshold of the LINEAR dispatch alone are left to the LINEAR unmasked modes.
"""
import math

import numpy as np

from tests import util_sa_backward_cases as BC
from tests import util_sa_forward64 as FW
from tests.util_sa_adjoint_backward64 import adjoint64
from tests.util_sa_backward_cases import PERMS, exact_case, general_case, rotation

F32, F64 = np.float32, np.float64
VS = BC.VS
VS_MID, VS_WIDE, VS_BIG = (40, 36, 44), (20, 44, 48), (20, 72, 72)

# name: (psf shape, volume, n, slice shape, res_slice, slices_mask?, small)
NEW_EXACT = {
    "multi_chunk": ((8, 9, 9), VS_MID, 6, (21, 19), 1.5, True, True),
    "tall": ((12, 7, 7), VS_MID, 6, (21, 19), 1.5, True, True),
    "wide": ((2, 30, 30), VS_WIDE, 6, (21, 19), 0.75, True, False),
    "plate_limit": ((4, 22, 22), VS_WIDE, 6, (21, 19), 0.75, False, False),
    "direct_only": ((5, 20, 20), VS_WIDE, 6, (21, 19), 0.75, False, False),
    "generic_big": ((1, 63, 64), VS_BIG, 3, (13, 11), 1.5, False, False),
    "sparse": ((3, 5, 7), VS, 5, (13, 11), 0.75, True, True),
    "sparse_zero": ((3, 5, 7), VS, 5, (13, 11), 0.75, True, True),
}
COUNTS_N, COUNTS_SS = (1, 8, 9, 17), ((13, 11), (37, 29))
SHAPES_SS = ((1, 1), (1, 40), (16, 16), (17, 4))
for _n in COUNTS_N:
    for _ss in COUNTS_SS:
        NEW_EXACT["counts_n%d_%dx%d" % (_n, *_ss)] = ((2, 2, 3), VS, _n, _ss, 1.5, False, True)
for _ss in SHAPES_SS:
    NEW_EXACT["shapes_%dx%d" % _ss] = ((2, 2, 3), VS, 2, _ss, 1.5, _ss != (1, 1), True)
NEW_EXACT["shapes_faces"] = ((2, 2, 3), VS, 6, (13, 11), 1.5, False, True)

LIN_GENERAL = {  # name: (psf shape, res_slice, seed)
    "lin_psf335": ((3, 3, 5), 0.75, 301),
    "lin_psf899": ((8, 9, 9), 1.5, 302),
}
EXACT_NAMES = tuple(BC.EXACT) + tuple(NEW_EXACT)
GEN_NAMES = tuple("gen_" + k for k in BC.GENERAL)
FORWARD_CASES = EXACT_NAMES + tuple(LIN_GENERAL) + GEN_NAMES
ADJOINT_CASES = tuple(BC.EXACT) + ("multi_chunk", "sparse") + GEN_NAMES
PER_SLICE = tuple(k for k in NEW_EXACT if k.startswith(("counts_", "shapes_")))


def _seed(name):
    return sum(map(ord, name)) + 1000


def _new_exact(name):
    pshape, vs, n, ss, res, with_sm, small = NEW_EXACT[name]
    rng = np.random.default_rng(_seed(name))
    tr = np.zeros((n, 3, 4), F32)
    first = 2 if name.startswith("shapes_") else len(name)  # (two slices: PERMS[2] is the plate kernel's, PERMS[3] the direct one's)
    for i in range(n):
        tr[i, :, :3] = PERMS[(i + first) % len(PERMS)]
        tr[i, :, 3] = rng.integers(-48, 49, 3) / 8.0  # some slices reach past a face
    psf = (rng.integers(1, 33, pshape) / 32.0).astype(F32)
    if name.startswith("sparse"):
        psf[rng.random(pshape) < 0.3] = 0
        psf[1] = 0  # an empty plane
        psf[0, 0, 0], psf[2, -1, -1] = 1.0, 1.0  # both ends of the raster stay taps
        if name == "sparse_zero":
            psf[:] = 0
    else:
        psf.reshape(-1)[rng.integers(1, psf.size - 1)] = 0  # a tap the kernels skip
    if name == "shapes_faces":
        # identity rotation; the nearest pixel centre 1.5 voxels beyond the face (PSF offsets reach 1; the fast kernels'
        # early-out radius is 3.06, so these pixels take the per-tap bounds test): (W-1)/2 + 5 * 1.5 + 1.5 and the like
        tr[:, :, :3] = np.eye(3)
        tr[:, :, 3] = 0
        for i, (axis, d) in enumerate(((0, 19.5), (0, -19.5), (1, 19.0), (1, -19.0), (2, 11.0), (2, -11.0))):
            tr[i, axis, 3] = d
    if name == "shapes_1x1":
        # the one pixel of each slice straddles a face: PERMS[2] puts it at y = ty + 8.5 = 0.25 (the tap at -1 fails the bounds
        # test), PERMS[3] at x = tx + 10.5 = 20.75 (the tap at +1 does)
        tr[0, :, 3], tr[1, :, 3] = (0.125, -8.25, -0.375), (10.25, 0.5, -0.125)
    vol = rng.standard_normal(vs).astype(F32)
    g = rng.standard_normal((n, *ss)).astype(F32)
    vm = rng.random(vs) < 0.8
    sm = (rng.random((n, *ss)) < 0.8) if with_sm else None
    return dict(tr=tr, vol=vol, vm=vm, psf=psf, sm=sm, g=g, res=res, ss=ss, vs=vs, kind="exact", small=small)


def _lin_general(name):
    pshape, res, seed = LIN_GENERAL[name]
    rng = np.random.default_rng(seed)
    n, ss = 6, (13, 11)
    tr = np.zeros((n, 3, 4), F32)
    for i in range(n):
        tr[i, :, :3] = rotation(rng, 1.0)
        tr[i, :, 3] = rng.uniform(-2, 2, 3)
    psf = rng.uniform(0.1, 1.0, pshape).astype(F32)
    vol = rng.standard_normal(VS_MID).astype(F32)
    g = rng.standard_normal((n, *ss)).astype(F32)
    return dict(tr=tr, vol=vol, vm=rng.random(VS_MID) < 0.8, psf=psf, sm=None, g=g, res=res, ss=ss, vs=VS_MID, kind="lin_general",
                small=False)


_CASES = {}


def case(name, interp_psf=False):
    """The case `name`; only the gen_* cases depend on interp_psf (their margin mask does)."""
    key = (name, bool(interp_psf) and name.startswith("gen_"))
    if key not in _CASES:
        if name in BC.EXACT:
            c = dict(exact_case(name, True), ss=BC.EXACT[name][2], vs=VS, kind="exact", small=True)
        elif name in NEW_EXACT:
            c = _new_exact(name)
        elif name in LIN_GENERAL:
            c = _lin_general(name)
        elif name in GEN_NAMES:
            c = dict(general_case(name[4:], key[1]), ss=(13, 11), vs=VS, kind="general", small=True)
            if c["vm"] is None:
                c["vm"] = np.random.default_rng(_seed(name)).random(VS) < 0.8
            # the adjoint drops pixels whose weight is below 0.5: the pixels within 1e-3 of that cut leave the mask as well
            pw = adjoint64(c["tr"], c["psf"], np.zeros_like(c["g"]), None, None, VS, c["res"], key[1], False)["pixel_weight"]
            c["sm"] = c["sm"] & ~(np.abs(pw - 0.5) <= 1e-3)
        else:
            raise KeyError(name)
        _CASES[key] = c
    return _CASES[key]


# ---- the modes -------------------------------------------------------------------------------------------------------------
# forward mode: (interp_psf, with vol_mask, form of the fp32 restatement)
FWD_MODES = {
    "lin_lerp": (False, False, "lerp"),  # tuning 0, SA_FWD_DIRECT, SA_FWD_PLATE (census route "generic": lin_weights instead)
    "lin_weights": (False, False, "weights"),  # PRECISE_MATH, and the generic route
    "lin_vm": (False, True, "weights"),
    "nn": (True, False, "weights"),
    "nn_vm": (True, True, "weights"),
}


def fwd_modes(name):
    """the forward modes that apply to a case"""
    c = case(name)
    if c["kind"] == "lin_general":
        return ("lin_lerp", "lin_weights")
    if c["kind"] == "general":
        return ("lin_vm", "nn", "nn_vm")  # LINEAR under the margin mask of LINEAR, NEAREST_PSF under its own
    return tuple(FWD_MODES) if c["small"] else ("lin_lerp", "lin_weights")


def forward_ref(name, mode, ft=F64, mutant=None):
    interp_psf, with_vm, form = FWD_MODES[mode]
    c = case(name, interp_psf)
    return FW.forward(c["tr"], c["vol"], c["vm"] if with_vm else None, c["psf"], c["sm"], c["ss"], c["res"], interp_psf, ft,
                      form if ft is F32 else "weights", mutant)


# adjoint mode: (interp_psf, with vol_mask); equalize is applied to the result (FW.equalized)
ADJ_MODES = {"lin": (False, False), "lin_vm": (False, True), "nn": (True, False), "nn_vm": (True, True)}


ADJ_ORDERS = ("raster", "reverse", 1, 2)  # the orders of the float32 additions E_CPU_ADJ is measured over (FW.adjoint32)


def adjoint_ref(name, mode, ft=F64, order="raster"):
    """float64: adjoint64 without equalisation; float32: FW.adjoint32, the float kernels' own sums (one float32 addition per
    contribution); plus `vol_eq`, the equalised volume"""
    interp_psf, with_vm = ADJ_MODES[mode]
    c = case(name, interp_psf)
    vm = c["vm"] if with_vm else None
    if ft is F32:
        r = FW.adjoint32(c["tr"], c["psf"], c["g"], c["sm"], vm, c["vs"], c["res"], interp_psf, order)
    else:
        r = adjoint64(c["tr"], c["psf"], c["g"], c["sm"], vm, c["vs"], c["res"], interp_psf, False, ft)
    r["vol_eq"] = FW.equalized(r, ft)
    return r


def adjoint_tile(name):
    """replica of the LDS adjoint's tile rule under the default tuning (sa_lds_plan: 16x16 while res * 15 + PSF extent <= 20)"""
    c = case(name)
    return 16 if c["res"] * 15 + max(c["psf"].shape[1:]) <= 20 else 8


# ---- the census: a host replica of the LINEAR unmasked forward's route selection (fsg_slice_acq_forward_f32) and of the plate
# kernel's chunk rule (sa_forward_plate_kernel), float64, right in counts only ---------------------------------------------------
SAP_CAP = 2048


def census(c):
    """-> dict: route ("single_tap" | "generic" | "direct_only" | "two_launches"), taps (non-zero), rounds (compaction rounds of
    64), groups, tiles, slices_direct / slices_plate (slices each launch takes), and over the 4 x 4 pixel tiles of the plate
    kernel's slices that have a live pixel: chunks_min / chunks_max (plate chunks with a tap per tile), tiles_multi_plane (a chunk
    of more than one plane), direct_planes (planes whose box does not fit, with a tap), empty_runs (chunks or planes without a tap);
    empty_planes: PSF planes without a non-zero tap"""
    psf, tr, vs, res = c["psf"], c["tr"].astype(F64), c["vs"], float(F32(c["res"]))
    pd, ph, pw = psf.shape
    D, H, W = vs
    n, (h, w) = tr.shape[0], c["ss"]
    np_ = pd * ph * pw
    out = dict(taps=int((psf != 0).sum()), rounds=(np_ + 63) // 64, groups=(n + 7) // 8, tiles=((w + 15) // 16) * ((h + 15) // 16),
               slices_direct=0, slices_plate=0, chunks_min=0, chunks_max=0, tiles_multi_plane=0, direct_planes=0, empty_runs=0)
    plane_taps = (psf != 0).reshape(pd, -1).sum(1)
    out["empty_planes"] = int((plane_taps == 0).sum())
    lds_p = np_ * 16 + (pd + 1) * 4 + 6 * pd * 4 + 16 + 4 * SAP_CAP * 4
    if np_ == 1:
        out["route"] = "single_tap"
    elif np_ > 4000:
        out["route"] = "generic"
    elif lds_p > 64000:
        out["route"] = "direct_only"
    else:
        out["route"] = "two_launches"
    if out["route"] in ("single_tap", "direct_only"):
        out["slices_direct"] = n
    if out["route"] != "two_launches":
        return out
    small = np_ < 400
    wy, thr = (30.0, 10.0 / max(res, 0.25)) if small else (10.0, 1.7)
    rad = 0.5 * math.sqrt(pw * pw + ph * ph + pd * pd) + 1.0
    x0, x1, y0, y1 = -(pw // 2), pw - 1 - pw // 2, -(ph // 2), ph - 1 - ph // 2
    sm = np.ones((n, h, w), bool) if c["sm"] is None else np.asarray(c["sm"], bool)
    chunks = []
    for i in range(n):
        T = tr[i].reshape(-1)
        if not (wy * abs(T[4]) + 35.0 * abs(T[8]) > thr):
            out["slices_direct"] += 1
            continue
        out["slices_plate"] += 1
        ext = np.zeros((pd, 6))
        for k in range(pd):
            for a in range(3):
                cs = [T[4 * a] * x + T[4 * a + 1] * y for x in (x0, x1) for y in (y0, y1)]
                zt = T[4 * a + 2] * (k - pd // 2)
                ext[k, a], ext[k, 3 + a] = min(cs) + zt - 0.01, max(cs) + zt + 0.01
        px = (np.arange(w) - (w - 1) / 2.0) * res + T[3]
        py = (np.arange(h) - (h - 1) / 2.0) * res + T[7]
        X, Y = np.meshgrid(px, py)
        cen = [T[4 * a] * X + T[4 * a + 1] * Y + T[4 * a + 2] * T[11] + (s - 1) / 2.0 for a, s in enumerate((W, H, D))]
        live = sm[i].copy()
        for a, s in enumerate((W, H, D)):
            live &= ~((cen[a] < -rad) | (cen[a] > s - 1 + rad))
        for ty in range(0, h, 4):
            for tx in range(0, w, 4):
                lv = live[ty:ty + 4, tx:tx + 4]
                if not lv.any():
                    continue
                lo = [cen[a][ty:ty + 4, tx:tx + 4][lv].min() for a in range(3)]
                hi = [cen[a][ty:ty + 4, tx:tx + 4][lv].max() for a in range(3)]
                kz, nchunks = 0, 0
                while kz < pd:
                    kz1, o = kz, [np.inf] * 3 + [-np.inf] * 3
                    for k in range(kz, pd):
                        a_ = [min(o[j], ext[k, j]) for j in range(3)] + [max(o[3 + j], ext[k, 3 + j]) for j in range(3)]
                        nb = []
                        for j, s in enumerate((W, H, D)):
                            t0 = min(max(math.floor(lo[j] + a_[j]), 0), s - 1)
                            t1 = min(max(math.floor(hi[j] + a_[3 + j]) + 1, 0), s - 1)
                            nb.append(max(t1 - t0 + 1, 1))
                        pt = 4 if nb[0] <= 4 else (8 if nb[0] <= 8 else (16 if nb[0] <= 16 else 32))
                        if nb[0] > 32 or pt * nb[1] * nb[2] > SAP_CAP:
                            break
                        o, kz1 = a_, k + 1
                    plate = kz1 > kz
                    if not plate:
                        kz1 = kz + 1
                    ntap = int(plane_taps[kz:kz1].sum())
                    if ntap == 0:
                        out["empty_runs"] += 1
                    elif plate:
                        nchunks += 1
                        out["tiles_multi_plane"] += kz1 - kz > 1
                    else:
                        out["direct_planes"] += 1
                    kz = kz1
                chunks.append(nchunks)
    if chunks:
        out["chunks_min"], out["chunks_max"] = min(chunks), max(chunks)
    return out


# ---- E_cpu: max |restatement(float32) - restatement(float64)| / max |float64| per case, mode and output, measured on the CPU
# (python -m tests.util_sa_forward_cases prints the tables), rounded up in the third digit, the measured value beside it.
# The adjoint's float32 restatement is FW.adjoint32: one float32 addition per contribution, which is what the kernels' atomics
# do, measured over the orders ADJ_ORDERS (raster, its reverse, two shuffles) and the largest value taken, because the order of the
# atomics is not fixed and the loss of a float32 sum depends on it (psf223 NEAREST_PSF vol_weight: 5.85e-9 in raster order and in
# its reverse, where the few inexact terms meet small partial sums; 3.65e-8 shuffled; the direct scatter on the MI355X 3.6e-8).  The form that carries the scatter sums in float64 (adjoint64(ft=float32)) was measured first -- LINEAR vol_weight 3.30e-8
# (psf335), 5.09e-8 (multi_chunk) -- and does NOT state the kernels' sums: a voxel of these stacks receives hundreds of
# contributions, many of them the same number, and the roundings of such a float32 sum grow with the number of terms
# (multi_chunk: 3.59e-6 in adjoint32; the MI355X gave 3.59e-6 as well, 18 times the bound of the float64-carried form). ---------
def ceil3(x):
    if x == 0:
        return 0.0
    e = math.floor(math.log10(x)) - 2
    return float("%.2e" % (math.ceil(x / 10.0 ** e * (1 - 1e-12)) * 10.0 ** e))


def rel_err(a, b):
    """max |a - b| / max |b| (0 when b is all zero and a equals it)"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    d, s = float(np.abs(a - b).max()), float(np.abs(b).max())
    return 0.0 if d == 0 else (d / s if s > 0 else np.inf)


def measure_fwd(name, mode, r64=None):
    r64 = forward_ref(name, mode) if r64 is None else r64
    r32 = forward_ref(name, mode, F32)
    return rel_err(r32["slices"], r64["slices"]), rel_err(r32["weight"], r64["weight"])


def measure_adj(name, mode, r64=None):
    r64 = adjoint_ref(name, mode) if r64 is None else r64
    keys = ("vol", "vol_weight", "vol_eq")
    runs = [adjoint_ref(name, mode, F32, order) for order in ADJ_ORDERS]
    return tuple(max(rel_err(r[k], r64[k]) for r in runs) for k in keys)


def row(name):
    """the row of the E_cpu tables a case belongs to: the stacks of `counts` and of `shapes` are one case each (one PSF, one volume
    size, one res_slice; a stack of two 1 x 1 slices alone is no sample to measure a rounding cost on)"""
    return "counts" if name.startswith("counts_") else ("shapes" if name.startswith("shapes_") else name)


def _table(names, modes_of, measure, width):
    worst = {}
    for nm in names:
        for md in modes_of(nm):
            e = measure(nm, md)
            worst[row(nm), md] = tuple(max(a, b) for a, b in zip(worst.get((row(nm), md), (0.0,) * width), e))
    for (r, md), e in worst.items():
        print('    ("%s", "%s"): (%s),  # %s' % (r, md, ", ".join("%.2e" % ceil3(v) for v in e), ", ".join("%.3e" % v for v in e)), flush=True)


# (row, mode): (slices, weight)
E_CPU_FWD = {
    ("psf335", "lin_lerp"): (1.71e-07, 0.00e+00),  # 1.708e-07, 0.000e+00
    ("psf335", "lin_weights"): (3.68e-07, 0.00e+00),  # 3.671e-07, 0.000e+00
    ("psf335", "lin_vm"): (3.75e-07, 0.00e+00),  # 3.746e-07, 0.000e+00
    ("psf335", "nn"): (8.54e-08, 0.00e+00),  # 8.534e-08, 0.000e+00
    ("psf335", "nn_vm"): (7.77e-08, 0.00e+00),  # 7.760e-08, 0.000e+00
    ("psf223", "lin_lerp"): (7.34e-08, 0.00e+00),  # 7.337e-08, 0.000e+00
    ("psf223", "lin_weights"): (1.07e-07, 0.00e+00),  # 1.064e-07, 0.000e+00
    ("psf223", "lin_vm"): (1.03e-07, 0.00e+00),  # 1.023e-07, 0.000e+00
    ("psf223", "nn"): (3.86e-08, 0.00e+00),  # 3.854e-08, 0.000e+00
    ("psf223", "nn_vm"): (3.86e-08, 0.00e+00),  # 3.854e-08, 0.000e+00
    ("psf133", "lin_lerp"): (7.51e-08, 0.00e+00),  # 7.504e-08, 0.000e+00
    ("psf133", "lin_weights"): (1.84e-07, 0.00e+00),  # 1.832e-07, 0.000e+00
    ("psf133", "lin_vm"): (1.85e-07, 0.00e+00),  # 1.841e-07, 0.000e+00
    ("psf133", "nn"): (0.00e+00, 0.00e+00),  # 0.000e+00, 0.000e+00
    ("psf133", "nn_vm"): (0.00e+00, 0.00e+00),  # 0.000e+00, 0.000e+00
    ("psf223_big", "lin_lerp"): (1.48e-07, 0.00e+00),  # 1.474e-07, 0.000e+00
    ("psf223_big", "lin_weights"): (2.62e-07, 0.00e+00),  # 2.618e-07, 0.000e+00
    ("psf223_big", "lin_vm"): (2.49e-07, 0.00e+00),  # 2.483e-07, 0.000e+00
    ("psf223_big", "nn"): (6.21e-08, 0.00e+00),  # 6.207e-08, 0.000e+00
    ("psf223_big", "nn_vm"): (5.84e-08, 0.00e+00),  # 5.830e-08, 0.000e+00
    ("delta", "lin_lerp"): (1.02e-07, 0.00e+00),  # 1.018e-07, 0.000e+00
    ("delta", "lin_weights"): (1.06e-07, 0.00e+00),  # 1.060e-07, 0.000e+00
    ("delta", "lin_vm"): (1.06e-07, 0.00e+00),  # 1.060e-07, 0.000e+00
    ("delta", "nn"): (0.00e+00, 0.00e+00),  # 0.000e+00, 0.000e+00
    ("delta", "nn_vm"): (0.00e+00, 0.00e+00),  # 0.000e+00, 0.000e+00
    ("multi_chunk", "lin_lerp"): (4.87e-07, 0.00e+00),  # 4.864e-07, 0.000e+00
    ("multi_chunk", "lin_weights"): (1.32e-06, 0.00e+00),  # 1.319e-06, 0.000e+00
    ("multi_chunk", "lin_vm"): (1.46e-06, 0.00e+00),  # 1.451e-06, 0.000e+00
    ("multi_chunk", "nn"): (2.74e-07, 0.00e+00),  # 2.734e-07, 0.000e+00
    ("multi_chunk", "nn_vm"): (7.01e-07, 0.00e+00),  # 7.002e-07, 0.000e+00
    ("tall", "lin_lerp"): (1.06e-06, 0.00e+00),  # 1.054e-06, 0.000e+00
    ("tall", "lin_weights"): (2.19e-06, 0.00e+00),  # 2.188e-06, 0.000e+00
    ("tall", "lin_vm"): (1.23e-06, 0.00e+00),  # 1.220e-06, 0.000e+00
    ("tall", "nn"): (3.71e-07, 0.00e+00),  # 3.706e-07, 0.000e+00
    ("tall", "nn_vm"): (2.59e-07, 0.00e+00),  # 2.589e-07, 0.000e+00
    ("wide", "lin_lerp"): (1.06e-06, 0.00e+00),  # 1.060e-06, 0.000e+00
    ("wide", "lin_weights"): (2.70e-06, 0.00e+00),  # 2.693e-06, 0.000e+00
    ("plate_limit", "lin_lerp"): (1.61e-06, 0.00e+00),  # 1.604e-06, 0.000e+00
    ("plate_limit", "lin_weights"): (3.39e-06, 0.00e+00),  # 3.385e-06, 0.000e+00
    ("direct_only", "lin_lerp"): (8.09e-07, 0.00e+00),  # 8.080e-07, 0.000e+00
    ("direct_only", "lin_weights"): (2.66e-06, 0.00e+00),  # 2.650e-06, 0.000e+00
    ("generic_big", "lin_lerp"): (1.75e-06, 0.00e+00),  # 1.743e-06, 0.000e+00
    ("generic_big", "lin_weights"): (4.29e-06, 0.00e+00),  # 4.283e-06, 0.000e+00
    ("sparse", "lin_lerp"): (1.69e-07, 0.00e+00),  # 1.682e-07, 0.000e+00
    ("sparse", "lin_weights"): (5.17e-07, 0.00e+00),  # 5.165e-07, 0.000e+00
    ("sparse", "lin_vm"): (2.90e-07, 0.00e+00),  # 2.899e-07, 0.000e+00
    ("sparse", "nn"): (5.06e-08, 0.00e+00),  # 5.054e-08, 0.000e+00
    ("sparse", "nn_vm"): (5.29e-08, 0.00e+00),  # 5.288e-08, 0.000e+00
    ("sparse_zero", "lin_lerp"): (0.00e+00, 0.00e+00),  # 0.000e+00, 0.000e+00
    ("sparse_zero", "lin_weights"): (0.00e+00, 0.00e+00),  # 0.000e+00, 0.000e+00
    ("sparse_zero", "lin_vm"): (0.00e+00, 0.00e+00),  # 0.000e+00, 0.000e+00
    ("sparse_zero", "nn"): (0.00e+00, 0.00e+00),  # 0.000e+00, 0.000e+00
    ("sparse_zero", "nn_vm"): (0.00e+00, 0.00e+00),  # 0.000e+00, 0.000e+00
    ("counts", "lin_lerp"): (1.52e-07, 0.00e+00),  # 1.516e-07, 0.000e+00
    ("counts", "lin_weights"): (4.16e-07, 0.00e+00),  # 4.151e-07, 0.000e+00
    ("counts", "lin_vm"): (2.70e-07, 0.00e+00),  # 2.690e-07, 0.000e+00
    ("counts", "nn"): (8.86e-08, 0.00e+00),  # 8.860e-08, 0.000e+00
    ("counts", "nn_vm"): (7.48e-08, 0.00e+00),  # 7.474e-08, 0.000e+00
    ("shapes", "lin_lerp"): (1.93e-07, 0.00e+00),  # 1.924e-07, 0.000e+00
    ("shapes", "lin_weights"): (3.96e-07, 0.00e+00),  # 3.952e-07, 0.000e+00
    ("shapes", "lin_vm"): (2.66e-07, 0.00e+00),  # 2.653e-07, 0.000e+00
    ("shapes", "nn"): (1.04e-07, 0.00e+00),  # 1.030e-07, 0.000e+00
    ("shapes", "nn_vm"): (7.46e-08, 0.00e+00),  # 7.456e-08, 0.000e+00
    ("lin_psf335", "lin_lerp"): (2.29e-06, 7.33e-08),  # 2.282e-06, 7.328e-08
    ("lin_psf335", "lin_weights"): (2.45e-06, 1.24e-06),  # 2.442e-06, 1.236e-06
    ("lin_psf899", "lin_lerp"): (1.91e-06, 3.56e-07),  # 1.909e-06, 3.551e-07
    ("lin_psf899", "lin_weights"): (2.36e-06, 3.75e-06),  # 2.356e-06, 3.748e-06
    ("gen_psf335", "lin_vm"): (1.50e-06, 6.74e-07),  # 1.497e-06, 6.740e-07
    ("gen_psf335", "nn"): (3.29e-07, 3.73e-07),  # 3.284e-07, 3.723e-07
    ("gen_psf335", "nn_vm"): (3.38e-07, 3.90e-07),  # 3.380e-07, 3.897e-07
    ("gen_psf223_vm", "lin_vm"): (7.28e-06, 4.77e-07),  # 7.278e-06, 4.766e-07
    ("gen_psf223_vm", "nn"): (3.05e-07, 4.93e-07),  # 3.046e-07, 4.920e-07
    ("gen_psf223_vm", "nn_vm"): (2.87e-07, 3.95e-07),  # 2.869e-07, 3.944e-07
}
# (row, mode): (vol, vol_weight, equalised vol)
E_CPU_ADJ = {
    ("psf335", "lin"): (6.22e-07, 4.80e-07, 3.04e-07),  # 6.214e-07, 4.795e-07, 3.031e-07
    ("psf335", "lin_vm"): (5.16e-07, 4.80e-07, 3.19e-07),  # 5.151e-07, 4.795e-07, 3.184e-07
    ("psf335", "nn"): (1.72e-07, 1.13e-07, 1.08e-07),  # 1.719e-07, 1.127e-07, 1.071e-07
    ("psf335", "nn_vm"): (1.49e-07, 1.85e-07, 1.08e-07),  # 1.489e-07, 1.847e-07, 1.071e-07
    ("psf223", "lin"): (1.78e-07, 1.34e-07, 1.96e-07),  # 1.778e-07, 1.339e-07, 1.952e-07
    ("psf223", "lin_vm"): (1.03e-07, 1.42e-07, 1.96e-07),  # 1.029e-07, 1.412e-07, 1.954e-07
    ("psf223", "nn"): (3.17e-08, 3.65e-08, 4.03e-08),  # 3.160e-08, 3.642e-08, 4.026e-08
    ("psf223", "nn_vm"): (5.00e-08, 3.65e-08, 4.03e-08),  # 4.997e-08, 3.642e-08, 4.026e-08
    ("psf133", "lin"): (7.74e-08, 1.90e-07, 1.85e-07),  # 7.737e-08, 1.895e-07, 1.846e-07
    ("psf133", "lin_vm"): (9.70e-08, 2.52e-07, 1.37e-07),  # 9.693e-08, 2.510e-07, 1.365e-07
    ("psf133", "nn"): (0.00e+00, 0.00e+00, 0.00e+00),  # 0.000e+00, 0.000e+00, 0.000e+00
    ("psf133", "nn_vm"): (0.00e+00, 0.00e+00, 0.00e+00),  # 0.000e+00, 0.000e+00, 0.000e+00
    ("psf223_big", "lin"): (4.25e-07, 5.05e-07, 2.58e-07),  # 4.244e-07, 5.040e-07, 2.577e-07
    ("psf223_big", "lin_vm"): (2.93e-07, 5.05e-07, 2.62e-07),  # 2.926e-07, 5.040e-07, 2.614e-07
    ("psf223_big", "nn"): (9.78e-08, 1.42e-07, 8.08e-08),  # 9.776e-08, 1.412e-07, 8.073e-08
    ("psf223_big", "nn_vm"): (8.53e-08, 1.42e-07, 8.08e-08),  # 8.522e-08, 1.412e-07, 8.073e-08
    ("delta", "lin"): (4.06e-08, 0.00e+00, 8.12e-08),  # 4.060e-08, 0.000e+00, 8.120e-08
    ("delta", "lin_vm"): (4.06e-08, 0.00e+00, 8.12e-08),  # 4.060e-08, 0.000e+00, 8.120e-08
    ("delta", "nn"): (0.00e+00, 0.00e+00, 0.00e+00),  # 0.000e+00, 0.000e+00, 0.000e+00
    ("delta", "nn_vm"): (0.00e+00, 0.00e+00, 0.00e+00),  # 0.000e+00, 0.000e+00, 0.000e+00
    ("multi_chunk", "lin"): (7.27e-07, 4.17e-06, 5.91e-07),  # 7.266e-07, 4.165e-06, 5.910e-07
    ("multi_chunk", "lin_vm"): (7.27e-07, 4.17e-06, 5.91e-07),  # 7.266e-07, 4.165e-06, 5.910e-07
    ("multi_chunk", "nn"): (1.89e-07, 4.69e-07, 1.11e-07),  # 1.882e-07, 4.688e-07, 1.107e-07
    ("multi_chunk", "nn_vm"): (2.42e-07, 4.44e-07, 1.26e-07),  # 2.418e-07, 4.439e-07, 1.258e-07
    ("sparse", "lin"): (3.23e-07, 4.52e-07, 1.90e-07),  # 3.229e-07, 4.519e-07, 1.892e-07
    ("sparse", "lin_vm"): (4.09e-07, 4.52e-07, 1.90e-07),  # 4.081e-07, 4.519e-07, 1.892e-07
    ("sparse", "nn"): (1.21e-07, 1.85e-07, 1.31e-07),  # 1.204e-07, 1.841e-07, 1.300e-07
    ("sparse", "nn_vm"): (8.98e-08, 1.48e-07, 8.25e-08),  # 8.974e-08, 1.472e-07, 8.240e-08
    ("gen_psf335", "lin"): (1.36e-06, 1.05e-06, 4.19e-05),  # 1.356e-06, 1.048e-06, 4.181e-05
    ("gen_psf335", "lin_vm"): (1.34e-06, 8.52e-07, 4.19e-05),  # 1.336e-06, 8.519e-07, 4.181e-05
    ("gen_psf335", "nn"): (5.10e-07, 1.87e-07, 4.29e-07),  # 5.093e-07, 1.867e-07, 4.283e-07
    ("gen_psf335", "nn_vm"): (5.10e-07, 1.92e-07, 4.29e-07),  # 5.093e-07, 1.920e-07, 4.283e-07
    ("gen_psf223_vm", "lin"): (1.17e-06, 2.37e-06, 1.91e-05),  # 1.169e-06, 2.362e-06, 1.906e-05
    ("gen_psf223_vm", "lin_vm"): (1.25e-06, 2.37e-06, 1.91e-05),  # 1.243e-06, 2.362e-06, 1.906e-05
    ("gen_psf223_vm", "nn"): (3.85e-07, 3.49e-07, 1.72e-07),  # 3.841e-07, 3.481e-07, 1.715e-07
    ("gen_psf223_vm", "nn_vm"): (3.93e-07, 3.49e-07, 1.72e-07),  # 3.928e-07, 3.481e-07, 1.715e-07
}


if __name__ == "__main__":
    print("E_CPU_FWD = {")
    _table(FORWARD_CASES, fwd_modes, measure_fwd, 2)
    print("}\nE_CPU_ADJ = {")
    _table(ADJOINT_CASES, lambda nm: ADJ_MODES, measure_adj, 3)
    print("}")
    for nm in EXACT_NAMES:
        print(nm, census(case(nm)))
