"""The case table of the warp-family tests, shared by the CPU tests of the references (tests/test_warp64_reference.py) and the GPU
tests of the kernels (tests/test_warp_kernels_edges.py), so that what the CPU tests establish about the bounds holds for the very
cases the GPU tests run (not a test module).

A case is a deformation (tests/util_warp64.Spec), an optional coarse bias grid and the kernel the launcher of csrc/fsg_deform.hip
must choose for it by default once the row workspace is prepared.  Every case runs with and without flip.  Shapes are the smallest
that reach the edge a group is named after; x and y stay tiny wherever only z matters.

group             what it reaches
  z extent        the lean kernel's 32-voxel steps and its two-step loop (n2 around 32, 64, 96), its limits n2 = 2 and 512; the row
                  kernel's register-cached z taps (n2 <= 256) and its uncached loop; the patch kernel's taps in LDS (n2 <= 512) and
                  from global memory; n2 = 1: the per-voxel kernel on every path
  x, y extent     extents of 1; tiles of 8 x 4 (lean), 4 x 4 (patch), 16 rows at stride 4 (row kernel) with dead rows; workgroup
                  counts that are and are not a multiple of 8 (xcd_tile)
  coarse grids    f2 across the lean kernel's 32, the patch kernel's 128 floats (3 * f2, and 3 * f2 + b2 only with the bias), the
                  row kernels' 512 floats (beyond: per-voxel warp and min/max, FSG_E_TOOBIG from the floor(min) entry, no row
                  workspace); b2 across the lean kernel's 32; grids beyond deform_rows_block_kernel's LDS slabs
  exact positions no field and an affine whose arithmetic is exact in float32: ties, zeros, the last plane / row / column, axis
                  permutations, both sides of the lean kernel's pacing threshold, a -0.0 coordinate
  outside         every position beyond one of the six faces
  nonzero margins floor(min) >= 1 on every axis; the floor(min) shortcut's case: every face voxel >= 1, an interior voxel below
  generic         rotations, shears, random fields; ragged shapes
"""
import zlib
from collections import namedtuple

import numpy as np

from fetalsyngen_amd import tables as T
from fetalsyngen_amd.utils.generation import make_affine_matrix
from tests.util_warp64 import make_spec

F = np.float32
Case = namedtuple("Case", "name spec bias bias_tabs kernel exact")
GROUPS = ("z extent", "x, y extent", "coarse grids", "exact positions", "outside", "nonzero margins", "generic")

LEAN_F2CAP = LEAN_B2CAP = 32
LEAN_TZCAP = 512
PATCH_ROWCAP = 128
ROWCAP = 512
RB_SLAB_F, RB_SLAB_B, RB_NEED = 2048, 256, 512


def grid_tabs(gshape, shape):
    tabs, new = T.zoom_tables(tuple(gshape[:3]), np.array(shape) / np.array(gshape[:3]))
    assert new == tuple(shape), (gshape, shape, new)
    return tabs


def rows_need(case, with_bias=True):
    f2 = case.spec.field.shape[2] if case.spec.field is not None else 0
    b2 = case.bias.shape[2] if (case.bias is not None and with_bias) else 0
    return 3 * f2 + b2


def has_workspace(case):
    """kernels.DeformSpec.prepare_rows leaves a workspace for 0 < need <= 512."""
    return 0 < rows_need(case) <= ROWCAP


def rows_block_fits(case):
    """rows_block_fits of csrc/fsg_deform.hip: deform_rows_block_kernel, else deform_rows_kernel."""
    fs = case.spec.field.shape if case.spec.field is not None else (0, 0, 0)
    bs = case.bias.shape if case.bias is not None else (0, 0, 0)
    return fs[1] * fs[2] * 3 <= RB_SLAB_F and bs[1] * bs[2] <= RB_SLAB_B and rows_need(case) <= RB_NEED


def warp_kernel(case, flags, TUNE, rows, with_bias):
    """launch_warp of csrc/fsg_deform.hip restated: the kernel a warp of `case` lands on under the tuning `flags`, with (`rows`)
    or without a prepared row workspace, with or without the bias in the epilogue.  A change of the launcher's conditions changes
    this function with it."""
    n0, n1, n2 = case.spec.shape
    f2 = case.spec.field.shape[2] if case.spec.field is not None else 0
    b2 = case.bias.shape[2] if (case.bias is not None and with_bias) else 0
    need = 3 * f2 + b2
    rows = rows and has_workspace(case)
    if not flags & (TUNE.GENERIC_WARP | TUNE.NO_PATCH | TUNE.NO_LEAN):
        if (need == 0 or rows) and f2 <= LEAN_F2CAP and b2 <= LEAN_B2CAP and 2 <= n2 <= LEAN_TZCAP and n1 * n2 < 1 << 22 \
                and n0 * n1 * n2 < 1 << 30:
            return "lean"
    if need <= PATCH_ROWCAP and n2 >= 2 and not flags & (TUNE.GENERIC_WARP | TUNE.NO_PATCH):
        return "patch"
    if need <= ROWCAP and n2 >= 2 and not flags & TUNE.GENERIC_WARP:
        return "rows"
    return "voxel"


def minmax_kernel(case, flags, TUNE):
    """fsg_coords_minmax_f32: the row kernel for 3 * f2 <= 512 unless GENERIC_WARP, else the per-voxel kernel."""
    f2 = case.spec.field.shape[2] if case.spec.field is not None else 0
    return "rows" if 3 * f2 <= ROWCAP and not flags & TUNE.GENERIC_WARP else "voxel"


def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def _case(name, shape, A=None, shift=(0.3, -0.2, 0.4), fshape=None, fstd=1.5, bshape=None, kernel="lean", exact=False, cen=None,
          c2=None, field=None):
    shape = tuple(shape)
    rs = _rs(name)
    if cen is None:
        cen = (np.array(shape) - 1) / 2
    if c2 is None:
        c2 = np.asarray(cen, dtype=F) + np.asarray(shift, dtype=F)
    if A is None:
        A = make_affine_matrix([0.12, -0.1, 0.15], [0.01, -0.02, 0.015], [1.04, 0.96, 1.02])
    tabs = None
    if field is None and fshape is not None:
        field = (rs.randn(*fshape, 3) * fstd).astype(F)
    if field is not None:
        tabs = grid_tabs(field.shape, shape)
    bias = btabs = None
    if bshape is not None:
        bias = (rs.randn(*bshape) * 0.3).astype(F)
        btabs = grid_tabs(bshape, shape)
    return Case(name, make_spec(shape, A, cen, c2, field, tabs), bias, btabs, kernel, exact)


def _z_extent():
    out = []
    for n2 in (2, 3, 31, 32, 33, 63, 64, 65, 96, 97):
        out.append(_case(f"(9,6,{n2})", (9, 6, n2), fshape=(3, 2, min(n2, 4)), bshape=(2, 2, 2)))
    for n2 in (255, 256, 257, 511, 512, 513, 520):
        out.append(_case(f"(3,5,{n2})", (3, 5, n2), fshape=(2, 2, 5), fstd=4.0, bshape=(2, 2, 3),
                         kernel="lean" if n2 <= LEAN_TZCAP else "patch"))
    out.append(_case("(5,4,1)", (5, 4, 1), fshape=(2, 2, 1), bshape=(2, 2, 1), kernel="voxel"))
    return out


def _xy_extent():
    out = [_case(f"{s}", s, fshape=(min(s[0], 3), min(s[1], 2), 3), bshape=(1, 1, 2))
           for s in ((1, 1, 2), (1, 5, 40), (9, 1, 40), (7, 3, 33), (8, 4, 33), (9, 5, 33), (17, 9, 40))]
    # lean: ceil(n0 / 8) * ceil(n1 / 4) workgroups; patch: ceil(n0 / 4) * ceil(n1 / 4); row kernel: n0 * ceil(n1 / 16)
    out.append(_case("(16,16,34): 8 lean, 16 patch, 16 row workgroups", (16, 16, 34), fshape=(3, 3, 3), bshape=(2, 2, 2)))
    out.append(_case("(24,12,34): 9 lean, 18 patch, 24 row workgroups", (24, 12, 34), fshape=(3, 3, 3), bshape=(2, 2, 2)))
    out.append(_case("(20,17,34): 15 lean, 25 patch, 40 row workgroups", (20, 17, 34), fshape=(3, 3, 3), bshape=(2, 2, 2)))
    return out


def _coarse_grids():
    out = []
    for f2 in (1, 2, 31, 32, 33, 42, 43, 170, 171):
        kernel = "lean" if f2 <= 32 else "patch" if 3 * f2 <= PATCH_ROWCAP else "rows" if 3 * f2 <= ROWCAP else "voxel"
        out.append(_case(f"f2={f2}", (4, 5, 2 * f2), fshape=(2, 2, f2), kernel=kernel))
    for b2 in (1, 32, 33):
        out.append(_case(f"b2={b2}", (4, 5, 66), fshape=(2, 2, 4), bshape=(2, 2, b2), kernel="lean" if b2 <= 32 else "patch"))
    # 3 * 42 = 126 floats without the bias (patch kernel), 129 with it (row kernel)
    out.append(_case("f2=42 b2=3: 128 floats crossed by the bias", (4, 5, 84), fshape=(2, 2, 42), bshape=(2, 2, 3), kernel="rows"))
    out.append(_case("f2=170 b2=2: 512 floats", (4, 5, 340), fshape=(2, 2, 170), bshape=(2, 2, 2), kernel="rows"))
    out.append(_case("f2=170 b2=3: 512 floats crossed by the bias, no workspace", (4, 5, 340), fshape=(2, 2, 170), bshape=(2, 2, 3),
                     kernel="voxel"))
    # deform_rows_kernel: f1 * f2 * 3 = 2100 > 2048; b1 * b2 = 260 > 256
    out.append(_case("field slab 5*140*3", (4, 5, 280), fshape=(2, 5, 140), kernel="rows"))
    out.append(_case("bias slab 5*52", (4, 5, 104), fshape=(2, 2, 3), bshape=(2, 5, 52), kernel="patch"))
    for c in out:
        assert c.spec.shape[0] <= 5 and c.spec.shape[1] <= 5
    assert all(has_workspace(c) and not rows_block_fits(c) for c in out[-2:]) and all(rows_block_fits(c) for c in out[:-2] if has_workspace(c))
    return out


EYE = np.eye(3)


def _exact(name, shape, A=EYE, s=(0, 0, 0), cen=None, c2=None, **kw):
    """No field, centre and shifts multiples of 0.5, matrix entries small dyadic numbers: every operation of the position is exact."""
    shape = tuple(shape)
    if cen is None:
        cen = (np.array(shape) - 1) / 2
    if c2 is None:
        c2 = np.asarray(cen) + np.asarray(s, dtype=np.float64)
    return _case(name, shape, A=A, cen=cen, c2=c2, exact=True, **kw)


def _exact_positions():
    n = (9, 6, 33)
    out = [_exact("identity (the last plane, row and column alone and at once)", n)]
    out += [_exact(f"identity, shift {s}", n, s=s) for s in ((1, 0, 0), (0, -2, 0), (0, 0, 3), (-1, 2, -30))]
    for a in range(3):
        s = [0.0, 0.0, 0.0]
        s[a] = 0.5
        out.append(_exact(f"shift 0.5 on axis {a} (ties)", n, s=s))
        s[a] = -0.5
        out.append(_exact(f"shift -0.5 on axis {a} (ties)", n, s=s))
    for a in range(3):  # a zero row and c2 = 0: the coordinate is exactly 0 everywhere, the image is 0
        A = EYE.copy()
        A[a, a] = 0.0
        c2 = (np.array(n) - 1) / 2
        c2[a] = 0.0
        out.append(_exact(f"coordinate {a} exactly 0", n, A=A, c2=c2))
    # twice the index: every voxel from the middle on sits exactly on the last plane, row and column; margins stay 0
    out.append(_exact("scale 2 about the origin", n, A=2 * EYE, cen=(0, 0, 0), c2=(0, 0, 0)))
    for a in range(3):
        A = EYE.copy()
        A[a, a] = 2.0
        out.append(_exact(f"scale 2 on axis {a}", n, A=A, cen=(0, 0, 0), c2=(0, 0, 0)))
    # axis permutations (90 degree rotations): |A[2]| or |A[5]| is 1
    out.append(_exact("x <- z, y <- x, z <- y", (9, 10, 12), A=[[0, 0, 1], [1, 0, 0], [0, 1, 0]], s=(0, 0.5, 0)))
    out.append(_exact("x <- y, y <- -z, z <- x", (9, 10, 12), A=[[0, 1, 0], [0, 0, -1], [1, 0, 0]], s=(0.5, 0, 0)))
    out.append(_exact("x <- -z, y <- y, z <- x", (12, 5, 12), A=[[0, 0, -1], [0, 1, 0], [1, 0, 0]]))
    # the lean kernel's pacing: slope = max(|A[2]|, |A[5]|) < 0.27 -> a barrier every second step, else every step
    for sl in (0.25, 0.5):
        out.append(_exact(f"shear {sl} of x along z", (9, 6, 70), A=[[1, 0, sl], [0, 1, 0], [0, 0, 1]]))
        out.append(_exact(f"shear {sl} of y along z", (9, 6, 70), A=[[1, 0, 0], [0, 1, sl], [0, 0, 1]]))
    # x = -i + (-0.0) * |..| + (-0.0): -0.0 at i = 0 and +0.0 (clamped) elsewhere: the minimum's key is key(-0.0)
    out.append(_exact("x is -0.0 at i = 0", (5, 6, 34), A=[[-1, 0, 0], [0, 1, 0], [0, 0, 1]], cen=(0, 6, 34), c2=(-0.0, 6, 34)))
    return out


def _outside():
    n = (9, 6, 33)
    out = []
    for a in range(3):
        for sign in (-1, 1):
            s = [0.25, -0.25, 0.25]
            s[a] = sign * (n[a] + 2)
            out.append(_case(f"beyond the {'low' if sign < 0 else 'high'} face of axis {a}", n, A=EYE, shift=s))
    return out


def _nonzero_margins():
    n = (12, 12, 40)
    out = [_case("translation 1.5, 2.25, 3.5", n, A=EYE, shift=(1.5, 2.25, 3.5), exact=True),
           _case("scale 0.5 about the far corner", n, A=0.5 * EYE, cen=np.array(n) - 1, c2=np.array(n) - 1.25, exact=True)]
    # every face voxel keeps its 1.25 (the coarse grid's face nodes are 0 and a face voxel interpolates face nodes only), the
    # middle node pulls the voxels around the centre below 1: the six-face pass leaves all three axes open, the full pass settles
    f = np.zeros((3, 3, 3, 3), F)
    f[1, 1, 1] = (-20.0, -20.0, -60.0)
    out.append(_case("floor(min) shortcut: only interior voxels below 1", n, A=EYE, shift=(1.25, 1.25, 1.25), field=f))
    return out


def _generic():
    A = lambda rot: make_affine_matrix([rot, -rot, rot], [0.01, -0.02, 0.015], [1.05, 0.95, 1.02])  # noqa: E731
    return [_case("typical (70,60,100)", (70, 60, 100), A=A(0.15), fshape=(5, 4, 7), fstd=2.0, bshape=(3, 2, 4)),
            _case("no field (33,17,48)", (33, 17, 48), A=A(0.2), bshape=(3, 2, 4)),
            _case("fine grid (40,40,40)", (40, 40, 40), A=A(0.1), fshape=(20, 20, 20), fstd=2.0, bshape=(3, 2, 4)),
            _case("extreme (64,64,64)", (64, 64, 64), A=A(0.7), fshape=(4, 4, 4), fstd=6.0, bshape=(3, 2, 4)),
            _case("ragged (50,37,70)", (50, 37, 70), A=A(0.2), fshape=(5, 4, 6), fstd=2.0, bshape=(2, 3, 2))]


_BUILDERS = {"z extent": _z_extent, "x, y extent": _xy_extent, "coarse grids": _coarse_grids, "exact positions": _exact_positions,
             "outside": _outside, "nonzero margins": _nonzero_margins, "generic": _generic}
_CACHE = {}


def cases(group):
    if group not in _CACHE:
        _CACHE[group] = _BUILDERS[group]()
    return _CACHE[group]


def all_cases():
    return [c for g in GROUPS for c in cases(g)]


def sources(case):
    """The sources of a case, all finite (the kernels' contract):
      img     float32 with structure, negative values, exact zeros and -0.0
      pos     a non-negative image on the 0..255 scale (the gamma cases)
      signs   -0.0 on the last column, negative on the column before it, positive elsewhere: the sign of an output zero depends
              on which neighbours a kernel multiplies by its zero weights
      lab8    uint8 labels over 0..255
      labf    float32 labels that are not integers
    The GPU tests also hand img and lab8 over as contiguous device views that start 4 bytes and 1 byte into their buffers."""
    shape = case.spec.shape
    rs = _rs("sources " + case.name)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    img = (90 * np.sin(0.9 * g[0] + 0.3) * np.cos(0.7 * g[1]) + 60 * np.sin(0.23 * g[2] + 0.1 * g[0]) + rs.randn(*shape) * 20).astype(F)
    u = rs.rand(*shape)
    img[u < 0.1] = 0.0
    img[u > 0.9] = -0.0
    pos = np.clip(np.abs(img) + rs.rand(*shape).astype(F) * 5, 0, 255).astype(F)
    pos[u < 0.1] = 0.0
    signs = (1 + rs.rand(*shape) * 9).astype(F)
    if shape[2] >= 2:
        signs[:, :, -2] *= -1
    signs[:, :, -1] = -0.0
    lab8 = rs.randint(0, 256, shape).astype(np.uint8)
    lab8.ravel()[:256] = np.arange(256)[:lab8.size]
    labf = (rs.rand(*shape) * 40 - 3.7).astype(F)
    assert all(np.isfinite(a).all() for a in (img, pos, signs, labf)) and (img.size < 64 or np.signbit(img[img == 0]).any())
    return dict(img=img, pos=pos, signs=signs, lab8=lab8, labf=labf)
