"""Float64 numpy restatement of the affine resample (csrc/fsg_regrid.hip `fsg_affine_resample`) and of the foreground box
(`fsg_bbox_gt_f32`).  tests/test_regrid64_reference.py pins it to scipy.ndimage.map_coordinates and to hand-computed
1-D cases; the GPU tests compare the kernels with it.

Contract restated: p = M (i,j,k,1); inside iff lo_a - 0.5 <= p_a <= hi_a + 0.5 on every axis (else fill); inside, p is
clamped to [lo_a, hi_a]; image = trilinear with f = floor(p), upper neighbour clamped to hi_a, weights 1-w and w, blended
z first, then y, then x; label = the voxel at rint(p) (round half to even)."""
import numpy as np


def coordinates(M, out_shape):
    """(3, d0, d1, d2) float64 source coordinates of every output voxel; M is used with the values it holds (a float32
    matrix is widened, not re-derived)."""
    M = np.asarray(M, dtype=np.float64).reshape(3, 4)
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in out_shape], indexing="ij")
    return np.stack([M[a, 0] * i + M[a, 1] * j + M[a, 2] * k + M[a, 3] for a in range(3)])


def inside_mask(p, box):
    box = np.asarray(box).reshape(3, 2)
    ok = np.ones(p.shape[1:], dtype=bool)
    for a in range(3):
        ok &= (p[a] >= box[a, 0] - 0.5) & (p[a] <= box[a, 1] + 0.5)
    return ok


def resample(image, label, M, box, out_shape, fill=0.0, fill_label=0, nan_is_zero=False):
    """-> (image float64 | None, label in the input's dtype | None, p, inside)."""
    box = np.asarray(box).reshape(3, 2)
    p = coordinates(M, out_shape)
    ok = inside_mask(p, box)
    c = np.stack([np.clip(p[a], box[a, 0], box[a, 1]) for a in range(3)])
    out_img = out_lab = None
    if image is not None:
        src = np.asarray(image, dtype=np.float64)
        if nan_is_zero:
            src = np.where(np.isnan(src), 0.0, src)
        f = np.floor(c)
        w = c - f
        i0 = f.astype(np.int64)
        i1 = np.stack([np.minimum(i0[a] + 1, box[a, 1]) for a in range(3)])

        def g(x, y, z):
            return src[x, y, z]

        wx, wy, wz = w
        z00 = (1 - wz) * g(i0[0], i0[1], i0[2]) + wz * g(i0[0], i0[1], i1[2])
        z01 = (1 - wz) * g(i0[0], i1[1], i0[2]) + wz * g(i0[0], i1[1], i1[2])
        z10 = (1 - wz) * g(i1[0], i0[1], i0[2]) + wz * g(i1[0], i0[1], i1[2])
        z11 = (1 - wz) * g(i1[0], i1[1], i0[2]) + wz * g(i1[0], i1[1], i1[2])
        y0 = (1 - wy) * z00 + wy * z01
        y1 = (1 - wy) * z10 + wy * z11
        out_img = np.where(ok, (1 - wx) * y0 + wx * y1, float(fill))
    if label is not None:
        lab = np.asarray(label)
        r = np.rint(c).astype(np.int64)  # numpy rounds half to even
        out_lab = np.where(ok, lab[r[0], r[1], r[2]], np.asarray(fill_label, dtype=lab.dtype)).astype(lab.dtype)
    return out_img, out_lab, p, ok


def near_decision(p, box, delta):
    """Voxels whose float64 coordinate lies within `delta` of a half-integer (label tie, and the inside test's faces,
    which sit on half-integers) on any axis: where a coordinate error below delta may change the decision."""
    box = np.asarray(box).reshape(3, 2)
    near = np.zeros(p.shape[1:], dtype=bool)
    for a in range(3):
        h = p[a] - 0.5
        near |= np.abs(h - np.rint(h)) <= delta
        near |= (np.abs(p[a] - (box[a, 0] - 0.5)) <= delta) | (np.abs(p[a] - (box[a, 1] + 0.5)) <= delta)
    return near


def bbox_gt(v, thr=0.0):
    """Inclusive index box lo0,hi0,lo1,hi1,lo2,hi2 of v > thr (NaN compares false); empty: lo = n, hi = -1."""
    v = np.asarray(v)
    with np.errstate(invalid="ignore"):
        m = v > thr
    out = []
    for a in range(3):
        idx = np.nonzero(m.any(axis=tuple(b for b in range(3) if b != a)))[0]
        out += [int(idx[0]), int(idx[-1])] if idx.size else [v.shape[a], -1]
    return out


def face_gradient(x):
    """Largest absolute difference between face neighbours, and the largest absolute value."""
    x = np.asarray(x, dtype=np.float64)
    g = max((float(np.abs(np.diff(x, axis=a)).max()) if x.shape[a] > 1 else 0.0) for a in range(3))
    return g, float(np.abs(x).max())


def rotation(deg_z, deg_x, deg_y):
    """Rz(deg_z) Rx(deg_x) Ry(deg_y), float64."""
    z, x, y = np.deg2rad([deg_z, deg_x, deg_y])
    Rz = np.array([[np.cos(z), -np.sin(z), 0], [np.sin(z), np.cos(z), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(x), -np.sin(x)], [0, np.sin(x), np.cos(x)]])
    Ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    return Rz @ Rx @ Ry
