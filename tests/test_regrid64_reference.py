"""CPU: the float64 restatement tests/util_regrid64.py against scipy.ndimage.map_coordinates away from the boundary, and its
own boundary, fill and tie rules against hand-computed 1-D cases."""
import numpy as np
from scipy import ndimage

from tests import util_regrid64 as R


def test_image_and_label_match_scipy_well_inside():
    rng = np.random.default_rng(0)
    shape, out_shape = (19, 23, 17), (37, 30, 42)
    img = rng.random(shape)
    lab = rng.integers(0, 9, shape).astype(np.int16)
    A = R.rotation(20, -11, 7) * 0.43
    M = np.concatenate([A, np.array([[3.1], [9.7], [2.2]])], axis=1)
    box = [0, 18, 0, 22, 0, 16]
    out, out_lab, p, ok = R.resample(img, lab, M, box, out_shape)
    well = np.ones(out_shape, dtype=bool)
    for a in range(3):
        well &= (p[a] >= 0.25) & (p[a] <= shape[a] - 1.25)
    assert well.mean() > 0.05 and ok[well].all()
    ref = ndimage.map_coordinates(img, p.reshape(3, -1), order=1, mode="nearest").reshape(out_shape)
    assert np.abs(out - ref)[well].max() <= 1e-13
    # order 0 rounds half away from zero / up in places: compare where no coordinate is near a tie
    clear = well & ~R.near_decision(p, box, 1e-9)
    ref_lab = ndimage.map_coordinates(lab, p.reshape(3, -1), order=0, mode="nearest").reshape(out_shape)
    assert np.array_equal(out_lab[clear], ref_lab[clear])
    # the whole inside region against scipy's border replication (mode="nearest" clamps the coordinate, as the box does)
    assert np.abs(out - ref)[ok].max() <= 1e-13
    assert (out[~ok] == 0).all() and (out_lab[~ok] == 0).all()


def _line(values, positions, lo, hi, fill=-1.0, label=None):
    """1-D cases along z: source (1,1,n), output position t reads source coordinate positions[t]."""
    n = len(values)
    src = np.asarray(values, dtype=np.float64).reshape(1, 1, n)
    out = []
    for pz in positions:
        M = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, pz]], dtype=np.float64)
        img, lab, _p, _ok = R.resample(src, None if label is None else np.asarray(label).reshape(1, 1, n), M,
                                       [0, 0, 0, 0, lo, hi], (1, 1, 1), fill=fill, fill_label=99)
        out.append((float(img[0, 0, 0]), None if lab is None else int(lab[0, 0, 0])))
    return out


def test_boundary_fill_and_ties_by_hand():
    values = [10.0, 20.0, 40.0, 80.0, 160.0]
    label = np.array([1, 2, 3, 4, 5], dtype=np.uint8)
    got = _line(values, [-0.75, -0.5, -0.25, 0.0, 0.5, 1.25, 1.5, 2.5, 3.5, 4.0, 4.25, 4.5, 4.51], 0, 4, label=label)
    want = [(-1.0, 99),      # beyond lo - 0.5: fill
            (10.0, 1),       # exactly lo - 0.5 is inside, clamped to lo
            (10.0, 1),       # replication
            (10.0, 1),
            (15.0, 1),       # 0.5 -> rint 0 (even)
            (25.0, 2),       # 0.75 * 20 + 0.25 * 40
            (30.0, 3),       # 1.5 -> rint 2 (even)
            (60.0, 3),       # 2.5 -> rint 2 (even)
            (120.0, 5),      # 3.5 -> rint 4 (even)
            (160.0, 5),      # on the last voxel: upper neighbour clamped, weight 0
            (160.0, 5),      # replication
            (160.0, 5),      # exactly hi + 0.5 is inside
            (-1.0, 99)]
    assert got == want
    # a box strictly inside: replication at the BOX, fill beyond it, the voxels outside the box are never read
    got = _line(values, [0.4, 0.5, 0.9, 1.0, 2.75, 3.0, 3.5, 3.6], 1, 3, label=label)
    assert got == [(-1.0, 99), (20.0, 2), (20.0, 2), (20.0, 2), (70.0, 4), (80.0, 4), (80.0, 4), (-1.0, 99)]
    # an extent of one: every inside position reads that voxel
    assert _line([7.0], [-0.5, 0.0, 0.5, 0.6], 0, 0, label=np.array([3], dtype=np.uint8)) == [(7.0, 3), (7.0, 3), (7.0, 3), (-1.0, 99)]


def test_blend_order_and_nan_rule():
    src = np.arange(8, dtype=np.float64).reshape(2, 2, 2)
    M = np.array([[0, 0, 0, 0.25], [0, 0, 0, 0.5], [0, 0, 0, 0.75]])
    out, _l, _p, _ok = R.resample(src, None, M, [0, 1, 0, 1, 0, 1], (1, 1, 1))
    assert out[0, 0, 0] == 0.25 * 4 + 0.5 * 2 + 0.75 * 1
    src[0, 0, 0] = np.nan
    out, _l, _p, _ok = R.resample(src, None, M, [0, 1, 0, 1, 0, 1], (1, 1, 1))
    assert np.isnan(out[0, 0, 0])
    out, _l, _p, _ok = R.resample(src, None, M, [0, 1, 0, 1, 0, 1], (1, 1, 1), nan_is_zero=True)
    assert np.isfinite(out[0, 0, 0])


def test_bbox_restatement():
    v = np.zeros((4, 5, 6), dtype=np.float32)
    assert R.bbox_gt(v) == [4, -1, 5, -1, 6, -1]
    v[1, 2, 3] = 1
    v[3, 0, 5] = np.nan
    assert R.bbox_gt(v) == [1, 1, 2, 2, 3, 3]
    v[2, 4, 0] = 0.5
    assert R.bbox_gt(v) == [1, 2, 2, 4, 0, 3] and R.bbox_gt(v, 0.75) == [1, 1, 2, 2, 3, 3]


def test_coordinate_error_of_float32_evaluation():
    """What the issue states for the kernel's coordinate arithmetic, checked here in numpy float32: the order
    (m0 i + m1 j) + m2 k + m3 stays within 2^-13 of float64 at extent 512 and is exact on a 2^-8 grid."""
    rng = np.random.default_rng(1)
    idx = rng.integers(0, 512, (3, 200000)).astype(np.float32)
    A = (R.rotation(20, -11, 7) * 0.77).astype(np.float32)
    t = np.array([20.3, -11.7, 31.9], dtype=np.float32)
    p32 = (A[:, 0:1] * idx[0] + A[:, 1:2] * idx[1]) + A[:, 2:3] * idx[2] + t[:, None]
    assert p32.dtype == np.float32
    p64 = A.astype(np.float64) @ idx.astype(np.float64) + t.astype(np.float64)[:, None]
    assert np.abs(p32 - p64).max() <= 2.0 ** -13
    G = (rng.integers(-512, 513, (3, 4)) / 256.0).astype(np.float32)
    q32 = (G[:, 0:1] * idx[0] + G[:, 1:2] * idx[1]) + G[:, 2:3] * idx[2] + G[:, 3:4]
    q64 = G[:, :3].astype(np.float64) @ idx.astype(np.float64) + G[:, 3:4].astype(np.float64)
    assert np.array_equal(q32.astype(np.float64), q64)
