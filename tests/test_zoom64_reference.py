"""CPU: the references of the zoom family (tests/util_zoom64.py) are right before anything on the GPU is trusted to them.

  * zoom32 is the golden zoom bit for bit (tests/golden/zoom.npz, captured from the reference's myzoom_torch) and, where the
    oracle package is present, the oracle's restatements of myzoom_torch (linear_zoom) and fast_3D_interp_torch (sample_linear);
  * zoom32 lies within util_resample64.error_bound of zoom64 on every case of the GPU file's case table, and reaches a stated
    fraction of it (the bound is neither violated by float32 itself nor vacuous);
  * normalise32 on hand-computed cases, and against the oracle's resize_back + scale01;
  * the order keys: round trip, -0.0 < +0.0 < denormal, identities.
"""
import numpy as np
import pytest
import torch

from fetalsyngen_amd import tables as T
from tests import util_zoom64 as Z
from tests.util_zoom_cases import all_cases, sources

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == F and np.array_equal(bits(a), bits(b))


def test_zoom32_is_the_golden_zoom_bit_for_bit(golden):
    g = golden("zoom")
    n = int(g["ncases"])
    assert n >= 1
    for i in range(n):
        x, factor = g[f"x_{i}"], g[f"factor_{i}"]
        tabs, new = T.zoom_tables(x.shape[:3], factor)
        y = Z.zoom32(x, tabs)
        assert y.shape[:3] == new
        assert same_bits(y, g[f"y_{i}"]), i


def test_zoom32_is_the_oracle_zoom_and_trilinear_gather_bit_for_bit():
    O = pytest.importorskip("oracle.fsg_oracle")
    rs = np.random.RandomState(5)
    for shape, factor in (((6, 10, 12), (2.0, 3.0, 7.3)), ((9, 7, 11), (0.5, 1.0, 0.34)), ((5, 4, 3, 3), (2.6, 1.0, 4.1))):
        x = (rs.rand(*shape) * 255).astype(F)
        tabs, _ = T.zoom_tables(shape[:3], np.array(factor))
        assert same_bits(Z.zoom32(x, tabs), O.linear_zoom(torch.from_numpy(x), np.array(factor)).numpy()), (shape, factor)
    # fast_3D_interp_torch at RandResample's axis-aligned positions (m == n: position 0 is outside)
    shape = (8, 9, 10)
    x = (rs.rand(*shape) * 255).astype(F)
    for m in ((4, 9, 3), (8, 1, 10), (7, 8, 9)):
        pos = []
        for a in range(3):
            f = np.float64(m[a]) / np.float64(shape[a])
            d = (1.0 - f) / (2.0 * f)
            pos.append(np.arange(d, d + m[a] / f, 1 / f)[: m[a]])
        ii, jj, kk = (torch.tensor(a, dtype=torch.float32) for a in np.meshgrid(*pos, sparse=False, indexing="ij"))
        want = O.sample_linear(torch.from_numpy(x), ii, jj, kk).numpy()
        tabs = [T._resample_axis_table(m[a], shape[a]) for a in range(3)]
        assert same_bits(Z.zoom32(x, tabs), want), m


# The largest |zoom32 - zoom64| / error_bound over the case table, measured here from zoom32 itself (this test prints it: 0.7560,
# at "rows=529984 (728x728)" with the twelve-decade source, where products of both signs cancel).  The bound is a worst case over
# six roundings that all go the same way; a float32 result that reaches three quarters of it shows the bound is not vacuous.
# The operations are IEEE, so the figure does not depend on the numpy at hand; the assertion asks for half, which leaves room
# for edits of the case table only.
MIN_RATIO = 0.5


def test_float32_zoom_lies_within_the_rounding_bound_and_reaches_half_of_it():
    worst = (0.0, None)
    for case in all_cases():
        for label, x in sources(case):
            y32 = Z.zoom32(x, case.tabs)
            y64 = Z.zoom64(x, case.tabs)
            bound = Z.zoom_bound(x, case.tabs)
            assert y32.shape == y64.shape == bound.shape
            nan = np.isnan(y64)
            assert np.array_equal(nan, np.isnan(y32)), (case.name, label)
            err = np.abs(y32.astype(np.float64) - y64)
            assert (err[~nan] <= bound[~nan]).all(), (case.name, label, float(np.nanmax(err / bound)))
            assert (y32[bound == 0] == 0).all(), (case.name, label)
            out = Z.outside_mask(case.tabs, x.ndim) & np.ones(y32.shape, bool)
            assert (bits(y32)[out] == 0).all(), (case.name, label)  # +0.0, not -0.0
            ok = ~nan & (bound > 0)
            if ok.any():
                r = float((err[ok] / bound[ok]).max())
                if r > worst[0]:
                    worst = (r, f"{case.name} / {label}")
    print(f"ZOOM64 largest error / bound = {worst[0]:.4f} at {worst[1]}")
    assert worst[0] <= 1.0
    assert worst[0] > MIN_RATIO, worst


def test_normalise32_by_hand():
    y = np.array([0.0, 1.0, 2.0, 3.0, 4.0], F)
    # mode 0: y / max
    assert same_bits(Z.normalise32(y, 0.0, 4.0, 0), np.array([0.0, 0.25, 0.5, 0.75, 1.0], F))
    # min == 0: mode 1 equals mode 0
    assert same_bits(Z.normalise32(y, 0.0, 4.0, 1), Z.normalise32(y, 0.0, 4.0, 0))
    # min 1, max 5: t = y / 5, q = 0.2, (t - q) / (1 - q); y = 1 -> 0, y = 5 -> 1
    y = np.array([1.0, 3.0, 5.0], F)
    t, q = y / F(5), F(1) / F(5)
    want = (t - q) / (F(1) - q)
    assert same_bits(Z.normalise32(y, 1.0, 5.0, 1), want) and want[0] == 0 and want[2] == 1
    # a flat image: mode 1 is all +0.0 (t * 0), for c > 0 and c < 0; mode 0 is all 1
    for c in (7.25, -3.5):
        flat = np.full(6, c, F)
        assert (bits(Z.normalise32(flat, c, c, 1)) == 0).all()
        assert same_bits(Z.normalise32(flat, c, c, 0), np.ones(6, F))
    # all negative: min -4, max -1: q = 4 > 1, the denominator 1 - q = -3 is negative; t = y / -1 = -y in [1, 4]
    y = np.array([-4.0, -2.5, -1.0], F)
    got = Z.normalise32(y, -4.0, -1.0, 1)
    assert same_bits(got, np.array([(4.0 - 4.0) / -3.0, (2.5 - 4.0) / -3.0, (1.0 - 4.0) / -3.0], F))
    assert same_bits(got, np.array([-0.0, 0.5, 1.0], F))  # the minimum maps to -0.0: (+0.0) / (-3)
    # max == 0: 0 / 0 is NaN in both modes, a negative over 0 is -inf in mode 0 and NaN in mode 1 (q = -inf or NaN)
    y = np.array([0.0, -2.0], F)
    m0, m1 = Z.normalise32(y, -2.0, 0.0, 0), Z.normalise32(y, -2.0, 0.0, 1)
    assert np.isnan(m0[0]) and m0[1] == -np.inf and np.isnan(m1).all()
    assert np.isnan(Z.normalise32(np.zeros(3, F), 0.0, 0.0, 0)).all() and np.isnan(Z.normalise32(np.zeros(3, F), 0.0, 0.0, 1)).all()
    # min -0.0: q = -0.0, t - q = t + 0.0: a -0.0 voxel becomes +0.0 in mode 1 and stays -0.0 in mode 0
    y = np.array([-0.0, 0.0, 2.0], F)
    assert same_bits(Z.normalise32(y, -0.0, 2.0, 0), np.array([-0.0, 0.0, 1.0], F))
    assert same_bits(Z.normalise32(y, -0.0, 2.0, 1), np.array([0.0, 0.0, 1.0], F))
    # NaN propagates
    assert np.isnan(Z.normalise32(np.array([np.nan, 1.0], F), 0.0, 1.0, 1)[0])


def test_normalise32_is_the_oracle_resize_back_and_scaling():
    O = pytest.importorskip("oracle.fsg_oracle")
    rs = np.random.RandomState(9)
    low = (rs.rand(5, 7, 6) * 200 + 3).astype(F)  # min > 0: the scaling's subtraction and second division do something
    factors = np.array([5 / 11, 7 / 9, 6 / 13])
    tabs, new = T.zoom_tables(low.shape, 1 / factors)
    assert new == (11, 9, 13)
    y = Z.zoom32(low, tabs)
    kmin, kmax = Z.minmax32(y)
    mn, mx = Z.key2f(kmin), Z.key2f(kmax)
    assert mn == y.min() > 0 and mx == y.max()
    back = O.resize_back(torch.from_numpy(low), factors)
    assert same_bits(Z.normalise32(y, mn, mx, 0), back.numpy())
    assert same_bits(Z.normalise32(y, mn, mx, 1), O.scale01(back).numpy())


def test_order_keys_round_trip_and_order():
    den = np.array(1, dtype=np.int32).view(F)  # the smallest denormal
    v = np.array([-np.inf, -3.0e38, -1.0, -den, -0.0, 0.0, den, 1.0e-38, 1.0, 3.0e38, np.inf], F)
    k = Z.f2key(v)
    assert k.dtype == np.int32 and (np.diff(k.astype(np.int64)) > 0).all()  # strictly increasing: -0.0 < +0.0 < denormal
    assert same_bits(Z.key2f(k), v)
    rs = np.random.RandomState(3)
    r = rs.randint(-2 ** 31, 2 ** 31, 100000).astype(np.int64).astype(np.int32).view(F)
    r = r[~np.isnan(r)]
    assert same_bits(Z.key2f(Z.f2key(r)), r)
    o = np.argsort(r, kind="stable")
    assert (np.diff(Z.f2key(r)[o].astype(np.int64)) >= 0).all()
    assert Z.f2key(F(np.inf)) == Z.KEY_MIN_IDENTITY and Z.f2key(F(-np.inf)) == Z.KEY_MAX_IDENTITY
    assert Z.f2key(F(0.0)) == 0 and Z.f2key(F(-0.0)) == -1
    # minmax32: -0.0 is the minimum of {-0.0, +0.0}, +0.0 the maximum; NaN ignored; all NaN: the identities
    assert Z.minmax32(np.array([0.0, -0.0, np.nan], F)) == (-1, 0)
    assert Z.minmax32(np.array([2.0, np.nan, -1.0], F)) == (int(Z.f2key(F(-1.0))), int(Z.f2key(F(2.0))))
    assert Z.minmax32(np.full(4, np.nan, F)) == (Z.KEY_MIN_IDENTITY, Z.KEY_MAX_IDENTITY)
