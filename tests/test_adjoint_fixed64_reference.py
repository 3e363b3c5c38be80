"""The rule of the deterministic slice-acquisition adjoint (include/fsg_hip.h, fsg_slice_acq_adjoint_det_f32), pinned on
the numpy restatement tests/util_fixed64.py by cases computed by hand.  tests/test_adjoint_det_gpu.py then holds the kernels
to that restatement bit for bit.  No GPU here."""
from fractions import Fraction

import numpy as np
import pytest

from tests import util_fixed64 as X

f32 = np.float32
Q = 2.0 ** -72  # the quantum


def q_total(c, value_scale=1.0):
    return X.total(*X.quantise(np.asarray(c, f32), value_scale))


def fin(values, value_scale=1.0):
    """finalise() of exact integers given as Python ints (split into limbs the way sums arrive: any split will do)."""
    hi = [v >> X.L for v in values]
    lo = [v - (h << X.L) for v, h in zip(values, hi)]
    return X.finalise(np.array(hi, np.int64), np.array(lo, np.int64), value_scale)


def test_constants_are_the_headers():
    from fetalsyngen_amd import _lib

    assert (_lib.SA.DET_FRAC_BITS, _lib.SA.DET_LIMB_BITS) == (X.F, X.L) == (72, 40)


def test_ties_go_to_even_and_signs_are_symmetric():
    # contributions below 2^-48 are the only ones that are rounded at all: (k + 1/2) quanta go to the even neighbour
    c = np.array([0.5 * Q, 1.5 * Q, 2.5 * Q, 3.5 * Q, -0.5 * Q, -1.5 * Q, -2.5 * Q, 0.75 * Q, 0.25 * Q], f32)
    assert q_total(c) == [0, 2, 2, 4, 0, -2, -2, 1, 0]
    # everything of 2^-48 and more enters exactly: 0.3f is 10066330 * 2^-25, so 10066330 * 2^47 quanta, and its negative
    # mirrors it; the limbs are hi = rint(0.3f * 2^32) = 10066330 * 2^7 and no remainder
    assert q_total([0.3, -0.3]) == [10066330 << 47, -(10066330 << 47)]
    hi, lo = X.quantise(np.array([0.3, 2.0 ** -33, 3 * 2.0 ** -34, -(2.0 ** -33)], f32))
    assert hi.tolist() == [10066330 << 7, 0, 1, 0]  # ties of the HIGH limb go to even too ...
    assert lo.tolist() == [0, 1 << 39, -(1 << 38), -(1 << 39)]  # ... and the low limb makes the pair exact either way
    rng = np.random.default_rng(5)
    c = (rng.standard_normal(3000) * np.exp2(rng.uniform(-80, 7, 3000))).astype(f32)
    for scale in (1.0, 2.0 ** -20, 2.0 ** 20):
        assert q_total(c, scale) == X.quantise_exact(c, scale)
    big = c[np.abs(c) >= 2.0 ** -48]
    assert len(big) > 1000 and all(Fraction(q, 1 << 72) == Fraction(float(v)) for q, v in zip(q_total(big), big))


def test_sum_wider_than_24_bits_is_rounded_once():
    one = 1 << 72
    # 1 + 2^-24 is a tie between two floats; one more quantum tips it upwards
    assert fin([one + (1 << 48)])[0] == f32(1.0)
    assert fin([one + (1 << 48) + 1])[0] == f32(1.0 + 2.0 ** -23)
    assert fin([one + (1 << 49) + (1 << 48)])[0] == f32(1.0 + 2.0 ** -22)  # a tie above an odd float: up
    # a detour through float64 would first drop the last 1 and then see a tie
    big = (1 << 100) + (1 << 76) + 1
    assert float(big) == float((1 << 100) + (1 << 76))
    assert fin([big, -big]).tolist() == [2.0 ** 28 + 2.0 ** 5, -(2.0 ** 28 + 2.0 ** 5)]
    # limb sums arrive unnormalised: a low limb beyond 2^40 in either direction, a negative high limb with a positive low
    assert X.finalise(np.array([0, 1, -1, -1]), np.array([3 << 40, -(1 << 40), 1 << 40, 1])).tolist() == \
        [3 * 2.0 ** -32, 0.0, 0.0, -(2.0 ** -32)]  # (the last: -2^40 + 1 quanta round to -2^40)
    z = X.finalise(np.array([0, 1]), np.array([0, -(1 << 40)]))
    assert z.tolist() == [0.0, 0.0] and not np.signbit(z).any()  # an untouched accumulator, and a cancelled one, are +0
    rng = np.random.default_rng(0)
    acc = rng.integers(-(1 << 62), 1 << 62, 4000) >> rng.integers(0, 62, 4000)
    acc = np.concatenate([acc, [(1 << 24) + 1, (1 << 25) + 2, (1 << 25) + 6, -((1 << 25) + 2), np.iinfo(np.int64).max]])
    assert np.array_equal(acc.astype(f32), X.int_to_f32(acc.tolist()))  # the cast the pixel weight relies on
    assert X.pixel_weight([(1 << 32) + (1 << 8) + 1])[0] == f32(1.0 + 2.0 ** -23)


def test_sums_do_not_depend_on_the_order_where_float_sums_do():
    rng = np.random.default_rng(1)
    c = (rng.standard_normal(5000) * np.exp(rng.uniform(-12, 0, 5000))).astype(f32)
    hi, lo = X.quantise(c)
    want = X.finalise([hi.sum()], [lo.sum()])[0]
    assert want == f32(sum(Fraction(float(v)) for v in c))  # every contribution is exact here: the exact sum, rounded once
    floats = set()
    for _ in range(20):
        p = rng.permutation(len(c))
        assert X.finalise([hi[p].sum()], [lo[p].sum()])[0] == want
        acc = f32(0)
        for v in c[p]:
            acc = f32(acc + v)
        floats.add(float(acc))
    assert len(floats) > 1  # the premise: fp32 sums of the same numbers in another order differ


def test_small_weights_keep_their_quotient():
    """Why one limb at 2^-32 would not do: a voxel reached only by a PSF's fringe has a weight of a few 2^-32, and
    equalisation divides by it.  At 2^-72 the quotient of such a voxel is that of the exact sums."""
    w = np.array([3.1e-10, 1.7e-10, 2.2e-12], f32)
    s = np.array([0.25, 0.75, 0.5], f32)
    v = (w * s).astype(f32)
    got = X.finalise(*[[x.sum()] for x in X.quantise(v)])[0] / X.finalise(*[[x.sum()] for x in X.quantise(w)])[0]
    exact = float(sum(Fraction(float(x)) for x in v) / sum(Fraction(float(x)) for x in w))
    assert abs(float(got) - exact) <= 2.0 ** -23 * exact
    one_limb = np.rint(v.astype(np.float64) * 2.0 ** 32).sum() / np.rint(w.astype(np.float64) * 2.0 ** 32).sum()
    assert abs(one_limb - exact) > 0.05  # (what the single 2^-32 limb would have given)


def test_value_scale_is_exact_and_checked():
    rng = np.random.default_rng(2)
    c = rng.standard_normal(1000).astype(f32)
    assert q_total(c * f32(1024), 1024.0) == q_total(c)
    hi, lo = X.quantise(c)
    assert np.array_equal(X.finalise(hi, lo, 1024.0), X.finalise(hi, lo) * f32(1024))
    for ok in (1.0, 2.0 ** -20, 2.0 ** 20, 0.5):
        X.check_value_scale(ok)
    for bad in (3.0, 2.0 ** 21, 2.0 ** -21, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            X.check_value_scale(bad)


def test_python_layer_refuses_before_it_touches_a_device():
    import torch

    from fetalsyngen_amd import kernels as K

    tr, psf, s = torch.zeros(1, 3, 4), torch.ones(2, 2, 2), torch.zeros(1, 4, 4)
    with pytest.raises(ValueError, match="CUDA semantics"):
        K.slice_acq_adjoint(tr, psf, s, None, None, (4, 4, 4), 1.0, deterministic=True, semantics="torch")
    for bad in (3.0, 2.0 ** 21, 0.0, float("nan")):
        with pytest.raises(ValueError, match="value_scale"):
            K.slice_acq_adjoint(tr, psf, s, None, None, (4, 4, 4), 1.0, deterministic=True, value_scale=bad)


def _aligned(n, t):
    tr = np.zeros((n, 3, 4), f32)
    tr[:, :, :3] = np.eye(3, dtype=f32)
    tr[:, :, 3] = np.asarray(t, f32)
    return tr


def test_restated_adjoint_by_hand_two_slices_on_one_plane():
    """PSF of eight ones, slices on the voxel grid (odd sizes, integer shifts): the taps at offsets (-1, 0) sit on voxels, the
    PSF re-interpolated there is defined only at offset 0 (position 0.5 of a two-tap axis) and is exactly 1, so every pixel
    has weight 1 and drops its own value on its own voxel.  Two slices on the same plane add up in fixed point."""
    psf = np.ones((2, 2, 2), f32)
    s = np.zeros((2, 3, 3), f32)
    s[0, 1, 1], s[1, 1, 1] = 0.3, 2.0 ** -24 * 0.3  # 0.3f (1 + 2^-24) is no float: the exact sum, rounded once (upwards)
    s[0, 0, 2], s[1, 0, 2] = 1.5 * Q, 2.5 * Q       # two ties: 2 + 2 quanta
    s[0, 2, 0], s[1, 2, 0] = -0.75, 0.5
    v, w = X.adjoint_nearest_psf(_aligned(2, (0, 0, 1)), psf, s, (5, 5, 5), 1.0)
    # pixel (iy, ix) of a 3 x 3 slice shifted by z = +1 lands on voxel (2 + 1, 1 + iy, 1 + ix)
    assert w[3, 1:4, 1:4].tolist() == [[2.0] * 3] * 3 and w.sum() == 18
    assert v[3, 2, 2] == f32(Fraction(float(f32(0.3))) * (1 + Fraction(1, 1 << 24))) == np.nextafter(f32(0.3), f32(1))
    assert v[3, 1, 3] == f32(4 * Q) and v[3, 3, 1] == f32(-0.25)
    assert np.count_nonzero(v) == 3
    # with a slice mask on the second slice's centre pixel, and a volume mask on the tie voxel
    sm = np.ones((2, 3, 3), bool)
    sm[1, 1, 1] = False
    vm = np.ones((5, 5, 5), bool)
    vm[3, 1, 3] = False
    v2, w2 = X.adjoint_nearest_psf(_aligned(2, (0, 0, 1)), psf, s, (5, 5, 5), 1.0, slices_mask=sm, vol_mask=vm)
    assert v2[3, 2, 2] == f32(0.3) and w2[3, 2, 2] == 1 and v2[3, 1, 3] == 0 and w2[3, 1, 3] == 0


def test_restated_adjoint_is_invariant_under_slice_order_and_ids():
    rng = np.random.default_rng(3)
    psf = rng.uniform(0.1, 1.0, (2, 3, 3)).astype(f32)
    n = 5
    tr = _aligned(n, np.stack([rng.integers(-2, 3, n), rng.integers(-2, 3, n), rng.integers(-3, 4, n)], 1))
    s = rng.standard_normal((n, 7, 6)).astype(f32)
    a = X.adjoint_nearest_psf(tr, psf, s, (9, 10, 11), 1.0)
    p = rng.permutation(n)
    b = X.adjoint_nearest_psf(tr[p], psf, s[p], (9, 10, 11), 1.0)
    c = X.adjoint_nearest_psf(tr[p], psf, s, (9, 10, 11), 1.0, slice_ids=p)
    assert a[1].sum() > 50
    for got in (b, c):
        assert np.array_equal(a[0], got[0]) and np.array_equal(a[1], got[1])
