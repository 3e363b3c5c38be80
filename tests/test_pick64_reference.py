"""CPU: the numpy restatement of the voxel picker's contract (tests/util_pick64.py) on cases worked out by hand.  The GPU
tests hold the kernels against this restatement bit for bit, so it is checked here first."""
import numpy as np

from tests import util_pick64 as P

ONE_M = 1.0 - 2.0 ** -53  # the largest double below 1


def test_uniform_weights_by_hand():
    pred = np.array([0, 1, 1, 0, 1, 1], np.float32)  # eligible: 1, 2, 4, 5; cdf 1, 2, 3, 4
    out = P.pick(pred, ">", 0.0, 3, [0.0, 0.30, 0.74, 0.76])
    # targets 0, 1.2, 2.96, 3.04 -> first S_e above: voxels 1, 2, 4, 5; the first three kept
    assert out.tolist() == [4, 3, 1, 2, 4]


def test_boundary_goes_to_the_next_voxel():
    pred = np.ones(4, np.float32)  # cdf 1, 2, 3, 4
    # u * total exactly on a boundary: S_e > t is strict, so t = 1 belongs to voxel 1, t = 3 to voxel 3
    assert P.candidates(pred, ">", 0.0, [0.25, 0.75, 0.5]).tolist() == [1, 3, 2]


def test_zero_negative_and_nan_weights_are_never_picked():
    pred = np.ones(6, np.float32)
    w = np.array([0.0, 2.0, -1.0, np.nan, 0.0, 2.0], np.float32)  # eligible: 1 and 5; cdf 2, 4
    u = np.linspace(0, ONE_M, 41)
    got = set(P.candidates(pred, ">", 0.0, u, w).tolist())
    assert got == {1, 5}
    out = P.pick(pred, ">", 0.0, 4, u, w)
    assert out.tolist() == [2, 2, 1, 5, -1, -1]


def test_u_zero_and_u_just_below_one():
    pred = np.array([0, 0, 1, 1, 1, 0], np.float32)
    w = np.array([9, 9, 0.5, 0.25, 0.25, 9], np.float32)
    assert P.candidates(pred, ">", 0.0, [0.0], w).tolist() == [2]      # the first eligible voxel
    assert P.candidates(pred, ">", 0.0, [ONE_M], w).tolist() == [4]    # the last one
    # a total for which u * total rounds to the total itself (3 * (1 - 2^-53) is not that case, 2^53 + 2 voxels would be):
    # the clamp to the last eligible voxel is what the contract asks for then
    idx, cdf = P.prefix(pred, ">", 0.0, w)
    assert idx.tolist() == [2, 3, 4] and cdf.tolist() == [0.5, 0.75, 1.0]
    assert np.minimum(np.searchsorted(cdf, [1.0], side="right"), 2).tolist() == [2]


def test_all_zero_total_and_empty_set():
    pred = np.ones(5, np.float32)
    assert P.pick(pred, ">", 0.0, 2, [0.1, 0.9], np.zeros(5, np.float32)).tolist() == [0, 0, -1, -1]
    assert P.pick(np.zeros(5, np.float32), ">", 0.0, 2, [0.1, 0.9]).tolist() == [0, 0, -1, -1]
    assert P.pick(np.zeros(0, np.float32), ">", 0.0, 3, [0.1, 0.9, 0.5]).tolist() == [0, 0, -1, -1, -1]


def test_repeats_keep_the_first_occurrence_and_pad():
    pred = np.array([3, 1, 3, 3, 2], np.uint8)  # == 3: voxels 0, 2, 3
    u = [0.9, 0.9, 0.1, 0.95, 0.4, 0.1]         # candidates 3, 3, 0, 3, 2, 0
    assert P.candidates(pred, "==", 3.0, u).tolist() == [3, 3, 0, 3, 2, 0]
    assert P.pick(pred, "==", 3.0, 5, u).tolist() == [3, 3, 3, 0, 2, -1, -1]
    assert P.pick(pred, "==", 3.0, 2, u).tolist() == [3, 2, 3, 0]  # k reached: the later distinct candidate is not reported
    assert P.pick(pred, "!=", 3.0, 1, [0.6]).tolist() == [2, 1, 4]


def test_weighted_by_hand():
    pred = np.array([5, 5, 0, 5], np.float32)
    w = np.array([1.0, 3.0, 100.0, 4.0], np.float32)  # eligible 0, 1, 3; cdf 1, 4, 8
    assert P.candidates(pred, "==", 5.0, [0.0, 0.124, 0.125, 0.49, 0.5, 0.99], w).tolist() == [0, 0, 1, 1, 3, 3]


def test_dyadic_sums_are_exact():
    w = P.dyadic_weights(3 * 4096 + 5, seed=1)
    _idx, cdf = P.prefix(np.ones(w.size, np.float32), ">", 0.0, w)
    assert (cdf * 1024 == np.round(cdf * 1024)).all() and cdf[-1] * 1024 == w.astype(np.float64).sum() * 1024


def test_random_case_leaves_out_no_candidate():
    """The seed of the GPU test's random-weight case: no u * total within 2^-40 total of a prefix boundary, and the 64
    candidates are distinct, so the kernels must reproduce every one of them."""
    pred, w, u = P.random_case()
    assert (P.boundary_distance(pred, ">", 0.0, u, w) > 2.0 ** -40).all()
    c = P.candidates(pred, ">", 0.0, u, w)
    assert len(set(c.tolist())) == P.RANDOM_M
