"""GPU: fsg_voxel_pick_f32 / _u8 against the float64 restatement of their contract (tests/util_pick64.py), bit for bit.

Sizes: one voxel, one below / exactly / one above a bucket (4096), several buckets with a ragged tail, 40 buckets + 1, and
once 1030 buckets + 3: from 1025 buckets on a segment of the bucket scan holds more than one bucket.  Weights: none, a 2^-10 grid (every partial sum is exact in float64 whatever the order,
so equality must be exact), and the same with zero, negative and NaN entries.  One case with float32 uniform weights, whose
sums are not exact: a candidate may differ only where u * total lies within 2^-40 total of a prefix boundary of the
restatement, and the CPU test `test_random_case_leaves_out_no_candidate` shows that none of its 64 does."""
import numpy as np
import pytest
import torch

from tests import util_pick64 as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ONE_M = 1.0 - 2.0 ** -53
SIZES = [1, 4095, 4096, 4097, 3 * 4096 + 5, 40 * 4096 + 1]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (and libfsg_hip.so); there is no fallback to skip to")
    from fetalsyngen_amd import kernels

    return kernels


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(K, pred, op, value, k, u, weight=None):
    out = K.voxel_pick(dev(pred), op, value, k, torch.from_numpy(np.asarray(u, dtype=np.float64)),
                       None if weight is None else dev(weight))
    return out.cpu().numpy()


def labels(n, seed, dtype):
    """Label-like volume: values 0..3, in runs, so that buckets differ in how many voxels pass."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 4, n)
    if n > 64:
        v[: n // 3] = 0          # a long stretch (whole buckets at the larger sizes) with nothing eligible for "> 0"
        v[n // 2: n // 2 + 40] = 2
    v[-1] = 3 if n > 1 else 1    # the very last voxel counts: the ragged tail is read
    return v.astype(dtype)


def uniforms(seed, m):
    u = np.random.default_rng(seed).random(m)
    u[0], u[1] = 0.0, ONE_M
    if m > 6:
        u[5] = u[2]  # repeats
        u[6] = u[3]
    return u


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_modes_sizes_and_weights(K, n, dtype):
    pred = labels(n, n, dtype)
    w_dyadic = P.dyadic_weights(n, seed=n + 1)
    w_bad = w_dyadic.copy()
    w_bad[::3] = 0.0
    w_bad[1::7] = -1.5
    w_bad[2::11] = np.nan
    for op, value in ((">", 0.0), ("==", 2.0), ("!=", 3.0)):
        for weight in (None, w_dyadic, w_bad):
            u = uniforms(n + len(op), 24)
            want = P.pick(pred, op, value, 9, u, weight)
            got = run(K, pred, op, value, 9, u, weight)
            assert np.array_equal(got, want), (n, dtype, op, weight is not None, got, want)


@pytest.mark.parametrize("n", [4097, 3 * 4096 + 5])
def test_targets_exactly_on_prefix_boundaries(K, n):
    """Dyadic weights: the total and every prefix sum are exact, so u = S_e / total can be hit exactly when the total is a
    power of two; S_e > t is strict, so such a target belongs to the NEXT eligible voxel."""
    pred = np.ones(n, np.float32)
    w = np.full(n, 0.25, np.float32)
    w[n - 1] = 0.25 * (2 ** int(np.ceil(np.log2(n))) - (n - 1))  # total = 0.25 * 2^p
    idx, cdf = P.prefix(pred, ">", 0.0, w)
    total = cdf[-1]
    assert total == 0.25 * 2 ** int(np.ceil(np.log2(n)))
    picks = np.array(sorted({p for p in (0, 1, 255, 256, 4094, 4095, 4096, n - 3) if p < n - 1}))
    u = cdf[picks] / total
    assert (u * total == cdf[picks]).all()
    want = P.pick(pred, ">", 0.0, len(u), u, w)
    assert want[2:].tolist() == (picks + 1).tolist()
    assert np.array_equal(run(K, pred, ">", 0.0, len(u), u, w), want)


def test_empty_set_and_all_zero_total(K):
    n = 4097
    u = uniforms(3, 16)
    want = np.array([0, 0] + [-1] * 5)
    assert np.array_equal(run(K, np.zeros(n, np.float32), ">", 0.0, 5, u), want)               # predicate never holds
    assert np.array_equal(run(K, np.ones(n, np.uint8), ">", 0.0, 5, u, np.zeros(n, np.float32)), want)  # total 0
    assert np.array_equal(run(K, np.ones(n, np.float32), ">", 0.0, 5, u, np.full(n, np.nan, np.float32)), want)
    assert np.array_equal(run(K, np.zeros(0, np.float32), ">", 0.0, 5, u), want)               # n == 0


def test_single_eligible_voxel_and_found_below_k(K):
    n = 3 * 4096 + 5
    pred = np.zeros(n, np.uint8)
    pred[[7, 5000, n - 1]] = 1
    u = uniforms(9, 40)
    want = P.pick(pred, ">", 0.0, 8, u)
    assert want[0] == 3 and want[1] == 3 and (want[5:] == -1).all()  # more asked for than there are distinct candidates
    assert np.array_equal(run(K, pred, ">", 0.0, 8, u), want)
    one = np.zeros(n, np.float32)
    one[n - 1] = 5.0
    assert run(K, one, "==", 5.0, 3, u).tolist() == [1, 1, n - 1, -1, -1]


def test_repeats_keep_candidate_order(K):
    n = 40 * 4096 + 1
    pred = np.ones(n, np.float32)
    base = np.array([0.9, 0.1, 0.5, 0.3, 0.7])
    u = np.concatenate([base, base[::-1], base, [0.2]])
    want = P.pick(pred, ">", 0.0, 8, u)
    assert want[1] == 6 and want[2:8].tolist() == P.candidates(pred, ">", 0.0, np.append(base, 0.2)).tolist()
    assert np.array_equal(run(K, pred, ">", 0.0, 8, u), want)


def test_limits(K):
    n = 40 * 4096 + 1
    pred, w = labels(n, 2, np.float32), P.dyadic_weights(n, 3)
    assert np.array_equal(run(K, pred, ">", 0.0, 1, [0.37], w), P.pick(pred, ">", 0.0, 1, [0.37], w))  # k = m = 1
    u = uniforms(4, 4096)
    assert np.array_equal(run(K, pred, ">", 0.0, 1, u, w), P.pick(pred, ">", 0.0, 1, u, w))
    want = P.pick(pred, ">", 0.0, 1024, u, w)
    assert want[1] == 1024
    assert np.array_equal(run(K, pred, ">", 0.0, 1024, u, w), want)
    u_rep = np.repeat(uniforms(5, 512), 8)  # 4096 candidates, at most 512 distinct: found < k
    want = P.pick(pred, ">", 0.0, 1024, u_rep, w)
    assert want[1] <= 512 and (want[2 + want[1]:] == -1).all()
    assert np.array_equal(run(K, pred, ">", 0.0, 1024, u_rep, w), want)


def test_more_buckets_than_scan_threads(K):
    """1030 buckets: the scan's segments hold two buckets each, the last segments none."""
    n = 1030 * 4096 + 3
    pred, w = labels(n, 6, np.uint8), P.dyadic_weights(n, 7)
    u = uniforms(8, 72)
    for weight in (None, w):
        want = P.pick(pred, "!=", 1.0, 32, u, weight)
        assert want[1] == 32
        assert np.array_equal(run(K, pred, "!=", 1.0, 32, u, weight), want)


def test_bad_arguments_are_refused_with_out_untouched(K):
    from fetalsyngen_amd import _lib

    pred = dev(np.ones(5000, np.float32))
    out = torch.full((1100,), -7, dtype=torch.int64, device=DEV)
    for k, m, code in ((1025, 4096, _lib.E_TOOBIG), (5, 4097, _lib.E_TOOBIG), (9, 8, _lib.E_BADARG), (0, 8, _lib.E_BADARG)):
        with pytest.raises(_lib.FsgError) as err:
            K.voxel_pick(pred, ">", 0.0, k, torch.rand(m, dtype=torch.float64), out=out)
        assert err.value.code == code, (k, m)
    torch.cuda.synchronize()
    assert (out == -7).all()


def test_two_identical_calls_agree_and_pick_voxels_coordinates(K):
    _pred, w, u = P.random_case(3)
    p, ud = torch.ones((17, 41, 235), dtype=torch.float32, device=DEV), torch.from_numpy(u)
    wd = dev(w[: p.numel()].reshape(p.shape))
    a = K.voxel_pick(p, ">", 0.0, 32, ud, wd).cpu()
    b = K.voxel_pick(p, ">", 0.0, 32, ud, wd).cpu()
    assert torch.equal(a, b) and int(a[1]) == 32
    eligible, coords = K.pick_voxels(p, ">", 0.0, 32, ud, wd)
    assert eligible == int(a[0]) and coords.shape == (32, 3)
    assert np.array_equal(np.ravel_multi_index(tuple(coords.numpy().T), tuple(p.shape)), a[2:].numpy())


def test_random_weights_within_the_contract_tolerance(K):
    pred, w, u = P.random_case()
    want = P.candidates(pred, ">", 0.0, u, w)
    near = P.boundary_distance(pred, ">", 0.0, u, w) <= 2.0 ** -40
    got = run(K, pred, ">", 0.0, P.RANDOM_M, u, w)
    assert got[0] == int((w > 0).sum())
    # the candidates away from a boundary, in order, must be what the kernels report (they are distinct, see the CPU test)
    keep = want[~near]
    assert near.sum() <= 1 and got[1] >= len(keep)
    reported = got[2:2 + got[1]].tolist()
    assert [c for c in reported if c in set(keep.tolist())] == keep.tolist()
    assert len(reported) - len(keep) <= int(near.sum())


def test_misaligned_views_take_the_element_loads(K):
    """A view that starts 4 bytes into an allocation: no 16-byte loads, the same answer."""
    n = 3 * 4096 + 5
    pred, w = labels(n + 1, 8, np.float32), P.dyadic_weights(n + 1, 9)
    u = uniforms(10, 24)
    out = K.voxel_pick(dev(pred)[1:], ">", 0.0, 9, torch.from_numpy(u), dev(w)[1:]).cpu().numpy()
    assert np.array_equal(out, P.pick(pred[1:], ">", 0.0, 9, u, w[1:]))
    p8 = labels(n + 1, 8, np.uint8)
    out = K.voxel_pick(dev(p8)[1:], "==", 2.0, 9, torch.from_numpy(u)).cpu().numpy()
    assert np.array_equal(out, P.pick(p8[1:], "==", 2.0, 9, u))
