"""GPU: every kernel of csrc/fsg_artifacts.hip and csrc/fsg_reduce.hip, called directly, against the float64 reference
(tests/util_artifacts64.py) at the places where the kernels branch: the 4096-voxel buckets and 64-lane ballots of the voxel-set
kernels, the 16-byte alignment switch and scalar tails of min/max and the float16 cast, the grid caps (n > 2^22), the block
widths at 64 / 128 / 256 / 1024 columns, the 4-wide tail and the blob skip of the mixture of Gaussians, radii from 0 to longer
than the axis, ties of the fuzzy-boundary rounding, and every argument check of the entry points.

Exact operations are compared bit for bit.  Rounded ones must lie within the float32 rounding bound of the operation
(util_artifacts64.*_bound, validated on the CPU by tests/test_artifacts64_reference.py); no tolerance is chosen by eye, and no
measured ratio is needed: the transcendental paths (v_exp_f32, expf, sqrtf) have documented 1-ulp errors, which are part of the
bounds.  The only elements left out of a comparison are the near-ties of the random `boundary_mask` case (p n - 1 within 2^-22
of a half-integer: n_dilate = 6 keeps the float32 product below 8, where half an ulp is 2^-22), capped at 1e-4 of the voxels.
The Philox path of `slice_noise_` takes its normals from K.randn of the same (seed, stream): the kernel under test then has
to use the right counter, lanes and pairing (two normals per pixel, block e >> 1) and the Rician arithmetic within its bound.
The draw itself (Philox words, Box-Muller through v_log / v_sqrt / v_sin / v_cos) is the same fsg_randn4 device code in both, so
this comparison does not check it; tests/test_keyed_draws.py holds K.randn to the numpy restatement
oracle/fsg_keyed_draws.device_normals, which closes the chain.
Every output buffer is preceded by poison(): an element a kernel never writes is NaN (or -7), not a lucky zero.

Deviations from a plain brute force, for time: the random 2 % and the full masks on 64x65x129 and 40x300x40 and the 256^3 case
use the separable int64 form, which the CPU tests hold to the brute force on 9x7x11; masks of up to 50 voxels (one, two, and 50
random ones at r = 30 on the two large shapes) use the brute force everywhere.

kernel -> test
  mog_tables_kernel, mog_sum_kernel<true/false>  test_mog3d
  perlin_kernel                                  test_perlin_fractal
  blend_kernel                                   test_blend, test_blend_large
  slice_noise_kernel                             test_slice_noise
  slice_void_kernel                              test_slice_void
  slice_sums_kernel                              test_slice_sums
  nonzero_count_kernel, nonzero_select_kernel    test_nonzero_ranks, test_nonzero_ranks_256
  compact_kernel                                 test_nonzero_ranks (float32 volumes), test_nonzero_ranks_256
  ewise_kernel, scatter_const_kernel             test_ewise_scatter
  dist_pass_kernel                               test_distance_to_mask, test_distance_256
  boundary_mask_kernel                           test_boundary_mask_exact, test_boundary_mask_random
  bernoulli_kernel                               test_bernoulli_keep
  box sums (blur kernels with unit taps)         test_box_sum3d
  minmax_kernel                                  test_reduce_minmax
  scale_kernel                                   test_scale
  cast_f16_kernel                                test_cast_f16
  argument checks of all entry points            test_bad_arguments, test_empty_is_success, test_slice_void_refuses_duplicates
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util_artifacts64 as R
from tests.util_artifact_cases import NEAR_TIE_CAP, boundary_random_inputs, mog_cases, perlin_octaves

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
BIG_N = 2 ** 22 + 3  # beyond 16384 blocks x 256 threads: the grid-stride loops take a second trip
BUCKET = 4096


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (and libfsg_hip.so); there is no fallback to skip to")
    from fetalsyngen_amd import kernels

    return kernels


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def poison(*shapes, dtype=torch.float32):
    """Hand the next allocations of these shapes blocks full of NaN (-7 for integers): the caching allocator reuses a freed
    block of the same size, so an output a kernel never writes fails the comparison instead of passing on a stale zero."""
    for s in shapes:
        t = torch.full(s if isinstance(s, tuple) else (int(s),), float("nan") if dtype.is_floating_point else -7, dtype=dtype,
                       device=DEV)
        del t


def within(name, got, ref, bound):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, name
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.size} outputs beyond the rounding bound, first at "
                           f"{np.argwhere(bad)[0].tolist()}: got {got[bad][0]!r}, want {ref[bad][0]!r} +- {bound[bad][0]:.3g}")
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"BOUND {name:48s} max err {err.max():.3e}  {ratio:.3f} of bound")
    return ratio


# ---- voxel sets: nonzero_count / nonzero_select / compact ---------------------------------------------------------------------
def set_masks(n, rs):
    m = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "half": rs.rand(n) < 0.5}
    for i in (0, n - 1, 4095, 4096):
        if 0 <= i < n:
            m[f"one@{i}"] = np.arange(n) == i
    if n > BUCKET:
        m["every4096th"] = np.arange(n) % BUCKET == 0
    if n >= 3 * BUCKET:
        e = np.ones(n, bool)
        e[BUCKET:2 * BUCKET] = False
        m["empty-bucket"] = e
    return m


def volume_for(kind, op, sel, rs):
    """A volume of `kind` whose voxels in `sel` (and no others) satisfy `op value`; returns (volume, value)."""
    n = sel.size
    if kind == "bool":
        return sel.copy(), {">": 0.0, "==": 1.0, "!=": 0.0}[op]
    if kind == "uint8":
        if op == ">":
            return np.where(sel, rs.randint(2, 256, n), rs.randint(0, 2, n)).astype(np.uint8), 1.0
        if op == "==":
            return np.where(sel, 7, rs.choice([0, 6, 8, 255], n)).astype(np.uint8), 7.0
        return np.where(sel, rs.randint(1, 256, n), 0).astype(np.uint8), 0.0
    if op == ">":
        return np.where(sel, rs.rand(n) + 0.5, rs.choice([0.0, -1.5, 0.25], n)).astype(F), 0.25
    if op == "==":
        return np.where(sel, 2.5, rs.rand(n)).astype(F), 2.5
    v = np.where(sel, rs.rand(n) + 0.5, rs.choice([0.0, -0.0], n)).astype(F)
    if sel.any():
        v[np.flatnonzero(sel)[0]] = np.nan  # NaN != 0 is true
    if not sel.all():
        v[np.flatnonzero(~sel)[0]] = -0.0   # -0.0 != 0 is false
    return v, 0.0


def bucket_edge_ranks(pred, rs, buckets=None):
    """0, total - 1, the first and last rank of every (given) bucket, a repeated rank."""
    n = pred.size
    nb = (n + BUCKET - 1) // BUCKET
    counts = np.add.reduceat(pred.astype(np.int64), np.arange(0, n, BUCKET))
    ends = np.cumsum(counts)
    total = int(ends[-1])
    r = [0, total - 1]
    for b in (range(nb) if buckets is None else buckets):
        if counts[b]:
            r += [int(ends[b] - counts[b]), int(ends[b] - 1)]
    r.append(r[len(r) // 2])
    return np.array(r, dtype=np.int64), total


def check_ranks(K, vol_np, shape, op, value, name, ranks=None, rs=None, compact=False):
    pred = R.pred64(vol_np, op, value).reshape(-1)
    vol = dev(vol_np.reshape(shape))
    poison((pred.size + BUCKET - 1) // BUCKET, dtype=torch.int32)
    total, select = K.nonzero_ranks(vol, op, value)
    assert total == int(pred.sum()), name
    assert tuple(select([]).shape) == (0, len(shape)) and tuple(select([], flat_device=True).shape) == (0,)
    if total == 0:
        with pytest.raises(IndexError):
            select([0])
    else:
        if ranks is None:
            ranks, _t = bucket_edge_ranks(pred, rs)
        poison(len(ranks), dtype=torch.int64)
        assert np.array_equal(select(ranks).numpy(), R.rank_coords64(vol_np.reshape(shape), op, value, ranks)), name
        poison(len(ranks), dtype=torch.int64)
        assert np.array_equal(host(select(ranks, flat_device=True)), R.rank_flat64(vol_np, op, value, ranks)), name
        with pytest.raises(IndexError):
            select([total])
    if compact:
        vals = (np.arange(pred.size) % 8191 + rs.rand(pred.size)).astype(F)
        poison(max(total, 1))
        got = host(K.compact_values(dev(vals), vol.reshape(-1), op, value))
        assert got.shape == (total,) and np.array_equal(got, R.compact64(vals, vol_np, op, value)), name


@pytest.mark.parametrize("op", [">", "==", "!="], ids=["gt", "eq", "ne"])
@pytest.mark.parametrize("kind", ["float32", "uint8", "bool"])
def test_nonzero_ranks(K, kind, op):
    rs = np.random.RandomState(11)
    for n in (1, 63, 64, 65, 4095, 4096, 4097, 3 * BUCKET + 1):
        shape = (n,) if n < 4095 else ((3, 1365) if n == 4095 else ((n,) if n % 2 else (2, n // 2)))
        for mname, sel in set_masks(n, rs).items():
            v, value = volume_for(kind, op, sel, rs)
            if not (kind == "float32" and op == "!="):
                assert np.array_equal(R.pred64(v, op, value), sel)
            check_ranks(K, v, shape, op, value, f"{kind} {op} n={n} {mname}", rs=rs, compact=kind == "float32")
    # 4097 ranks in one call
    n = 3 * BUCKET + 1
    v, value = volume_for(kind, op, rs.rand(n) < 0.5, rs)
    total = int(R.pred64(v, op, value).sum())
    check_ranks(K, v, (n,), op, value, f"{kind} {op} 4097 ranks", ranks=np.resize(rs.permutation(total), 4097), rs=rs)


def test_nonzero_ranks_256(K):
    """256^3 once: 4096 buckets, first and last rank of 64 random buckets; compaction of the same volume."""
    rs = np.random.RandomState(12)
    n = 256 ** 3
    v = np.where(rs.rand(n) < 0.5, rs.rand(n) + 0.5, 0.0).astype(F)
    v[-1], v[0] = 3.0, 2.0
    ranks, _total = bucket_edge_ranks(v > 0, rs, buckets=rs.choice(n // BUCKET, 64, replace=False))
    check_ranks(K, v, (256, 256, 256), ">", 0.0, "256^3", ranks=ranks, rs=rs, compact=True)


# ---- box sums and distances ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("shape", [(5, 4, 3), (64, 65, 129), (33, 72, 130)], ids=str)
def test_box_sum3d(K, shape, k):
    rs = np.random.RandomState(k)
    m = (rs.rand(*shape) < 0.4).astype(F)
    m[0, 0, 0] = m[-1, -1, -1] = 1
    m[shape[0] // 2:, :, : max(shape[2] // 3, 1)] = 1  # a solid block, so that k^3 occurs where the shape allows it
    poison(shape, shape, shape)
    got = K.box_sum3d(dev(m), k)
    ref = R.box_sum64(m, k)
    assert np.array_equal(host(got), ref.astype(F))
    # the three thresholdings of the boundary stage
    for fn, want in ((lambda: K.threshold(got, 0.0), ref > 0), (lambda: K.threshold(got, float(k * k)), ref > k * k),
                     (lambda: K.equals(got, float(k ** 3)), ref == k ** 3)):
        poison(shape)
        assert np.array_equal(host(fn()), want.astype(F))


DIST_SHAPES = [(1, 1, 1), (7, 5, 1), (9, 7, 11), (64, 65, 129), (40, 300, 40)]


def dist_masks(shape, r, rs):
    z = np.zeros(shape, F)
    out = {"empty": z, "full": np.ones(shape, F)}
    c = z.copy()
    c[-1, 0, -1] = 1
    out["corner"] = c
    c = z.copy()
    c[tuple(s // 2 for s in shape)] = 1
    out["centre"] = c
    for gap in (r, r + 1):  # two voxels r and r + 1 apart along the longest axis
        a = int(np.argmax(shape))
        if shape[a] > gap:
            c = z.copy()
            i = [s // 3 for s in shape]
            i[a] = 0
            c[tuple(i)] = 1
            i[a] = gap
            c[tuple(i)] = 1
            out[f"pair{gap}"] = c
    out["random2%"] = (rs.rand(*shape) < 0.02).astype(F)
    if r == 30 and z.size > 10 ** 5:  # 50 random voxels: few enough for the brute force, at the radius longer than two axes
        c = z.copy()
        c.reshape(-1)[rs.choice(z.size, 50, replace=False)] = 1
        out["sparse50"] = c
    return out


def check_distance(K, m, r, metric, name):
    cap = r * r if metric == "euclid2" else r
    poison(m.shape, m.shape, m.shape)
    d = K.distance_to_mask(dev(m), r, metric)
    got = host(d)
    few = int(m.sum()) <= 50 or m.size <= 1000
    ref = R.distance_brute64(m, r, metric) if few else R.distance_separable64(m, r, metric)
    inside = ref <= cap
    assert np.array_equal(got[inside], ref[inside].astype(F)), name
    assert (got[~inside] > cap).all(), name
    poison(m.shape)
    assert np.array_equal(host(K.less_equal(d, float(cap))), inside.astype(F)), name
    return inside


@pytest.mark.parametrize("metric", ["euclid2", "l1"])
@pytest.mark.parametrize("r", [0, 1, 2, 5, 30])
def test_distance_to_mask(K, r, metric):
    rs = np.random.RandomState(r)
    for shape in DIST_SHAPES:
        for mname, m in dist_masks(shape, r, rs).items():
            inside = check_distance(K, m, r, metric, f"{metric} r={r} {shape} {mname}")
            if shape == (9, 7, 11) and r <= 5:  # the dilation the stage means
                want = R.ball_dilate64(m, r) if metric == "euclid2" else R.cross_dilate64(m, r)
                assert np.array_equal(inside, want)


def test_distance_256(K):
    rs = np.random.RandomState(3)
    check_distance(K, (rs.rand(256, 256, 256) < 1e-4).astype(F), 30, "l1", "256^3 r=30 l1")


# ---- element-wise helpers, scatter, scale ---------------------------------------------------------------------------------------
FLAT_N = (1, 255, 256, 257, BIG_N)


@pytest.mark.parametrize("n", FLAT_N)
def test_ewise_scatter(K, n):
    rs = np.random.RandomState(n % 1000)
    a, b = (rs.randn(n) * 3).astype(F), (rs.randn(n) * 3).astype(F)
    a[rs.randint(0, n, n // 7 + 1)] = 0.5
    b[rs.randint(0, n, n // 7 + 1)] = 0.5
    a[-1], b[0] = -0.75, 0.5
    da, db = dev(a), dev(b)
    for op, fn in (("add", lambda: K.axpy(da, db)), ("gt", lambda: K.threshold(da, 0.5)), ("eq", lambda: K.equals(da, 0.5)),
                   ("mul", lambda: K.mul(da, db)), ("mul_gt", lambda: K.mask_mul(da, db, 0.5)),
                   ("max", lambda: K.maximum(da, db)), ("sub_gt", lambda: K.sub_gt(da, db, 0.5)),
                   ("le", lambda: K.less_equal(da, 0.5))):
        poison(n)
        assert np.array_equal(host(fn()), R.ewise64(op, a, b, 0.5)), (op, n)
    idx = np.concatenate([[0, n - 1, n - 1, 0, -1, n], rs.randint(0, n, min(n, 5000))]).astype(np.int64)
    assert np.array_equal(host(K.scatter_ones((n,), dev(idx), DEV)), R.scatter64((n,), idx))
    assert not host(K.scatter_ones((n,), dev(np.array([-1, n], np.int64)), DEV)).any()
    # scale mode 1 on a flat input: all zeros
    flat = np.full(n, 3.25, F)
    poison(n)
    assert np.array_equal(host(K.scale(dev(flat), K.reduce_minmax(dev(flat)), 1)), np.zeros(n, F))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_scale(K, mode):
    for n in FLAT_N:
        rs = np.random.RandomState(n % 1000 + mode)
        x = (rs.randn(n) * 300 + 20).astype(F)
        x[0] = 777.0  # the maximum is positive (mode 0 divides by it)
        mm = K.reduce_minmax(dev(x))
        mn, mx = K.key_to_float(int(host(mm)[0])), K.key_to_float(int(host(mm)[1]))
        assert (mn, mx) == (float(x.min()), float(x.max()))
        poison(n)
        got = host(K.scale(dev(x), mm, mode))
        if n == 1 and mode == 2:  # flat input: 0 / 0, NaN in the reference's formula as well (only mode 1 has the flat rule)
            assert np.isnan(got).all() and np.isnan(R.scale64(x, mn, mx, mode)).all()
            continue
        within(f"scale mode {mode} n={n}", got, R.scale64(x, mn, mx, mode), R.scale_bound(x, mn, mx, mode))


# ---- min / max and the float16 cast: alignment switch, vector body, scalar tail ------------------------------------------------------
MM_N = (1, 2, 3, 4, 5, 7, 8, 1023, 2 ** 22 + 5)


def bits(x):
    return np.asarray(x, F).view(np.uint32)


@pytest.mark.parametrize("off", [0, 1, 2, 3], ids=lambda o: f"{4 * o}B")
def test_reduce_minmax(K, off):
    rs = np.random.RandomState(off)
    for n in MM_N:
        places = sorted({0, n - 1, max(n - 1 - (n % 4) // 2, 0), max((n // 4) * 4 - 1, 0), n // 2})
        for lo_at in places:
            hi_at = places[(places.index(lo_at) + 1) % len(places)]
            x = (rs.rand(n) * 2 - 1).astype(F)
            x[hi_at] = 5.5
            x[lo_at] = -7.25 if lo_at != hi_at or n == 1 else x[lo_at]
            buf = dev(np.concatenate([np.full(off, -1e30, F), x, np.full(4, 1e30, F)]))  # the neighbours would win
            view = buf[off:off + n]
            assert view.data_ptr() % 16 == 4 * off
            mm = host(K.reduce_minmax(view))
            got = (K.key_to_float(int(mm[0])), K.key_to_float(int(mm[1])))
            assert got == (float(x.min()), float(x.max())), (n, off, lo_at, hi_at)
    for vals in ([0.0, -0.0, 0.0, 0.0, 0.0], [-0.0, 0.0], [np.inf, -np.inf, 1.0, 2.0, 3.0, 4.0, 5.0],
                 [1e-45, 2e-45, 1.0, 3e-45, 2.0], [-1e-45, 0.0, -0.0]):
        x = np.array(vals, F)
        buf = dev(np.concatenate([np.zeros(off, F), x]))
        mm = host(K.reduce_minmax(buf[off:]))
        got = np.array([K.key_to_float(int(mm[0])), K.key_to_float(int(mm[1]))], F)
        # the keys order -0 below +0; numpy's min / max do not distinguish them, so compare the bits with that order
        order = np.lexsort((np.signbit(x) == 0, x))
        assert bits(got).tolist() == bits([x[order[0]], x[order[-1]]]).tolist(), vals
    # NaN is ignored (fminf / fmaxf); an all-NaN input leaves the identities: documented in fsg_hip.h and DESIGN.md
    x = np.array([np.nan, 3.0, -2.0, np.nan, 1.0, np.nan, 0.5, 0.25, np.nan], F)
    buf = dev(np.concatenate([np.zeros(off, F), x]))
    mm = host(K.reduce_minmax(buf[off:]))
    assert (K.key_to_float(int(mm[0])), K.key_to_float(int(mm[1]))) == R.minmax64(x) == (-2.0, 3.0)
    mm = host(K.reduce_minmax(dev(np.full(9 + off, np.nan, F))[off:]))
    assert (K.key_to_float(int(mm[0])), K.key_to_float(int(mm[1]))) == (np.inf, -np.inf)


@pytest.mark.parametrize("ooff", [0, 1, 2, 4], ids=lambda o: f"out+{2 * o}B")
@pytest.mark.parametrize("ioff", [0, 1, 2, 3], ids=lambda o: f"in+{4 * o}B")
def test_cast_f16(K, ioff, ooff):
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    rs = np.random.RandomState(ioff * 4 + ooff)
    special = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 65504.0, 65519.9, 65520.0, 1e6,
                        -1e6, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 3 * 2.0 ** -25, 6e-8, -0.0, 0.0, 2.0 ** -14, -2.0 ** -15,
                        np.inf, -np.inf], F)
    # 2^23 + 6149: more than 4096 blocks x 256 threads of 8-wide vectors, so the vector body takes a second trip too
    for n in MM_N + ((2 ** 23 + 6149,) if (ioff, ooff) == (0, 0) else ()):
        if n > 2 ** 20 and (ioff, ooff) not in ((0, 0), (1, 0), (0, 1)):
            continue  # the large sizes once per body: vector, unaligned input, unaligned output
        x = (rs.randn(n) * np.exp(rs.randn(n) * 4)).astype(F)
        k = min(n, special.size)
        x[n - k:] = special[:k]       # the specials sit in the scalar tail ...
        x[:k] = special[:k][::-1]     # ... and in the first vector
        xb = dev(np.concatenate([np.zeros(ioff, F), x]))
        ob = torch.full((ooff + n + 8,), float("nan"), dtype=torch.float16, device=DEV)
        xin, out = xb[ioff:], ob[ooff:ooff + n]
        assert xin.data_ptr() % 16 == 4 * ioff and out.data_ptr() % 16 == 2 * ooff
        _lib.check(lib.fsg_cast_f32_to_f16(C.c_void_p(xin.data_ptr()), n, C.c_void_p(out.data_ptr()), K._stream(xin)), "cast")
        got = host(ob)
        assert np.array_equal(got[ooff:ooff + n].view(np.uint16), R.cast_f16_64(x).view(np.uint16)), (n, ioff, ooff)
        assert np.isnan(got[:ooff]).all() and np.isnan(got[ooff + n:]).all()  # nothing outside the output
    x = dev((rs.randn(1023) * 100).astype(F))
    poison((1023,), dtype=torch.float16)
    assert np.array_equal(host(K.cast_f16(x)).view(np.uint16), R.cast_f16_64(host(x)).view(np.uint16))


# ---- Bernoulli thinning, fuzzy boundary -------------------------------------------------------------------------------------------
def test_bernoulli_keep(K):
    rs = np.random.RandomState(5)
    a = np.where(rs.rand(BIG_N) < 0.8, rs.rand(BIG_N) + 0.5, 0.0).astype(F)
    a[-1], a[0] = 2.0, -3.0
    da = dev(a)
    seed, stream = 0x1234_5678_9ABC_DEF1, 0x2_0000_0007  # both words of the key and of the stream in use
    for p in (0.0, 0.1, 0.5, 1.0):
        poison(BIG_N)
        got = host(K.bernoulli_keep(da, p, seed, stream))
        assert np.array_equal(got, R.bernoulli64(a, p, seed, stream)), p
        assert (got[a == 0] == 0).all()
        nz = int((a != 0).sum())
        kept = int((got != 0).sum())
        print(f"bernoulli p={p}: kept {kept / nz:.5f} of {nz}")
        assert abs(kept - p * nz) <= 5 * np.sqrt(max(p * (1 - p), 0) * nz)  # sanity line, not the test


def run_boundary(K, kw, with_image=True):
    n = kw["mask"].size
    d = {k: dev(v) for k, v in kw.items() if k != "n_dilate" and v is not None}
    poison(n, n)
    out, mo = K.boundary_mask(d["image"] if with_image else None, d["mask"], d["mask_modif"], d["mog"], d["dist"],
                              kw["n_dilate"], want_mask=True)
    return (host(out) if with_image else out), host(mo)


@pytest.mark.parametrize("n_dilate", [6, 12, 30])
def test_boundary_mask_exact(K, n_dilate):
    """p on the 2^-10 grid: p n_dilate is exact in float32, every k from 0 to n_dilate - 1 and every half-way p of the grid
    occurs (ties to even), against every distance 0..n_dilate: bit for bit."""
    p, dist = np.meshgrid(np.arange(1025, dtype=np.float64) / 1024, np.arange(n_dilate + 1, dtype=np.float64), indexing="ij")
    x = p * n_dilate - 1
    assert set(np.maximum(np.rint(x), 0).reshape(-1).astype(int)) >= set(range(n_dilate)) and (x % 1 == 0.5).any()
    n = p.size
    rs = np.random.RandomState(n_dilate)
    mask = (rs.rand(n) < 0.25).astype(F)                      # on mask voxels p counts as 0
    kw = dict(image=(rs.rand(n) * 100 + 1).astype(F), mask=mask, mask_modif=np.maximum(mask, (rs.rand(n) < 0.9).astype(F)),
              mog=p.reshape(-1).astype(F), dist=dist.reshape(-1).astype(F), n_dilate=n_dilate)
    ro, rm, _near = R.boundary64(**kw)
    out, mo = run_boundary(K, kw)
    assert np.array_equal(mo, rm.astype(F)) and np.array_equal(out, ro.astype(F))
    none, mo2 = run_boundary(K, kw, with_image=False)       # image=None form
    assert none is None and np.array_equal(mo2, mo)
    d = {k: dev(v) for k, v in kw.items() if k != "n_dilate"}
    poison(n)
    only = K.boundary_mask(d["image"], d["mask"], d["mask_modif"], d["mog"], d["dist"], n_dilate)  # want_mask=False form
    assert np.array_equal(host(only), out)


def test_boundary_mask_random(K):
    kw = boundary_random_inputs()
    ro, rm, near = R.boundary64(**kw)
    assert near.mean() < NEAR_TIE_CAP
    out, mo = run_boundary(K, kw)
    assert np.array_equal(mo[~near], rm[~near].astype(F)) and np.array_equal(out[~near], ro[~near].astype(F))
    m01 = np.isin(mo[near], (0.0, 1.0)).all()  # a near-tie still yields one of the two candidates, not garbage
    assert m01 and not np.isnan(out).any()


# ---- weight fields ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precise", [False, True], ids=["v_exp", "expf"])
def test_mog3d(K, precise):
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    prev = lib.fsg_set_tuning(int(_lib.TUNE.PRECISE_MATH) if precise else 0)
    try:
        for name, (shape, c, s) in mog_cases().items():
            poison(shape)
            got = host(K.mog3d(shape, c, s, DEV))
            within(f"mog3d {name} {'expf' if precise else 'v_exp'}", got, R.mog64(shape, c, s), R.mog_bound(shape, c, s))
            assert got.max() <= 1.0 and got.min() >= 0.0
        shape, c, s = mog_cases()["clamp"]
        assert host(K.mog3d(shape, c, s, DEV))[1, 2, 3] == 1.0
    finally:
        lib.fsg_set_tuning(prev)


@pytest.mark.parametrize("noct", [1, 8])
@pytest.mark.parametrize("n2", [1, 63, 64, 65, 128, 129, 255, 256, 257])
def test_perlin_fractal(K, n2, noct):
    shape = (3, 5, n2)
    octs = perlin_octaves(shape, noct, n2)
    plan = K.PerlinPlan(shape, octs, DEV)
    poison(shape)
    out, mm = K.perlin_fractal(plan)
    got, mm = host(out), host(mm)
    ref_in = [(g.numpy(), [v.numpy() for v in lins], r, a) for g, lins, r, a in octs]
    ref, _mn, _mx = R.perlin_fractal64(shape, ref_in)
    within(f"perlin n2={n2} octaves={noct}", got, ref, R.perlin_fractal_bound(shape, ref_in))
    # the keys are the min / max of the kernel's own output, bit for bit
    assert bits(K.key_to_float(int(mm[0]))) == bits(got.min()) and bits(K.key_to_float(int(mm[1]))) == bits(got.max())


def blend_inputs(n, seed):
    rs = np.random.RandomState(seed)
    a, b = (rs.rand(n) * 200).astype(F), (rs.randn(n) * 50).astype(F)
    return a, b, (rs.rand(n) > 0.2).astype(F), rs


def run_blend(K, n, wm, bm, use_seg, name):
    a, b, seg, rs = blend_inputs(n, n % 1000 + 2 * wm + bm)
    w = ((rs.rand(n) * 1.6 - 0.3) if wm else rs.rand(n)).astype(F)  # mode 1: below 0 and above 1 before the clamp
    kw, gk = dict(seg=seg if use_seg else None), dict(seg=dev(seg) if use_seg else None)
    if wm:
        kw.update(w_mm=R.minmax64(w), increase=0.15)
        gk.update(w_mm=K.reduce_minmax(dev(w)), increase=0.15)
    if bm:
        kw.update(noise_std=7.5, b_mm=R.minmax64(b), a_mm=R.minmax64(a))
        gk.update(noise_std=7.5, b_mm=K.reduce_minmax(dev(b)), a_mm=K.reduce_minmax(dev(a)))
    (ro, rw), (bo, bw) = R.blend64(a, b, w, **kw), R.blend_bound(a, b, w, **kw)
    da, db, dw = dev(a), dev(b), dev(w)
    poison(n, n)
    out, wo = K.blend(da, db, dw, want_weight=True, **gk)
    within(f"blend {name} out", host(out), ro, bo)
    within(f"blend {name} weight", host(wo), rw, bw)
    assert host(wo).min() >= 0.0 and host(wo).max() <= (1.0 if wm else float(w.max()))
    poison(n)
    assert np.array_equal(host(K.blend(da, db, dw, **gk)), host(out))                       # want_out only
    poison(n)
    only_w = K.blend(None, None, dw, want_weight=True, want_out=False, **{k: v for k, v in gk.items() if k in ("seg", "w_mm", "increase")})
    assert only_w[0] is None and np.array_equal(host(only_w[1]), host(wo))                  # weight only


@pytest.mark.parametrize("use_seg", [False, True], ids=["noseg", "seg"])
@pytest.mark.parametrize("bm", [0, 1], ids=["b-plain", "b-struct"])
@pytest.mark.parametrize("wm", [0, 1], ids=["w-plain", "w-perlin"])
def test_blend(K, wm, bm, use_seg):
    for n in (1, 257):
        if n == 1 and (wm or bm):
            continue  # a single element has max == min: the normalisations divide by zero, in the reference too
        run_blend(K, n, wm, bm, use_seg, f"n={n} w{wm} b{bm} seg{int(use_seg)}")


def test_blend_large(K):
    run_blend(K, BIG_N, 1, 1, True, f"n={BIG_N} w1 b1 seg1")


# ---- scanner corruptions ------------------------------------------------------------------------------------------------------------
def test_slice_noise(K):
    rs = np.random.RandomState(13)
    for n in (1, 257, BIG_N):
        s = (rs.rand(n) * (rs.rand(n) > 0.3)).astype(F)
        thr = F(0.25)
        s[rs.randint(0, n, n // 9 + 1)] = thr  # exactly the threshold: strict >, left alone
        z1, z2 = rs.randn(n).astype(F), rs.randn(n).astype(F)
        got = host(K.slice_noise_(dev(s), thr, 0.07, dev(z1), dev(z2)))
        within(f"slice_noise given normals n={n}", got, R.rician64(s, thr, 0.07, z1, z2), R.rician_bound(s, thr, 0.07, z1, z2))
        assert np.array_equal(got[s <= thr], s[s <= thr])
    for n in (1, 255, 2 ** 20 + 1):  # odd: the last Philox block is half used
        s = (rs.rand(n) * (rs.rand(n) > 0.3)).astype(F)
        seed, stream = 0x0BAD_5EED_1234_5678, 0x1_0000_0003
        z = host(K.randn((2 * n,), seed, stream, DEV))  # pixel e takes normals 2e, 2e + 1 (block e >> 1)
        got = host(K.slice_noise_(dev(s), 0.1, 0.05, seed=seed, stream_id=stream))
        within(f"slice_noise Philox n={n}", got, R.rician64(s, 0.1, 0.05, z[0::2], z[1::2]), R.rician_bound(s, 0.1, 0.05, z[0::2], z[1::2]))
        assert np.array_equal(got[s <= F(0.1)], s[s <= F(0.1)]) and (got != s)[s > F(0.1)].mean() > 0.99


def void_params(rs, nv, h, w):
    th = rs.rand(nv) * 2 * np.pi
    a, sx = 30 + rs.rand(nv) * 90, rs.rand(nv) * 30 + 39
    sy = a ** 2 / sx
    return np.stack([(rs.rand(nv) - 0.5) * (h - 1), (rs.rand(nv) - 0.5) * (w - 1), np.cos(th), np.sin(th), rs.rand(nv) * 0.5 + 0.5,
                     -0.5 / sx ** 2, -0.5 / sy ** 2], 1).astype(F)


@pytest.mark.parametrize("case", [(1, 1, 1, 1), (300, 7, 300, 300), (5, 320, 320, 1), (5, 320, 320, 3)], ids=str)
def test_slice_void(K, case):
    ns, h, w, nv = case
    rs = np.random.RandomState(ns + nv)
    s = (rs.rand(ns, h, w) * 100 + 1).astype(F)
    ids = rs.permutation(ns)[:nv].astype(np.int32)
    par = void_params(rs, nv, h, w)
    par[0, :2] = [-(h + 40.0), w + 25.0]  # a void centred outside the slice
    if h > 1:
        par[-1, 5:] = [-0.5 / 4.0 ** 2, -0.5 / 6.0 ** 2]  # a narrow one: the exponent runs down to underflow
        par[-1, :2] = [0.25, -0.5]
    yl, xl = torch.linspace(-(h - 1) / 2, (h - 1) / 2, h).numpy(), torch.linspace(-(w - 1) / 2, (w - 1) / 2, w).numpy()
    got = host(K.slice_void_(dev(s), torch.from_numpy(ids), dev(par), dev(yl), dev(xl)))
    within(f"slice_void {case}", got, R.void64(s, ids.tolist(), par, yl, xl), R.void_bound(s, ids.tolist(), par, yl, xl))
    rest = np.setdiff1d(np.arange(ns), ids)
    assert np.array_equal(got[rest], s[rest])


def test_slice_void_refuses_duplicates(K):
    """Two voids on one slice would race inside fsg_slice_void_f32: refused on the host, nothing is launched."""
    s = dev(np.ones((4, 3, 5), F))
    par, yl, xl = dev(void_params(np.random.RandomState(0), 2, 3, 5)), dev(np.zeros(3, F)), dev(np.zeros(5, F))
    for ids in ([1, 1], [0, 4], [-1, 2]):
        with pytest.raises(ValueError):
            K.slice_void_(s, torch.tensor(ids, dtype=torch.int32), par, yl, xl)
    with pytest.raises(TypeError):
        K.slice_void_(s, torch.tensor([0, 1], dtype=torch.int32, device=DEV), par, yl, xl)
    assert (host(s) == 1).all()


@pytest.mark.parametrize("hw", [1, 1023, 1024, 1025, 320 * 320])
def test_slice_sums(K, hw):
    rs = np.random.RandomState(hw % 1000)
    s = (rs.randn(3, hw) * 1000 + 10).astype(F)
    s[1] = np.abs(s[1])
    poison(3)
    within(f"slice_sums hw={hw}", host(K.slice_sums(dev(s))), R.slice_sums64(s), R.slice_sums_bound(s))


# ---- arguments ----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(K):
    """Every FSG_E_BADARG / FSG_E_TOOBIG branch of the entry points of the two files, once; these return before any launch, and
    the poisoned outputs stay untouched."""
    from fetalsyngen_amd import _lib

    lib, st = _lib.load(), K._stream(None)
    BAD, BIG = -1, -2  # FSG_E_BADARG, FSG_E_TOOBIG
    f = torch.full((64,), 5.0, device=DEV)            # inputs
    o = torch.full((64,), -9.0, device=DEV)           # outputs: must stay -9
    o2 = torch.full((64,), -9.0, device=DEV)
    i32 = torch.zeros(64, dtype=torch.int32, device=DEV)
    i64 = torch.zeros(64, dtype=torch.int64, device=DEV)
    u8 = torch.zeros(64, dtype=torch.uint8, device=DEV)
    mm = K.new_minmax(DEV)
    P = lambda t: C.c_void_p(t.data_ptr())            # noqa: E731
    N = C.c_void_p(0)
    calls = []

    def bad(code, fn, *args):
        calls.append(fn)
        assert getattr(lib, fn)(*args) == code, (fn, len(calls))

    # fsg_mog3d_f32(centers, sigmas, k, D, H, W, tables, out, stream)
    for a in ((N, P(f), 1, 2, 2, 2, P(f), P(o)), (P(f), N, 1, 2, 2, 2, P(f), P(o)), (P(f), P(f), 1, 2, 2, 2, N, P(o)),
              (P(f), P(f), 1, 2, 2, 2, P(f), N), (P(f), P(f), 0, 2, 2, 2, P(f), P(o)), (P(f), P(f), -1, 2, 2, 2, P(f), P(o)),
              (P(f), P(f), 1, 0, 2, 2, P(f), P(o)), (P(f), P(f), 1, 2, -2, 2, P(f), P(o)), (P(f), P(f), 1, 2, 2, 0, P(f), P(o))):
        bad(BAD, "fsg_mog3d_f32", *a, st)
    bad(BIG, "fsg_mog3d_f32", P(f), P(f), 1, 2048, 2048, 2048, P(f), P(o), st)
    bad(BIG, "fsg_mog3d_f32", P(f), P(f), 1, 2, 65536, 2, P(f), P(o), st)
    bad(BIG, "fsg_mog3d_f32", P(f), P(f), 1, 65536, 2, 2, P(f), P(o), st)
    # fsg_perlin_fractal_f32(grads, lins, res, amps, noct, n0, n1, n2, out, mm, stream)
    ptrs, nul = (C.c_void_p * 8)(*[f.data_ptr()] * 8), (C.c_void_p * 8)(*[0] * 8)
    res, res0, amps = (C.c_int32 * 24)(*[1] * 24), (C.c_int32 * 24)(*[0] * 24), (C.c_float * 8)(*[1.0] * 8)
    good = [ptrs, ptrs, res, amps, 1, 2, 2, 2, P(o), P(mm)]
    for i, v in ((0, None), (1, None), (2, None), (3, None), (8, N), (9, N), (4, 0), (4, 9), (4, -1), (5, 0), (6, -1), (7, 0),
                 (0, nul), (1, nul), (2, res0)):
        a = list(good)
        a[i] = v
        bad(BAD, "fsg_perlin_fractal_f32", *a, st)
    for dims in ((2048, 2048, 2048), (65536, 2, 2), (2, 65536, 2)):
        bad(BIG, "fsg_perlin_fractal_f32", ptrs, ptrs, res, amps, 1, *dims, P(o), P(mm), st)
    # fsg_blend_f32(a, b, w, n, w_mode, w_mm, increase, seg, b_mode, b_mm, a_mm, std, out, w_out, stream)
    good = [P(f), P(f), P(f), 64, 0, N, 0.0, N, 0, N, N, 0.0, P(o), P(o2)]
    for i, v in ((2, N), (4, -1), (4, 2), (8, -1), (8, 2), (0, N), (1, N), (4, 1), (8, 1)):
        a = list(good)
        a[i] = v
        bad(BAD, "fsg_blend_f32", *a, st)
    a = list(good)
    a[12] = a[13] = N                                                         # neither output
    bad(BAD, "fsg_blend_f32", *a, st)
    a = list(good)
    a[8], a[9] = 1, P(mm)                                                     # b_mm without a_mm
    bad(BAD, "fsg_blend_f32", *a, st)
    # fsg_slice_noise_f32(slices, n, threshold, sigma, noise1, noise2, seed, stream_id, stream)
    bad(BAD, "fsg_slice_noise_f32", N, 64, 0.0, 1.0, N, N, 1, 1, st)
    bad(BAD, "fsg_slice_noise_f32", P(o), 64, 0.0, 1.0, P(f), N, 1, 1, st)    # noise1 without noise2
    bad(BAD, "fsg_slice_noise_f32", P(o), 64, 0.0, 1.0, N, P(f), 1, 1, st)
    # fsg_slice_void_f32(slices, h, w, slice_ids, params, nvoid, ylin, xlin, stream)
    good = [P(o), 2, 2, P(i32), P(f), 1, P(f), P(f)]
    for i, v in ((0, N), (3, N), (4, N), (6, N), (7, N), (1, 0), (1, -1), (2, 0), (5, 0), (5, -1), (5, 65536)):
        a = list(good)
        a[i] = v
        bad(BAD, "fsg_slice_void_f32", *a, st)
    # fsg_slice_sums_f32(slices, n, hw, sums, stream)
    for a in ((N, 1, 8, P(o)), (P(f), 1, 8, N), (P(f), 0, 8, P(o)), (P(f), -1, 8, P(o)), (P(f), 1, 0, P(o))):
        bad(BAD, "fsg_slice_sums_f32", *a, st)
    # fsg_nonzero_count_{f32,u8}(v, n, mode, value, counts, stream); _select(v, n, mode, value, bucket, rank, nreq, out, stream)
    for fn, v in (("f32", f), ("u8", u8)):
        for a in ((N, 64, 0, 0.0, P(i32)), (P(v), 64, 0, 0.0, N), (P(v), 64, -1, 0.0, P(i32)), (P(v), 64, 3, 0.0, P(i32))):
            bad(BAD, f"fsg_nonzero_count_{fn}", *a, st)
        good = [P(v), 64, 0, 0.0, P(i32), P(i32), 1, P(i64)]
        for i, val in ((0, N), (4, N), (5, N), (7, N), (6, 0), (6, -1), (2, -1), (2, 3)):
            a = list(good)
            a[i] = val
            bad(BAD, f"fsg_nonzero_select_{fn}", *a, st)
    # fsg_compact_f32(values, pred, n, mode, value, offsets, out, stream)
    good = [P(f), P(f), 64, 0, 0.0, P(i64), P(o)]
    for i, v in ((0, N), (1, N), (5, N), (6, N), (3, -1), (3, 3)):
        a = list(good)
        a[i] = v
        bad(BAD, "fsg_compact_f32", *a, st)
    # fsg_ewise_f32(a, b, n, op, value, out, stream)
    for a in ((N, P(f), 64, 0, 0.0, P(o)), (P(f), P(f), 64, 0, 0.0, N), (P(f), P(f), 64, -1, 0.0, P(o)), (P(f), P(f), 64, 8, 0.0, P(o)),
              *[(P(f), N, 64, op, 0.0, P(o)) for op in (0, 3, 4, 5, 6)]):
        bad(BAD, "fsg_ewise_f32", *a, st)
    # fsg_dist_pass_f32(src, dst, n0, n1, n2, axis, radius, metric, first, stream)
    good = [P(f), P(o), 2, 2, 2, 0, 1, 0, 1]
    for i, v in ((0, N), (1, N), (1, P(f)), (2, 0), (3, -1), (4, 0), (5, -1), (5, 3), (6, -1), (6, 1025), (7, -1), (7, 2)):
        a = list(good)
        a[i] = v
        bad(BAD, "fsg_dist_pass_f32", *a, st)
    for dims in ((2048, 2048, 2048), (65536, 2, 2), (2, 65536, 2)):
        bad(BIG, "fsg_dist_pass_f32", P(f), P(o), *dims, 0, 1, 0, 1, st)
    # fsg_boundary_mask_f32(image, mask, mask_modif, mog, dist, n_dilate, n, out, mask_out, stream)
    good = [P(f), P(f), P(f), P(f), P(f), 6, 64, P(o), P(o2)]
    for i, v in ((1, N), (2, N), (3, N), (4, N), (5, 0), (5, -1), (0, N)):
        a = list(good)
        a[i] = v
        bad(BAD, "fsg_boundary_mask_f32", *a, st)
    bad(BAD, "fsg_boundary_mask_f32", P(f), P(f), P(f), P(f), P(f), 6, 64, N, N, st)
    # fsg_bernoulli_keep_f32(a, n, p, seed, stream_id, out, stream); fsg_scatter_const_f32(out, n, idx, k, value, stream)
    bad(BAD, "fsg_bernoulli_keep_f32", N, 64, 0.5, 1, 1, P(o), st)
    bad(BAD, "fsg_bernoulli_keep_f32", P(f), 64, 0.5, 1, 1, N, st)
    for a in ((N, 64, P(i64), 1, 1.0), (P(o), 64, N, 1, 1.0), (P(o), 64, P(i64), 0, 1.0), (P(o), 64, P(i64), -1, 1.0)):
        bad(BAD, "fsg_scatter_const_f32", *a, st)
    # fsg_reduce.hip: fsg_reduce_minmax_f32(x, n, mm), fsg_scale_f32(x, n, mm, mode, out), fsg_cast_f32_to_f16(x, n, out)
    bad(BAD, "fsg_reduce_minmax_f32", N, 64, P(mm), st)
    bad(BAD, "fsg_reduce_minmax_f32", P(f), 64, N, st)
    for a in ((N, 64, P(mm), 0, P(o)), (P(f), 64, N, 0, P(o)), (P(f), 64, P(mm), 0, N), (P(f), 64, P(mm), -1, P(o)),
              (P(f), 64, P(mm), 3, P(o))):
        bad(BAD, "fsg_scale_f32", *a, st)
    bad(BAD, "fsg_cast_f32_to_f16", N, 64, P(o), st)
    bad(BAD, "fsg_cast_f32_to_f16", P(f), 64, N, st)
    torch.cuda.synchronize()
    assert (host(o) == -9).all() and (host(o2) == -9).all() and (host(f) == 5).all() and not host(i64).any()
    assert host(mm).tolist() == host(K.new_minmax(DEV)).tolist()
    assert len(set(calls)) == 19  # the 16 entry points of fsg_artifacts.hip and the 3 of fsg_reduce.hip


def test_empty_is_success(K):
    """The entry points of the two files whose work is one flat range of n elements: n == 0 is success with no launch (pointers
    may be null, outputs untouched); fsg_hip.h lists which calls follow the rule and which do not."""
    from fetalsyngen_amd import _lib

    lib, st, N = _lib.load(), K._stream(None), C.c_void_p(0)
    assert lib.fsg_blend_f32(N, N, N, 0, 0, N, 0.0, N, 0, N, N, 0.0, N, N, st) == 0
    assert lib.fsg_slice_noise_f32(N, 0, 0.0, 1.0, N, N, 1, 1, st) == 0
    assert lib.fsg_nonzero_count_f32(N, 0, 0, 0.0, N, st) == 0 and lib.fsg_nonzero_count_u8(N, 0, 0, 0.0, N, st) == 0
    assert lib.fsg_nonzero_select_f32(N, 0, 0, 0.0, N, N, 0, N, st) == 0 and lib.fsg_nonzero_select_u8(N, 0, 0, 0.0, N, N, 0, N, st) == 0
    assert lib.fsg_compact_f32(N, N, 0, 0, 0.0, N, N, st) == 0 and lib.fsg_ewise_f32(N, N, 0, 0, 0.0, N, st) == 0
    assert lib.fsg_boundary_mask_f32(N, N, N, N, N, 6, 0, N, N, st) == 0 and lib.fsg_bernoulli_keep_f32(N, 0, 0.5, 1, 1, N, st) == 0
    assert lib.fsg_scatter_const_f32(N, 0, N, 1, 1.0, st) == 0 and lib.fsg_cast_f32_to_f16(N, 0, N, st) == 0
    mm = K.new_minmax(DEV)
    assert lib.fsg_reduce_minmax_f32(N, 0, C.c_void_p(mm.data_ptr()), st) == 0 and lib.fsg_scale_f32(N, 0, N, 1, N, st) == 0
    assert (K.key_to_float(int(host(mm)[0])), K.key_to_float(int(host(mm)[1]))) == (np.inf, -np.inf)  # the identities stay
    e = torch.empty(0, device=DEV)
    total, select = K.nonzero_ranks(e)
    assert total == 0 and tuple(select([]).shape) == (0, 1)
    assert K.compact_values(e, e).numel() == 0 and K.axpy(e, e).numel() == 0 and K.cast_f16(e).numel() == 0
    assert K.bernoulli_keep(e, 0.5, 1).numel() == 0 and K.scale(e, mm, 1).numel() == 0
