"""GPU: every kernel of csrc/fsg_intensity.hip, the GMM loop of csrc/fsg_common.h and the GMM jobs of the one-launch sample head
(csrc/fsg_deform.hip: sample_head_kernel, csrc/fsg_ride.h: gmm_codes_job), called directly, against the reference
(tests/util_intensity64.py, validated on the CPU by tests/test_intensity64_reference.py) at the places where the kernels branch:
the 4-voxel Philox groups and their ragged tails, the 16-byte store switch of gmm_kernel (outputs that start 4 and 8 bytes into
an allocation), the grid caps (a second grid trip beyond 8192 x 256 x 4 and 8192 x 256 elements, the head's 4096-workgroup
cap), tables of 1 and 256 entries, labels at and beyond the table, the int64 clamp, the lean and the general branch of
fsg_gmm_x4_loop, absent parts in the middle, the key reset of the _mm entry, the 64 x 4 tiles of bias_kernel, the peel loop of
label_stats_kernel (one label per wave, 64 labels per wave, labels >= nlabels beside valid ones, partial waves and
workgroups), and every argument check of the entry points.

Comparisons.  The GMM draws and add_noise are compared BIT FOR BIT (the sign of a zero included) with the float32 restatement;
their normals are the injected ones, or K.randn of the same (seed, stream, shape), which test_randn holds to the float64
Box-Muller of the reference.  The only tolerances are
  * 4e-5 absolute for the normals (tests/test_keyed_draws.py: v_log / v_sqrt / v_sin / v_cos against libm, |z| <= 5.77);
  * ATOL 1e-3 + RTOL 1e-5 of tests/test_hip_parity.py for powf / expf on the 0..255 scale (gamma, bias);
  * label_sums_bound, derived from the kernel's accumulation order (70 u / 71 u of the label's sum of |v| / v^2).
Figures measured on an MI355X (BOUND lines): randn 8.5e-7 = 0.021 of the bar; gamma <= 0.012, bias <= 0.009 of their
tolerance; label sums <= 0.087, sums of squares <= 0.108 of the bound (both with 64 labels in every wave).
Every output is preceded by poison() or is a NaN-filled buffer with guard elements on both sides; large cases (about 2^23
elements, there only to reach the second grid trip) are compared at sampled indices (the first 4096, the last 4101, 2^16 at a
stride) and checked for unwritten elements as a whole.  The large sizes run at ntab = 50 only.

kernel -> test
  randn_kernel                                   test_randn
  gmm_kernel<uint8_t>, gmm_kernel<int64_t>       test_gmm_kernel
  gmm_x4_kernel (fsg_gmm_x4_loop lean, general)  test_gmm_x4, test_gmm_x4_tables
  gmm_x4_kernel key reset (fsg_gmm_sample_u8x4_mm)  test_gmm_x4_mm_reset
  add_noise_kernel                               test_add_noise
  gamma_kernel                                   test_gamma
  bias_kernel                                    test_bias_mul
  label_stats_kernel                             test_label_stats
  sample_head_kernel, volumes (fsg_gmm_x4_loop)  test_sample_head_volumes
  sample_head_kernel, codes (gmm_codes_job)      test_sample_head_codes
  argument checks of all entry points            test_bad_arguments, test_empty_is_success, test_wrappers_check_table_lengths
"""
import ctypes as C

import numpy as np
import pytest
import torch

from fetalsyngen_amd import tables as T
from tests import util_intensity64 as R
from tests import util_warp64 as W
from tests.util_warp_cases import cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
ATOL, RTOL = 1e-3, 1e-5          # tests/test_hip_parity.py
BIG_GROUPS = 2 ** 23             # beyond 8192 workgroups x 256 lanes x 4 voxels
N = C.c_void_p(0)


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (and libfsg_hip.so); there is no fallback to skip to")
    from fetalsyngen_amd import kernels

    return kernels


@pytest.fixture(scope="module")
def lib(K):
    from fetalsyngen_amd import _lib

    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def P(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


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
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.size} outputs beyond the bound, first at "
                           f"{np.argwhere(bad)[0].tolist()}: got {got[bad][0]!r}, want {ref[bad][0]!r} +- {bound[bad][0]:.3g}")
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"BOUND {name:48s} max err {err.max():.3e}  {ratio:.3f} of bound")
    return ratio


def guarded(n, lead=0, tail=4):
    """(buffer of NaN, its view of n elements that starts `lead` elements in): what lies outside the view must stay NaN."""
    buf = torch.full((lead + n + tail,), float("nan"), device=DEV)
    return buf, buf[lead:lead + n]


def guards_intact(buf, lead, n):
    return bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + n:]).all())


def same_bits(name, got, want, idx=None):
    """Bit for bit on the host (at `idx` when given)."""
    g = host(got).reshape(-1)
    g = g if idx is None else g[idx]
    gb, wb = bits(g), bits(want)
    bad = gb != wb
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.size} outputs differ, first at {np.flatnonzero(bad)[0]}: "
                           f"got {g[bad][0]!r}, want {np.asarray(want)[bad][0]!r}")


def normals(K, n, seed, stream):
    poison(n)
    z = K.randn((n,), seed, stream, DEV)
    assert not bool(torch.isnan(z).any())
    return z


# ---- randn_kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", R.RANDN_KEYS, ids=lambda k: f"{k[0]:#x}-{k[1]:#x}")
def test_randn(K, lib, key):
    seed, stream = key
    worst, big = 0.0, None
    for n in sorted(R.RANDN_N, reverse=True):
        buf, out = guarded(n, lead=1)  # 4 bytes into the allocation: the kernel stores element by element
        assert lib.fsg_randn_f32(P(out), n, seed, stream, K._stream(out)) == 0
        assert guards_intact(buf, 1, n) and not bool(torch.isnan(out).any()), n
        if big is None:
            big = out
        assert torch.equal(out.view(torch.int32), big[:n].view(torch.int32)), n  # element e depends on e alone: a prefix
        idx = R.sample_indices(n)
        got, ref = host(out)[idx].astype(np.float64), R.normals64(seed, stream, idx)
        err = np.abs(got - ref)
        assert err.max() <= R.NORMALS_ATOL, (f"n={n}: |z - normals64| = {err.max():.3e} at element {idx[err.argmax()]} "
                                             f"(lane {idx[err.argmax()] & 3}), reference {ref[err.argmax()]!r}")
        worst = max(worst, float(err.max()))
        poison(n)
        assert torch.equal(K.randn((n,), seed, stream, DEV).view(torch.int32), out.view(torch.int32))  # the wrapper, aligned
    z = host(big)
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.var() - 1) < 5 * np.sqrt(2 / z.size)  # sanity line, not the test
    print(f"BOUND randn {key}: max err {worst:.3e}  {worst / R.NORMALS_ATOL:.3f} of bound")


# ---- gmm_kernel<uint8_t>, gmm_kernel<int64_t> ---------------------------------------------------------------------------------------------
GMM_N = tuple(range(1, 10)) + (255, 256, 257, 1025, BIG_GROUPS + 5)


@pytest.mark.parametrize("ntab", [1, 50, 256])
@pytest.mark.parametrize("i64", [False, True], ids=["u8", "i64"])
def test_gmm_kernel(K, lib, i64, ntab):
    fn = lib.fsg_gmm_sample_i64 if i64 else lib.fsg_gmm_sample_u8
    mus, sigmas = R.gmm_tables(ntab)
    dmu, dsg = dev(mus), dev(sigmas)
    seed, stream = 2 ** 63 + 5 + ntab, 2 ** 40 + 3
    for n in GMM_N:
        if n > 2 ** 20 and ntab != 50:
            continue
        lab = R.gmm_labels(n, ntab, i64)
        dlab = dev(lab)
        idx = R.sample_indices(n)
        zs = {"injected": dev(R.gmm_noise(n)), "philox": normals(K, n, seed, stream)}
        refs = {k: R.gmm32(lab[idx], mus, sigmas, ntab, host(z)[idx]) for k, z in zs.items()}
        for lead in (0, 1, 2):  # 0: 16-byte stores; 4 and 8 bytes in: the element-wise branch for every group
            if n > 2 ** 20 and lead == 2:
                continue
            for mode, z in zs.items():
                buf, out = guarded(n, lead)
                assert out.data_ptr() % 16 == 4 * lead
                rc = fn(P(dlab), n, P(dmu), P(dsg), ntab, P(z) if mode == "injected" else N, seed, stream, P(out), K._stream(out))
                what = f"gmm {'i64' if i64 else 'u8'} ntab={ntab} n={n} out+{4 * lead}B {mode}"
                assert rc == 0 and guards_intact(buf, lead, n) and not bool(torch.isnan(out).any()), what
                same_bits(what, out, refs[mode], idx)
        poison(n)
        same_bits("wrapper", K.gmm_sample(dlab, dmu, dsg, seed=seed, stream_id=stream), refs["philox"], idx)


# ---- gmm_x4_kernel: fsg_gmm_x4_loop ---------------------------------------------------------------------------------------------------------
LEAN_N = (4, 8, 1024, BIG_GROUPS + 8)
GENERAL_N = (1, 2, 3, 5, 7, 1023, BIG_GROUPS + 5)
ARRANGEMENTS = {"1": (0,), "2": (0, 1), "3": (0, 1, 2), "4": (0, 1, 2, 3), "l0,-,l2,-": (0, None, 1, None), "l0,-,-,l3": (0, None, None, 1)}


def x4_call(K, lib, slots, n, dmu, dsg, ntab, noise, seed, stream, mm=None, nmin=0, nmax=0):
    """fsg_gmm_sample_u8x4[_mm] into a NaN buffer with a guard behind it (the output must be 16-byte aligned)."""
    buf, out = guarded(n)
    ptrs = [N if s is None else P(s) for s in slots]
    if mm is None:
        rc = lib.fsg_gmm_sample_u8x4(*ptrs, n, P(dmu), P(dsg), ntab, N if noise is None else P(noise), seed, stream, P(out), K._stream(out))
    else:
        rc = lib.fsg_gmm_sample_u8x4_mm(*ptrs, n, P(dmu), P(dsg), ntab, N if noise is None else P(noise), seed, stream, P(out),
                                        P(mm), nmin, nmax, K._stream(out))
    assert rc == 0 and guards_intact(buf, 0, n) and not bool(torch.isnan(out).any())
    return out


def x4_inputs(n, ntab, arrangement, seed=0):
    """(summed label volume, the four slots as host arrays or None)."""
    rs = np.random.RandomState(n % 1000 + seed)
    lab = R.gmm_labels(n, ntab, False, seed)
    order = ARRANGEMENTS[arrangement]
    parts = R.split_parts(lab, sum(o is not None for o in order), rs)
    slots = [None if o is None else parts[o] for o in order] + [None] * (4 - len(order))
    assert np.array_equal(R.parts_label(slots), lab)
    return lab, slots


@pytest.mark.parametrize("arrangement", list(ARRANGEMENTS))
def test_gmm_x4(K, lib, arrangement):
    ntab = 50
    mus, sigmas = R.gmm_tables(ntab)
    dmu, dsg = dev(mus), dev(sigmas)
    seed, stream = 2 ** 64 - 1, 2 ** 33 + 1
    for n in sorted(LEAN_N + GENERAL_N):
        if n > 2 ** 20 and arrangement not in ("4", "l0,-,l2,-"):
            continue
        lab, slots = x4_inputs(n, ntab, arrangement)
        dslots = [None if s is None else dev(s) for s in slots]
        dlab, idx = dev(lab), R.sample_indices(n)
        z = normals(K, n, seed, stream)
        what = f"gmm_x4 [{arrangement}] n={n}"
        out = x4_call(K, lib, dslots, n, dmu, dsg, ntab, None, seed, stream)  # n % 4 == 0: the lean branch, else the general one
        same_bits(what + " philox", out, R.gmm32(lab[idx], mus, sigmas, ntab, host(z)[idx]), idx)
        poison(n)
        assert torch.equal(out.view(torch.int32), K.gmm_sample(dlab, dmu, dsg, seed=seed, stream_id=stream).view(torch.int32)), what
        gen = x4_call(K, lib, dslots, n, dmu, dsg, ntab, z, seed ^ 1, stream + 1)  # the general branch on the same normals
        assert torch.equal(out.view(torch.int32), gen.view(torch.int32)), what + ": lean and general branch differ"
        inj = dev(R.gmm_noise(n))
        out = x4_call(K, lib, dslots, n, dmu, dsg, ntab, inj, seed, stream)
        same_bits(what + " injected", out, R.gmm32(lab[idx], mus, sigmas, ntab, host(inj)[idx]), idx)
        if arrangement in "1234" and n in (1023, 1024):  # the wrapper
            poison(n)
            got = K.gmm_sample_parts([s for s in dslots if s is not None], dmu, dsg, seed=seed, stream_id=stream)
            same_bits(what + " wrapper", got, R.gmm32(lab, mus, sigmas, ntab, host(z)))


@pytest.mark.parametrize("ntab", [1, 256])
def test_gmm_x4_tables(K, lib, ntab):
    mus, sigmas = R.gmm_tables(ntab, seed=1)
    dmu, dsg = dev(mus), dev(sigmas)
    for n in (8, 1023, 1024):
        lab, slots = x4_inputs(n, ntab, "4", seed=1)
        assert (lab >= ntab).any() or ntab == 256
        dslots = [dev(s) for s in slots]
        z = normals(K, n, 7, 9)
        out = x4_call(K, lib, dslots, n, dmu, dsg, ntab, None, 7, 9)
        same_bits(f"gmm_x4 ntab={ntab} n={n}", out, R.gmm32(lab, mus, sigmas, ntab, host(z)))


SENTINEL = 0x5A5A5A5A


@pytest.mark.parametrize("nmm", [(0, 0), (1, 1), (3, 3), (64, 0), (32, 32)], ids=str)
def test_gmm_x4_mm_reset(K, lib, nmm):
    nmin, nmax = nmm
    ntab, n = 50, 1024
    mus, sigmas = R.gmm_tables(ntab)
    dmu, dsg = dev(mus), dev(sigmas)
    lab, slots = x4_inputs(n, ntab, "4")
    dslots = [dev(s) for s in slots]
    z = normals(K, n, 11, 12)
    want = np.concatenate([R.minmax_identities(nmin, nmax), np.full(72 - nmin - nmax, SENTINEL, np.int32)])
    mm = torch.full((72,), SENTINEL, dtype=torch.int32, device=DEV)
    out = x4_call(K, lib, dslots, n, dmu, dsg, ntab, None, 11, 12, mm, nmin, nmax)
    same_bits(f"gmm_x4_mm {nmm}", out, R.gmm32(lab, mus, sigmas, ntab, host(z)))
    assert np.array_equal(host(mm), want), nmm
    # n == 0 with mm given still resets the keys (pointers may be null then), and nothing else
    mm.fill_(SENTINEL)
    assert lib.fsg_gmm_sample_u8x4_mm(N, N, N, N, 0, N, N, 0, N, 0, 0, N, P(mm), nmin, nmax, K._stream(mm)) == 0
    assert np.array_equal(host(mm), want), nmm
    if nmin + nmax:
        assert np.array_equal(host(K.new_minmax(DEV, nmin, nmax)), want[:nmin + nmax])  # fsg_minmax_init writes the same keys


# ---- add_noise_kernel, gamma_kernel, bias_kernel -----------------------------------------------------------------------------------------------
POINT_N = (1, 3, 5, 257, 2 ** 21 + 3)  # the last: beyond 8192 workgroups x 256 threads


@pytest.mark.parametrize("std", [0.0, 0.5, 40.0])
def test_add_noise(K, std):
    seed, stream = 2 ** 63 + 11, 2 ** 40 + 5
    for n in POINT_N:
        rs = np.random.RandomState(n % 1000)
        x = (rs.rand(n) * 255).astype(F)
        dx = dev(x)
        inj = R.gmm_noise(n)
        poison(n)
        same_bits(f"add_noise injected n={n} std={std}", K.add_noise(dx, std, noise=dev(inj)), R.add_noise32(x, std, inj))
        z = host(normals(K, n, seed, stream))
        poison(n)
        got = K.add_noise(dx, std, seed=seed, stream_id=stream)
        same_bits(f"add_noise philox n={n} std={std}", got, R.add_noise32(x, std, z))
        assert not np.signbit(host(got)).any()


@pytest.mark.parametrize("g", [float(np.exp(-0.5)), 1.0, float(np.exp(0.5))], ids=["exp(-0.5)", "1", "exp(0.5)"])
def test_gamma(K, g):
    worst = 0.0
    for n in POINT_N:
        x = R.gamma_inputs(n)
        ref = R.gamma64(x, g)
        poison(n)
        got = host(K.gamma(dev(x), g))
        worst = max(worst, within(f"gamma g={g:.4f} n={n}", got, ref, ATOL + RTOL * np.abs(ref)))
        assert (got[x == 0] == 0).all()
    neg = np.array([-1e-3, -1.0, -255.0, -300.0, 17.0], F)
    poison(5)
    got, ref = host(K.gamma(dev(neg), g)), R.gamma64(neg, g)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref[:4]).all() == (g != 1.0)
    ok = ~np.isnan(ref)
    within(f"gamma g={g:.4f} negative x", got[ok], ref[ok], ATOL + RTOL * np.abs(ref[ok]))
    print(f"BOUND gamma g={g:.4f}: {worst:.3f} of the tolerance")


@pytest.mark.parametrize("nz", [1, 63, 64, 65])
def test_bias_mul(K, nz):
    worst = 0.0
    for ny in (1, 3, 4, 5):
        for nx in (1, 2, 7):
            shape = (nx, ny, nz)
            rs = np.random.RandomState(nx * 100 + ny * 10 + nz)
            x = (rs.rand(*shape) * 255).astype(F)
            x.reshape(-1)[0] = 0
            dx = dev(x)
            for bshape in ((1, 1, 1), (2, 3, 4), (nx + 1, 2, nz + 3)):  # the last: larger than the volume on two axes
                bias = (rs.randn(*bshape) * 0.3).astype(F)
                tabs, new = T.zoom_tables(bshape, np.array(shape) / np.array(bshape))
                assert new == shape
                poison(shape)
                got = host(K.bias_mul(dx, dev(bias), K.DeviceTables(tabs, DEV)))
                ref = R.bias64(x, bias, tabs)
                worst = max(worst, within(f"bias {shape} grid {bshape}", got, ref, ATOL + RTOL * np.abs(ref)))
    print(f"BOUND bias nz={nz}: {worst:.3f} of the tolerance")


# ---- label_stats_kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", R.STATS_PATTERNS)
def test_label_stats(K, lib, pattern):
    worst = [0.0, 0.0]
    for n in R.STATS_N:
        for nlabels in (1, 50, 256):
            for signed in (0, 1):
                l, v = R.stats_inputs(n, pattern, nlabels, signed)
                dl, dv = dev(l), dev(v)
                cnt_ref, s1, s2 = R.label_sums64(l, v, nlabels)
                b1, b2 = R.label_sums_bound(l, v, nlabels)
                # 256 cells each: the first nlabels zeroed by the caller, the rest a sentinel nothing may touch
                cnt = torch.full((256,), -7, dtype=torch.int64, device=DEV)
                sums = torch.full((2, 256), -7.5, dtype=torch.float64, device=DEV)
                cnt[:nlabels], sums[:, :nlabels] = 0, 0
                for call in (1, 2):  # the second call accumulates into what the first one left
                    rc = lib.fsg_label_stats_u8(P(dl), P(dv), n, nlabels, P(cnt), P(sums[0]), P(sums[1]), K._stream(dv))
                    assert rc == 0
                    c, s = host(cnt), host(sums)
                    what = f"label_stats [{pattern}] n={n} nlabels={nlabels} signed={signed} call {call}"
                    assert np.array_equal(c[:nlabels], call * cnt_ref), what
                    assert (c[nlabels:] == -7).all() and (s[:, nlabels:] == -7.5).all(), what
                    r1 = within(what + " sum", s[0, :nlabels], call * s1, call * b1)
                    r2 = within(what + " sumsq", s[1, :nlabels], call * s2, call * b2)
                    worst = [max(worst[0], r1), max(worst[1], r2)]
    # the wrapper: counts, mean and variance from the same sums
    l, v = R.stats_inputs(4097, pattern, 50, 0)
    cnt, mean, var = K.label_stats(dev(l), dev(v), 50)
    cnt_ref, s1, s2 = R.label_sums64(l, v, 50)
    assert np.array_equal(host(cnt), cnt_ref)
    b1, _b2 = R.label_sums_bound(l, v, 50)
    den = np.maximum(cnt_ref, 1)
    within(f"label_stats [{pattern}] wrapper mean", host(mean), s1 / den, b1 / den + 1e-15 * np.abs(s1 / den))
    print(f"BOUND label_stats [{pattern}]: {worst[0]:.3f} / {worst[1]:.3f} of the bounds (sum / sum of squares)")


# ---- the one-launch sample head --------------------------------------------------------------------------------------------------------------
def plain_spec(K, shape):
    """No coarse field: an affine close to the identity about the centre."""
    cen = (np.array(shape, dtype=np.float64) - 1) / 2
    A = np.array([[1.02, 0.01, 0.0], [-0.01, 0.98, 0.02], [0.0, 0.015, 1.01]])
    return K.DeformSpec(shape, A, cen, cen + np.array([0.3, -0.2, 0.4]), False, device=DEV)


def floors(K, mm3):
    return [int(np.floor(K.key_to_float(int(k)))) for k in host(mm3)[:3]]


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 7, 9), (3, 4, 8), (4, 2, 2 ** 19 + 1)], ids=str)
def test_sample_head_volumes(K, shape):
    """No field and no bias: the launch has no rows job.  (4, 2, 2^19 + 1): n > 2^22, the GMM job's 4096-workgroup cap."""
    ntab, n = 50, int(np.prod(shape))
    mus, sigmas = R.gmm_tables(ntab)
    dmu, dsg = dev(mus), dev(sigmas)
    seed, stream = 2 ** 63 + 21, 2 ** 40 + 9
    idx = R.sample_indices(n)
    z = normals(K, n, seed, stream)
    for arrangement in (("1", "4") if n > 2 ** 20 else ("1", "2", "3", "4")):
        lab, slots = x4_inputs(n, ntab, arrangement)
        parts = [dev(s.reshape(shape)) for s in slots if s is not None]
        for mode, noise in (("philox", None), ("injected", dev(R.gmm_noise(n)))):
            spec = plain_spec(K, shape)
            poison(shape)
            img, mm3 = K.sample_head(parts, dmu, dsg, spec, noise=noise, seed=seed, stream_id=stream)
            zz = host(z if noise is None else noise)[idx]
            same_bits(f"head {shape} [{arrangement}] {mode}", img, R.gmm32(lab[idx], mus, sigmas, ntab, zz), idx)
            assert not bool(torch.isnan(img).any())
            K.coords_floormin_rest(spec, mm3)
            assert floors(K, mm3) == floors(K, K.coords_floormin(plain_spec(K, shape))), (shape, arrangement, mode)


def test_sample_head_volumes_field_and_bias(K):
    """The (7, 3, 33) field-and-bias case of tests/util_warp_cases.py: rows job, faces job and GMM job in one launch."""
    case = next(c for c in cases("x, y extent") if c.spec.shape == (7, 3, 33))
    s, shape, ntab = case.spec, case.spec.shape, 50
    n = int(np.prod(shape))
    mus, sigmas = R.gmm_tables(ntab)
    dmu, dsg = dev(mus), dev(sigmas)
    bias, bt = dev(case.bias), K.DeviceTables(case.bias_tabs, DEV)
    need = 3 * s.field.shape[2] + case.bias.shape[2]
    rows_ref = W.rows32(s, case.bias, case.bias_tabs).reshape(-1, need)
    keys = W.minmax32(W.positions32(s))
    z = normals(K, n, 5, 6)

    def new_spec():
        return K.DeformSpec(shape, s.A, s.cen, s.c2, False, dev(s.field), K.DeviceTables(s.tabs, DEV), device=DEV)

    for arrangement in ("1", "2", "3", "4"):
        lab, slots = x4_inputs(n, ntab, arrangement)
        parts = [dev(p.reshape(shape)) for p in slots if p is not None]
        for mode, noise in (("philox", None), ("injected", dev(R.gmm_noise(n)))):
            spec = new_spec()
            poison(shape, (shape[0] * shape[1] * ((need + 3) // 4 * 4),))
            img, mm3 = K.sample_head(parts, dmu, dsg, spec, bias, bt, noise=noise, seed=5, stream_id=6)
            what = f"head (7,3,33) [{arrangement}] {mode}"
            same_bits(what, img, R.gmm32(lab, mus, sigmas, ntab, host(z if noise is None else noise)))
            rows = spec._keep[-1].view(-1, int(spec.c.row_stride))[:, :need].contiguous()
            same_bits(what + " rows", rows, rows_ref.reshape(-1))
            spec2 = new_spec().prepare_rows(bias, bt)  # fsg_deform_rows_f32
            assert torch.equal(rows.view(torch.int32), spec2._keep[-1].view(-1, int(spec2.c.row_stride))[:, :need].contiguous().view(torch.int32))
            K.coords_floormin_rest(spec, mm3)
            assert floors(K, mm3) == floors(K, K.coords_floormin(spec2)) == W.margins(keys)[:3], what


CODES_MAX = 2048


def codes_inputs(n, ntuples, stride, seed):
    rs = np.random.RandomState(seed + n % 1000 + ntuples + stride)
    tuples = rs.randint(0, 24, (ntuples, stride)).astype(np.uint8)
    tuples[:, stride - 1] = 0                       # the zero column (a meta label without a seed volume)
    tuples[rs.randint(0, ntuples, max(ntuples // 8, 1)), :4] = 200  # sums beyond 255: the label is taken modulo 256
    codes = rs.randint(0, ntuples, n).astype(np.uint16)  # every code < ntuples: the kernel's table has no entry beyond
    codes[[0, -1]] = ntuples - 1
    assert int(codes.max()) < ntuples
    return codes, tuples


@pytest.mark.parametrize("stride", [25, 256])
@pytest.mark.parametrize("ntuples", [1, 37, CODES_MAX])
def test_sample_head_codes(K, lib, ntuples, stride):
    ntab = 50
    mus, sigmas = R.gmm_tables(ntab)
    dmu, dsg = dev(mus), dev(sigmas)
    seed, stream = 2 ** 64 - 3, 2 ** 35 + 2
    sels = ((0, 5, 9, 13), (3, 3, 3, 3), (2, 2, stride - 1, stride - 1), (stride - 1,) * 4, (0, 1, 2, 3))
    for shape in ((2, 2, 2), (2, 2, 4), (2, 4, 257), (2, 4, 2 ** 20 + 1)):
        n = int(np.prod(shape))
        if n > 2 ** 20 and (ntuples, stride) not in ((CODES_MAX, 256), (37, 25)):
            continue
        codes, tuples = codes_inputs(n, ntuples, stride, 0)
        dcodes, dtup = dev(codes.view(np.int16)), dev(tuples)
        assert dcodes.data_ptr() % 16 == 0 and dcodes.numel() == n and dtup.numel() == ntuples * stride
        idx = R.sample_indices(n)
        z = host(normals(K, n, seed, stream))[idx]
        beyond = False
        for sel in (sels[:2] if n > 2 ** 20 else sels):
            lab = R.codes_label(codes[idx], tuples, sel)
            beyond |= bool((lab >= ntab).any())
            spec = plain_spec(K, shape)
            epi = K._epilogue(None, None, None, shape)
            rows = torch.empty(shape[0] * shape[1] * 4, device=DEV)
            mm3 = K.new_minmax(DEV, 3, 0)
            buf, out = guarded(n)
            rc = lib.fsg_sample_head_codes_f32(P(dcodes), P(dtup), ntuples, stride, (C.c_int32 * 4)(*sel), n, P(dmu), P(dsg), ntab, seed,
                                               stream, P(out), C.byref(spec.c), C.byref(epi), P(rows), 4, P(mm3), K._stream(out))
            what = f"head codes {shape} ntuples={ntuples} stride={stride} sel={sel}"
            assert rc == 0 and guards_intact(buf, 0, n) and not bool(torch.isnan(out).any()), what
            same_bits(what, out, R.gmm32(lab, mus, sigmas, ntab, z), idx)
            if sel == (stride - 1,) * 4:
                assert (lab == 0).all()
            K.coords_floormin_rest(spec, mm3)
            assert floors(K, mm3) == floors(K, K.coords_floormin(plain_spec(K, shape))), what
        assert beyond or ntuples == 1, "no selection with a label >= ntab"


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
def test_wrappers_check_table_lengths(K):
    """kernels.gmm_sample_parts / sample_head refuse tables of different lengths (the kernels read both to one length) on the host."""
    part = torch.zeros(2, 2, 4, dtype=torch.uint8, device=DEV)
    for nm, ns in ((50, 49), (49, 50), (0, 0), (257, 257)):
        mus, sigmas = torch.zeros(nm, device=DEV), torch.zeros(ns, device=DEV)
        for call in (lambda: K.gmm_sample_parts([part], mus, sigmas), lambda: K.sample_head([part], mus, sigmas, plain_spec(K, (2, 2, 4))),
                     lambda: K.gmm_sample(part, mus, sigmas)):
            with pytest.raises(ValueError, match="mus/sigmas"):
                call()


def test_bad_arguments(K, lib):
    """Every refusal of the entry points of csrc/fsg_intensity.hip and of the two sample-head entry points, once.  They return
    before any launch: the sentinel-filled outputs stay untouched."""
    from fetalsyngen_amd import _lib

    st = K._stream(None)
    BAD, BIG, ALIGN = _lib.E_BADARG, _lib.E_TOOBIG, _lib.E_ALIGN
    f = torch.full((256,), 5.0, device=DEV)                              # inputs, tables
    u8 = torch.zeros(256, dtype=torch.uint8, device=DEV)
    i64 = torch.zeros(256, dtype=torch.int64, device=DEV)
    u16 = torch.zeros(256, dtype=torch.int16, device=DEV)
    o = torch.full((256,), -9.0, device=DEV)                             # outputs: must stay -9
    rows = torch.full((256,), -9.0, device=DEV)
    mm = torch.full((72,), SENTINEL, dtype=torch.int32, device=DEV)
    cnt = torch.full((256,), -7, dtype=torch.int64, device=DEV)
    sums = torch.full((2, 256), -7.5, dtype=torch.float64, device=DEV)
    calls = []

    def bad(code, fn, *args):
        calls.append(fn)
        assert getattr(lib, fn)(*args, st) == code, (fn, len(calls))

    def each(code, fn, good, changes):
        for i, v in changes:
            a = list(good)
            a[i] = v
            bad(code, fn, *a)

    bad(BAD, "fsg_randn_f32", N, 64, 1, 1)
    # fsg_gmm_sample_{u8,i64}(labels, n, mus, sigmas, ntab, noise, seed, stream_id, out)
    for fn, lab in (("fsg_gmm_sample_u8", u8), ("fsg_gmm_sample_i64", i64)):
        each(BAD, fn, [P(lab), 64, P(f), P(f), 50, N, 1, 1, P(o)], ((0, N), (2, N), (3, N), (8, N), (4, 0), (4, -1), (4, 257)))
    # fsg_gmm_sample_u8x4(l0, l1, l2, l3, n, mus, sigmas, ntab, noise, seed, stream_id, out)
    good = [P(u8), P(u8), P(u8), P(u8), 64, P(f), P(f), 50, N, 1, 1, P(o)]
    each(BAD, "fsg_gmm_sample_u8x4", good, ((0, N), (5, N), (6, N), (11, N), (7, 0), (7, -1), (7, 257)))
    each(ALIGN, "fsg_gmm_sample_u8x4", good, ((0, P(u8, 1)), (1, P(u8, 2)), (2, P(u8, 3)), (3, P(u8, 1)), (11, P(o, 4)), (11, P(o, 8))))
    # fsg_gmm_sample_u8x4_mm(..., out, mm, nmin, nmax): the key counts are checked first, also for n == 0
    good = good + [P(mm), 1, 1]
    each(BAD, "fsg_gmm_sample_u8x4_mm", good, ((13, 64), (13, 65), (14, 64), (13, -1), (14, -1), (0, N), (5, N), (6, N), (11, N), (7, 0), (7, 257)))
    each(ALIGN, "fsg_gmm_sample_u8x4_mm", good, ((1, P(u8, 1)), (11, P(o, 4))))
    a = list(good)
    a[4], a[13] = 0, 64
    bad(BAD, "fsg_gmm_sample_u8x4_mm", *a)
    # fsg_label_stats_u8(labels, values, n, nlabels, count, sum, sumsq)
    good = [P(u8), P(f), 64, 50, P(cnt), P(sums[0]), P(sums[1])]
    each(BAD, "fsg_label_stats_u8", good, ((0, N), (1, N), (4, N), (5, N), (6, N), (3, 0), (3, -1), (3, 257)))
    # fsg_gamma_f32(x, n, gamma, out); fsg_add_noise_f32(x, n, noise, seed, stream_id, std, out)
    each(BAD, "fsg_gamma_f32", [P(f), 64, 1.0, P(o)], ((0, N), (3, N)))
    each(BAD, "fsg_add_noise_f32", [P(f), 64, N, 1, 1, 1.0, P(o)], ((0, N), (6, N)))
    # fsg_bias_mul_f32(x, nx, ny, nz, bias, b0, b1, b2, bx, by, bz, out)
    good = [P(f), 2, 2, 2, P(f), 1, 1, 1, P(f), P(f), P(f), P(o)]
    each(BAD, "fsg_bias_mul_f32", good, ((0, N), (4, N), (8, N), (9, N), (10, N), (11, N), (1, 0), (2, 0), (3, 0), (1, -1), (2, -2), (3, -3),
                                         (5, 0), (6, 0), (7, 0), (5, -1), (6, -1), (7, -1)))
    # fsg_sample_head_f32(l0, l1, l2, l3, n, mus, sigmas, ntab, noise, seed, stream_id, out, d, epi, rows, row_stride, mm3)
    spec = plain_spec(K, (2, 4, 8))
    epi = K._epilogue(None, None, None, (2, 4, 8))
    good = [P(u8), P(u8), P(u8), P(u8), 64, P(f), P(f), 50, N, 1, 1, P(o), C.byref(spec.c), C.byref(epi), P(rows), 4, P(mm)]
    each(BAD, "fsg_sample_head_f32", good, ((4, 0), (0, N), (5, N), (6, N), (11, N), (16, N), (7, 0), (7, 257), (4, 56), (4, 72), (12, None)))
    each(ALIGN, "fsg_sample_head_f32", good, ((0, P(u8, 2)), (3, P(u8, 1)), (11, P(o, 4))))
    # fsg_sample_head_codes_f32(codes, tuples, ntuples, stride, sel, n, mus, sigmas, ntab, seed, stream_id, out, d, epi, rows, row_stride, mm3)
    sel = lambda *v: (C.c_int32 * 4)(*v)  # noqa: E731
    good = [P(u16), P(u8), 4, 25, sel(0, 1, 2, 24), 64, P(f), P(f), 50, 1, 1, P(o), C.byref(spec.c), C.byref(epi), P(rows), 4, P(mm)]
    each(BAD, "fsg_sample_head_codes_f32", good, ((5, 0), (0, N), (1, N), (4, None), (6, N), (7, N), (11, N), (16, N), (8, 0), (8, 257), (2, 0),
                                                  (2, -1), (3, 0), (3, 257), (4, sel(0, 1, 2, 25)), (4, sel(25, 0, 0, 0)), (4, sel(0, -1, 0, 0)),
                                                  (12, None)))
    each(BIG, "fsg_sample_head_codes_f32", good, ((2, CODES_MAX + 1),))
    each(ALIGN, "fsg_sample_head_codes_f32", good, ((0, P(u16, 2)), (0, P(u16, 8)), (11, P(o, 4))))
    spec60 = plain_spec(K, (3, 4, 5))  # n = 60 agrees with the shape, but is no multiple of 8
    a = list(good)
    a[5], a[12] = 60, C.byref(spec60.c)
    bad(ALIGN, "fsg_sample_head_codes_f32", *a)
    a = list(good)
    a[5] = 72                          # a multiple of 8 that disagrees with the shape
    bad(BAD, "fsg_sample_head_codes_f32", *a)
    torch.cuda.synchronize()
    assert (host(o) == -9).all() and (host(rows) == -9).all() and (host(mm) == SENTINEL).all()
    assert (host(cnt) == -7).all() and (host(sums) == -7.5).all() and (host(f) == 5).all()
    assert len(set(calls)) == 11  # the 9 entry points of fsg_intensity.hip and the 2 sample heads


def test_empty_is_success(K, lib):
    """n == 0 is success with no launch in every flat-range entry point of fsg_intensity.hip; pointers, ntab and nlabels are
    not looked at.  (fsg_gmm_sample_u8x4_mm with mm given still resets the keys: test_gmm_x4_mm_reset.)"""
    st = K._stream(None)
    assert lib.fsg_randn_f32(N, 0, 1, 1, st) == 0
    assert lib.fsg_gmm_sample_u8(N, 0, N, N, 0, N, 1, 1, N, st) == 0 and lib.fsg_gmm_sample_i64(N, 0, N, N, 0, N, 1, 1, N, st) == 0
    assert lib.fsg_gmm_sample_u8x4(N, N, N, N, 0, N, N, 0, N, 1, 1, N, st) == 0
    assert lib.fsg_gmm_sample_u8x4_mm(N, N, N, N, 0, N, N, 0, N, 1, 1, N, N, 0, 0, st) == 0
    assert lib.fsg_label_stats_u8(N, N, 0, 0, N, N, N, st) == 0
    assert lib.fsg_gamma_f32(N, 0, 1.0, N, st) == 0 and lib.fsg_add_noise_f32(N, 0, N, 1, 1, 1.0, N, st) == 0
    e = torch.empty(0, device=DEV)
    e8 = torch.empty(0, dtype=torch.uint8, device=DEV)
    mus = dev(np.ones(3, F))
    assert K.randn((0,), 1, 2, DEV).numel() == 0 and K.randn((3, 0, 2), 1, 2, DEV).shape == (3, 0, 2)
    assert K.gamma(e, 1.3).numel() == 0 and K.add_noise(e, 1.0).numel() == 0 and K.add_noise(e, 1.0, noise=e).numel() == 0
    assert K.gmm_sample(e8, mus, mus).numel() == 0 and K.gmm_sample_parts([e8, e8], mus, mus).numel() == 0
    cnt, mean, var = K.label_stats(e8, e, 5)
    assert host(cnt).tolist() == [0] * 5 and host(mean).tolist() == [0.0] * 5 and host(var).tolist() == [0.0] * 5
