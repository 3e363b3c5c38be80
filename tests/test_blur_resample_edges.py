"""GPU: K6 + K7 + K8 -- the fused pair (kernels.blur_resample: blur_rs_x_kernel<R> + blur_rs_yz_kernel<R>) and the unfused
sequence (blur_axis / blur_yz, then resample_noise) -- against the float64 reference (tests/util_resample64.py) at the edges
of the kernels: every radius on every axis, m == n, m = n - 1, m = 1, m = n / 2, axes shorter than the blur window and
around the 16-row chunks, short and ragged rows, the LDS and row-length limits of the y,z launch, Philox quads that cross
rows, misaligned views, hand-made tables, a large dynamic range with exact zeros, and the x kernel's 32-bit row offsets.

Every output must lie within the float32 rounding bound of the operation (util_resample64.error_bound; tighter than the
blur's atol 1e-3 / rtol 1e-5 on 0..255 inputs): "outside" outputs, outputs whose inputs are all zero and clamped outputs are
therefore exactly 0.  Configurations outside the fused pair's domain must be refused (None), never computed wrongly.
"""
import numpy as np
import pytest
import torch

from tests.util_resample64 import blur_resample64, error_bound

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL, RTOL = 1e-3, 1e-5


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (and libfsg_hip.so); there is no fallback to skip to")
    from fetalsyngen_amd import kernels

    return kernels


def down_table(m, n):
    """RandResample's table for m outputs of an n-long axis (positions delta + j n / m; m == n: output 0 outside)."""
    from fetalsyngen_amd import tables as T

    return T._resample_axis_table(m, n)


def radius_taps(R, seed):
    """2R + 1 positive, asymmetric taps (a tap read from the wrong row or in the wrong order shows)."""
    k = np.random.RandomState(seed).rand(2 * R + 1) + 0.2
    return (k / k.sum()).astype(np.float32)


def poison(*shapes):
    """Hand the next allocations of these shapes blocks full of NaN (the caching allocator reuses a freed block of the
    same size): an output a kernel never writes then fails the comparison instead of passing on a lucky zero."""
    for s in shapes:
        t = torch.full(s, float("nan"), device=DEV)
        del t


def unfused(K, x, taps, tabs, **kw):
    y = K.blur_axis(x, 0, taps[0])
    yz = K.blur_yz(y, taps[1], taps[2])
    if yz is None:
        yz = K.blur_axis(K.blur_axis(y, 1, taps[1]), 2, taps[2])
    return K.resample_noise(yz, tabs, **kw)


def check(name, path, out, x, taps, tabs, z, std, outside_axes):
    """`out` against the reference; returns (max |error|, max error / bound)."""
    o = out.detach().cpu().numpy().astype(np.float64)
    ref = blur_resample64(x, taps, tabs, std, z)
    bound = error_bound(x, taps, tabs, std, z)
    assert o.shape == ref.shape, (name, path)
    err = np.abs(o - ref)
    bad = ~(err <= bound)
    assert not bad.any(), (f"{name} [{path}]: {int(bad.sum())} outputs beyond the rounding bound, first at "
                           f"{np.argwhere(bad)[0].tolist()}: got {o[bad][0]!r}, want {ref[bad][0]!r} +- {bound[bad][0]:.3g}")
    np.testing.assert_allclose(o, ref, rtol=RTOL, atol=ATOL)
    assert (o[bound == 0] == 0).all(), (name, path)  # zero in, zero out: exactly
    for a in outside_axes:  # an output at position 0 (m == n) is "outside": exactly 0 (before the noise)
        if z is None:
            assert (np.take(o, 0, axis=a) == 0).all(), (name, path, a)
    if z is not None:
        assert (o >= 0).all(), (name, path)
        pre = blur_resample64(x, taps, tabs) + np.float64(np.float32(std)) * z.astype(np.float64)
        assert (o[pre < -bound] == 0).all(), (name, path)  # clamped: exactly 0
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    return float(err.max()), ratio


def run_case(K, name, x, taps, m, noise=None, fused_ok=True, tabs=None, xd=None):
    n = x.shape
    if tabs is None:
        tabs = [down_table(m[a], n[a]) for a in range(3)]
    new = tuple(len(t) for t in tabs)
    rt = K.DeviceTables(tabs, DEV)
    if xd is None:
        xd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    kw, z, std = {}, None, None
    if noise is not None:
        mode, std = noise[0], noise[1]
        if mode == "pointer":
            zd = K.randn(new, 7, 3, DEV)
            kw = dict(noise_std=std, noise=zd)
        else:  # Philox: the epilogue's field is K.randn of the output shape
            kw = dict(noise_std=std, seed=noise[2], stream_id=noise[3])
            zd = K.randn(new, noise[2], noise[3], DEV)
        z = zd.cpu().numpy()
    outside = [a for a in range(3) if tabs[a]["lo"][0] < 0]
    poison(new, (new[0], n[1], n[2]))
    f = K.blur_resample(xd, rt, taps, **kw)
    u = unfused(K, xd, taps, rt, **kw)
    torch.cuda.synchronize()
    eu = check(name, "unfused", u, x, taps, tabs, z, std, outside)
    line = f"EDGE {name:34s} n={n} m={new} R={tuple(len(t) // 2 for t in taps)} noise={noise and noise[0]}"
    if f is not None:  # refused or right: a result is checked before asking whether it should exist
        ef = check(name, "fused", f, x, taps, tabs, z, std, outside)
        np.testing.assert_allclose(f.cpu().numpy(), u.cpu().numpy(), rtol=RTOL, atol=ATOL)
        assert fused_ok, f"{name}: outside the fused pair's domain, but it computed a result (a right one)"
        print(f"{line} fused {ef[0]:.3e} ({ef[1]:.3f} of bound) unfused {eu[0]:.3e} ({eu[1]:.3f})")
    else:
        assert not fused_ok, f"{name}: the fused pair refused a configuration inside its domain"
        print(f"{line} fused refused, unfused {eu[0]:.3e} ({eu[1]:.3f})")


def vol(shape, seed):
    x = (np.random.RandomState(seed).rand(*shape) * 255).astype(np.float32)
    x[: max(shape[0] // 3, 1)] *= 0.1  # structure along x, not only white noise
    return x


PHILOX = ("philox", 40.0, 99, 2)
POINTER = ("pointer", 11.0)

# (name, shape, m, radii (x, y, z), noise, fused domain)
CASES = []
for R in range(1, 9):  # every radius on every axis; ntaps_y != ntaps_z (the y,z kernel pads the narrower set)
    CASES.append((f"radius x{R} y{R} z{9 - R}", (37, 29, 44), (18, 14, 21), (R, R, 9 - R), (None, POINTER, PHILOX)[R % 3], True))
for R in (1, 5, 8):    # one tap set on y and z (the kernel's SAME instance)
    CASES.append((f"isotropic R{R}", (24, 20, 16), (11, 9, 7), (R, R, R), PHILOX, True))
CASES += [
    ("m == n axis 0", (20, 18, 24), (20, 9, 12), (2, 3, 2), None, False),
    ("m == n axis 1", (20, 18, 24), (10, 18, 12), (2, 3, 2), None, False),
    ("m == n axis 2", (20, 18, 24), (10, 9, 24), (2, 3, 2), None, False),
    ("m == n axis 0, noise", (20, 18, 24), (20, 9, 12), (2, 3, 2), PHILOX, False),
    ("m = n - 1", (21, 19, 28), (20, 18, 27), (3, 3, 3), PHILOX, True),
    ("m = n - 1, R 8", (21, 19, 28), (20, 18, 27), (8, 8, 8), None, True),
    ("m = 1", (12, 10, 8), (1, 1, 1), (4, 4, 4), None, True),
    ("m = 1, noise", (12, 10, 8), (1, 1, 1), (4, 2, 6), POINTER, True),
    ("m = n / 2", (32, 24, 40), (16, 12, 20), (2, 2, 2), None, True),
    ("m = n / 2, R 7", (32, 24, 40), (16, 12, 20), (7, 7, 7), PHILOX, True),
    ("n0 = 2 < 2R + 1", (2, 12, 16), (1, 6, 8), (8, 2, 2), None, True),
    ("n0 = 5 < 2R + 1", (5, 12, 16), (2, 6, 8), (6, 2, 2), None, True),
    ("n0 = 15", (15, 12, 16), (14, 6, 8), (5, 2, 2), None, True),
    ("n0 = 16k - 1", (31, 12, 16), (30, 6, 8), (5, 2, 2), None, True),
    ("n0 = 16k", (32, 12, 16), (31, 6, 8), (5, 2, 2), None, True),
    ("n0 = 16k + 1", (33, 12, 16), (32, 6, 8), (5, 2, 2), None, True),
    ("n0 = 16k + 1, m0 = 19", (33, 12, 16), (19, 6, 8), (8, 2, 2), None, True),
    ("n0 = 48, m0 = 47", (48, 12, 16), (47, 6, 8), (3, 2, 2), None, True),
    ("n1 = 5 < 8", (20, 5, 16), (10, 2, 8), (2, 6, 2), None, True),
    ("n1 = 7 < 8, m1 = 6", (20, 7, 16), (10, 6, 8), (2, 3, 2), PHILOX, True),
    ("n1 = 33", (20, 33, 16), (10, 32, 8), (2, 4, 2), None, True),
    ("n1 = 45", (20, 45, 16), (10, 30, 8), (2, 8, 2), PHILOX, True),
    ("n2 = 4", (20, 16, 4), (10, 8, 3), (2, 2, 1), None, True),
    ("n2 = 4, m2 = 1", (20, 16, 4), (10, 8, 1), (2, 2, 4), PHILOX, True),
    ("m2 = 13 (1 mod 4)", (16, 13, 24), (8, 11, 13), (3, 3, 3), PHILOX, True),
    ("m2 = 14 (2 mod 4)", (16, 13, 24), (8, 11, 14), (3, 3, 3), PHILOX, True),
    ("m2 = 15 (3 mod 4)", (16, 13, 24), (8, 11, 15), (3, 3, 3), PHILOX, True),
    ("m2 = 255 (3 mod 4)", (6, 9, 300), (5, 7, 255), (2, 2, 2), PHILOX, True),
    ("m2 = 301 (1 mod 4)", (6, 9, 436), (5, 7, 301), (2, 2, 2), PHILOX, True),
    ("m2 = 301, pointer noise", (6, 9, 436), (5, 7, 301), (2, 2, 2), POINTER, True),
    ("lds 63936 (n2 436, R 4)", (6, 9, 436), (5, 7, 435), (4, 4, 4), None, True),
    ("lds 64512 (n2 440, R 4)", (6, 9, 440), (5, 7, 439), (4, 4, 4), None, False),
    ("lds 63936 (n2 428, R 8)", (6, 9, 428), (5, 7, 214), (2, 3, 8), None, True),
    ("lds 64512 (n2 432, R 8)", (6, 9, 432), (5, 7, 216), (2, 3, 8), None, False),
    ("n2 = 512", (6, 9, 512), (5, 7, 256), (2, 2, 2), None, False),
    ("n2 = 516", (6, 9, 516), (5, 7, 258), (2, 2, 2), None, False),
    ("n2 = 18 (n2 % 4 != 0)", (12, 9, 18), (6, 7, 9), (2, 2, 2), None, False),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fused_and_unfused_equal_the_float64_reference(K, case):
    name, shape, m, radii, noise, fused_ok = case
    # equal y and z radii give equal tap sets: the y,z kernel's one-tap-set instance and the unfused blur_yz launch
    taps = [radius_taps(r, seed) for r, seed in zip(radii, (radii[0], 100 + radii[1], 100 + radii[2]))]
    run_case(K, name, vol(shape, sum(shape)), taps, m, noise, fused_ok)


def test_gaussian_taps_at_radius_8(K):
    """The generator's own taps (tables.gaussian_taps) at the largest radius the fused pair takes."""
    from fetalsyngen_amd import tables as T

    taps = [T.gaussian_taps(s) for s in (2.6, 2.1, 1.7)]
    assert [len(t) // 2 for t in taps] == [8, 7, 6]
    run_case(K, "gaussian R 8/7/6", vol((40, 36, 28), 3), taps, (17, 15, 12), PHILOX, True)


def test_dynamic_range_and_exact_zeros(K):
    """Values over twelve decades with both signs, a zero slab wider than the blur window and scattered zeros: the bound is
    relative to each output's own magnitude, zero-support outputs must be exactly 0, and with noise the clamped ones."""
    rs = np.random.RandomState(8)
    shape = (40, 28, 36)
    x = (10.0 ** rs.uniform(-6, 6, shape) * rs.choice([-1.0, 1.0], shape, p=[0.2, 0.8])).astype(np.float32)
    x[14:30] = 0  # 16 rows of zeros: outputs whose window lies inside are 0
    x[:, :, 8:20] = 0
    x[rs.rand(*shape) < 0.3] = 0
    taps = [radius_taps(r, r) for r in (3, 2, 4)]
    run_case(K, "dynamic range, zero slabs", x, taps, (20, 14, 17), None, True)
    run_case(K, "dynamic range, zero slabs, noise", x, taps, (20, 14, 17), ("pointer", 1e3), True)


def test_misaligned_and_strided_views(K):
    """A view that starts 4 bytes into its buffer is refused by the fused pair (the x launch reads 16-byte rows) and the
    unfused sequence computes it; a non-contiguous view is refused by the front-end."""
    shape, m = (20, 12, 16), (10, 6, 8)
    x = vol(shape, 5)
    flat = torch.empty(1 + x.size, device=DEV)
    xd = flat[1:].view(shape)
    xd.copy_(torch.from_numpy(x))
    assert xd.is_contiguous() and xd.data_ptr() % 16 == 4
    taps = [radius_taps(r, r) for r in (2, 3, 2)]
    run_case(K, "view x[1:] (4-byte offset)", x, taps, m, PHILOX, False, xd=xd)
    wide = torch.from_numpy(vol((20, 12, 20), 6)).to(DEV)
    rt = K.DeviceTables([down_table(m[a], shape[a]) for a in range(3)], DEV)
    with pytest.raises(ValueError):
        K.blur_resample(wide[:, :, :16], rt, taps)


def test_hand_made_tables_are_refused(K):
    """Tables the fused kernels cannot take (two outputs sharing a lower neighbour, lo not monotone, an outside output at
    the end, hi not next to lo): blur_resample says None, the unfused path matches the reference."""
    shape = (24, 20, 16)
    good = [down_table(12, 24), down_table(10, 20), down_table(8, 16)]
    w = lambda k: np.linspace(0.1, 0.9, k).astype(np.float32)  # noqa: E731
    from fetalsyngen_amd import tables as T

    def tab(lo, hi):
        k = len(lo)
        return T._pack(np.asarray(lo), np.asarray(hi), 1 - w(k), w(k))

    bad = {
        "shared lower neighbour (x)": (0, tab([1, 1, 5, 9, 12, 20], [2, 2, 6, 10, 13, 21])),
        "lo not monotone (y)": (1, tab([2, 6, 4, 10, 15], [3, 7, 5, 11, 16])),
        "outside at the end (z)": (2, tab([0, 4, 8, 12, -1], [1, 5, 9, 13, 0])),
        "hi two rows past lo (x)": (0, tab([0, 4, 8, 12], [2, 5, 9, 13])),
    }
    for name, (axis, t) in bad.items():
        tabs = list(good)
        tabs[axis] = t
        taps = [radius_taps(r, r) for r in (3, 2, 2)]
        run_case(K, f"table: {name}", vol(shape, 9), taps, None, None, False, tabs=tabs)
    run_case(K, "table: all plain", vol(shape, 9), [radius_taps(r, r) for r in (3, 2, 2)], None, None, True, tabs=good)


def test_x_row_offsets_do_not_wrap(K):
    """An input whose x-launch row offsets wrapped back into range before the bound: 2 x 248552 x 432 floats (859 MB), R = 8,
    the smallest n1 for which row -8 of chunk 0 lands at 2^32 - 8 rowb < 2 rowb, inside row 1 (with n0 = 2, the shortest axis
    0 the fused pair takes, about the smallest such input in bytes).  Row -8 was read instead of the zero padding for the
    first 2816 columns, and row 9 (9 rowb + colb past 2^32) for the last 2816: output errors up to 3.1 on values ~12.6.  It
    must be refused (or be right), by blur_resample and by the x launch itself; the unfused path must be right.  The input
    is constant, so the reference is the outer product of three 1-D operators."""
    import ctypes as C

    from fetalsyngen_amd import _lib

    n = (2, 248552, 432)
    m = (1, n[1] // 2, n[2] // 2)
    taps = [radius_taps(8, 1), radius_taps(1, 2), radius_taps(1, 3)]
    tabs = [down_table(m[a], n[a]) for a in range(3)]
    rt = K.DeviceTables(tabs, DEV)
    xd = torch.full(n, 100.0, device=DEV)
    ax = [blur_resample64(np.ones((n[a], 1, 1)), [taps[a], None, None], [tabs[a], None, None])[:, 0, 0] for a in range(3)]
    want = 100.0 * np.einsum("i,j,k->ijk", *ax)
    tol = 1.01 * 2.0 ** -24 * (17 + 3 + 3 + 6) * want  # util_resample64.error_bound for a positive constant input

    def within(got, name):
        err = np.abs(got.cpu().numpy() - want)
        assert (err <= tol).all(), f"{name}: max error {float(err.max()):.3g} at {np.unravel_index(err.argmax(), err.shape)}"
        return float(err.max())

    poison(m, (1, n[1], n[2]))
    f = K.blur_resample(xd, rt, taps)
    if f is not None:
        within(f, "fused pair")
    mid = torch.full((m[0], n[1], n[2]), float("nan"), device=DEV)
    rc = _lib.load().fsg_blur_resample_x_f32(C.c_void_p(xd.data_ptr()), *n, rt.ptrs[0], m[0],
                                               taps[0].ctypes.data_as(C.POINTER(C.c_float)), len(taps[0]),
                                               C.c_void_p(mid.data_ptr()), C.c_void_p(0))
    torch.cuda.synchronize()
    if rc == 0:  # launched: axis 0 of the constant
        c0 = 100.0 * ax[0][0]
        err = float((mid.double() - c0).abs().max())
        assert err <= 1.01 * 2.0 ** -24 * 19 * c0, f"x launch with wrapped row offsets: max error {err:.3g}"
    else:
        assert rc == _lib.E_TOOBIG, rc
    del mid
    eu = within(unfused(K, xd, taps, rt), "unfused")
    print(f"EDGE x row offsets n={n} m={m} R=(8, 1, 1) fused {'refused' if f is None else 'ran'}, x launch rc {rc}, "
          f"unfused {eu:.3e}")
