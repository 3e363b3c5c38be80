"""GPU: the deterministic slice-acquisition adjoint (fsg_slice_acq_adjoint_det_f32; the rule is in include/fsg_hip.h).

What is pinned: the same call gives the same bits; so does any LDS tuning, the direct kernel, any order of the slices and
`slice_ids` against gathered slices; the result equals the numpy restatement tests/util_fixed64.py bit for bit where the
slices are aligned with the volume axes; it lies within the float path's own tolerances of the float64 oracle; value_scale
is exact; refusals leave the outputs untouched; the float entry is what it was.
Shapes are those of test_sr_parity.py::test_adjoint_lds_presum_matches_direct_atomics unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import fsg_oracle_sr as S
from tests import util_fixed64 as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TUNINGS = [(4096, 0, 20), (4096, 3, 20), (8192, 6, 20), (512, 1, 0), (2048, 2, 0), (16384, 64, 1000)]
N, SS, VS, RES = 12, 96, (72, 80, 88), 1.4


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (and libfsg_hip.so); there is no fallback to skip to")
    from fetalsyngen_amd import kernels

    return kernels


@pytest.fixture(scope="module")
def lib():
    from fetalsyngen_amd import _lib

    return _lib.load()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(x):
    return x.detach().cpu().numpy()


def _random_rigid(rng, n, max_rot, max_t):
    ax = np.concatenate([rng.uniform(-max_rot, max_rot, (n, 3)), rng.uniform(-max_t, max_t, (n, 3))], 1).astype(np.float32)
    return S.axisangle2mat(torch.from_numpy(ax)).numpy()


@pytest.fixture(scope="module")
def case():
    """The inputs of the existing LDS-against-direct test (read only)."""
    rng = np.random.default_rng(11)
    psf = dev(S.get_psf(res_ratio=(1.4, 1.4, 5.0)).numpy())
    tr = _random_rigid(rng, N, 1.2, 12.0)
    tr[:, 2, 3] += np.linspace(-20, 20, N, dtype=np.float32)
    g = torch.Generator(device=DEV).manual_seed(5)
    s = torch.rand((N, SS, SS), device=DEV, generator=g) - 0.25
    sm = torch.rand((N, SS, SS), device=DEV, generator=g) > 0.1
    vm = torch.rand(VS, device=DEV, generator=g) > 0.1
    return {"tr": dev(tr), "psf": psf, "s": s, "sm": sm, "vm": vm}


def det(K, c, masks=False, vs=VS, res=RES, **kw):
    kw.setdefault("interp_psf", True)
    kw.setdefault("return_weight", True)
    return K.slice_acq_adjoint(kw.pop("tr", c["tr"]), kw.pop("psf", c["psf"]), kw.pop("s", c["s"]), c["sm"] if masks else None,
                               c["vm"] if masks else None, vs, res, deterministic=True, **kw)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


class tuned:
    """`with tuned(lib, direct=True)` / `with tuned(lib, tuning=(cap, zc, t16))`: restored on exit."""

    def __init__(self, lib, tuning=None, direct=False):
        self.lib, self.tuning, self.direct = lib, tuning, direct

    def __enter__(self):
        from fetalsyngen_amd import _lib

        if self.direct:
            self.prev = self.lib.fsg_set_tuning(_lib.TUNE.SA_DIRECT)
        if self.tuning:
            assert self.lib.fsg_slice_acq_set_tuning(*self.tuning) == 0

    def __exit__(self, *exc):
        if self.direct:
            self.lib.fsg_set_tuning(self.prev)
        self.lib.fsg_slice_acq_set_tuning(3072, 0, 20)


@pytest.mark.parametrize("masks", [False, True])
def test_same_call_twice_same_bits(K, case, masks):
    a, b = det(K, case, masks), det(K, case, masks)
    assert float(a[1].sum()) > 1000 and same(a, b)
    with torch.cuda.stream(torch.cuda.Stream()):
        c = det(K, case, masks)
        torch.cuda.current_stream().synchronize()
    assert same(a, c)
    for eq in (False, True):  # interp_psf=False: the direct kernel is its only kernel
        assert same(det(K, case, masks, interp_psf=False, equalize=eq), det(K, case, masks, interp_psf=False, equalize=eq))


@pytest.mark.parametrize("masks", [False, True])
def test_bits_do_not_depend_on_tuning_or_kernel(K, lib, case, masks):
    """Both tile sizes, the LDS path, the per-chunk fallback (512 cells) and the direct kernel."""
    ref = det(K, case, masks)
    with tuned(lib, direct=True):
        assert same(ref, det(K, case, masks)), "direct kernel"
    for t in TUNINGS:
        with tuned(lib, tuning=t):
            assert same(ref, det(K, case, masks)), t


def test_bits_do_not_depend_on_slice_order_or_on_slice_ids(K, case):
    ref = det(K, case)
    p = torch.from_numpy(np.random.default_rng(2).permutation(N))
    pd_ = p.to(DEV)
    assert same(ref, det(K, case, tr=case["tr"][pd_].contiguous(), s=case["s"][pd_].contiguous()))
    keep = p[:7]
    kd = keep.to(DEV)
    gathered = det(K, case, tr=case["tr"][kd].contiguous(), s=case["s"][kd].contiguous(), equalize=True)
    in_place = det(K, case, tr=case["tr"][kd].contiguous(), slice_ids=keep, equalize=True)
    assert same(gathered, in_place) and not same(gathered, ref)


@pytest.mark.parametrize("interp_psf", [False, True])
@pytest.mark.parametrize("mk", ["nomask", "masks"])
@pytest.mark.parametrize("pk", ["aniso", "iso"])
def test_accuracy_against_the_float64_oracle(K, golden, interp_psf, mk, pk):
    """The tolerances of test_sr_parity.py::test_cuda_semantics_vs_oracle, on its case."""
    g = golden("slice_acq")
    vs, ss, res = (20, 24, 28), (14, 18), 1.3
    vm = g["vol_mask"] if mk == "masks" else None
    sm = g["slices_mask"] if mk == "masks" else None
    tr, psf = g["transforms"], g[f"psf_{pk}"]
    es, _ = S.slice_acq_forward_cuda(tr, g["vol"], vm, sm, psf, ss, res, True, interp_psf)
    for eq in (False, True):
        ev, evw = S.slice_acq_adjoint_cuda(tr, psf, es, sm, vm, vs, res, interp_psf, eq)
        err = {}
        for name, d in (("deterministic", True), ("float", False)):
            v, vw = K.slice_acq_adjoint(dev(tr), dev(psf), dev(es), dev(sm), dev(vm), vs, res, interp_psf=interp_psf,
                                        equalize=eq, return_weight=True, deterministic=d)
            err[name] = (float(np.abs(host(v) - ev).max()), float(np.abs(host(vw) - evw).max()))
            if d:
                got = (host(v), host(vw))
        print(f"oracle interp_psf={interp_psf} {mk} {pk} eq={eq}: max |value err|, |weight err| "
              f"deterministic {err['deterministic'][0]:.3e} {err['deterministic'][1]:.3e}  "
              f"float {err['float'][0]:.3e} {err['float'][1]:.3e}")
        np.testing.assert_allclose(got[1], evw, rtol=0, atol=2e-5)
        np.testing.assert_allclose(got[0], ev, rtol=0, atol=5e-4)


def _aligned(rng, n, tmax, zmax):
    tr = np.zeros((n, 3, 4), np.float32)
    tr[:, :, :3] = np.eye(3, dtype=np.float32)
    tr[:, 0, 3], tr[:, 1, 3] = rng.integers(-tmax, tmax + 1, n), rng.integers(-tmax, tmax + 1, n)
    tr[:, 2, 3] = rng.integers(-zmax, zmax + 1, n)
    return tr


@pytest.mark.parametrize("which", ["arbitrary_psf", "ties"])
def test_bit_for_bit_against_the_numpy_restatement(K, lib, which):
    """Axis-aligned slices (identity rotation, integer shifts, pitch 1): every fp32 operation of the kernel is restated in
    numpy, so value and weight must agree in every bit -- the quantiser, the tie rule, the fixed-point pixel weight and the
    single rounding back.  Even and odd volume extents: voxel positions on the grid and on half-integers (rounding ties)."""
    rng = np.random.default_rng(21)
    n, h, w, vs = 7, 21, 18, (16, 23, 22)
    tr = _aligned(rng, n, 3, 7)
    tr[0, :, 3] = (0, 0, 20)  # wholly outside
    if which == "arbitrary_psf":
        psf = rng.uniform(0.05, 1.0, (2, 3, 4)).astype(np.float32)
        s = rng.standard_normal((n, h, w)).astype(np.float32)
    else:
        # eight ones: on an odd-sized grid every pixel has weight exactly 1 and drops its own value on one voxel, so the
        # contributions are the slice values themselves: (k + 1/2) quanta, ties of both signs, on top of ordinary values
        psf, vs, h, w = np.ones((2, 2, 2), np.float32), (15, 23, 21), 21, 17
        tr[:, 2, 3] = rng.integers(-2, 3, n)  # several slices per plane: sums of many ties
        k = rng.integers(-40, 40, (n, h, w))
        s = ((k + 0.5) * 2.0 ** -X.F).astype(np.float32)
        s[::2] += rng.standard_normal((len(s[::2]), h, w)).astype(np.float32).round(2)
    sm = rng.uniform(size=(n, h, w)) > 0.1
    vm = rng.uniform(size=vs) > 0.1
    for masks in ((None, None), (sm, vm)):
        want_v, want_w = X.adjoint_nearest_psf(tr, psf, s, vs, 1.0, slices_mask=masks[0], vol_mask=masks[1])
        assert want_w.sum() > 500 and (want_v < 0).any() and (want_v > 0).any()
        for ctx in (tuned(lib), tuned(lib, direct=True), tuned(lib, tuning=(512, 1, 0))):
            with ctx:
                v, vw = K.slice_acq_adjoint(dev(tr), dev(psf), dev(s), dev(masks[0]), dev(masks[1]), vs, 1.0, interp_psf=True,
                                            return_weight=True, deterministic=True)
            assert np.array_equal(host(vw), want_w), f"weight: {np.abs(host(vw) - want_w).max()}"
            assert np.array_equal(host(v), want_v), f"value: {np.abs(host(v) - want_v).max()}"
            assert not np.signbit(host(v)[want_w == 0]).any()  # untouched accumulators are +0


@pytest.mark.parametrize("vs", [(9, 23, 19), (10, 24, 20)], ids=["odd", "even"])
def test_float_lds_kernel_is_the_fixed_point_kernel_where_order_cannot_matter(K, lib, vs):
    """The float and the fixed-point LDS adjoint are one kernel body with two accumulators, so where no sum has more than
    one term they must agree in every bit.  Axis-aligned slices at a pitch of 4 voxels (wider than the 3 x 3 PSF), 3 voxels
    apart in z (more than its 2 planes): no two (pixel, tap) pairs land on one voxel, which the single-pixel adjoints of the
    numpy restatement confirm below.  PSF and slice values are multiples of 1/16, so the pixel weight is the same number
    summed in fp32 in any order and in 2^-32 integers; a lone contribution fl32(pv / wsum * s) is far above 2^-48 and
    passes the 2^-72 quantiser and the single rounding back unchanged.  Odd extents put the voxels on the grid, even ones
    on rounding ties."""
    rng = np.random.default_rng(41)
    n, h, w, res = 3, 5, 4, 4.0
    tr = _aligned(rng, n, 1, 0)
    tr[:, 2, 3] = (-3, 0, 3)
    psf = (rng.integers(4, 17, (2, 3, 3)) / 16.0).astype(np.float32)
    s = (rng.integers(1, 33, (n, h, w)) * rng.choice([-1, 1], (n, h, w)) / 16.0).astype(np.float32)
    sm = rng.uniform(size=(n, h, w)) > 0.1
    vm = rng.uniform(size=vs) > 0.1
    # CPU: every voxel receives at most one contribution -- the supports of the single-pixel adjoints are disjoint
    hits = np.zeros(vs, np.int64)
    for z in range(n):
        for p in range(h * w):
            one = np.zeros((1, h, w), bool)
            one.reshape(-1)[p] = True
            hits += X.adjoint_nearest_psf(tr[z:z + 1], psf, s[z:z + 1], vs, res, slices_mask=one)[1] != 0
    assert hits.max() == 1
    for masks in ((None, None), (sm, vm)):
        want_v, want_w = X.adjoint_nearest_psf(tr, psf, s, vs, res, slices_mask=masks[0], vol_mask=masks[1])
        assert np.count_nonzero(want_w) > 50
        if masks[0] is None:
            assert np.array_equal(want_w != 0, hits == 1)
        args = (dev(tr), dev(psf), dev(s), dev(masks[0]), dev(masks[1]), vs, res)
        for ctx in (tuned(lib), tuned(lib, tuning=(512, 1, 0)), tuned(lib, tuning=(16384, 64, 1000))):
            with ctx:
                f = K.slice_acq_adjoint(*args, interp_psf=True, return_weight=True)
                d = K.slice_acq_adjoint(*args, interp_psf=True, return_weight=True, deterministic=True)
            assert torch.equal(f[1], d[1]), f"weight: {float((f[1] - d[1]).abs().max())}"
            assert torch.equal(f[0], d[0]), f"value: {float((f[0] - d[0]).abs().max())}"
            assert np.array_equal(host(d[1]), want_w) and np.array_equal(host(d[0]), want_v)
            assert np.array_equal(host(f[1]), want_w) and np.array_equal(host(f[0]), want_v)


def test_value_scale_is_exact_and_bad_scales_are_refused_untouched(K, lib, case):
    a = det(K, case)
    b = det(K, case, s=case["s"] * 1024, value_scale=1024.0)
    assert torch.equal(b[0], a[0] * 1024) and torch.equal(b[1], a[1])
    c = det(K, case, s=case["s"] / 64, value_scale=2.0 ** -6)
    assert torch.equal(c[0] * 64, a[0]) and torch.equal(c[1], a[1])
    # the entry point itself: refusals come before the first write
    D, H, W = VS
    vol = torch.full(VS, 7.0, device=DEV)
    wgt = torch.full(VS, 7.0, device=DEV)
    ws = torch.full((4 * D * H * W,), 7, dtype=torch.int64, device=DEV)
    assert lib.fsg_slice_acq_adjoint_det_ws_bytes(D, H, W, 1) == ws.numel() * 8 == 2 * lib.fsg_slice_acq_adjoint_det_ws_bytes(D, H, W, 0)

    def call(scale, mode=1, ws_bytes=ws.numel() * 8, ws_ptr=ws.data_ptr()):
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        return lib.fsg_slice_acq_adjoint_det_f32(p(case["tr"]), p(case["psf"]), *case["psf"].shape, p(case["s"]), None, None,
                                                 None, p(vol), p(wgt), D, H, W, N, SS, SS, RES, mode, C.c_void_p(ws_ptr),
                                                 ws_bytes, scale, None)

    for scale in (3.0, 2.0 ** 21, 2.0 ** -21, 0.0, -2.0, float("nan"), float("inf")):
        assert call(scale) == -1, scale
    assert call(1.0, mode=2) == -1                              # FSG_SA_TORCH
    assert call(1.0, ws_bytes=ws.numel() * 8 - 8) == -1         # workspace too small
    assert call(1.0, ws_ptr=ws.data_ptr() + 4) == -3            # FSG_E_ALIGN
    torch.cuda.synchronize()
    assert bool((vol == 7).all()) and bool((wgt == 7).all()) and bool((ws == 7).all())
    with pytest.raises(ValueError):
        det(K, case, value_scale=3.0)
    with pytest.raises(ValueError):
        det(K, case, semantics="torch")
    assert call(1.0) == 0 and torch.equal(vol, a[0]) and torch.equal(wgt, a[1])  # and the same buffers, accepted


def _edge(K, lib, tr, psf, s, vs, res, interp_psf=True, min_weight=1.0):
    """An edge case holds when: twice the same bits, the same bits from the direct kernel and a tiny LDS capacity, the value
    volume the same with and without the weight volume, and the float path within its own order noise of it."""
    args = (dev(tr), dev(psf), dev(s), None, None, vs, res)
    a = K.slice_acq_adjoint(*args, interp_psf=interp_psf, return_weight=True, deterministic=True)
    assert same(a, K.slice_acq_adjoint(*args, interp_psf=interp_psf, return_weight=True, deterministic=True))
    for ctx in (tuned(lib, direct=True), tuned(lib, tuning=(256, 1, 0)), tuned(lib, tuning=(18432, 64, 1000))):
        with ctx:
            assert same(a, K.slice_acq_adjoint(*args, interp_psf=interp_psf, return_weight=True, deterministic=True))
    assert torch.equal(a[0], K.slice_acq_adjoint(*args, interp_psf=interp_psf, deterministic=True))  # vol_weight not requested
    f = K.slice_acq_adjoint(*args, interp_psf=interp_psf, return_weight=True)
    np.testing.assert_allclose(host(a[1]), host(f[1]), rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(host(a[0]), host(f[0]), rtol=1e-5, atol=2e-5)
    assert float(a[1].sum()) >= min_weight
    return a


def test_edges(K, lib):
    rng = np.random.default_rng(31)
    vs = (40, 44, 48)
    psf = S.get_psf(res_ratio=(1.4, 1.4, 5.0)).numpy()
    tr = _random_rigid(rng, 5, 1.0, 6.0)
    s = rng.uniform(-0.5, 1.0, (5, 37, 29)).astype(np.float32)
    _edge(K, lib, tr, psf, s, vs, 1.4, min_weight=500)                    # 37 x 29: no multiple of either tile
    _edge(K, lib, tr, psf, s, vs, 1.4, interp_psf=False, min_weight=500)
    _edge(K, lib, tr[:1], psf, s[:1], vs, 1.4, min_weight=100)            # a single slice
    out = tr.copy()
    out[:, :, 3] += np.array([[0, 0, 30], [25, 0, 0], [0, 0, 300], [0, -28, 0], [0, 0, -21]], np.float32)
    a = _edge(K, lib, out, psf, s, vs, 1.4, min_weight=50)                # partly and (slice 2) wholly outside the volume
    b = _edge(K, lib, np.delete(out, 2, 0), psf, np.delete(s, 2, 0), vs, 1.4, min_weight=50)
    assert same(a, b)
    far = _edge(K, lib, out[2:3], psf, s[2:3], vs, 1.4, min_weight=0.0)   # nothing reaches the volume: every voxel is +0
    assert not far[0].any() and not far[1].any() and not torch.signbit(far[0]).any()
    odd = rng.uniform(0.05, 1.0, (2, 2, 3)).astype(np.float32)            # LDS prefix of an odd number of floats
    assert (odd.size + 3 * sum(odd.shape) + 256) % 2 == 1
    _edge(K, lib, tr, odd, s, vs, 1.0, min_weight=500)
    flat = rng.uniform(0.05, 1.0, (1, 5, 5)).astype(np.float32)           # pd = 1
    _edge(K, lib, tr, flat, s, vs, 1.4, interp_psf=False, min_weight=500)
    z = _edge(K, lib, tr, flat, s, vs, 1.4, min_weight=0.0)               # (re-interpolation needs two planes: nothing lands)
    assert not z[1].any()


def test_float_path_is_the_float_entry(K, lib, case):
    """deterministic=False is fsg_slice_acq_adjoint_f32 as before: within the tolerance between two float runs."""
    D, H, W = VS
    vol, wgt = torch.empty(VS, device=DEV), torch.empty(VS, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.fsg_slice_acq_adjoint_f32(p(case["tr"]), p(case["psf"]), *case["psf"].shape, p(case["s"]), p(case["sm"]), None,
                                       p(case["vm"]), p(vol), p(wgt), D, H, W, N, SS, SS, RES, 1, None)
    assert rc == 0
    torch.cuda.synchronize()
    for kw in ({}, {"deterministic": False}):
        v, vw = K.slice_acq_adjoint(case["tr"], case["psf"], case["s"], case["sm"], case["vm"], VS, RES, interp_psf=True,
                                    return_weight=True, **kw)
        np.testing.assert_allclose(host(vw), host(wgt), rtol=1e-5, atol=2e-5)
        np.testing.assert_allclose(host(v), host(vol), rtol=1e-5, atol=2e-5)
    d = det(K, case, masks=True)
    np.testing.assert_allclose(host(d[1]), host(wgt), rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(host(d[0]), host(vol), rtol=1e-5, atol=2e-5)
