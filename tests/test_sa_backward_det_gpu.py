"""GPU: the deterministic grad_vol of the slice-acquisition backward (fsg_slice_acq_backward_det_f32; the rule is in
include/fsg_hip.h and DESIGN.md section 20): bit-identical from run to run, across streams, slice orders and with or without
grad_transforms; bit for bit the CPU restatement tests/util_sa_backward_fixed64.py on the exact-geometry cases; within the
float backward's bound plus the quantisation term of the float64 restatement; and the autograd path on top of it.

Tolerances (none is derived from what the kernel gives):
  exact-geometry cases   per element (K + 16) * 2^-24 * S + K * 2^-73 * grad_scale: the bound of tests/test_sa_backward_gpu.py
                         plus half a quantum for each of the K contributions.
  general rotations      4 * E_cpu * max|float64| with the E_CPU of tests/test_sa_backward_gpu.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util_sa_backward_cases as CS
from tests import util_sa_backward_fixed64 as FX
from tests.test_sa_backward_gpu import E_CPU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
SENTINEL = -77.25
NVOX = int(np.prod(CS.VS))
MODES = pytest.mark.parametrize("interp_psf", [False, True], ids=["linear", "nearest_psf"])
MASKS = pytest.mark.parametrize("masks", [False, True], ids=["nomask", "masks"])


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (and libfsg_hip.so); there is no fallback to skip to")
    from fetalsyngen_amd import kernels

    return kernels


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (and libfsg_hip.so); there is no fallback to skip to")
    from fetalsyngen_amd import _lib

    return _lib


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(K, case, interp_psf, deterministic=True, **kw):
    return K.slice_acq_backward(dev(case["tr"]), dev(case["vol"]), dev(case["vm"]), dev(case["sm"]), dev(case["psf"]),
                                dev(case["g"]), case["res"], interp_psf=interp_psf, deterministic=deterministic, **kw)


_REF = {}


def ref(name, masks, interp_psf):
    """An exact-geometry case, its float64 restatement and its fixed-point one, computed once and shared (read only)."""
    key = (name, masks, interp_psf)
    if key not in _REF:
        case = CS.exact_case(name, masks)
        _REF[key] = (case, CS.reference(case, interp_psf), FX.of_case(case, interp_psf))
    return _REF[key]


def bound(r, grad_scale=1.0):
    return (r["k_vol"] + 16) * U * r["s_vol"] + r["k_vol"] * 2.0 ** -73 * grad_scale


def bits_equal(gv, want):
    """bit for bit, the sign of zero included"""
    return np.array_equal(gv.cpu().numpy().view(np.int32), np.asarray(want, np.float32).view(np.int32))


# ---- the same bits whatever the run, the stream, the slice order, the other output ------------------------------------------
@MASKS
@MODES
def test_run_to_run_and_on_a_side_stream(K, interp_psf, masks):
    case, _, fx = ref("psf335", masks, interp_psf)
    assert fx["k_vol"].max() >= 8  # voxels really receive many contributions, from several slices
    a, _ = run(K, case, interp_psf)
    b, _ = run(K, case, interp_psf)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c, _ = run(K, case, interp_psf)
    side.synchronize()
    assert bool(a.abs().max() > 0) and torch.equal(a, b) and torch.equal(a, c)


@MODES
def test_any_order_of_the_slices(K, interp_psf):
    case, _, fx = ref("psf335", True, interp_psf)
    a, _ = run(K, case, interp_psf)
    for seed in (0, 1):
        p = np.random.default_rng(seed).permutation(CS.N)
        b, _ = run(K, dict(case, tr=case["tr"][p], g=case["g"][p], sm=case["sm"][p]), interp_psf)
        assert torch.equal(a, b)
    assert bits_equal(a, fx["grad_vol"])


@MODES
def test_with_and_without_grad_transforms(K, interp_psf):
    case, _, _ = ref("psf223_big", True, interp_psf)
    gv, gt = run(K, case, interp_psf)
    gv2, none = run(K, case, interp_psf, need_transforms_grad=False)
    none2, gt2 = run(K, case, interp_psf, need_vol_grad=False)
    _, gt_float = run(K, case, interp_psf, deterministic=False)
    assert none is None and none2 is None and bool(gt.abs().max() > 0)
    assert torch.equal(gv, gv2)
    assert torch.equal(gt, gt_float) and torch.equal(gt2, gt_float)  # grad_transforms has the float entry's bits


# ---- against the restatements ------------------------------------------------------------------------------------------------
WORST = {"exact": 0.0, "float_vs_fixed": 0.0}


@MASKS
@MODES
@pytest.mark.parametrize("name", list(CS.EXACT))
def test_exact_geometry_bit_for_bit_and_within_the_bound(K, name, interp_psf, masks):
    case, r, fx = ref(name, masks, interp_psf)
    gv, gt = run(K, case, interp_psf)
    assert tuple(gv.shape) == CS.VS and gv.dtype == torch.float32
    assert bits_equal(gv, fx["grad_vol"])
    got = gv.cpu().numpy().astype(np.float64)
    b = bound(r)
    err = np.abs(got - r["grad_vol"])
    gf, gtf = run(K, case, interp_psf, deterministic=False)
    dif = np.abs(got - gf.cpu().numpy().astype(np.float64))
    WORST["exact"] = max(WORST["exact"], float((err / np.maximum(b, 1e-300)).max()))
    WORST["float_vs_fixed"] = max(WORST["float_vs_fixed"], float((dif / np.maximum(b, 1e-300)).max()))
    print("worst error/bound so far: against float64 %.4f, float against fixed point %.4f" % (WORST["exact"], WORST["float_vs_fixed"]))
    assert np.all(err <= b)
    assert np.all(dif <= b)  # float and fixed point agree within the same bound
    assert torch.equal(gt, gtf)
    empty = interp_psf and case["psf"].shape[0] == 1  # pd = 1: NEAREST_PSF accepts no PSF coordinate and gives zeros
    assert bool(np.any(got != 0)) != empty


@MODES
def test_small_gradients_stay_within_the_bound_of_their_own_size(K, interp_psf):
    """grad_slices 2^-30 times smaller under grad_scale 1: the contributions are near 2^-32, where the high limb alone holds a
    few bits of each.  The bound shrinks with them (S scales, the quantisation term does not), so an accumulator that kept
    the high limb only is caught here without the fixed-point restatement: this case needs the float64 one alone."""
    case, r, _ = ref("psf335", True, interp_psf)
    s = 2.0 ** -30
    small = dict(r, grad_vol=r["grad_vol"] * s, s_vol=r["s_vol"] * s)  # float64 scales exactly
    gv, _ = run(K, dict(case, g=case["g"] * np.float32(s)), interp_psf)
    err = np.abs(gv.cpu().numpy().astype(np.float64) - small["grad_vol"])
    b = bound(small)
    print("small gradients: worst error/bound %.4f" % float((err / np.maximum(b, 1e-300)).max()))
    assert np.abs(small["grad_vol"]).max() < 2.0 ** -20 and np.all(err <= b)


def _tie_case():
    """Two slices on the same plane, a 1x1x1 PSF, pixel centres on half-integers along z and on half-integers or integers
    along x and y: every corner weight is 1, 1/2, 1/4 or 1/8, the pixel weight is 1, and the gradients are odd multiples of
    2^-70, so an eighth of one is an odd multiple of half a quantum: a tie, which goes to the even neighbour."""
    case = CS.exact_case("delta", False, n=2)
    case["tr"][:, :, :3] = np.eye(3)
    case["tr"][:, :, 3] = 0
    case["psf"][:] = 1
    rng = np.random.default_rng(72)
    case["g"] = ((2 * rng.integers(-8, 8, case["g"].shape) + 1) * 2.0 ** -70).astype(np.float32)
    return case


def test_ties_of_half_a_quantum_go_to_even(K):
    case = _tie_case()
    idx, c = FX.contributions(case["tr"], CS.VS, None, case["psf"], case["g"], None, case["res"], False)
    d = c.astype(np.float64) * 2.0 ** 72
    assert (np.abs(d - np.floor(d)) == 0.5).sum() > 50  # the case is what it says
    fx = FX.of_case(case, False)
    exact = np.zeros(NVOX)
    np.add.at(exact, idx, c.astype(np.float64))  # (sums of a few multiples of 2^-73: exact in float64)
    assert np.any(exact.astype(np.float32) != fx["grad_vol"].reshape(-1))  # and rounding each contribution is seen in the result
    gv, _ = run(K, case, False)
    assert bits_equal(gv, fx["grad_vol"])


@MODES
def test_general_rotations_within_four_times_the_fp32_cost_of_the_formula(K, interp_psf):
    worst = 0.0
    for name in CS.GENERAL:
        case = CS.general_case(name, interp_psf)
        r = CS.reference(case, interp_psf)
        assert min(r["dist"].values()) > 1e-3 and case["sm"].sum() > 200
        gv, gt = run(K, case, interp_psf)
        _, gtf = run(K, case, interp_psf, deterministic=False)
        assert torch.equal(gt, gtf)
        e = np.abs(gv.cpu().numpy().astype(np.float64) - r["grad_vol"]).max() / np.abs(r["grad_vol"]).max()
        print(f"{name} grad_vol: fixed point {e:.3e} of max|float64| (allowed {4 * E_CPU[interp_psf, 'grad_vol']:.3e})")
        worst = max(worst, e)
    assert worst <= 4 * E_CPU[interp_psf, "grad_vol"]


# ---- the entry point itself: edges and refusals ------------------------------------------------------------------------------
def _raw(L, case, interp_psf, gv, gt, ws=None, ws_bytes=None, det=None, det_bytes=None, scale=1.0, mode=None):
    """-> rc, ws, det_ws (the two workspaces as float32 / int64 tensors full of sentinels unless given)"""
    lib = L.load()
    n, h, w = case["g"].shape
    pd, ph, pw = case["psf"].shape
    t = {k: dev(case[k]) for k in ("tr", "vol", "vm", "psf", "g", "sm")}
    p = lambda x: C.c_void_p(0 if x is None else (x if isinstance(x, int) else x.data_ptr()))  # noqa: E731
    if ws is None:
        ws = torch.full((lib.fsg_slice_acq_backward_ws_bytes(n, h, w) // 4,), SENTINEL, device=DEV)
    if ws_bytes is None:
        ws_bytes = ws.numel() * 4 if isinstance(ws, torch.Tensor) else 0
    if det is None:
        det = torch.full((lib.fsg_slice_acq_backward_det_ws_bytes(*CS.VS) // 8,), -77, dtype=torch.int64, device=DEV)
    if det_bytes is None:
        det_bytes = det.numel() * 8 if isinstance(det, torch.Tensor) else 0
    if mode is None:
        mode = L.SA.NEAREST_PSF if interp_psf else L.SA.LINEAR
    rc = lib.fsg_slice_acq_backward_det_f32(p(t["tr"]), p(t["vol"]), p(t["vm"]), p(t["psf"]), pd, ph, pw, p(t["g"]), p(t["sm"]),
                                            p(gv), p(gt), *CS.VS, n, h, w, float(case["res"]), mode, p(ws), ws_bytes, p(det),
                                            det_bytes, scale, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return rc, ws, det


def _sentinels(n):
    return torch.full(CS.VS, SENTINEL, device=DEV), torch.full((n, 12), SENTINEL, device=DEV)


def _face_case(distance):
    """six slices, one pushed `distance` voxels towards each face of the volume along its own normal or in its plane"""
    case = CS.exact_case("psf223", False, n=6)
    case["tr"][:, :, :3] = np.eye(3)
    case["tr"][:, :, 3] = 0
    for i in range(6):
        case["tr"][i, i % 3, 3] = distance * (1 if i < 3 else -1)
    return case


def _all_plus_zero(gv):
    return bool((gv.view(torch.int32) == 0).all())  # +0.0f has no bit set: the sign bit is checked too


@MODES
def test_slices_wholly_outside_every_face_write_plus_zero(L, interp_psf):
    gv, gt = _sentinels(6)
    rc, _, _ = _raw(L, _face_case(64.0), interp_psf, gv, gt)
    assert rc == 0 and _all_plus_zero(gv) and bool((gt == 0).all())


@MODES
def test_slices_partly_outside_every_face(L, interp_psf):
    case = _face_case(9.25)
    r, fx = CS.reference(case, interp_psf), FX.of_case(case, interp_psf)
    assert np.count_nonzero(fx["grad_vol"]) > 100
    gv, gt = _sentinels(6)
    rc, _, _ = _raw(L, case, interp_psf, gv, gt)
    assert rc == 0 and bits_equal(gv, fx["grad_vol"])
    assert np.all(np.abs(gv.cpu().numpy().astype(np.float64) - r["grad_vol"]) <= bound(r))


@pytest.mark.parametrize("what", ["zero_grad", "mask_all_false", "one_slice", "one_plane_psf"])
def test_degenerate_inputs(L, what):
    case = CS.exact_case("psf133" if what == "one_plane_psf" else "psf223", what == "mask_all_false",
                         n=1 if what == "one_slice" else CS.N)
    if what == "zero_grad":
        case["g"][:] = 0
    elif what == "mask_all_false":
        case["sm"][:] = False
    n = case["g"].shape[0]
    for interp_psf in (False, True):
        gv, gt = _sentinels(n)
        rc, _, _ = _raw(L, case, interp_psf, gv, gt)
        assert rc == 0
        if what == "one_slice" or (what == "one_plane_psf" and not interp_psf):
            fx = FX.of_case(case, interp_psf)
            assert np.count_nonzero(fx["grad_vol"]) > 100 and bits_equal(gv, fx["grad_vol"])
        else:
            assert _all_plus_zero(gv)


def test_grad_vol_not_requested_needs_no_fixed_point_workspace(L, K):
    case, _, _ = ref("psf223", True, False)
    _, gt = _sentinels(CS.N)
    rc, _, _ = _raw(L, case, False, None, gt, det=0, det_bytes=0)
    assert rc == 0 and torch.equal(gt.reshape(CS.N, 3, 4), run(K, case, False, deterministic=False)[1])
    # and grad_vol alone needs no workspace for the transform sums
    gv, _ = _sentinels(CS.N)
    rc, _, det = _raw(L, case, False, gv, None, ws=0, ws_bytes=0)
    assert rc == 0 and bits_equal(gv, ref("psf223", True, False)[2]["grad_vol"])


@MODES
@pytest.mark.parametrize("k", [-20, 0, 20])
def test_grad_scale_is_exact(K, interp_psf, k):
    case, _, fx = ref("psf223", True, interp_psf)
    s = np.float32(2.0 ** k)
    gv, _ = run(K, dict(case, g=case["g"] * s), interp_psf, grad_scale=2.0 ** k)
    assert np.count_nonzero(fx["grad_vol"]) > 100 and bits_equal(gv, fx["grad_vol"] * s)


def test_refusals_leave_outputs_and_both_workspaces_untouched(L):
    case = CS.exact_case("psf223", True)
    lib = L.load()
    need, dneed = lib.fsg_slice_acq_backward_ws_bytes(*case["g"].shape), lib.fsg_slice_acq_backward_det_ws_bytes(*CS.VS)
    assert dneed == 16 * NVOX
    odd = torch.full((dneed // 8 + 1,), -77, dtype=torch.int64, device=DEV)
    oddf = torch.full((need // 4 + 1,), SENTINEL, device=DEV)
    big = dict(case, psf=np.ones((17, 17, 17), np.float32))
    for label, want, kw in (
        ("both outputs NULL", L.E_BADARG, dict(null=True)),
        ("FSG_SA_TORCH", L.E_BADARG, dict(mode=L.SA.TORCH)),
        ("grad_scale 3", L.E_BADARG, dict(scale=3.0)),
        ("grad_scale 2^21", L.E_BADARG, dict(scale=2.0 ** 21)),
        ("grad_scale 2^-21", L.E_BADARG, dict(scale=2.0 ** -21)),
        ("grad_scale 0", L.E_BADARG, dict(scale=0.0)),
        ("grad_scale nan", L.E_BADARG, dict(scale=float("nan"))),
        ("short det_ws", L.E_BADARG, dict(det_bytes=dneed - 8)),
        ("no det_ws", L.E_BADARG, dict(det=0, det_bytes=dneed)),
        ("misaligned det_ws", L.E_ALIGN, dict(det=odd.data_ptr() + 4, det_bytes=dneed)),
        ("short ws", L.E_BADARG, dict(ws_bytes=need - 4)),
        ("no ws", L.E_BADARG, dict(ws=0, ws_bytes=need)),
        ("misaligned ws", L.E_ALIGN, dict(ws=oddf.data_ptr() + 4, ws_bytes=need)),
        ("PSF of 4913 elements", L.E_TOOBIG, dict(case=big)),
    ):
        gv, gt = _sentinels(CS.N)
        c = kw.pop("case", case)
        null = kw.pop("null", False)
        rc, ws, det = _raw(L, c, False, None if null else gv, None if null else gt, **kw)
        assert rc == want, label
        assert bool((gv == SENTINEL).all()) and bool((gt == SENTINEL).all()), label
        for t, s in ((ws, SENTINEL), (det, -77)):
            if isinstance(t, torch.Tensor):
                assert bool((t == s).all()), label
        assert bool((odd == -77).all()) and bool((oddf == SENTINEL).all()), label


# ---- autograd ------------------------------------------------------------------------------------------------------------------
def _tensors(case):
    n, h, w = case["g"].shape
    return (dev(case["sm"]).reshape(n, 1, h, w), dev(case["vm"]).reshape(1, 1, *CS.VS), dev(case["psf"]),
            dev(case["g"]).reshape(n, 1, h, w), (h, w))


@MODES
def test_autograd_backward_twice_gives_the_same_bits(K, interp_psf):
    from fetalsyngen_amd import rng
    from fetalsyngen_amd.generator.artifacts.svort import slice_acquisition

    case, _, fx = ref("psf335", True, interp_psf)
    sm, vm, psf, g, ss = _tensors(case)

    def grads(**kw):
        tr = dev(case["tr"]).requires_grad_()
        vol = dev(case["vol"]).reshape(1, 1, *CS.VS).requires_grad_()
        out = slice_acquisition(tr, vol, vm, sm, psf, ss, case["res"], False, interp_psf, **kw)
        (out * g).sum().backward()
        return vol.grad, tr.grad

    a, ta = grads(deterministic=True)
    b, tb = grads(deterministic=True)
    assert tuple(a.shape) == (1, 1, *CS.VS) and torch.equal(a, b) and torch.equal(ta, tb)
    assert bits_equal(a.reshape(CS.VS), fx["grad_vol"])
    with rng.keyed_scope(5, 0):
        c, tc = grads()  # inside a keyed scope the default takes the fixed-point path
    assert torch.equal(a, c) and torch.equal(ta, tc)
    with pytest.raises(ValueError):
        slice_acquisition(dev(case["tr"]), dev(case["vol"]).reshape(1, 1, *CS.VS), vm, sm, psf, ss, case["res"], False, interp_psf,
                          semantics="torch", deterministic=True)


def test_a_fit_of_volume_and_poses_replays_bit_for_bit(K):
    """Five Adam steps over the volume and the (n,6) poses through the acquisition and its equalised adjoint, both summed in
    fixed point, run twice from the same start: every parameter has the same bits at the end."""
    from fetalsyngen_amd.generator.artifacts.svort import slice_acquisition, slice_acquisition_adjoint
    from fetalsyngen_amd.generator.artifacts.svort.autograd import axisangle2mat_autograd

    fc = CS.fit_case()
    psf, ss, res = dev(fc["psf"]), fc["ss"], fc["res"]
    truth = dev(fc["vol"]).reshape(1, 1, *CS.VS)
    with torch.no_grad():
        target = slice_acquisition(axisangle2mat_autograd(dev(fc["true"])), truth, None, None, psf, ss, res, False, False)

    def fit():
        vol = (truth * 0.5).clone().requires_grad_()
        ax = dev(fc["start"]).clone().requires_grad_()
        opt = torch.optim.Adam([vol, ax], lr=0.02)
        for _ in range(5):
            tr = axisangle2mat_autograd(ax)
            slices = slice_acquisition(tr, vol, None, None, psf, ss, res, False, False, deterministic=True)
            back = slice_acquisition_adjoint(tr, psf, slices - target, None, None, CS.VS, res, False, True, deterministic=True)
            loss = ((slices - target) ** 2).sum() + (back ** 2).sum()
            opt.zero_grad()
            loss.backward()
            opt.step()
        return vol.detach().clone(), ax.detach().clone(), float(loss.detach())

    v1, a1, l1 = fit()
    v2, a2, l2 = fit()
    assert bool((v1 != truth * 0.5).any()) and bool((a1 != dev(fc["start"])).any())  # the parameters moved
    assert torch.equal(v1, v2) and torch.equal(a1, a2) and l1 == l2
