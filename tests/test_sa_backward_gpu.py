"""GPU: backward of the slice-acquisition forward operator (fsg_slice_acq_backward_f32; the rule is in include/fsg_hip.h and
DESIGN.md section 18) against the float64 restatement tests/util_sa_backward64.py, and the autograd path on top of it.

Tolerances (none is derived from what the kernel gives):
  exact-geometry cases   per element (K + 16) * 2^-24 * S, K the number of finest-grain terms the restatement sums into the
                         element and S the sum of their magnitudes: coordinates, trilinear weights and per-pixel weights are
                         exact in fp32 there, so only the rounding of at most 16 products per term and the order of the K - 1
                         additions remain.
  general rotations      per output tensor and mode 4 * E_cpu * max|float64|, E_cpu the difference of the fp32-operation
                         restatement (float64 accumulation) to the float64 one over the same cases, measured on the CPU; the
                         factor 4 is for the kernel's own fp32 reduction tree and atomic order.  The cases keep every decision
                         distance above 1e-3 (asserted), so no floor, round or range test can flip and no outlier cap is needed.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util_sa_backward_cases as CS
from tests.util_sa_backward64 import backward32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
SENTINEL = -77.25

# max |backward32 - backward64| / max |backward64| over CS.GENERAL, per mode and output, measured on the CPU
# (LINEAR: 1.247e-6 / 1.138e-6; NEAREST_PSF: 4.724e-7 / 1.337e-6), rounded up in the third digit.
E_CPU = {
    (False, "grad_vol"): 1.25e-6, (False, "grad_transforms"): 1.14e-6,
    (True, "grad_vol"): 4.73e-7, (True, "grad_transforms"): 1.34e-6,
}


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (and libfsg_hip.so); there is no fallback to skip to")
    from fetalsyngen_amd import kernels

    return kernels


@pytest.fixture(scope="module")
def L():
    from fetalsyngen_amd import _lib

    return _lib


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(x):
    return x.detach().cpu().numpy().astype(np.float64)


def run(K, case, interp_psf, **kw):
    return K.slice_acq_backward(dev(case["tr"]), dev(case["vol"]), dev(case["vm"]), dev(case["sm"]), dev(case["psf"]),
                                dev(case["g"]), case["res"], interp_psf=interp_psf, **kw)


_REF = {}


def ref(kind, name, extra, interp_psf):
    """The case and its float64 restatement, computed once and shared (read only)."""
    key = (kind, name, extra, interp_psf)
    if key not in _REF:
        case = CS.exact_case(name, extra) if kind == "exact" else CS.general_case(name, interp_psf)
        _REF[key] = (case, CS.reference(case, interp_psf))
    return _REF[key]


def check_bound(gv, gt, r):
    """per element |gpu - float64| <= (K + 16) * 2^-24 * S; prints the largest ratio before asserting"""
    ev = np.abs(host(gv) - r["grad_vol"])
    bv = (r["k_vol"] + 16) * U * r["s_vol"]
    et = np.abs(host(gt).reshape(-1, 12) - r["grad_transforms"])
    bt = (r["k_tr"] + 16) * U * r["s_tr"]
    print("grad_vol: worst error/bound %.3f; grad_transforms: %.5f" % ((ev / np.maximum(bv, 1e-300)).max(),
                                                                      (et / np.maximum(bt, 1e-300)).max()))
    assert np.all(ev <= bv) and np.all(et <= bt)


# ---- exact geometry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masks", [False, True], ids=["nomask", "masks"])
@pytest.mark.parametrize("interp_psf", [False, True], ids=["linear", "nearest_psf"])
@pytest.mark.parametrize("name", list(CS.EXACT))
def test_exact_geometry_against_float64(K, name, interp_psf, masks):
    case, r = ref("exact", name, masks, interp_psf)
    gv, gt = run(K, case, interp_psf)
    assert tuple(gv.shape) == CS.VS and tuple(gt.shape) == (CS.N, 3, 4)
    check_bound(gv, gt, r)
    empty = interp_psf and case["psf"].shape[0] == 1  # a one-plane PSF accepts no PSF coordinate in NEAREST_PSF
    assert bool(np.any(r["grad_vol"] != 0)) != empty and bool(np.any(r["grad_transforms"] != 0)) != empty


# ---- general rotations ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp_psf", [False, True], ids=["linear", "nearest_psf"])
def test_general_rotations_within_four_times_the_fp32_cost_of_the_formula(K, interp_psf):
    worst = {"grad_vol": 0.0, "grad_transforms": 0.0}
    for name in CS.GENERAL:
        case, r = ref("general", name, None, interp_psf)
        assert min(r["dist"].values()) > 1e-3, r["dist"]  # precondition: no decision can flip between fp32 and float64
        assert case["sm"].sum() > 200  # and the mask that secures it leaves a real stack
        r32 = CS.reference(case, interp_psf, backward32)
        gv, gt = run(K, case, interp_psf)
        for key, got in (("grad_vol", host(gv)), ("grad_transforms", host(gt).reshape(-1, 12))):
            scale = np.abs(r[key]).max()
            e_cpu = np.abs(r32[key] - r[key]).max() / scale
            e_gpu = np.abs(got - r[key]).max() / scale
            print(f"{name} {key}: E_cpu {e_cpu:.3e} (constant {E_CPU[interp_psf, key]:.3e}), GPU {e_gpu:.3e}")
            assert e_cpu <= E_CPU[interp_psf, key]  # the constants are what this CPU measures
            worst[key] = max(worst[key], e_gpu)
    for key in worst:
        assert worst[key] <= 4 * E_CPU[interp_psf, key], (key, worst[key])


# ---- determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp_psf", [False, True], ids=["linear", "nearest_psf"])
def test_grad_transforms_is_bit_identical(K, interp_psf):
    case, _ = ref("exact", "psf223_big", True, interp_psf)
    _, a = run(K, case, interp_psf)
    _, b = run(K, case, interp_psf)
    none, c = run(K, case, interp_psf, need_vol_grad=False)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        _, d = run(K, case, interp_psf)
    side.synchronize()
    assert none is None and bool(a.abs().max() > 0)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def test_grad_vol_is_bit_identical_where_voxels_get_one_contribution(K):
    """One slice, a 1x1x1 PSF, a pixel pitch of 2 voxels along the volume axes: the 2x2x2 cells of neighbouring pixels are
    disjoint, so every voxel receives at most one atomic and the order of the atomics cannot matter."""
    case = CS.exact_case("delta", False, n=1)
    case["res"] = 2.0
    r = CS.reference(case, False)
    assert r["k_vol"].max() == 1 and (r["k_vol"] == 1).sum() > 100
    gv, gt = run(K, case, False)
    gv2, none = run(K, case, False, need_transforms_grad=False)
    assert none is None and torch.equal(gv, gv2) and torch.equal(gv, run(K, case, False)[0])
    check_bound(gv, gt, r)


def test_grad_vol_with_and_without_grad_transforms_stays_within_the_bound(K):
    case, r = ref("exact", "psf335", True, False)
    gv, _ = run(K, case, False, need_transforms_grad=False)
    _, gt = run(K, case, False, need_vol_grad=False)
    check_bound(gv, gt, r)


# ---- edges -----------------------------------------------------------------------------------------------------------------
def _face_case(distance):
    """six slices, one pushed `distance` voxels towards each face of the volume along its own normal or in its plane"""
    case = CS.exact_case("psf223", False, n=6)
    case["tr"][:, :, :3] = np.eye(3)
    case["tr"][:, :, 3] = 0
    for i in range(6):
        case["tr"][i, i % 3, 3] = distance * (1 if i < 3 else -1)
    return case


def _raw(L, case, interp_psf, gv, gt, ws=None, ws_bytes=None, mode=None):
    lib = L.load()
    n, h, w = case["g"].shape
    pd, ph, pw = case["psf"].shape
    t = {k: dev(case[k]) for k in ("tr", "vol", "vm", "psf", "g", "sm")}
    p = lambda x: C.c_void_p(0 if x is None else (x if isinstance(x, int) else x.data_ptr()))  # noqa: E731
    if ws is None:
        ws = torch.full((lib.fsg_slice_acq_backward_ws_bytes(n, h, w) // 4,), SENTINEL, device=DEV)
    if ws_bytes is None:
        ws_bytes = ws.numel() * 4 if isinstance(ws, torch.Tensor) else 0
    if mode is None:
        mode = L.SA.NEAREST_PSF if interp_psf else L.SA.LINEAR
    rc = lib.fsg_slice_acq_backward_f32(p(t["tr"]), p(t["vol"]), p(t["vm"]), p(t["psf"]), pd, ph, pw, p(t["g"]), p(t["sm"]), p(gv),
                                        p(gt), *CS.VS, n, h, w, float(case["res"]), mode, p(ws), ws_bytes,
                                        C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return rc, ws


def _sentinels(n):
    return torch.full(CS.VS, SENTINEL, device=DEV), torch.full((n, 12), SENTINEL, device=DEV)


@pytest.mark.parametrize("interp_psf", [False, True], ids=["linear", "nearest_psf"])
def test_slices_wholly_outside_every_face_write_zeros(L, interp_psf):
    case = _face_case(64.0)
    gv, gt = _sentinels(6)
    rc, _ = _raw(L, case, interp_psf, gv, gt)
    assert rc == 0 and bool((gv == 0).all()) and bool((gt == 0).all())


@pytest.mark.parametrize("interp_psf", [False, True], ids=["linear", "nearest_psf"])
def test_slices_partly_outside_every_face(L, interp_psf):
    # in plane the 19.5 x 16.5 voxel slices straddle a face of the 22 x 18 x 20 volume; along the normal the slice plane stops
    # a quarter voxel from the last accepted plane, so one of the PSF's two planes is outside
    case = _face_case(9.25)
    r = CS.reference(case, interp_psf)
    assert np.all(np.abs(r["grad_transforms"]).max(1) > 0)
    gv, gt = _sentinels(6)
    rc, _ = _raw(L, case, interp_psf, gv, gt)
    assert rc == 0
    check_bound(gv, gt, r)


@pytest.mark.parametrize("what", ["zero_grad", "mask_all_false", "one_slice"])
def test_degenerate_inputs(L, what):
    case = CS.exact_case("psf223", what == "mask_all_false", n=1 if what == "one_slice" else CS.N)
    if what == "zero_grad":
        case["g"][:] = 0
    elif what == "mask_all_false":
        case["sm"][:] = False
    n = case["g"].shape[0]
    for interp_psf in (False, True):
        gv, gt = _sentinels(n)
        rc, _ = _raw(L, case, interp_psf, gv, gt)
        assert rc == 0
        if what == "one_slice":
            r = CS.reference(case, interp_psf)
            assert np.any(r["grad_transforms"] != 0)
            check_bound(gv, gt, r)
        else:
            assert bool((gv == 0).all()) and bool((gt == 0).all())


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_and_workspace_untouched(L):
    case = CS.exact_case("psf223", True)
    lib = L.load()
    need = lib.fsg_slice_acq_backward_ws_bytes(*case["g"].shape)
    assert need == CS.N * 1 * 12 * 4 and lib.fsg_slice_acq_backward_ws_bytes(5, 37, 29) == 5 * 6 * 48
    assert lib.fsg_slice_acq_backward_ws_bytes(0, 13, 11) == 0
    big = dict(case, psf=np.ones((17, 17, 17), np.float32))
    wide = dict(case, psf=np.ones((1, 1, 65), np.float32))
    odd = torch.full((need // 4 + 1,), SENTINEL, device=DEV)
    for label, want, kw in (
        ("both outputs NULL", L.E_BADARG, dict(null=True)),
        ("FSG_SA_TORCH", L.E_BADARG, dict(mode=L.SA.TORCH)),
        ("short ws", L.E_BADARG, dict(ws_bytes=need - 4)),
        ("no ws", L.E_BADARG, dict(ws=0, ws_bytes=need)),
        ("misaligned ws", L.E_ALIGN, dict(ws=odd.data_ptr() + 4, ws_bytes=need)),
        ("PSF of 4913 elements", L.E_TOOBIG, dict(case=big)),
        ("PSF 65 wide", L.E_TOOBIG, dict(case=wide)),
    ):
        gv, gt = _sentinels(CS.N)
        c = kw.pop("case", case)
        null = kw.pop("null", False)
        rc, ws = _raw(L, c, False, None if null else gv, None if null else gt, **kw)
        assert rc == want, label
        assert bool((gv == SENTINEL).all()) and bool((gt == SENTINEL).all()), label
        if isinstance(ws, torch.Tensor):
            assert bool((ws == SENTINEL).all()), label
        assert bool((odd == SENTINEL).all()), label
    # grad_vol alone needs no workspace
    gv, _ = _sentinels(CS.N)
    rc, _ = _raw(L, case, False, gv, None, ws=0, ws_bytes=0)
    assert rc == 0 and bool((gv != SENTINEL).all())


# ---- autograd end to end -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp_psf", [False, True], ids=["linear", "nearest_psf"])
def test_autograd_fills_both_grads_with_the_kernel_results(K, interp_psf):
    from fetalsyngen_amd.generator.artifacts.svort import slice_acquisition

    case, _ = ref("exact", "psf223", True, interp_psf)
    tr = dev(case["tr"]).requires_grad_()
    vol = dev(case["vol"]).reshape(1, 1, *CS.VS).requires_grad_()
    n, h, w = case["g"].shape
    sm, vm = dev(case["sm"]).reshape(n, 1, h, w), dev(case["vm"]).reshape(1, 1, *CS.VS)
    out, weight = slice_acquisition(tr, vol, vm, sm, dev(case["psf"]), (h, w), case["res"], True, interp_psf)
    assert out.grad_fn is not None and tuple(out.shape) == (n, 1, h, w) and tuple(weight.shape) == (n, 1, h, w)
    plain = slice_acquisition(tr.detach(), vol.detach(), vm, sm, dev(case["psf"]), (h, w), case["res"], False, interp_psf)
    assert plain.grad_fn is None and torch.equal(plain, out.detach())
    (out * dev(case["g"]).reshape(n, 1, h, w)).sum().backward()
    gv, gt = run(K, case, interp_psf)
    assert torch.equal(tr.grad, gt)  # deterministic
    assert tuple(vol.grad.shape) == (1, 1, *CS.VS)
    _, r = ref("exact", "psf223", True, interp_psf)
    check_bound(vol.grad.reshape(CS.VS), tr.grad, r)
    with pytest.raises(NotImplementedError):
        slice_acquisition(tr, vol, vm, sm, dev(case["psf"]), (h, w), case["res"], False, interp_psf, semantics="torch")


def test_fit_recovers_a_slice_translation(K):
    from fetalsyngen_amd.generator.artifacts.svort import slice_acquisition
    from fetalsyngen_amd.generator.artifacts.svort.autograd import axisangle2mat_autograd

    fc = CS.fit_case()
    vol, psf = dev(fc["vol"]).reshape(1, 1, *CS.VS), dev(fc["psf"])
    acquire = lambda ax: slice_acquisition(axisangle2mat_autograd(ax), vol, None, None, psf, fc["ss"], fc["res"], False, False)  # noqa: E731
    true, start = dev(fc["true"]), dev(fc["start"])
    target = acquire(true)
    assert target.grad_fn is None
    p = torch.zeros(3, device=DEV, requires_grad=True)
    place = torch.zeros(CS.N, 6, 3, device=DEV)
    for a in range(3):
        place[CS.FIT_SLICE, 3 + a, a] = 1
    opt = torch.optim.Adam([p], lr=CS.FIT_LR, betas=CS.FIT_BETAS)
    losses = []
    for _ in range(CS.FIT_STEPS):
        ax = start + place @ p
        assert ax.is_cuda and ax.requires_grad
        loss = ((acquire(ax) - target) ** 2).sum()
        losses.append(loss.detach())
        opt.zero_grad()
        loss.backward()
        opt.step()
    with torch.no_grad():
        ax = start + place @ p
        final = float(((acquire(ax) - target) ** 2).sum())
        err = float((ax - true)[CS.FIT_SLICE, 3:].norm())
    first = float(losses[0])
    print(f"loss {first:.4f} -> {final:.6f}, translation error {CS.FIT_OFFSET} -> {err:.4f} voxel")
    assert final * 10 <= first and err < 0.25
