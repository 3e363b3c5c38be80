"""GPU: backward of the slice-acquisition adjoint (fsg_slice_acq_adjoint_backward_f32; the rule is in include/fsg_hip.h and
DESIGN.md section 19) against the float64 restatement tests/util_sa_adjoint_backward64.py, and the autograd path on top of it.

Tolerances (none is derived from what the kernel gives):
  exact-geometry cases   per element (K + 16) * 2^-24 * S, K the number of finest-grain terms the restatement sums into the
                         element and S the sum of their magnitudes: coordinates, trilinear weights and per-pixel weights are
                         exact in fp32 there (and vol_weight is a power of two or under the 1e-3 floor, so the division of the
                         gradient costs one rounding), so only the rounding of at most 16 products per term and the order of the
                         K - 1 additions remain.
  general rotations      per output tensor, mode and equalize setting 4 * E_cpu * max|float64|, E_cpu the difference of the
                         fp32-operation restatement to the float64 one over the same cases, measured on the CPU; the factor 4 is
                         section 18's, for the kernel ordering products and its reduction tree differently.  The cases keep every
                         decision distance above 1e-3 (asserted), so no floor, round or range test can flip.
A pose fit through the equalised reconstruction is NOT here: run on the CPU in float64 with the restatement behind Adam
(section 18's fit_case, translation of one slice, lr 0.15, 30 steps) the loss went 103.5 -> 96.8 and the error 1.5 -> 0.88 voxel
(lr 0.1: 0.70): it does not converge, for the reason DESIGN.md section 19 gives.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util_sa_adjoint_backward_cases as AC
from tests.util_sa_adjoint_backward64 import adjoint_backward32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
SENTINEL = -77.25

# max |adjoint_backward32 - adjoint_backward64| / max |adjoint_backward64| over AC.GENERAL, per (interp_psf, equalize, output),
# measured on the CPU, rounded up in the third digit:
#   LINEAR       plain 2.435e-6 / 1.201e-6, equalize 8.756e-6 / 4.204e-6
#   NEAREST_PSF  plain 3.284e-7 / 1.298e-6, equalize 2.570e-7 / 1.988e-6
E_CPU = {
    (False, False, "grad_slices"): 2.44e-6, (False, False, "grad_transforms"): 1.21e-6,
    (False, True, "grad_slices"): 8.76e-6, (False, True, "grad_transforms"): 4.21e-6,
    (True, False, "grad_slices"): 3.29e-7, (True, False, "grad_transforms"): 1.30e-6,
    (True, True, "grad_slices"): 2.58e-7, (True, True, "grad_transforms"): 1.99e-6,
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
    eq = case["vol"] is not None
    return K.slice_acq_adjoint_backward(dev(case["tr"]), dev(case["gvol"]), dev(case["psf"]), dev(case["sl"]), dev(case["sm"]),
                                        dev(case["vm"]), case["res"], interp_psf=interp_psf, equalize=eq, vol=dev(case["vol"]),
                                        vol_weight=dev(case["vw"]), **kw)


_REF = {}


def ref(kind, name, extra, interp_psf, equalize):
    """The case and its float64 restatement, computed once and shared (read only)."""
    key = (kind, name, extra, interp_psf, equalize)
    if key not in _REF:
        case = (AC.exact_case(name, extra, interp_psf, equalize) if kind == "exact"
                else AC.general_case(name, interp_psf, equalize))
        _REF[key] = (case, AC.reference(case, interp_psf))
    return _REF[key]


def check_bound(gs, gt, r):
    """per element |gpu - float64| <= (K + 16) * 2^-24 * S; prints the largest ratio before asserting"""
    worst = []
    for got, key, k, s in ((gs, "grad_slices", "k_sl", "s_sl"), (gt, "grad_transforms", "k_tr", "s_tr")):
        if got is None:
            continue
        e = np.abs(host(got).reshape(r[key].shape) - r[key])
        b = (r[k] + 16) * U * r[s]
        worst.append("%s: worst error/bound %.4f" % (key, (e / np.maximum(b, 1e-300)).max()))
        assert np.all(e <= b), worst
    print("; ".join(worst))


# ---- exact geometry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("equalize", [False, True], ids=["plain", "equalize"])
@pytest.mark.parametrize("masks", [False, True], ids=["nomask", "masks"])
@pytest.mark.parametrize("interp_psf", [False, True], ids=["linear", "nearest_psf"])
@pytest.mark.parametrize("name", list(AC.EXACT))
def test_exact_geometry_against_float64(K, name, interp_psf, masks, equalize):
    case, r = ref("exact", name, masks, interp_psf, equalize)
    n, h, w = case["sl"].shape
    gs, gt = run(K, case, interp_psf)
    assert tuple(gs.shape) == (n, h, w) and tuple(gt.shape) == (n, 3, 4)
    check_bound(gs, gt, r)
    empty = interp_psf and case["psf"].shape[0] == 1  # a one-plane PSF accepts no PSF coordinate in NEAREST_PSF: zeros
    assert bool(np.any(r["grad_slices"] != 0)) != empty and bool(np.any(r["grad_transforms"] != 0)) != empty
    if empty:
        assert bool((gs == 0).all()) and bool((gt == 0).all())
    if equalize and np.any(case["vw"] > 0):  # (the adjoint drops every pixel of a case whose PSF weighs less than 0.5)
        assert np.any(case["vw"] == np.float32(2.0 ** -11))  # the floor is exercised


# ---- general rotations ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("equalize", [False, True], ids=["plain", "equalize"])
@pytest.mark.parametrize("interp_psf", [False, True], ids=["linear", "nearest_psf"])
def test_general_rotations_within_four_times_the_fp32_cost_of_the_formula(K, interp_psf, equalize):
    worst = {"grad_slices": 0.0, "grad_transforms": 0.0}
    for name in AC.GENERAL:
        case, r = ref("general", name, None, interp_psf, equalize)
        assert min(r["dist"].values()) > 1e-3, r["dist"]  # precondition: no decision can flip between fp32 and float64
        assert case["sm"].sum() > 200  # and the mask that secures it leaves a real stack
        r32 = AC.reference(case, interp_psf, adjoint_backward32)
        gs, gt = run(K, case, interp_psf)
        for key, got in (("grad_slices", host(gs)), ("grad_transforms", host(gt).reshape(-1, 12))):
            scale = np.abs(r[key]).max()
            e_cpu = np.abs(r32[key] - r[key]).max() / scale
            e_gpu = np.abs(got - r[key]).max() / scale
            print(f"{name} {key}: E_cpu {e_cpu:.3e} (constant {E_CPU[interp_psf, equalize, key]:.3e}), GPU {e_gpu:.3e}")
            assert e_cpu <= E_CPU[interp_psf, equalize, key]  # the constants are what this CPU measures
            worst[key] = max(worst[key], e_gpu)
    for key in worst:
        assert worst[key] <= 4 * E_CPU[interp_psf, equalize, key], (key, worst[key])


# ---- determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("equalize", [False, True], ids=["plain", "equalize"])
@pytest.mark.parametrize("interp_psf", [False, True], ids=["linear", "nearest_psf"])
def test_both_outputs_are_bit_identical(K, interp_psf, equalize):
    case, _ = ref("exact", "psf223_big", True, interp_psf, equalize)
    gvol = dev(case["gvol"])
    keep = gvol.clone()
    args = (dev(case["tr"]), gvol, dev(case["psf"]), dev(case["sl"]), dev(case["sm"]), dev(case["vm"]), case["res"])
    kw = dict(interp_psf=interp_psf, equalize=equalize, vol=dev(case["vol"]), vol_weight=dev(case["vw"]))
    a_s, a_t = K.slice_acq_adjoint_backward(*args, **kw)
    b_s, b_t = K.slice_acq_adjoint_backward(*args, **kw)
    c_s, none_t = K.slice_acq_adjoint_backward(*args, need_transforms_grad=False, **kw)
    none_s, d_t = K.slice_acq_adjoint_backward(*args, need_slices_grad=False, **kw)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        e_s, e_t = K.slice_acq_adjoint_backward(*args, **kw)
    side.synchronize()
    assert none_t is None and none_s is None and bool(a_s.abs().max() > 0) and bool(a_t.abs().max() > 0)
    assert torch.equal(a_s, b_s) and torch.equal(a_s, c_s) and torch.equal(a_s, e_s)
    assert torch.equal(a_t, b_t) and torch.equal(a_t, d_t) and torch.equal(a_t, e_t)
    assert torch.equal(gvol, keep)  # the incoming gradient is read, never written (the reference equalises it in place)


# ---- edges -----------------------------------------------------------------------------------------------------------------
def _face_case(distance):
    """six slices, one pushed `distance` voxels towards each face of the volume along its own normal or in its plane"""
    case = AC.exact_case("psf223", False, n=6)
    case["tr"][:, :, :3] = np.eye(3)
    case["tr"][:, :, 3] = 0
    for i in range(6):
        case["tr"][i, i % 3, 3] = distance * (1 if i < 3 else -1)
    return case


def _raw(L, case, interp_psf, gs, gt, ws=None, ws_bytes=None, mode=None, equalize=None, vw="case"):
    lib = L.load()
    n, h, w = case["sl"].shape
    pd, ph, pw = case["psf"].shape
    t = {k: dev(case[k]) for k in ("tr", "gvol", "vw", "vol", "vm", "psf", "sl", "sm")}
    if vw is None:
        t["vw"] = None
    if equalize is None:
        equalize = case["vol"] is not None
    p = lambda x: C.c_void_p(0 if x is None else (x if isinstance(x, int) else x.data_ptr()))  # noqa: E731
    if ws is None:
        need = lib.fsg_slice_acq_adjoint_backward_ws_bytes(*AC.VS, n, h, w, int(equalize), int(gt is not None))
        ws = torch.full(((need + 7) // 8 * 2,), SENTINEL, device=DEV)
    if ws_bytes is None:
        ws_bytes = ws.numel() * 4 if isinstance(ws, torch.Tensor) else 0
    if mode is None:
        mode = L.SA.NEAREST_PSF if interp_psf else L.SA.LINEAR
    rc = lib.fsg_slice_acq_adjoint_backward_f32(p(t["tr"]), p(t["gvol"]), p(t["vw"]), p(t["vol"]), p(t["vm"]), p(t["psf"]), pd,
                                                ph, pw, p(t["sl"]), p(t["sm"]), p(gs), p(gt), *AC.VS, n, h, w,
                                                float(case["res"]), mode, int(equalize), p(ws), ws_bytes,
                                                C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return rc, ws


def _sentinels(case):
    n, h, w = case["sl"].shape
    return torch.full((n, h, w), SENTINEL, device=DEV), torch.full((n, 12), SENTINEL, device=DEV)


@pytest.mark.parametrize("interp_psf", [False, True], ids=["linear", "nearest_psf"])
def test_slices_wholly_outside_every_face_write_zeros(L, interp_psf):
    case = _face_case(64.0)
    gs, gt = _sentinels(case)
    rc, _ = _raw(L, case, interp_psf, gs, gt)
    assert rc == 0 and bool((gs == 0).all()) and bool((gt == 0).all())


@pytest.mark.parametrize("interp_psf", [False, True], ids=["linear", "nearest_psf"])
def test_slices_partly_outside_every_face(L, interp_psf):
    # in plane the 19.5 x 16.5 voxel slices straddle a face of the 22 x 18 x 20 volume; along the normal the slice plane stops
    # a quarter voxel from the last accepted plane, so one of the PSF's two planes is outside
    case = _face_case(9.25)
    r = AC.reference(case, interp_psf)
    assert np.all(np.abs(r["grad_transforms"]).max(1) > 0) and np.any(r["grad_slices"] == 0) and np.any(r["grad_slices"] != 0)
    gs, gt = _sentinels(case)
    rc, _ = _raw(L, case, interp_psf, gs, gt)
    assert rc == 0
    check_bound(gs, gt, r)


@pytest.mark.parametrize("what", ["zero_grad", "mask_all_false", "one_slice"])
def test_degenerate_inputs(L, what):
    case = AC.exact_case("psf223", what == "mask_all_false", n=1 if what == "one_slice" else AC.N)
    if what == "zero_grad":
        case["gvol"][:] = 0
    elif what == "mask_all_false":
        case["sm"][:] = False
    for interp_psf in (False, True):
        gs, gt = _sentinels(case)
        rc, _ = _raw(L, case, interp_psf, gs, gt)
        assert rc == 0
        if what == "one_slice":
            r = AC.reference(case, interp_psf)
            assert np.any(r["grad_transforms"] != 0)
            check_bound(gs, gt, r)
        else:
            assert bool((gs == 0).all()) and bool((gt == 0).all())


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_and_workspace_untouched(L):
    case = AC.exact_case("psf223", True, False, True)
    lib = L.load()
    n, h, w = case["sl"].shape
    nv = int(np.prod(AC.VS))
    need = lib.fsg_slice_acq_adjoint_backward_ws_bytes(*AC.VS, n, h, w, 1, 1)
    assert need == AC.N * 1 * 12 * 4 + 4 * nv
    assert lib.fsg_slice_acq_adjoint_backward_ws_bytes(*AC.VS, 5, 37, 29, 0, 1) == 5 * 6 * 48
    assert lib.fsg_slice_acq_adjoint_backward_ws_bytes(*AC.VS, n, h, w, 1, 0) == 4 * nv
    assert lib.fsg_slice_acq_adjoint_backward_ws_bytes(*AC.VS, n, h, w, 0, 0) == 0
    assert lib.fsg_slice_acq_adjoint_backward_ws_bytes(*AC.VS, 0, 13, 11, 1, 1) == 0
    big = dict(case, psf=np.ones((17, 17, 17), np.float32))
    wide = dict(case, psf=np.ones((1, 1, 65), np.float32))
    odd = torch.full((need // 4 + 2,), SENTINEL, device=DEV)
    for label, want, kw in (
        ("both outputs NULL", L.E_BADARG, dict(null=True)),
        ("FSG_SA_TORCH", L.E_BADARG, dict(mode=L.SA.TORCH)),
        ("short ws", L.E_BADARG, dict(ws_bytes=need - 4)),
        ("no ws", L.E_BADARG, dict(ws=0, ws_bytes=need)),
        ("misaligned ws", L.E_ALIGN, dict(ws=odd.data_ptr() + 4, ws_bytes=need)),
        ("equalize without vol_weight", L.E_BADARG, dict(vw=None)),
        ("PSF of 4913 elements", L.E_TOOBIG, dict(case=big)),
        ("PSF 65 wide", L.E_TOOBIG, dict(case=wide)),
    ):
        gs, gt = _sentinels(case)
        c = kw.pop("case", case)
        null = kw.pop("null", False)
        rc, ws = _raw(L, c, False, None if null else gs, None if null else gt, **kw)
        assert rc == want, label
        assert bool((gs == SENTINEL).all()) and bool((gt == SENTINEL).all()), label
        if isinstance(ws, torch.Tensor):
            assert bool((ws == SENTINEL).all()), label
        assert bool((odd == SENTINEL).all()), label
    # grad_slices alone without equalize needs no workspace
    gs, _ = _sentinels(case)
    rc, _ = _raw(L, case, False, gs, None, ws=0, ws_bytes=0, equalize=False)
    assert rc == 0 and bool((gs != SENTINEL).all())


# ---- autograd end to end -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("equalize", [False, True], ids=["plain", "equalize"])
@pytest.mark.parametrize("interp_psf", [False, True], ids=["linear", "nearest_psf"])
def test_autograd_fills_both_grads_with_the_kernel_results(K, interp_psf, equalize):
    from fetalsyngen_amd.generator.artifacts.svort import slice_acquisition_adjoint
    from fetalsyngen_amd.generator.artifacts.svort.autograd import axisangle2mat_autograd
    from fetalsyngen_amd.generator.artifacts.svort.rigid import mat2axisangle

    case, _ = ref("general", "psf223_vm", None, interp_psf, False)
    n, h, w = case["sl"].shape
    # (n,6) poses on the device; the transforms the kernels see are the fp32 matrices these poses give
    ax = mat2axisangle(torch.from_numpy(case["tr"])).to(DEV).requires_grad_()
    tr = axisangle2mat_autograd(ax)
    sl = dev(case["sl"]).reshape(n, 1, h, w).requires_grad_()
    sm, vm, psf = dev(case["sm"]).reshape(n, 1, h, w), dev(case["vm"]).reshape(1, 1, *AC.VS), dev(case["psf"])
    out = slice_acquisition_adjoint(tr, psf, sl, sm, vm, AC.VS, case["res"], interp_psf, equalize, deterministic=True)
    assert out.grad_fn is not None and tuple(out.shape) == (1, 1, *AC.VS)
    with torch.no_grad():
        quiet = slice_acquisition_adjoint(tr, psf, sl, sm, vm, AC.VS, case["res"], interp_psf, equalize, deterministic=True)
    plain = slice_acquisition_adjoint(tr.detach(), psf, sl.detach(), sm, vm, AC.VS, case["res"], interp_psf, equalize,
                                      deterministic=True)
    assert quiet.grad_fn is None and plain.grad_fn is None
    assert torch.equal(plain, out.detach()) and torch.equal(quiet, plain)  # the deterministic adjoint: bit for bit
    gvol = dev(case["gvol"])
    tr.retain_grad()
    (out * gvol.reshape(1, 1, *AC.VS)).sum().backward()
    kw = {}
    if equalize:
        vol, vw = K.slice_acq_adjoint(tr.detach(), psf, sl.detach().reshape(n, h, w), sm.reshape(n, h, w), vm.reshape(AC.VS),
                                      AC.VS, case["res"], interp_psf=interp_psf, equalize=True, return_weight=True,
                                      deterministic=True)
        kw = dict(vol=vol, vol_weight=vw)
    gs, gt = K.slice_acq_adjoint_backward(tr.detach(), gvol, psf, sl.detach().reshape(n, h, w), sm.reshape(n, h, w),
                                          vm.reshape(AC.VS), case["res"], interp_psf=interp_psf, equalize=equalize, **kw)
    assert torch.equal(sl.grad.reshape(n, h, w), gs) and torch.equal(tr.grad, gt)  # deterministic
    assert bool(gs.abs().max() > 0) and bool(gt.abs().max() > 0)
    assert tuple(ax.grad.shape) == (n, 6) and bool(torch.isfinite(ax.grad).all()) and bool((ax.grad.abs().max(1).values > 0).all())
    with pytest.raises(NotImplementedError):
        slice_acquisition_adjoint(tr, psf, sl, sm, vm, AC.VS, case["res"], interp_psf, equalize, semantics="torch")
    with pytest.raises(NotImplementedError):
        slice_acquisition_adjoint(tr, psf, sl, sm, vm, AC.VS, case["res"], interp_psf, equalize, slice_ids=torch.arange(n))


def test_psf_reconstruction_differentiates(K):
    from fetalsyngen_amd.generator.artifacts.simulate_reco import PSFreconstruction

    case, _ = ref("general", "psf335", None, True, False)
    n, h, w = case["sl"].shape
    tr = dev(case["tr"]).requires_grad_()
    sl = dev(case["sl"]).reshape(n, 1, h, w).requires_grad_()
    params = {"psf": dev(case["psf"]), "volume_shape": AC.VS, "res_s": case["res"], "res_r": 1.0, "interp_psf": True}
    out = PSFreconstruction(tr, sl, dev(case["sm"]).reshape(n, 1, h, w), None, params, deterministic=True)
    assert out.grad_fn is not None
    plain = PSFreconstruction(tr.detach(), sl.detach(), dev(case["sm"]).reshape(n, 1, h, w), None, params, deterministic=True)
    assert plain.grad_fn is None and torch.equal(plain, out.detach())
    gvol = dev(case["gvol"])
    (out * gvol.reshape(1, 1, *AC.VS)).sum().backward()
    vol, vw = K.slice_acq_adjoint(tr.detach(), params["psf"], sl.detach().reshape(n, h, w), dev(case["sm"]), None, AC.VS,
                                  case["res"], interp_psf=True, equalize=True, return_weight=True, deterministic=True)
    gs, gt = K.slice_acq_adjoint_backward(tr.detach(), gvol, params["psf"], sl.detach().reshape(n, h, w), dev(case["sm"]), None,
                                          case["res"], interp_psf=True, equalize=True, vol=vol, vol_weight=vw)
    assert torch.equal(sl.grad.reshape(n, h, w), gs) and torch.equal(tr.grad, gt) and bool(gt.abs().max() > 0)
