"""CPU: the float64 restatement of the slice-acquisition backward (tests/util_sa_backward64.py) is pinned to the forward it
differentiates, and the Python layers are wired to the new entry points.  Nothing here touches a device.

The forward map is oracle/fsg_oracle_sr.py's `slice_acq_forward_cuda`, imported as it is; its working precision is the module
attribute `F32`, which these tests point at float64 for the duration of a call, so the same loops give a float64 forward.
"""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from fetalsyngen_amd import _lib
from fetalsyngen_amd.generator.artifacts.svort import rigid
from fetalsyngen_amd.generator.artifacts.svort import slice_acq as SA
from fetalsyngen_amd.generator.artifacts.svort.autograd import axisangle2mat_autograd
from oracle import fsg_oracle_sr as S
from tests.util_sa_backward64 import backward32, backward64

VS = (20, 18, 22)


def _rot(rng, max_angle):
    ax = rng.uniform(-1, 1, 3)
    ax = ax / np.linalg.norm(ax) * rng.uniform(0.2, max_angle)
    return S.axisangle2mat(torch.tensor(np.r_[ax, 0, 0, 0][None], dtype=torch.float32))[0, :, :3].numpy()


def _transforms(rng, n, max_angle=0.6, shift=2.0):
    tr = np.zeros((n, 3, 4), np.float32)
    for i in range(n):
        tr[i, :, :3] = _rot(rng, max_angle)
        tr[i, :, 3] = rng.uniform(-shift, shift, 3)
    return tr


def _psf(rng, shape):
    return rng.uniform(0.2, 1.0, shape).astype(np.float32)


@pytest.fixture
def forward64(monkeypatch):
    monkeypatch.setattr(S, "F32", np.float64)

    def fwd(tr, vol, psf, slice_shape, res, interp_psf):
        return S.slice_acq_forward_cuda(np.asarray(tr, np.float64), np.asarray(vol, np.float64), None, None,
                                        np.asarray(psf, np.float64), slice_shape, res, False, interp_psf)
    return fwd


# ---- adjointness -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp_psf", [False, True])
@pytest.mark.parametrize("pshape", [(3, 3, 5), (2, 2, 3)])
def test_grad_vol_is_the_transpose_of_the_forward(forward64, interp_psf, pshape):
    rng = np.random.default_rng(11)
    tr, psf = _transforms(rng, 5, shift=6.0), _psf(rng, pshape)  # shifts large enough that slices leave the volume
    v = rng.standard_normal(VS).astype(np.float32)
    g = rng.standard_normal((5, 13, 11)).astype(np.float32)
    Av = forward64(tr, v, psf, (13, 11), 1.5, interp_psf)
    ATg = backward64(tr, v, None, psf, g, None, 1.5, interp_psf)["grad_vol"]
    lhs, rhs = float((Av * g).sum()), float((v.astype(np.float64) * ATg).sum())
    assert np.any(Av == 0) and np.any(Av != 0)  # some pixels outside, some inside
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs))


# ---- finite differences ------------------------------------------------------------------------------------------------
def test_grad_transforms_equals_central_differences_of_the_forward(forward64):
    """LINEAR, every PSF footprint strictly inside the volume: the weight does not depend on the transform, and the transform
    gradient is the derivative of the forward.  All 12 entries of every slice."""
    rng = np.random.default_rng(5)
    n, ss, res, h = 2, (3, 3), 1.5, 1e-5
    tr, psf = _transforms(rng, n, shift=1.0), _psf(rng, (2, 2, 3))
    # a smooth volume keeps the third derivative along a transform entry, and with it the O(h^2) error, small
    zz, yy, xx = np.meshgrid(*(np.arange(s) for s in VS), indexing="ij")
    vol = (np.sin(0.31 * xx) * np.cos(0.27 * yy) + 0.05 * zz + 0.02 * xx * yy / 10).astype(np.float32)
    g = rng.standard_normal((n, *ss)).astype(np.float32)
    ref = backward64(tr, vol, None, psf, g, None, res, False)
    # preconditions: nothing near the faces (constant weight), no tap within reach of a cell boundary under a +-h step
    assert ref["dist"]["bounds"] > 2.0 and ref["dist"]["grid"] > 1e-3, ref["dist"]
    loss = lambda t: float((forward64(t, vol, psf, ss, res, False) * g).sum())  # noqa: E731
    fd = np.zeros((n, 12))
    for i in range(n):
        for k in range(12):
            tp, tm = tr.astype(np.float64), tr.astype(np.float64)
            tp.reshape(n, 12)[i, k] += h
            tm.reshape(n, 12)[i, k] -= h
            fd[i, k] = (loss(tp) - loss(tm)) / (2 * h)
    got = ref["grad_transforms"]
    assert np.all(np.abs(fd) > 1e-3)  # every entry carries a gradient: the relative test below tests all 12
    assert np.all(np.abs(got - fd) <= 1e-6 * np.abs(fd)), (got, fd)


# ---- non-finite safety -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp_psf", [False, True])
@pytest.mark.parametrize("bad", ["nan_rotation", "nan_translation", "inf_translation", "inf_rotation", "nan_res"])
def test_non_finite_geometry_gives_zero_gradients(interp_psf, bad):
    rng = np.random.default_rng(3)
    n = 3
    tr, psf = _transforms(rng, n), _psf(rng, (2, 2, 3))
    vol = rng.standard_normal(VS).astype(np.float32)
    g = rng.standard_normal((n, 5, 4)).astype(np.float32)
    res = 1.5
    if bad == "nan_rotation":
        tr[1, 0, 1] = np.nan
    elif bad == "nan_translation":
        tr[1, 2, 3] = np.nan
    elif bad == "inf_translation":
        tr[1, 0, 3] = np.inf
    elif bad == "inf_rotation":
        tr[1, 2, 2] = -np.inf
    else:
        res = float("nan")
    hit = range(n) if bad == "nan_res" else [1]
    for fn in (backward64, backward32):
        out = fn(tr, vol, None, psf, g, None, res, interp_psf)
        assert np.all(np.isfinite(out["grad_vol"])) and np.all(np.isfinite(out["grad_transforms"]))
        for i in hit:
            assert np.all(out["grad_transforms"][i] == 0)
        alone = fn(tr, vol, None, psf, np.where(np.isin(np.arange(n), list(hit))[:, None, None], g, 0), None, res, interp_psf)
        assert np.all(alone["grad_vol"] == 0) and np.all(alone["k_vol"] == 0)
        if bad != "nan_res":  # the other slices are untouched by their neighbour's transform
            good = np.delete(np.arange(n), 1)
            clean = fn(tr[good], vol, None, psf, g[good], None, res, interp_psf)
            assert np.array_equal(out["grad_transforms"][good], clean["grad_transforms"])
            assert np.any(clean["grad_transforms"] != 0)


# ---- the two quirks, on hand-built two-tap cases --------------------------------------------------------------------------
def _two_tap_case():
    """One slice of one pixel, identity transform, at the centre voxel of a 5^3 volume; a (1,1,2) PSF: tap 0 at x - 1, tap 1
    at x (tap offsets -1, 0).  Integer positions: each tap puts all its trilinear weight on one voxel."""
    tr = np.eye(3, 4, dtype=np.float32)[None]
    vol = np.arange(125, dtype=np.float32).reshape(5, 5, 5)
    return tr, vol, np.array([[[2.0]]], np.float32)


def test_quirk_the_weight_ignores_vol_mask():
    tr, vol, g = _two_tap_case()
    psf = np.array([[[1.0, 3.0]]], np.float32)
    vm = np.ones((5, 5, 5), bool)
    vm[2, 2, 2] = False  # the voxel under tap 1
    out = backward64(tr, vol, vm, psf, g, None, 1.0, False)
    # the forward would normalise by the unmasked weight 1 and give d slice / d vol[2,2,1] = 1; the backward divides by 1 + 3
    assert out["grad_vol"][2, 2, 1] == 2.0 * 1.0 / 4.0
    assert out["grad_vol"][2, 2, 2] == 0 and np.count_nonzero(out["grad_vol"]) == 1
    fwd = S.slice_acq_forward_cuda(tr, vol, vm, None, psf, (1, 1), 1.0, True, False)
    assert fwd[1][0, 0, 0] == 1.0 and fwd[0][0, 0, 0] == vol[2, 2, 1]  # the forward's own weight does leave the voxel out


def test_quirk_a_negative_weight_goes_on_and_a_zero_weight_stops():
    tr, vol, g = _two_tap_case()
    neg = backward64(tr, vol, None, np.array([[[1.0, -3.0]]], np.float32), g, None, 1.0, False)
    assert neg["grad_vol"][2, 2, 1] == 2.0 * 1.0 / -2.0 and neg["grad_vol"][2, 2, 2] == 2.0 * -3.0 / -2.0
    assert np.any(neg["grad_transforms"] != 0)
    fwd = S.slice_acq_forward_cuda(tr, vol, None, None, np.array([[[1.0, -3.0]]], np.float32), (1, 1), 1.0, False, False)
    assert fwd[0, 0, 0] == 0  # the forward drops the pixel (weight > 0 fails): a gradient where the output is constant
    zero = backward64(tr, vol, None, np.array([[[1.0, -1.0]]], np.float32), g, None, 1.0, False)
    assert np.all(zero["grad_vol"] == 0) and np.all(zero["grad_transforms"] == 0) and np.all(zero["k_vol"] == 0)


def test_masked_pixels_and_zero_gradients_contribute_nothing():
    rng = np.random.default_rng(8)
    tr, psf = _transforms(rng, 2), _psf(rng, (1, 3, 3))
    vol = rng.standard_normal(VS).astype(np.float32)
    g = rng.standard_normal((2, 6, 5)).astype(np.float32)
    sm = rng.random((2, 6, 5)) < 0.5
    a = backward64(tr, vol, None, psf, g, sm, 1.5, False)
    b = backward64(tr, vol, None, psf, np.where(sm, g, 0), None, 1.5, False)
    assert np.array_equal(a["grad_vol"], b["grad_vol"]) and np.array_equal(a["grad_transforms"], b["grad_transforms"])
    assert np.array_equal(a["k_vol"], b["k_vol"])


def test_fp32_restatement_stays_close_to_the_yardstick():
    """On the general-rotation cases of the GPU test no decision can flip between the two precisions (asserted), and fp32
    coordinates near 20 carry about 1e-6: the two restatements agree to 1e-5 of the largest element."""
    from tests import util_sa_backward_cases as CS

    for interp_psf in (False, True):
        case = CS.general_case("psf223_vm", interp_psf)
        a, b = CS.reference(case, interp_psf), CS.reference(case, interp_psf, backward32)
        assert min(a["dist"].values()) > 1e-3 and case["sm"].sum() > 200
        for key in ("grad_vol", "grad_transforms"):
            assert np.abs(a[key] - b[key]).max() <= 1e-5 * np.abs(a[key]).max()
            assert np.any(a[key] != b[key])  # and they are two computations, not one


# ---- header and wiring ---------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_abi_8():
    assert {"fsg_slice_acq_backward_f32", "fsg_slice_acq_backward_ws_bytes"} <= set(_lib.PROTOTYPES)
    assert _lib.ABI_VERSION == 8
    text = _lib.HEADER_PATH.read_text()
    assert re.search(r"#define FSG_ABI_VERSION 8\b", text)
    res, args = _lib.PROTOTYPES["fsg_slice_acq_backward_f32"]
    assert len(args) == 22
    assert (Path(_lib.PKG) / "csrc" / "fsg_slice_acq_bwd.hip").exists()
    from fetalsyngen_amd import _build
    assert "fsg_slice_acq_bwd.hip" in _build.SOURCES


@pytest.fixture
def seen(monkeypatch):
    calls = []

    def fwd(transforms, vol, vm, sm, psf, slice_shape, res_slice, need_weight=False, interp_psf=False, semantics="cuda"):
        calls.append(("forward", semantics, interp_psf))
        out = torch.zeros(transforms.shape[0], *slice_shape)
        return (out, torch.ones_like(out)) if need_weight else out

    def bwd(transforms, vol, vm, sm, psf, grad_slices, res_slice, interp_psf=False, need_vol_grad=True,
            need_transforms_grad=True):
        calls.append(("backward", need_vol_grad, need_transforms_grad, interp_psf, tuple(grad_slices.shape)))
        return (torch.full_like(vol, 2.0) if need_vol_grad else None,
                torch.full_like(transforms, 3.0) if need_transforms_grad else None)

    monkeypatch.setattr(SA.K, "slice_acq_forward", fwd)
    monkeypatch.setattr(SA.K, "slice_acq_backward", bwd)
    return calls


def _args(vol_grad, tr_grad):
    return (torch.zeros(2, 3, 4, requires_grad=tr_grad), torch.zeros(1, 1, 6, 6, 6, requires_grad=vol_grad), None, None,
            torch.ones(2, 2, 2), (5, 4), 1.0)


def test_plain_inputs_take_todays_path_only(seen):
    out = SA.slice_acquisition(*_args(False, False), False, False)
    assert out.grad_fn is None and tuple(out.shape) == (2, 1, 5, 4)
    with torch.no_grad():
        SA.slice_acquisition(*_args(True, True), False, True)
    assert seen == [("forward", "cuda", False), ("forward", "cuda", True)]


@pytest.mark.parametrize("vol_grad, tr_grad", [(True, False), (False, True), (True, True)])
def test_grad_requiring_inputs_route_through_the_autograd_function(seen, vol_grad, tr_grad):
    tr, vol, *rest = _args(vol_grad, tr_grad)
    out = SA.slice_acquisition(tr, vol, *rest, False, True)
    assert out.grad_fn is not None and tuple(out.shape) == (2, 1, 5, 4)
    out.sum().backward()
    assert seen == [("forward", "cuda", True), ("backward", vol_grad, tr_grad, True, (2, 5, 4))]
    assert (vol.grad is not None) == vol_grad and (tr.grad is not None) == tr_grad
    if vol_grad:
        assert tuple(vol.grad.shape) == (1, 1, 6, 6, 6) and bool((vol.grad == 2).all())
    if tr_grad:
        assert tuple(tr.grad.shape) == (2, 3, 4) and bool((tr.grad == 3).all())


def test_the_weight_output_is_returned_and_its_gradient_ignored(seen):
    tr, vol, *rest = _args(True, True)
    slices, weight = SA.slice_acquisition(tr, vol, *rest, True, False)
    assert tuple(weight.shape) == (2, 1, 5, 4) and slices.grad_fn is not None
    (slices.sum() + 7 * weight.sum()).backward()
    assert seen[-1][0] == "backward" and bool((vol.grad == 2).all())


def test_torch_semantics_with_grad_raises(seen):
    with pytest.raises(NotImplementedError, match="semantics='cuda'"):
        SA.slice_acquisition(*_args(True, False), False, False, semantics="torch")
    SA.slice_acquisition(*_args(False, False), False, False, semantics="torch")  # without grad: today's path
    assert seen == [("forward", "torch", False)]


# ---- axisangle2mat_autograd -------------------------------------------------------------------------------------------
def test_axisangle2mat_autograd_equals_the_detaching_one_bit_for_bit():
    g = torch.Generator().manual_seed(4)
    big = torch.randn(32, 6, generator=g)
    small = torch.cat((torch.randn(32, 3, generator=g) * 3e-4, torch.randn(32, 3, generator=g)), 1)
    ax = torch.cat((big, small, torch.zeros(1, 6)))
    th2 = (ax[:, :3] ** 2).sum(1)
    assert bool((th2 > rigid.EPS).any()) and bool((th2 <= rigid.EPS).any())  # both branches
    a = axisangle2mat_autograd(ax.clone().requires_grad_())
    assert a.grad_fn is not None and a.dtype == torch.float32
    assert torch.equal(a.detach(), rigid.axisangle2mat(ax))


def test_axisangle2mat_autograd_gradcheck_away_from_the_branch_point():
    g = torch.Generator().manual_seed(6)
    big = torch.randn(3, 6, generator=g, dtype=torch.float64).requires_grad_()
    small = (torch.randn(3, 6, generator=g, dtype=torch.float64) * 1e-4).requires_grad_()
    assert bool(((big[:, :3] ** 2).sum(1) > 0.01).all()) and bool(((small[:, :3] ** 2).sum(1) < 1e-7).all())
    assert torch.autograd.gradcheck(axisangle2mat_autograd, (big,))
    assert torch.autograd.gradcheck(axisangle2mat_autograd, (small,))
