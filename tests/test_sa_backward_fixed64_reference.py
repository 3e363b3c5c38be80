"""The rule of the deterministic grad_vol of the slice-acquisition backward (include/fsg_hip.h, fsg_slice_acq_backward_det_f32;
DESIGN.md section 20), pinned on its numpy restatement tests/util_sa_backward_fixed64.py, with the refusals of the entry point
(they come before any device call, so they run here) and the wiring of the Python layers.  tests/test_sa_backward_det_gpu.py
then holds the kernels to the restatement bit for bit.  No GPU here."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from fetalsyngen_amd import _lib
from fetalsyngen_amd.generator.artifacts.svort import slice_acq as SA
from tests import util_fixed64 as X
from tests import util_sa_backward_cases as CS
from tests import util_sa_backward_fixed64 as FX
from tests.util_sa_backward64 import backward32

f32 = np.float32
U = 2.0 ** -24
NVOX = int(np.prod(CS.VS))
MODES = pytest.mark.parametrize("interp_psf", [False, True], ids=["linear", "nearest_psf"])


def _contrib(case, interp_psf):
    return FX.contributions(case["tr"], CS.VS, case["vm"], case["psf"], case["g"], case["sm"], case["res"], interp_psf)


# ---- the restatement itself ------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("kind, name", [("exact", "psf335"), ("exact", "psf223_big"), ("general", "psf335"), ("general", "psf223_vm")])
def test_contributions_are_those_of_backward32(kind, name, interp_psf):
    """Same formula, two writings: backward32 adds the float32 contributions in float64, so the float64 sum of the ones listed
    here agrees with it to the rounding of K float64 additions, and the counts agree exactly."""
    case = CS.exact_case(name, True) if kind == "exact" else CS.general_case(name, interp_psf)
    r = CS.reference(case, interp_psf, backward32)
    idx, c = _contrib(case, interp_psf)
    k, s = np.zeros(NVOX, np.int64), np.zeros(NVOX)
    np.add.at(k, idx, 1)
    np.add.at(s, idx, c.astype(np.float64))
    assert np.array_equal(k.reshape(CS.VS), r["k_vol"]) and k.max() > 1
    assert np.all(np.abs(s.reshape(CS.VS) - r["grad_vol"]) <= (r["k_vol"] + 1) * 2.0 ** -52 * r["s_vol"])


@MODES
def test_result_does_not_depend_on_the_order_where_a_float_sum_does(interp_psf):
    case = CS.exact_case("psf335", False)
    idx, c = _contrib(case, interp_psf)
    want = FX.accumulate(idx, c, NVOX)
    rng = np.random.default_rng(11)
    floats = []
    for _ in range(3):
        p = rng.permutation(len(idx))
        assert np.array_equal(FX.accumulate(idx[p], c[p], NVOX), want)
        acc = np.zeros(NVOX, f32)
        np.add.at(acc, idx[p], c[p])  # unbuffered: a float32 running sum per voxel in the order given
        floats.append(acc)
    assert np.count_nonzero(want) > 800
    # the premise: the same contributions in another order give other float32 sums on this very case
    assert not np.array_equal(floats[0], floats[1]) or not np.array_equal(floats[0], floats[2])


@MODES
@pytest.mark.parametrize("masks", [False, True], ids=["nomask", "masks"])
@pytest.mark.parametrize("name", list(CS.EXACT))
def test_exact_geometry_against_float64(name, interp_psf, masks):
    """The bound of the GPU test: the float backward's (K + 16) * 2^-24 * S plus half a quantum per contribution."""
    case = CS.exact_case(name, masks)
    r = CS.reference(case, interp_psf)
    got = FX.of_case(case, interp_psf)
    assert np.array_equal(got["k_vol"], r["k_vol"])
    err = np.abs(got["grad_vol"].astype(np.float64) - r["grad_vol"])
    assert np.all(err <= (r["k_vol"] + 16) * U * r["s_vol"] + r["k_vol"] * 2.0 ** -73)
    assert got["grad_vol"].dtype == f32 and not np.signbit(got["grad_vol"][r["k_vol"] == 0]).any()


@MODES
@pytest.mark.parametrize("k", [-20, 7, 20])
def test_grad_scale_is_exact(interp_psf, k):
    """grad_slices and grad_scale times the same 2^k: the same integers, and the result times exactly 2^k."""
    case = CS.exact_case("psf223", True)
    base = FX.of_case(case, interp_psf)["grad_vol"]
    scaled = FX.of_case(dict(case, g=case["g"] * f32(2.0 ** k)), interp_psf, grad_scale=2.0 ** k)["grad_vol"]
    assert np.count_nonzero(base) > 100 and np.array_equal(scaled, base * f32(2.0 ** k))


# ---- header, exports, refusals ------------------------------------------------------------------------------------------
NAMES = ("fsg_slice_acq_backward_det_f32", "fsg_slice_acq_backward_det_ws_bytes")


def test_header_states_the_rule_and_the_abi_stays_8():
    text = _lib.HEADER_PATH.read_text()
    assert re.search(r"#define FSG_ABI_VERSION 8\b", text) and _lib.ABI_VERSION == 8
    assert set(NAMES) <= set(_lib.PROTOTYPES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NAMES)
    _, args = _lib.PROTOTYPES["fsg_slice_acq_backward_det_f32"]
    assert len(args) == len(_lib.PROTOTYPES["fsg_slice_acq_backward_f32"][1]) + 3 == 25
    for phrase in ("Q = rint_half_even(c * 2^F / grad_scale)", "sum(hi) * 2^L + sum(lo)", "gives +0.0f",
                   "never derived from the data", "grad_transforms is untouched", "16 bytes per voxel"):
        assert phrase in text, phrase
    assert (_lib.SA.DET_FRAC_BITS, _lib.SA.DET_LIMB_BITS) == (X.F, X.L)


def _entry(lib, gv=64, gt=0, ws=0, ws_bytes=0, det=128, det_bytes=None, scale=1.0, mode=None, vol=16):
    """The entry point on made-up addresses: every call here must be refused before anything is read or launched."""
    p = C.c_void_p
    need = lib.fsg_slice_acq_backward_det_ws_bytes(*CS.VS)
    return lib.fsg_slice_acq_backward_det_f32(p(8), p(vol), p(0), p(24), 2, 2, 3, p(32), p(0), p(gv), p(gt), *CS.VS, 5, 13, 11,
                                              1.5, _lib.SA.LINEAR if mode is None else mode, p(ws), ws_bytes, p(det),
                                              need if det_bytes is None else det_bytes, scale, p(0))


def test_refusal_table():
    lib = _lib.load()
    assert lib.fsg_slice_acq_backward_det_ws_bytes(*CS.VS) == 16 * NVOX
    assert lib.fsg_slice_acq_backward_det_ws_bytes(0, 18, 22) == 0 and lib.fsg_slice_acq_backward_det_ws_bytes(20, 18, -1) == 0
    need = 16 * NVOX
    for label, want, kw in (
        ("FSG_SA_TORCH", _lib.E_BADARG, dict(mode=_lib.SA.TORCH)),
        ("both outputs NULL", _lib.E_BADARG, dict(gv=0, gt=0)),
        ("no vol", _lib.E_BADARG, dict(vol=0)),
        ("grad_scale 3", _lib.E_BADARG, dict(scale=3.0)),
        ("grad_scale 2^21", _lib.E_BADARG, dict(scale=2.0 ** 21)),
        ("grad_scale 2^-21", _lib.E_BADARG, dict(scale=2.0 ** -21)),
        ("grad_scale 0", _lib.E_BADARG, dict(scale=0.0)),
        ("grad_scale -1", _lib.E_BADARG, dict(scale=-1.0)),
        ("grad_scale nan", _lib.E_BADARG, dict(scale=float("nan"))),
        ("grad_scale inf", _lib.E_BADARG, dict(scale=float("inf"))),
        ("short det_ws", _lib.E_BADARG, dict(det_bytes=need - 8)),
        ("no det_ws", _lib.E_BADARG, dict(det=0)),
        ("misaligned det_ws", _lib.E_ALIGN, dict(det=132)),
        ("grad_transforms without ws", _lib.E_BADARG, dict(gt=256)),
        ("grad_transforms with a short ws", _lib.E_BADARG, dict(gt=256, ws=512, ws_bytes=5 * 48 - 4)),
        ("grad_transforms with a misaligned ws", _lib.E_ALIGN, dict(gt=256, ws=516, ws_bytes=5 * 48)),
    ):
        assert _entry(lib, **kw) == want, label


def test_python_layer_refuses_before_it_touches_a_device():
    from fetalsyngen_amd import kernels as K

    tr, vol, psf, g = torch.zeros(1, 3, 4), torch.zeros(4, 4, 4), torch.ones(2, 2, 2), torch.zeros(1, 4, 4)
    for bad in (3.0, 2.0 ** 21, 2.0 ** -21, 0.0, float("nan")):
        with pytest.raises(ValueError, match="grad_scale"):
            K.slice_acq_backward(tr, vol, None, None, psf, g, 1.0, deterministic=True, grad_scale=bad)
    assert K.slice_acq_backward(tr, vol, None, None, psf, g, 1.0, need_vol_grad=False, need_transforms_grad=False,
                                deterministic=True) == (None, None)


# ---- wiring -----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def seen(monkeypatch):
    calls = []

    def fwd(transforms, vol, vm, sm, psf, slice_shape, res_slice, need_weight=False, interp_psf=False, semantics="cuda"):
        calls.append(("forward", semantics))
        out = torch.zeros(transforms.shape[0], *slice_shape)
        return (out, torch.ones_like(out)) if need_weight else out

    def bwd(transforms, vol, vm, sm, psf, grad_slices, res_slice, interp_psf=False, need_vol_grad=True,
            need_transforms_grad=True, **kw):
        calls.append(("backward", kw))
        return (torch.full_like(vol, 2.0) if need_vol_grad else None,
                torch.full_like(transforms, 3.0) if need_transforms_grad else None)

    monkeypatch.setattr(SA.K, "slice_acq_forward", fwd)
    monkeypatch.setattr(SA.K, "slice_acq_backward", bwd)
    return calls


def _args(grad=True):
    return (torch.zeros(2, 3, 4, requires_grad=grad), torch.zeros(1, 1, 6, 6, 6, requires_grad=grad), None, None,
            torch.ones(2, 2, 2), (5, 4), 1.0, False, False)


def test_a_call_that_does_not_ask_runs_todays_call(seen):
    SA.slice_acquisition(*_args()).sum().backward()  # the reference's positional signature
    SA.slice_acquisition(*_args(), deterministic=False, grad_scale=4.0).sum().backward()
    assert seen == [("forward", "cuda"), ("backward", {})] * 2


def test_deterministic_reaches_the_backward_only(seen):
    tr, vol, *rest = _args()
    SA.slice_acquisition(tr, vol, *rest, deterministic=True).sum().backward()
    SA.slice_acquisition(tr, vol, *rest, None, True, 0.25).sum().backward()  # semantics, deterministic, grad_scale in place
    assert seen == [("forward", "cuda"), ("backward", dict(deterministic=True, grad_scale=1.0)),
                    ("forward", "cuda"), ("backward", dict(deterministic=True, grad_scale=0.25))]
    assert bool((vol.grad == 4).all()) and bool((tr.grad == 6).all())
    del seen[:]
    out = SA.slice_acquisition(*_args(False), deterministic=True)  # nothing to differentiate: the plain forward launch
    assert out.grad_fn is None and seen == [("forward", "cuda")]


def test_none_resolves_through_the_keyed_scope(seen, monkeypatch):
    asked = []
    monkeypatch.setattr(SA._rng, "in_keyed_scope", lambda: asked.append(1) or True)
    SA.slice_acquisition(*_args()).sum().backward()
    assert asked and seen[-1] == ("backward", dict(deterministic=True, grad_scale=1.0))
    SA.slice_acquisition(*_args(), deterministic=False).sum().backward()
    assert seen[-1] == ("backward", {})
    # under "torch" semantics None is the float rule, as for the adjoint: the plain launch, and the usual refusal of a gradient
    SA.slice_acquisition(*_args(False), semantics="torch")
    assert seen[-1] == ("forward", "torch")
    with pytest.raises(NotImplementedError):
        SA.slice_acquisition(*_args(), semantics="torch")
    monkeypatch.setattr(SA._rng, "in_keyed_scope", lambda: False)
    SA.slice_acquisition(*_args()).sum().backward()
    assert seen[-1] == ("backward", {})


def test_true_under_torch_semantics_raises(seen):
    for grad in (False, True):
        with pytest.raises(ValueError, match="CUDA semantics"):
            SA.slice_acquisition(*_args(grad), semantics="torch", deterministic=True)
    prev = SA.set_semantics("torch")
    try:
        with pytest.raises(ValueError, match="CUDA semantics"):
            SA.slice_acquisition(*_args(False), deterministic=True)
    finally:
        SA.set_semantics(prev)
    assert seen == []
