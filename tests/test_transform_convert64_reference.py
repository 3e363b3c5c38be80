"""CPU: the restatement of the pose-conversion kernels (tests/util_transform_convert64.py) is itself checked -- against rigid.py's
host conversions (pinned to fixtures of a CPU run of the reference), against central differences, and by three mutants -- and
the parts of the feature that need no device: the header, the build list, the refusals of the four entries, the namespace.
DESIGN.md section 21."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import util_transform_convert64 as U

REPO = Path(__file__).resolve().parent.parent
ENTRIES = ("fsg_axisangle2mat_f32", "fsg_axisangle2mat_backward_f32", "fsg_mat2axisangle_f32", "fsg_mat2axisangle_backward_f32")


@pytest.fixture(scope="module")
def C():
    return U.cases()


# ---- the cases are what the tests need -----------------------------------------------------------------------------------------
def test_cases_cover_every_branch(C):
    keep, branch, flipped = C["keep"], C["branch"], C["flipped"]
    assert len(keep) == 257 and (~keep).sum() <= 0.05 * len(keep)
    per_branch = [int((keep & (branch == b)).sum()) for b in range(4)]
    flips = [int((keep & flipped & (branch == b)).sum()) for b in range(4)]
    print("kept", int(keep.sum()), "per branch", per_branch, "with w < 0 before the flip", flips)
    assert min(per_branch) >= 20
    assert min(flips[1:]) >= 1
    ang = np.linalg.norm(C["ax"][:, :3].astype(np.float64), axis=1)
    assert ang.min() >= 0.05 - 1e-6 and ang.max() <= 3.05 + 1e-6 and np.abs(C["ax"][:, 3:]).max() <= 20
    th2 = (C["small_ax"].astype(np.float32)[:, :3] ** 2).sum(1)
    assert th2[0] == 0 and np.allclose(th2[1:], (1.4e-7, 9.0e-7), rtol=1e-5) and (th2 < np.float32(1e-6)).all()
    # the matrices of the small poses take mat2axisangle's small branch
    _, w, x, y, z, _ = U.quaternion(C["small_mat"])
    assert ((x * x + y * y + z * z) <= 1e-6).all()
    assert not any(v.flags.writeable for v in C.values())


def test_float_compare_with_the_double_literal_is_the_float_compare():
    """No float32 lies between float32(1e-6) and the double 1e-6.  So `v > 1e-6` in double and `v > float32(1e-6)` agree for
    every float32 v, and `v < 1e-6` and `v < float32(1e-6)` for every v but float32(1e-6) itself, which is below the double."""
    f = np.float32(1e-6)
    down, up = np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(1))
    assert float(f) < 1e-6 < float(up)
    for v in (down, f, up):
        assert (float(v) > 1e-6) == bool(v > f)
    for v in (down, up):
        assert (float(v) < 1e-6) == bool(v < f)
    assert float(f) < 1e-6 and not bool(f < f)  # the one value at which `r22 < 1e-6` and rigid.py's float32 compare part


# ---- against rigid.py ------------------------------------------------------------------------------------------------------------
def test_forwards_agree_with_the_host_conversions(C):
    from fetalsyngen_amd.generator.artifacts.svort import rigid
    E_CPU = U.E_CPU
    ax = np.concatenate((C["ax"], C["small_ax"]))
    ref = U.axisangle2mat(ax)
    got = rigid.axisangle2mat(torch.from_numpy(ax)).numpy()
    e = U.rel_err(U.rot_part(got), U.rot_part(ref))
    print("axisangle2mat: rigid.py against float64 %.3e, bound %.3e" % (e, 4 * E_CPU["a2m"]))
    assert e <= 4 * E_CPU["a2m"]
    assert np.array_equal(U.trans_part(got), U.trans_part(ref).astype(np.float32))
    assert np.array_equal(U.trans_part(ref), ax[:, 3:].astype(np.float64))  # bit-equal: copied
    k = C["keep"]
    mat = np.concatenate((C["mat"][k], C["small_mat"]))
    ref = U.mat2axisangle(mat)
    got = rigid.mat2axisangle(torch.from_numpy(mat)).numpy()
    e = U.rel_err(U.rot_part(got), U.rot_part(ref))
    print("mat2axisangle: rigid.py against float64 %.3e, bound %.3e" % (e, 4 * E_CPU["m2a"]))
    assert e <= 4 * E_CPU["m2a"]
    assert np.array_equal(U.trans_part(got), mat[:, :, 3]) and np.array_equal(U.trans_part(ref), mat[:, :, 3].astype(np.float64))


def test_round_trip(C):
    k = C["keep"]
    ax = C["ax"][k].astype(np.float64)
    assert np.abs(U.mat2axisangle(U.axisangle2mat(ax)) - ax).max() <= 1e-6


def test_restatement_writes_every_element(C):
    for dt in (np.float64, np.float32):
        assert np.isfinite(U.axisangle2mat(np.concatenate((C["ax"], C["small_ax"])), dt)).all()
        assert np.isfinite(U.mat2axisangle_backward(np.concatenate((C["mat"], C["small_mat"])),
                                                    np.concatenate((C["gax"], C["small_gax"])), dt)).all()


# ---- against central differences ---------------------------------------------------------------------------------------------------
H = 1e-6


def _cd_axisangle2mat(ax, g):
    out = np.zeros((len(ax), 6))
    for j in range(6):
        d = np.zeros(6)
        d[j] = H
        out[:, j] = ((U.axisangle2mat(ax + d) - U.axisangle2mat(ax - d)) / (2 * H) * g).sum((1, 2))
    return out


def _cd_mat2axisangle(m, g):
    out = np.zeros((len(m), 3, 4))
    for i in range(3):
        for j in range(4):  # all 12 entries free
            d = np.zeros((3, 4))
            d[i, j] = H
            out[:, i, j] = ((U.mat2axisangle(m + d) - U.mat2axisangle(m - d)) / (2 * H) * g).sum(1)
    return out


@pytest.fixture(scope="module")
def differences(C):
    k = C["keep"]
    ax = np.concatenate((C["ax"], C["small_ax"])).astype(np.float64)  # both branches
    gm = np.concatenate((C["gmat"], C["small_gmat"])).astype(np.float64)
    m, ga = C["mat"][k].astype(np.float64), C["gax"][k].astype(np.float64)  # kept rows only: the small branch is no derivative
    return dict(ax=ax, gm=gm, m=m, ga=ga, a2m=_cd_axisangle2mat(ax, gm), m2a=_cd_mat2axisangle(m, ga))


def _miss(got, cd):
    return float(np.abs(got - cd).max() / np.abs(cd).max())


def test_backward_rules_are_derivatives(differences):
    d = differences
    e1 = _miss(U.axisangle2mat_backward(d["gm"], d["ax"]), d["a2m"])
    e2 = _miss(U.mat2axisangle_backward(d["m"], d["ga"]), d["m2a"])
    print("central differences: axisangle2mat %.2e, mat2axisangle %.2e of the largest entry" % (e1, e2))
    assert e1 <= 1e-6 and e2 <= 1e-6


@pytest.mark.parametrize("mutant", ["no_sign_restore", "swap23", "no_over_theta"])
def test_mutants_fail_the_difference_check(differences, mutant):
    d = differences
    if mutant == "no_over_theta":
        e = _miss(U.axisangle2mat_backward(d["gm"], d["ax"], mutant=mutant), d["a2m"])
    else:
        e = _miss(U.mat2axisangle_backward(d["m"], d["ga"], mutant=mutant), d["m2a"])
    print(mutant, "%.3f of the largest entry" % e)
    assert e > 1e-3


def test_small_norm_backward_is_finite_and_near_the_derivative(C):
    """The quirk: for tmp <= 1e-6 the rule differentiates a fac the forward does not use, with a floored sine.  The term it
    gets wrong is of second order in the angle: on these rows the rule is finite (the zero pose included, where theta / si is
    0 / 0) and misses the differences of the forward by 2.8e-8 of the largest entry, thirty times what a derivative misses by.
    The tests hold the kernels to the rule on such rows, not to the differences."""
    m, g = C["small_mat"].astype(np.float64), C["small_gax"].astype(np.float64)
    rule = U.mat2axisangle_backward(m, g)
    assert np.isfinite(rule).all()
    miss = _miss(rule[1:], _cd_mat2axisangle(m[1:], g[1:]))
    print("small-norm rule against central differences: %.2e of the largest entry" % miss)
    assert miss < 1e-6


def test_e_cpu_constants_are_the_restatements(C):
    E_CHAIN, E_CPU, R_A2M_BWD = U.E_CHAIN, U.E_CPU, U.R_A2M_BWD
    e = U.e_cpu()
    print({k: "%.3e" % v for k, v in e.items()})
    for k, const in E_CPU.items():
        # the float32 sine, cosine and arctangent of the host's numpy differ between builds in the last unit: the constants
        # were measured once, and a host must find the same figure within that play
        assert 0.5 * const <= e[k] <= 1.25 * const, (k, e[k], const)
    assert abs(e["a2m_bwd_R"] - R_A2M_BWD) <= 1e-3 * R_A2M_BWD
    ch = U.chain_case()
    assert len(ch["t"]) >= 100
    for leaf in (0, 1):
        for part, name in ((slice(0, 3), "chain_rot"), (slice(3, 6), "chain_trans")):
            got = U.rel_err(ch["g32"][leaf][:, part], ch["g64"][leaf][:, part])
            assert got <= 1.25 * E_CHAIN[name], (leaf, name, got)


# ---- header, build list, refusals, namespace -------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_abi_stays_8():
    from fetalsyngen_amd import _build, _lib

    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "fsg_hip.h").read_text(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and args[-2:] == [ctypes.c_int, ctypes.c_void_p]
        assert len(args) == (5 if "backward" in name else 4)
    assert _lib.ABI_VERSION == 8
    assert "fsg_transform_convert.hip" in _build.SOURCES and (_build.CSRC / "fsg_transform_convert.hip").exists()
    assert "-ffp-contract=off" in _build.FLAGS


def test_entries_refuse_before_any_launch():
    """no device is needed: every refusal, and n == 0, returns before the first launch"""
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    null, a, b, c = (ctypes.c_void_p(v) for v in (0, 1 << 20, 2 << 20, 3 << 20))
    big = (2 ** 31 - 1) // 12 + 1
    for name in ENTRIES:
        fn = getattr(lib, name)
        three = "backward" in name
        ptrs = (a, b, c) if three else (a, b)
        nulls = (null,) * len(ptrs)
        assert fn(*nulls, 0, null) == 0 and fn(*ptrs, 0, null) == 0  # nothing to do
        assert fn(*ptrs, -1, null) == _lib.E_BADARG
        for i in range(len(ptrs)):
            assert fn(*(null if j == i else p for j, p in enumerate(ptrs)), 4, null) == _lib.E_BADARG, (name, i)
        assert fn(*ptrs, big, null) == _lib.E_TOOBIG
    # an output that shares a byte with an input (n = 4: 192 bytes of matrices, 96 of axis-angle rows)
    at = lambda v: ctypes.c_void_p((1 << 20) + v)  # noqa: E731
    assert lib.fsg_axisangle2mat_f32(a, a, 4, null) == _lib.E_BADARG
    assert lib.fsg_axisangle2mat_f32(a, at(95), 4, null) == _lib.E_BADARG  # the output begins in the input's last byte
    assert lib.fsg_axisangle2mat_f32(at(191), a, 4, null) == _lib.E_BADARG  # the input begins in the output's last byte
    assert lib.fsg_mat2axisangle_f32(a, at(191), 4, null) == _lib.E_BADARG
    assert lib.fsg_mat2axisangle_f32(at(95), a, 4, null) == _lib.E_BADARG
    assert lib.fsg_axisangle2mat_backward_f32(a, b, a, 4, null) == _lib.E_BADARG  # grad_mat
    assert lib.fsg_axisangle2mat_backward_f32(a, b, at((1 << 20) + 95), 4, null) == _lib.E_BADARG  # axisangle
    assert lib.fsg_mat2axisangle_backward_f32(a, b, at(191), 4, null) == _lib.E_BADARG  # mat
    assert lib.fsg_mat2axisangle_backward_f32(a, b, at((1 << 20) - 191), 4, null) == _lib.E_BADARG  # grad_axisangle


def test_front_end_refuses_cpu_tensors():
    from fetalsyngen_amd import kernels as K

    for fn, args in ((K.axisangle2mat, (torch.zeros(2, 6),)), (K.mat2axisangle, (torch.zeros(2, 3, 4),)),
                     (K.axisangle2mat_backward, (torch.zeros(2, 3, 4), torch.zeros(2, 6))),
                     (K.mat2axisangle_backward, (torch.zeros(2, 3, 4), torch.zeros(2, 6)))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(*args)
    # the two tensors of a backward call must share a device: the check itself, on tensors that need none
    K._tc_same(2, 2, "a", "b", torch.zeros(1), torch.zeros(1))
    with pytest.raises(ValueError, match="is on"):
        K._tc_same(2, 2, "a", "b", torch.zeros(1), torch.zeros(1, device="meta"))
    with pytest.raises(ValueError, match="rows"):
        K._tc_same(2, 3, "a", "b", torch.zeros(1), torch.zeros(1))


def test_namespace_keeps_the_host_names():
    from fetalsyngen_amd.generator.artifacts import svort
    from fetalsyngen_amd.generator.artifacts.svort import autograd, rigid, transform_convert

    assert svort.axisangle2mat is rigid.axisangle2mat and svort.mat2axisangle is rigid.mat2axisangle
    assert svort.RigidTransform is rigid.RigidTransform
    assert svort.transform_convert is transform_convert and svort.DeviceRigidTransform is transform_convert.DeviceRigidTransform
    assert svort.axisangle2mat_autograd is autograd.axisangle2mat_autograd
    for name in ("Axisangle2MatFunction", "Mat2AxisangleFunction", "axisangle2mat", "mat2axisangle"):
        assert hasattr(transform_convert, name)
    ax = torch.from_numpy(U.cases()["ax"][:3].copy()).requires_grad_()
    assert svort.RigidTransform(ax).matrix().grad_fn is None  # the host class still detaches
    with pytest.raises(NotImplementedError):
        svort.RigidTransform(ax).mean(simple_mean=False)
