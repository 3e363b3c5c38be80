"""CPU: the restatement of the grouped registration and of the stack alignment (tests/util_svr_group64.py)
held to the convention stated directly and to central differences, with three mutants; the float64 figures of the two
experiments and the all-stacks row that pins why the moving stack is left out of its target; and the host side of the new
entries (header, build list, refusals before any launch, the parsing of `groups`, both launch sequences of `svort.svr`).

Everything above "the host side of the new entries" exercises only the restatement; the tests below it touch the library or
the front-ends and fail without them."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests import util_svr64 as U
from tests import util_svr_group64 as GU
from tests import util_transform_convert64 as TC

ROOT = Path(__file__).resolve().parents[1]
F32, F64 = np.float32, np.float64
PHI = np.array([[0.21, -0.13, 0.08, 0.6, -0.4, 0.3], [-0.05, 0.3, 0.11, -1.2, 0.7, 0.25]])
GROUP = [0, 1, 0, -1, 1]


def _base():
    return TC.axisangle2mat(U.capability_case()["true"], F64)


# ---- compose ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", (PHI, np.zeros((2, 6))), ids=("general", "zero"))
def test_compose_is_the_convention_and_its_jac_the_derivative(phi):
    tr_err, jac_err = GU.fd_error(phi, _base(), GROUP)
    print("transforms", tr_err, "jac against central differences", jac_err)  # measured 4.4e-16 and 4.3e-10 at most
    assert tr_err <= 1e-14 and jac_err <= GU.JAC_FD_BOUND
    _, jac = GU.compose(*GU.group_operands(phi, F64), _base(), GROUP, F64)
    assert np.all(jac[3] == 0) and np.abs(jac[0]).max() > 0.1  # the fixed slice has no derivative


@pytest.mark.parametrize("mutant", ("old_R", "no_dd", "RQ"))
def test_compose_mutants_fail_the_difference_check(mutant):
    tr_err, jac_err = GU.fd_error(PHI, _base(), GROUP, mutant)
    print(mutant, tr_err, jac_err)
    assert tr_err > 1e-3 or jac_err > 1e-3


@pytest.mark.parametrize("ft", (F32, F64))
def test_zero_increment_gives_the_base_bit_for_bit(ft):
    base = _base().astype(ft)
    tr, jac = GU.compose(*GU.group_operands(np.zeros((2, 6), ft), ft), base, GROUP, ft)
    assert tr.dtype == ft and np.array_equal(tr.view(np.uint32 if ft is F32 else np.uint64), base.view(np.uint32 if ft is F32 else np.uint64))
    # at 0 the rotation columns of the Jacobian are the generators and the translation columns the rows of R
    assert np.allclose(jac[0, [3, 7, 11], 3:], base[0, :, :3].T, atol=1e-6)


def test_out_of_range_ids_are_fixed():
    base = _base().astype(F32)
    tr, jac = GU.compose(*GU.group_operands(PHI.astype(F32), F32), base, [0, 2, -1, 7, 1], F32)
    for s in (1, 2, 3):
        assert np.array_equal(tr[s].view(np.uint32), base[s].view(np.uint32)) and np.all(jac[s] == 0)
    assert not np.array_equal(tr[0], base[0]) and not np.array_equal(tr[4], base[4])


# ---- the reduce ---------------------------------------------------------------------------------------------------------------
def test_group_reduce_is_the_sum_in_the_listed_order():
    rng = np.random.default_rng(4)
    stats = rng.standard_normal((6, 32)) * 10.0 ** rng.integers(-8, 8, (6, 32))
    members, offsets = np.array([4, 0, 2, 5, 1], np.int32), np.array([0, 3, 3, 5], np.int32)  # group 1 is empty; slice 3 in none
    got = GU.group_reduce(stats, members, offsets)
    assert np.array_equal(got[0], ((0.0 + stats[4]) + stats[0]) + stats[2])
    assert np.all(got[1] == 0) and not np.signbit(got[1]).any()
    assert np.array_equal(got[2], (0.0 + stats[5]) + stats[1])
    back = GU.group_reduce(stats, np.array([2, 0, 4, 5, 1], np.int32), offsets)  # another order: the same up to rounding only
    assert np.allclose(back, got, rtol=1e-12) and not np.array_equal(back, got)


def test_singleton_groups_at_round_0_carry_the_per_slice_cost_slots():
    c = U.capability_case()
    n = c["start"].shape[0]
    base = TC.axisangle2mat(c["start"], F32)
    per = U.stats_device(U.pixels(base, U.jacobian(c["start"], F32), c["vol"], c["psf"], c["y"], None, None, c["res"], 0.5, F32)["terms"])
    _, group, members, offsets = GU.relabel(range(n))
    tr, jac = GU.compose(*GU.group_operands(np.zeros((n, 6), F32), F32), base, group, F32)
    grouped = GU.group_reduce(GU.slice_stats(tr, jac, c["vol"], c["psf"], c["y"], None, None, c["res"], 0.5, F32, True), members, offsets)
    assert np.array_equal(grouped[:, 27:30].view(np.uint64), per[:, 27:30].view(np.uint64)) and per[:, 29].min() > 0
    assert not np.array_equal(grouped[:, :27], per[:, :27])  # other parameters: another H and g


# ---- the two experiments in float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (1, 2, 3))
def test_float64_grouped_solve_recovers_one_motion_and_beats_per_slice_under_noise(seed):
    c = GU.group_case(seed)
    rot0, trans0 = GU.pose_errors(c["start"], c["true"])
    rot, trans = GU.run_a(seed, 0.0)[:2]
    print("start", rot0, trans0, "sigma 0", rot, trans)
    assert 0.019 < rot0 < 0.03 and 0.69 < trans0 < 0.85
    assert rot < 1e-13 and trans < 1e-13  # measured 5e-16 / 4.8e-15 at most
    grouped, single = GU.run_a(seed, 0.03)[:2], GU.run_a_per_slice(seed, 0.03)
    print("sigma 0.03 grouped", grouped, "per slice", single)
    assert grouped[1] <= GU.A_RATIO64 * single[1]  # measured 0.100, 0.308, 0.138
    assert single[1] > trans0  # 81 noisy pixels: the per-slice fit ends further away than it started


def test_float64_two_groups_in_one_batch():
    rot, trans, _, st = GU.run_a(1, 0.0, two_groups=True)
    assert rot < 1e-13 and trans < 1e-13 and st["cost"].shape == (GU.N_ITER_A + 1, 2)


@pytest.mark.parametrize("seed", (1, 2))
def test_float64_alignment_lowers_the_translation_error(seed):
    errs, _ = GU.run_b(seed)
    print([("%.3g" % r, "%.3g" % t) for r, t in errs])
    assert errs[-1][1] < GU.B_START_FRACTION * errs[0][1]  # measured 0.056 and 0.054 of the start
    assert errs[1][1] < 0.2 * errs[0][1]  # round 0 alone, against the template only


def test_all_stacks_target_does_not_lower_the_translation_error():
    """the same groups against a reconstruction of ALL stacks (6 CG iterations, lam 0): DESIGN.md section 23's failure"""
    errs, _ = GU.run_b(1, all_stacks=True)
    print([("%.3g" % r, "%.3g" % t) for r, t in errs])  # measured 0.833 -> 0.864, 0.875, 0.880
    assert all(e[1] >= errs[0][1] for e in errs[1:])


def test_alignment_leaves_the_template_alone():
    c = GU.align_case(1)
    trs = GU.align_stacks(c["start"], c["y"], c["stack"], c["psf"], c["ss"], c["res"], n_rounds=1)
    assert np.array_equal(trs[-1][:GU.N_STACK], c["start"][:GU.N_STACK]) and not np.array_equal(trs[-1][GU.N_STACK:], c["start"][GU.N_STACK:])


def test_fp32_restatement_gives_the_recorded_figures():
    for seed, (rot, trans) in GU.A32.items():
        r, t = GU.run_a(seed, 0.0, F32)[:2]
        print("A32", seed, r, t)
        assert 0.98 * rot <= r <= rot and 0.98 * trans <= t <= trans
        r, t = GU.run_a(seed, 0.0, F32, through_poses=True)[:2]
        assert 0.98 * GU.A32_POSES[seed][0] <= r <= GU.A32_POSES[seed][0] and 0.98 * GU.A32_POSES[seed][1] <= t <= GU.A32_POSES[seed][1]
    r, t = GU.run_a(1, 0.0, F32, two_groups=True, through_poses=True)[:2]
    assert 0.98 * GU.A32_POSES_TWO[0] <= r <= GU.A32_POSES_TWO[0] and 0.98 * GU.A32_POSES_TWO[1] <= t <= GU.A32_POSES_TWO[1]
    for seed, trans in GU.B32.items():
        t = GU.run_b(seed, ft=F32)[0][-1][1]
        print("B32", seed, t)
        assert 0.98 * trans <= t <= trans


# ---- the host side of the new entries -----------------------------------------------------------------------------------------
ENTRIES = ("fsg_svr_compose_f32", "fsg_svr_group_reduce_f64")


def test_header_build_list_and_abi():
    from fetalsyngen_amd import _build, _lib

    text = (ROOT / "include" / "fsg_hip.h").read_text()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", text) and name in _lib.PROTOTYPES
    assert _lib.ABI_VERSION == 8 and _lib.load().fsg_abi_version() == 8  # entries added, nothing older changed
    assert "fsg_svr_group.hip" in _build.SOURCES and (ROOT / "fetalsyngen_amd" / "csrc" / "fsg_svr_group.hip").exists()
    assert _lib.PROTOTYPES["fsg_svr_compose_f32"][1][6:8] == [ctypes.c_int, ctypes.c_int]


def _compose_call(lib, **kw):
    a = dict(gm=1 << 24, gj=2 << 24, base=3 << 24, group=4 << 24, tr=5 << 24, jac=6 << 24, n=5, G=2)
    a.update(kw)
    p = ctypes.c_void_p
    return lib.fsg_svr_compose_f32(p(a["gm"]), p(a["gj"]), p(a["base"]), p(a["group"]), p(a["tr"]), p(a["jac"]), a["n"], a["G"], None)


def _reduce_call(lib, **kw):
    a = dict(stats=1 << 24, members=2 << 24, offsets=3 << 24, gstats=4 << 24, n=5, n_members=4, G=3)
    a.update(kw)
    p = ctypes.c_void_p
    return lib.fsg_svr_group_reduce_f64(p(a["stats"]), p(a["members"]), p(a["offsets"]), p(a["gstats"]), a["n"], a["n_members"], a["G"],
                                        None)


def test_entries_refuse_before_any_launch():
    """no device is needed: every refusal returns before the first launch (the addresses are made up)"""
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    BAD, BIG, ALIGN = _lib.E_BADARG, _lib.E_TOOBIG, _lib.E_ALIGN
    for key in ("gm", "gj", "base", "group", "tr", "jac"):
        assert _compose_call(lib, **{key: 0}) == BAD, key
        assert _compose_call(lib, **{key: (9 << 24) + 2}) == ALIGN, key
    for kw in (dict(n=0), dict(n=-3), dict(G=0), dict(G=-1)):
        assert _compose_call(lib, **kw) == BAD, kw
    for kw in (dict(n=65536), dict(G=65536)):
        assert _compose_call(lib, **kw) == BIG, kw
    n, G = 5, 2
    for kw in (dict(tr=3 << 24), dict(tr=(3 << 24) + 48 * n - 4), dict(tr=(3 << 24) - 48 * n + 4), dict(jac=3 << 24),
               dict(tr=(1 << 24) + 48 * G - 4), dict(jac=(2 << 24) + 288 * G - 4), dict(tr=(4 << 24) + 4 * n - 4), dict(jac=4 << 24),
               dict(jac=(5 << 24) + 48 * n - 4), dict(tr=(6 << 24) + 288 * n - 4), dict(jac=1 << 24), dict(tr=2 << 24)):
        assert _compose_call(lib, **kw) == BAD, kw
    # touching is not sharing
    assert _compose_call(lib, n=0, tr=(3 << 24) + 48 * n) == BAD  # (sizes are refused first)

    for key in ("stats", "members", "offsets", "gstats"):
        assert _reduce_call(lib, **{key: 0}) == BAD, key
    for kw in (dict(n=0), dict(G=0), dict(n_members=0), dict(n_members=-1)):
        assert _reduce_call(lib, **kw) == BAD, kw
    for kw in (dict(n=65536), dict(G=65536), dict(n_members=65536)):
        assert _reduce_call(lib, **kw) == BIG, kw
    for kw in (dict(stats=(1 << 24) + 4), dict(gstats=(4 << 24) + 4), dict(members=(2 << 24) + 2), dict(offsets=(3 << 24) + 1)):
        assert _reduce_call(lib, **kw) == ALIGN, kw
    for kw in (dict(gstats=1 << 24), dict(gstats=(1 << 24) + 256 * 5 - 8), dict(gstats=(2 << 24) + 8), dict(gstats=(3 << 24) + 8),
               dict(gstats=(3 << 24) - 256 * 3 + 8)):
        assert _reduce_call(lib, **kw) == BAD, kw


def test_front_ends_refuse_cpu_tensors_and_bad_arguments():
    import torch

    from fetalsyngen_amd import kernels as K

    gm, gj, base, group = torch.zeros(2, 3, 4), torch.zeros(2, 12, 6), torch.zeros(5, 3, 4), torch.zeros(5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="MI355X"):
        K.svr_compose(gm, gj, base, group)
    with pytest.raises(RuntimeError, match="MI355X"):
        K.svr_group_reduce(torch.zeros(5, 32, dtype=torch.float64), group, torch.zeros(3, dtype=torch.int32))


# ---- the parsing of `groups` ---------------------------------------------------------------------------------------------------
def test_groups_are_relabelled_in_increasing_order():
    import torch

    from fetalsyngen_amd.generator.artifacts.svort.svr import parse_groups

    given = [7, -1, 3, 7, 3, 40, -1]
    for form in (given, np.array(given), np.array(given, np.int16), torch.tensor(given), tuple(given)):
        ids, group, members, offsets = parse_groups(form, 7)
        assert ids.tolist() == [3, 7, 40] and group.tolist() == [1, -1, 0, 1, 0, 2, -1] and group.dtype == np.int32
        assert members.tolist() == [2, 4, 0, 3, 5] and offsets.tolist() == [0, 2, 4, 5]
        assert members.dtype == np.int32 and offsets.dtype == np.int32
    want = GU.relabel(given)
    assert want[0] == [3, 7, 40] and all(np.array_equal(a, b) for a, b in zip(want[1:], parse_groups(given, 7)[1:]))
    with pytest.raises(TypeError, match="synchronise"):
        parse_groups(torch.empty(7, dtype=torch.int64, device="meta"), 7)
    with pytest.raises(TypeError):
        parse_groups([0.0, 1.0], 2)
    with pytest.raises(TypeError):
        parse_groups(torch.zeros(2), 2)
    for bad in ([0, 1, 2], [[0, 1]], [-1, -1], [0, -2]):
        with pytest.raises(ValueError):
            parse_groups(bad, 2)


# ---- the launch sequences ---------------------------------------------------------------------------------------------------
def _recorders(monkeypatch, log, n, G):
    import torch

    from fetalsyngen_amd import kernels as K

    def a2m(theta):
        log.append(("a2m", tuple(theta.shape)))
        return torch.zeros(theta.shape[0], 3, 4)

    def a2m_bwd(gmat, theta):
        log.append(("a2m_bwd", tuple(gmat.shape), tuple(theta.shape)))
        rows = theta.shape[0] // 12
        assert torch.equal(gmat, torch.eye(12).repeat(rows, 1).view(12 * rows, 3, 4))  # the constant one-hot block
        assert torch.equal(theta.view(rows, 12, 6), theta.view(rows, 12, 6)[:, :1].expand(rows, 12, 6))  # every pose 12 times
        return torch.zeros(theta.shape[0], 6)

    def m2a(mat):
        log.append(("m2a", tuple(mat.shape)))
        return torch.zeros(mat.shape[0], 6)

    def compose(gm, gj, base, group, out=None):
        log.append(("compose", tuple(gm.shape), tuple(gj.shape), tuple(base.shape), group.tolist(), out is not None))
        return out

    def normal(tr, jac, vol, psf, y, sm, wt, res, min_weight, out=None, ws=None):
        log.append(("normal", tuple(jac.shape), tuple(y.shape), min_weight, out is not None, ws is not None))
        return out

    def reduce(stats, members, offsets, out=None):
        log.append(("reduce", tuple(stats.shape), members.tolist(), offsets.tolist(), tuple(out.shape)))
        return out

    def update(state, k, stats, theta, **kw):
        log.append(("update", k, state.n, tuple(stats.shape), tuple(theta.shape), kw["lambda0"], kw["tol"]))

    for name, fn in (("axisangle2mat", a2m), ("axisangle2mat_backward", a2m_bwd), ("mat2axisangle", m2a), ("svr_compose", compose),
                     ("svr_normal", normal), ("svr_group_reduce", reduce), ("svr_update", update)):
        monkeypatch.setattr(K, name, fn)


def test_svr_launch_sequence_without_groups_is_the_parents(monkeypatch):
    """`groups=None`: n_iter + 1 rounds of axisangle2mat, ONE axisangle2mat_backward over 12 n rows, svr_normal, svr_update and
    nothing else, call for call what tests/test_svr64_reference.py records of the parent"""
    import torch

    from fetalsyngen_amd.generator.artifacts import svort

    log, n, n_iter = [], 3, 4
    _recorders(monkeypatch, log, n, 0)
    poses = torch.arange(18, dtype=torch.float32).view(n, 6)
    for kw in (dict(), dict(groups=None)):
        log.clear()
        out, info = svort.svr(poses, torch.zeros(n, 1, 5, 7), torch.zeros(1, 1, 4, 4, 4), torch.ones(1, 1, 1), 1.0, n_iter=n_iter,
                              lambda0=0.5, tol=0.25, min_weight=0.75, return_info=True, **kw)
        assert tuple(out.shape) == (n, 6) and set(info) == {"cost", "lambda", "accepted", "frozen"}
        assert len(log) == 4 * (n_iter + 1)
        for k in range(n_iter + 1):
            assert log[4 * k:4 * k + 4] == [("a2m", (n, 6)), ("a2m_bwd", (12 * n, 3, 4), (12 * n, 6)),
                                            ("normal", (n, 12, 6), (n, 5, 7), 0.75, True, True), ("update", k, n, (n, 32), (n, 6), 0.5, 0.25)]


def test_svr_launch_sequence_with_groups(monkeypatch):
    """base = axisangle2mat(poses) once; n_iter + 1 rounds of axisangle2mat(phi), axisangle2mat_backward over 12 G rows,
    svr_compose, svr_normal, svr_group_reduce, svr_update on G rows; then axisangle2mat and svr_compose at the accepted phi and
    one mat2axisangle for the poses that are returned"""
    import torch

    from fetalsyngen_amd.generator.artifacts import svort

    log, n, n_iter, G = [], 5, 3, 2
    _recorders(monkeypatch, log, n, G)
    poses = torch.arange(30, dtype=torch.float32).view(n, 6)
    out, info = svort.svr(poses, torch.zeros(n, 1, 5, 7), torch.zeros(1, 1, 4, 4, 4), torch.ones(1, 1, 1), 1.0, n_iter=n_iter,
                          lambda0=0.5, tol=0.25, min_weight=0.75, return_info=True, groups=[9, 4, -1, 9, 4])
    assert tuple(out.shape) == (n, 6) and set(info) == {"cost", "lambda", "accepted", "frozen", "group_poses", "group_ids"}
    assert info["group_ids"] == [4, 9] and tuple(info["group_poses"].shape) == (G, 6) and tuple(info["cost"].shape) == (n_iter + 1, G)
    assert torch.equal(out[2], poses[2])  # the fixed slice: its input row
    group = [1, 0, -1, 1, 0]
    assert log[0] == ("a2m", (n, 6)) and len(log) == 1 + 6 * (n_iter + 1) + 3
    for k in range(n_iter + 1):
        assert log[1 + 6 * k:7 + 6 * k] == [
            ("a2m", (G, 6)), ("a2m_bwd", (12 * G, 3, 4), (12 * G, 6)), ("compose", (G, 3, 4), (G, 12, 6), (n, 3, 4), group, True),
            ("normal", (n, 12, 6), (n, 5, 7), 0.75, True, True), ("reduce", (n, 32), [1, 4, 0, 3], [0, 2, 4], (G, 32)),
            ("update", k, G, (G, 32), (G, 6), 0.5, 0.25)]
    assert log[-3:] == [("a2m", (G, 6)), ("compose", (G, 3, 4), (G, 12, 6), (n, 3, 4), group, True), ("m2a", (n, 3, 4))]


def test_matrix_front_end_with_groups_makes_no_round_trip(monkeypatch):
    import torch

    from fetalsyngen_amd.generator.artifacts import svort

    log, n = [], 4
    _recorders(monkeypatch, log, n, 1)
    mats = torch.eye(3, 4).repeat(n, 1, 1)
    out = svort.SVR(n_iter=2, groups=[0, 0, -1, 0])(mats, torch.zeros(n, 1, 5, 7), torch.zeros(4, 4, 4), torch.ones(1, 1, 1), 1.0)
    assert tuple(out.shape) == (n, 3, 4) and not [e for e in log if e[0] == "m2a"] and log[0] == ("a2m", (1, 6))
    assert [e[0] for e in log].count("compose") == 4


def test_grouped_solvers_are_not_differentiable_and_are_exported():
    import torch

    from fetalsyngen_amd import kernels as K
    from fetalsyngen_amd.generator.artifacts import svort

    assert callable(svort.align_stacks) and callable(K.svr_compose) and callable(K.svr_group_reduce)
    poses, y, vol, psf = torch.zeros(2, 6), torch.zeros(2, 1, 4, 4), torch.zeros(4, 4, 4), torch.ones(1, 1, 1)
    with pytest.raises(NotImplementedError, match="poses"):
        svort.svr(poses.clone().requires_grad_(True), y, vol, psf, 1.0, n_iter=1, groups=[0, 0])
    tr = torch.eye(3, 4).repeat(2, 1, 1)
    for name in ("transforms", "slices"):
        a = dict(transforms=tr, slices=y)
        a[name] = a[name].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match=name):
            svort.align_stacks(a["transforms"], a["slices"], [0, 1], psf, (4, 4, 4), 1.0)
    with pytest.raises(TypeError, match="synchronise"):
        svort.align_stacks(tr, y, torch.empty(2, dtype=torch.int64, device="meta"), psf, (4, 4, 4), 1.0)
    for kw in (dict(stack_ids=[0, 0]), dict(stack_ids=[0, -1]), dict(stack_ids=[0, 1], template=5), dict(stack_ids=[0, 1], n_rounds=0),
               dict(stack_ids=[0, 1], svr=dict(groups=[0, 0]))):
        ids = kw.pop("stack_ids")
        with pytest.raises(ValueError):
            svort.align_stacks(tr, y, ids, psf, (4, 4, 4), 1.0, **kw)
