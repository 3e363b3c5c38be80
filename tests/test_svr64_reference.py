"""CPU: the restatement of the per-slice Levenberg-Marquardt registration (tests/util_svr64.py) held to
the restatements it is built beside, the update rule by hand, the solver in float64 with three mutants, and the host side of
the new entries (header, build list, refusals before any launch, front-end checks, the launch sequence of `svort.svr`)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests import util_srr64 as SR
from tests import util_svr64 as U
from tests import util_transform_convert64 as TC
from tests.util_sa_backward64 import backward64

ROOT = Path(__file__).resolve().parents[1]
F32, F64 = np.float32, np.float64


# ---- the normal equations --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.GENERAL)
def test_s_is_the_linear_forward(name):
    c = U.general_case(name)
    p = U.pixels(c["tr"], c["jac"], c["vol"], c["psf"], c["y"], c["sm"], None, c["res"], 0.0, F64)
    want, _ = SR.forward(c["tr"], c["vol"], c["psf"], c["sm"], c["y"].shape[1:], c["res"], False, F64)
    assert np.abs(p["s"] - want).max() <= 1e-12 * np.abs(want).max()
    assert c["kept"] >= U.MIN_KEPT  # 0.526 and 0.888 measured


def _pose_case():
    """the capability case at its start poses, with weights: poses, their fp32 matrices and the float64 Jacobian"""
    c = U.capability_case()
    theta = c["start"]
    tr = TC.axisangle2mat(theta, F64).astype(F32)
    sw = np.random.default_rng(3).uniform(0.5, 1.5, c["y"].shape).astype(F32)
    return c, theta, tr, U.jacobian(theta, F64), sw


def test_g_is_the_backward_chained_through_the_pose_conversion():
    c, theta, tr, jac, sw = _pose_case()
    p = U.pixels(tr, jac, c["vol"], c["psf"], c["y"], None, sw, c["res"], 0.5, F64)
    ge = np.where(p["part"], p["w"] * p["e"], 0.0)
    # backward64 takes fp32 grad_slices and is linear in them: hand it w e as the sum of two fp32 arrays
    hi = ge.astype(F32)
    lo = (ge - hi).astype(F32)
    gt = sum(backward64(tr, c["vol"], None, c["psf"], part, p["part"], c["res"], False)["grad_transforms"] for part in (hi, lo))
    want = TC.axisangle2mat_backward(gt.reshape(-1, 3, 4), theta, F64)
    got = U.stats64(p["terms"])[:, 21:27]
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    assert np.abs(want).max() > 1e-3


def test_j6_is_the_derivative_of_the_forward_and_h_is_jtwj():
    c, theta, _, _, sw = _pose_case()
    assert c["weight"].min() == 1.0 and c["weight"].max() == 1.0  # every footprint inside the volume: the weight is constant
    th = theta.astype(F64)
    p = U._pixels64(TC.axisangle2mat(th, F64), U.jacobian(th, F64), c["vol"], c["psf"], c["y64"], None, sw, c["res"], 0.5)
    step = 1e-5
    fd = np.zeros_like(p["J6"])
    for a in range(6):
        d = np.zeros(6)
        d[a] = step
        fd[..., a] = (U.forward_at(th + d, c["vol"], c["psf"], c["ss"], c["res"])[0]
                      - U.forward_at(th - d, c["vol"], c["psf"], c["ss"], c["res"])[0]) / (2 * step)
    err = np.abs(p["J6"] - fd).max()
    print("largest |J6 - central difference|", err, "of", np.abs(fd).max())
    assert err <= 1e-6
    n = th.shape[0]
    J, w = fd.reshape(n, -1, 6), sw.astype(F64).reshape(n, -1)
    H = np.einsum("npa,np,npb->nab", J, w, J)
    got = U.stats64(p["terms"])
    for o, (a, b) in enumerate(U.PAIRS):
        assert np.abs(got[:, o] - H[:, a, b]).max() <= 1e-5 * np.abs(H).max()
    assert np.array_equal(got[:, 29], np.full(n, 81.0)) and np.all(got[:, 30:] == 0)


def test_reduce_follows_lane_wave_and_tile_order():
    rng = np.random.default_rng(11)
    terms = (rng.standard_normal((2, 37, 29, U.TERMS)) * 10.0 ** rng.integers(-3, 4, (2, 37, 29, 1))).astype(F32)
    got = U.stats_device(terms)
    tiles_y, tiles_x = 3, 2
    want = np.zeros((2, U.SLOTS))
    for s in range(2):
        for tile in range(tiles_y * tiles_x):  # the reduce kernel's loop
            ty, tx = divmod(tile, tiles_x)
            red = np.zeros((4, U.TERMS), F32)
            for wave in range(4):
                lanes = np.zeros((64, U.TERMS), F32)
                for lane in range(64):
                    tid = wave * 64 + lane
                    yy, xx = ty * 16 + tid // 16, tx * 16 + tid % 16
                    if yy < 37 and xx < 29:
                        lanes[lane] = terms[s, yy, xx]
                for o in (32, 16, 8, 4, 2, 1):  # shuffle-down: lane i reads lane i + o, a lane past the end reads itself
                    src = np.where(np.arange(64) + o < 64, np.arange(64) + o, np.arange(64))
                    lanes = lanes + lanes[src]
                red[wave] = lanes[0]
            part = red[0].copy()
            for wave in range(1, 4):
                part = part + red[wave]
            want[s, :U.TERMS] = want[s, :U.TERMS] + part.astype(F64)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, U.stats64(terms))  # and the order matters on these values


def test_e_cpu_constants_are_what_is_measured():
    m = U.measure_e_cpu()
    assert set(m) == set(U.E_CPU)
    for key, bound in U.E_CPU.items():
        assert 0.98 * bound <= m[key] <= bound, (key, m[key], bound)


# ---- the update rule by hand -------------------------------------------------------------------------------------------------
def _stats(H=None, g=None, swe2=1.0, sw=2.0, m=10.0):
    s = np.zeros((1, U.SLOTS))
    H = np.diag([4.0, 2.0, 1.0, 8.0, 16.0, 0.5]) if H is None else np.asarray(H, F64)
    for o, (a, b) in enumerate(U.PAIRS):
        s[0, o] = H[a, b]
    s[0, 21:27] = [1.0, -2.0, 0.5, 4.0, -8.0, 0.25] if g is None else g
    s[0, 27], s[0, 28], s[0, 29] = swe2, sw, m
    return s


THETA0 = np.array([[0.1, -0.2, 0.3, 1.0, 2.0, -3.0]], F32)


def test_update_diagonal_h_gives_minus_g_over_h_times_one_plus_lambda():
    st = U.new_state(1, 3)
    th = U.update(st, 0, _stats(), THETA0.copy(), lambda0=0.25)
    h, g = np.array([4.0, 2.0, 1.0, 8.0, 16.0, 0.5]), np.array([1.0, -2.0, 0.5, 4.0, -8.0, 0.25])
    want = (THETA0[0].astype(F64) + -g / (h * 1.25)).astype(F32)
    assert np.array_equal(th[0], want)
    assert st["cost"][0, 0] == 0.5 and st["lambda_hist"][0, 0] == 0.25 and st["frozen"][0, 0] == 0 and st["m0"][0] == 10
    assert np.array_equal(st["theta_cur"], THETA0)


def test_update_accept_divides_lambda_and_reject_multiplies_it():
    st = U.new_state(1, 4)
    th = U.update(st, 0, _stats(), THETA0.copy())
    t1 = th.copy()
    th = U.update(st, 1, _stats(swe2=0.5), th)  # cost 0.25 < 0.5: accepted
    assert st["accepted"][1, 0] == 1 and st["lambda_hist"][1, 0] == 1e-3 / 10.0 and np.array_equal(st["theta_cur"], t1)
    assert st["cost"][1, 0] == 0.25
    th = U.update(st, 2, _stats(swe2=0.5), th)  # equal cost: rejected
    assert st["accepted"][2, 0] == 0 and st["lambda_hist"][2, 0] == (1e-3 / 10.0) * 10.0 and np.array_equal(st["theta_cur"], t1)
    assert st["cost"][2, 0] == 0.25 and st["frozen"][2, 0] == 0
    assert not np.array_equal(th, t1)  # a new trial from the kept pose under the larger lambda


def test_update_lambda_min_floor_and_tol_freeze():
    st = U.new_state(1, 3)
    th = U.update(st, 0, _stats(), THETA0.copy(), lambda0=1e-9)
    th = U.update(st, 1, _stats(swe2=0.999), th, lambda0=1e-9, tol=0.01)  # accepted, but the gain is below tol * cost
    assert st["accepted"][1, 0] == 1 and st["lambda_hist"][1, 0] == 1e-9 and st["frozen"][1, 0] == 1
    assert np.array_equal(th, st["theta_cur"])


def test_update_lambda_max_freezes():
    st = U.new_state(1, 3)
    th = U.update(st, 0, _stats(), THETA0.copy(), lambda0=1e9)
    th = U.update(st, 1, _stats(swe2=2.0), th, lambda0=1e9)
    assert st["frozen"][1, 0] == 0 and st["lambda_hist"][1, 0] == 1e10
    th = U.update(st, 2, _stats(swe2=2.0), th, lambda0=1e9)
    assert st["frozen"][2, 0] == 1 and st["lambda_hist"][2, 0] == 1e11 and np.array_equal(th, THETA0)
    th = U.update(st, 3, _stats(swe2=0.1), th, lambda0=1e9)  # frozen: a better trial changes nothing
    assert st["accepted"][3, 0] == 0 and st["lambda_hist"][3, 0] == 1e11 and st["cost"][3, 0] == 0.5


def test_update_rejects_a_nan_and_too_little_overlap():
    for bad in ("nan", "inf", "overlap"):
        st = U.new_state(1, 2)
        th = U.update(st, 0, _stats(), THETA0.copy())
        trial = _stats(swe2=0.1, m=4.0 if bad == "overlap" else 10.0)
        if bad != "overlap":
            trial[0, 3] = np.nan if bad == "nan" else np.inf
        th = U.update(st, 1, trial, th)
        assert st["accepted"][1, 0] == 0 and st["cost"][1, 0] == 0.5 and st["lambda_hist"][1, 0] == 1e-2, bad
    st = U.new_state(1, 2)
    th = U.update(st, 0, _stats(), THETA0.copy())
    th = U.update(st, 1, _stats(swe2=0.1, m=5.0), th)  # exactly min_overlap * m0: accepted
    assert st["accepted"][1, 0] == 1


def test_update_freezes_at_k0_without_pixels_weight_or_finite_sums():
    for kw in (dict(m=0.0), dict(sw=0.0), dict(swe2=np.nan), dict(g=[np.inf, 0, 0, 0, 0, 0])):
        st = U.new_state(1, 2)
        th = U.update(st, 0, _stats(**kw), THETA0.copy())
        assert st["frozen"][0, 0] == 1 and np.array_equal(th, THETA0), kw
        th = U.update(st, 1, _stats(swe2=0.01), th)
        assert st["accepted"][1, 0] == 0 and np.array_equal(th, THETA0) and np.array_equal(st["theta_cur"], THETA0)


def test_update_non_positive_pivot_freezes_and_zero_diagonal_does_not_move():
    H = np.diag([4.0, 2.0, 1.0, 8.0, 16.0, 0.5])
    H[0, 1] = H[1, 0] = 3.0  # 4 * 2 * (1 + lambda)^2 < 9: the second pivot is negative
    st = U.new_state(1, 2)
    th = U.update(st, 0, _stats(H=H), THETA0.copy())
    assert st["frozen"][0, 0] == 1 and np.array_equal(th, THETA0)
    H = np.diag([4.0, 0.0, 1.0, 8.0, 16.0, 0.5])
    H[0, 1] = H[1, 0] = 3.0  # off-diagonal entries of a parameter that is taken out play no part
    st = U.new_state(1, 2)
    th = U.update(st, 0, _stats(H=H), THETA0.copy(), lambda0=0.25)
    assert st["frozen"][0, 0] == 0 and th[0, 1] == THETA0[0, 1]
    assert th[0, 0] == F32(F64(THETA0[0, 0]) - 1.0 / 5.0) and th[0, 2] == F32(F64(THETA0[0, 2]) - 0.5 / 1.25)


def test_last_slot_returns_the_current_pose():
    st = U.new_state(1, 1)
    th = U.update(st, 0, _stats(), THETA0.copy())
    t1 = th.copy()
    th = U.update(st, 1, _stats(swe2=0.5), th)
    assert st["accepted"][1, 0] == 1 and np.array_equal(th, t1) and np.array_equal(st["theta_cur"], t1)


# ---- the solver ------------------------------------------------------------------------------------------------------------
def test_float64_solver_converges_on_the_capability_case_and_the_mutants_do_not():
    c = U.capability_case()
    rot0, trans0 = U.pose_errors(c["start"], c["true"])
    assert 0.029 < rot0 <= 0.03 and 0.70 < trans0 <= 0.75
    r = U.measure_capability(F64, unrounded=True)
    print("float64:", r["cost0"], r["cost"], r["rot"], r["trans"], r["accepted"])
    assert r["cost0"].min() > 2.8e-4 and r["cost0"].max() < 2.9e-2
    assert r["cost"].max() < 1e-30 and r["rot"] < 1e-14 and r["trans"] < 1e-14  # measured 1.5e-31, 2.2e-15, 5.8e-15
    assert r["accepted"].min() >= 7 and r["accepted"].max() <= 10
    for mutant in ("delta_sign", "lambda_swapped", "identity_damping"):
        m = U.measure_capability(F64, mutant, unrounded=True)
        print(mutant, m["cost"], m["rot"], m["trans"])
        assert m["cost"].max() > 1e-8 and m["trans"] > 1e-3, mutant


def test_fp32_restatement_gives_the_recorded_capability_figures():
    r = U.measure_capability(F32)
    print("fp32:", r["factor"], r["rot"], r["trans"])
    assert 0.98 * U.CAP32_COST_FACTOR <= r["factor"] <= 1.02 * U.CAP32_COST_FACTOR
    assert 0.98 * U.CAP32_ROT_ERR <= r["rot"] <= U.CAP32_ROT_ERR
    assert 0.98 * U.CAP32_TRANS_ERR <= r["trans"] <= U.CAP32_TRANS_ERR


# ---- the host side of the new entries ---------------------------------------------------------------------------------------
ENTRIES = ("fsg_svr_ws_bytes", "fsg_svr_normal_f32", "fsg_svr_state_bytes", "fsg_svr_update_f32")


def test_header_build_list_and_abi():
    from fetalsyngen_amd import _build, _lib

    text = (ROOT / "include" / "fsg_hip.h").read_text()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", text) and name in _lib.PROTOTYPES
    assert _lib.ABI_VERSION == 8
    assert "fsg_svr.hip" in _build.SOURCES and (ROOT / "fetalsyngen_amd" / "csrc" / "fsg_svr.hip").exists()


def _normal_call(lib, **kw):
    a = dict(tr=1 << 24, jac=2 << 24, vol=3 << 24, psf=4 << 24, y=5 << 24, sm=0, sw=0, stats=6 << 24, ws=7 << 24, pd=3, ph=3, pw=5,
             D=20, H=18, W=22, n=5, h=37, w=29, res=1.0, min_weight=0.5, mode=0, ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = lib.fsg_svr_ws_bytes(a["n"], a["h"], a["w"])
    p = ctypes.c_void_p
    return lib.fsg_svr_normal_f32(p(a["tr"]), p(a["jac"]), p(a["vol"]), p(a["psf"]), a["pd"], a["ph"], a["pw"], p(a["y"]), p(a["sm"]),
                                  p(a["sw"]), p(a["stats"]), a["D"], a["H"], a["W"], a["n"], a["h"], a["w"], a["res"],
                                  a["min_weight"], a["mode"], p(a["ws"]), a["ws_bytes"], None)


def _update_call(lib, **kw):
    a = dict(stats=1 << 24, theta=2 << 24, state=3 << 24, state_bytes=None, n=5, k=0, K=12, lambda0=1e-3, factor=10.0,
             lambda_min=1e-9, lambda_max=1e10, min_overlap=0.5, tol=0.0)
    a.update(kw)
    if a["state_bytes"] is None:
        a["state_bytes"] = lib.fsg_svr_state_bytes(a["n"], a["K"])
    p = ctypes.c_void_p
    return lib.fsg_svr_update_f32(p(a["stats"]), p(a["theta"]), p(a["state"]), a["state_bytes"], a["n"], a["k"], a["K"],
                                  a["lambda0"], a["factor"], a["lambda_min"], a["lambda_max"], a["min_overlap"], a["tol"], None)


def test_entries_refuse_before_any_launch():
    """no device is needed: every refusal returns before the first launch (the addresses are made up)"""
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    BAD, BIG, ALIGN = _lib.E_BADARG, _lib.E_TOOBIG, _lib.E_ALIGN
    assert lib.fsg_svr_ws_bytes(5, 37, 29) == 5 * 6 * 128 and lib.fsg_svr_ws_bytes(1, 13, 11) == 128
    assert lib.fsg_svr_ws_bytes(0, 4, 4) == 0 and lib.fsg_svr_ws_bytes(1, 0, 4) == 0
    for key in ("tr", "jac", "vol", "psf", "y", "stats", "ws"):
        assert _normal_call(lib, **{key: 0}) == BAD, key
    for kw in (dict(n=0), dict(h=0), dict(w=-1), dict(D=1), dict(pd=0), dict(mode=_lib.SA.NEAREST_PSF), dict(mode=_lib.SA.TORCH),
               dict(mode=7), dict(min_weight=-0.5), dict(min_weight=float("nan")), dict(ws_bytes=5 * 6 * 128 - 1)):
        assert _normal_call(lib, **kw) == BAD, kw
    for kw in (dict(pd=65, ws_bytes=1 << 30), dict(pd=17, ph=17, pw=17), dict(n=65536, ws_bytes=1 << 40)):
        assert _normal_call(lib, **kw) == BIG, kw
    assert _normal_call(lib, ws=(7 << 24) + 4) == ALIGN and _normal_call(lib, stats=(6 << 24) + 4) == ALIGN

    n, K = 5, 12
    s = K + 1
    assert lib.fsg_svr_state_bytes(n, K) == (8 * (32 * n + 2 * n + 2 * s * n) + 4 * (6 * n + n + 2 * s * n) + 7) // 8 * 8
    assert lib.fsg_svr_state_bytes(0, K) == 0 and lib.fsg_svr_state_bytes(n, 0) == 0 and lib.fsg_svr_state_bytes(n, 4097) == 0
    for kw in (dict(stats=0), dict(theta=0), dict(state=0), dict(n=0), dict(k=-1), dict(k=13), dict(K=0), dict(K=4097, state_bytes=1 << 30),
               dict(state_bytes=lib.fsg_svr_state_bytes(n, K) - 1), dict(lambda0=0.0), dict(lambda0=float("nan")), dict(factor=1.0),
               dict(lambda_min=0.0), dict(lambda_max=1e-12), dict(min_overlap=-1.0), dict(tol=-1.0), dict(tol=float("nan")),
               dict(stats=(3 << 24) + 8), dict(theta=(3 << 24) + lib.fsg_svr_state_bytes(n, K) - 4), dict(theta=(1 << 24) + 8)):
        assert _update_call(lib, **kw) == BAD, kw
    for kw in (dict(state=(3 << 24) + 4), dict(stats=(1 << 24) + 4), dict(theta=(2 << 24) + 2)):
        assert _update_call(lib, **kw) == ALIGN, kw


@pytest.mark.parametrize("K", (1, 2, 12, 4096))
@pytest.mark.parametrize("n", (1, 5, 1024, 1025))
def test_state_bytes_is_the_headers_formula(n, K):
    """fsg_svr_state_bytes against the layout paragraph of include/fsg_hip.h, written out; s = K + 1 and n take both parities,
    so the rounding to 8 is exercised"""
    from fetalsyngen_amd import _lib

    lib, s = _lib.load(), K + 1
    assert lib.fsg_svr_state_bytes(n, K) == (8 * (32 * n + 2 * n + 2 * s * n) + 4 * (6 * n + n + 2 * s * n) + 7) // 8 * 8
    assert lib.fsg_svr_state_bytes(n, 0) == 0 and lib.fsg_svr_state_bytes(n, 4096 + 1) == 0


def test_front_ends_refuse_cpu_tensors_and_bad_arguments():
    import torch

    from fetalsyngen_amd import kernels as K
    from fetalsyngen_amd.generator.artifacts import svort

    tr, jac, vol, psf, y = torch.zeros(2, 3, 4), torch.zeros(2, 12, 6), torch.zeros(4, 4, 4), torch.ones(1, 1, 1), torch.zeros(2, 4, 4)
    with pytest.raises(RuntimeError, match="MI355X"):
        K.svr_normal(tr, jac, vol, psf, y, None, None, 1.0)
    st = K.svr_state(2, 3, "cpu")  # the layout is checked against fsg_svr_state_bytes on any device
    assert st.cost.shape == (4, 2) and st.theta_cur.shape == (2, 6) and st.stats_cur.shape == (2, 32)
    assert set(st.info()) == {"cost", "lambda", "accepted", "frozen"}
    with pytest.raises(RuntimeError, match="MI355X"):
        K.svr_update(st, 0, torch.zeros(2, 32, dtype=torch.float64), torch.zeros(2, 6))
    for n, k in ((0, 3), (2, 0), (2, 4097)):
        with pytest.raises(ValueError):
            K.svr_state(n, k, "cpu")
    with pytest.raises(RuntimeError, match="MI355X"):
        svort.svr(torch.zeros(2, 6), torch.zeros(2, 1, 4, 4), vol, psf, 1.0, n_iter=1)


def test_svr_is_not_differentiable():
    import torch

    from fetalsyngen_amd.generator.artifacts import svort

    args = dict(poses=torch.zeros(2, 6), slices=torch.zeros(2, 1, 4, 4), vol=torch.zeros(4, 4, 4), psf=torch.ones(1, 1, 1))
    for name in ("poses", "slices", "vol"):
        a = {k: (v.clone().requires_grad_(True) if k == name else v) for k, v in args.items()}
        with pytest.raises(NotImplementedError, match=name):
            svort.svr(a["poses"], a["slices"], a["vol"], a["psf"], 1.0, n_iter=1)


def test_namespace_exports():
    import importlib

    from fetalsyngen_amd import kernels as K
    from fetalsyngen_amd.generator.artifacts import svort

    module = importlib.import_module("fetalsyngen_amd.generator.artifacts.svort.svr")
    assert svort.svr is module.svr and svort.SVR is module.SVR
    for name in ("svr_normal", "svr_state", "svr_update", "svr_ws_bytes", "SVRState"):
        assert callable(getattr(K, name))


def test_svr_launch_sequence(monkeypatch):
    """n_iter + 1 rounds of axisangle2mat, ONE axisangle2mat_backward over 12 n rows, svr_normal, svr_update; recorders in
    place of the kernels, so no device is needed"""
    import torch

    from fetalsyngen_amd import kernels as K
    from fetalsyngen_amd.generator.artifacts import svort

    log = []
    n, n_iter = 3, 4

    def a2m(theta):
        log.append(("a2m", tuple(theta.shape)))
        return torch.zeros(theta.shape[0], 3, 4)

    def a2m_bwd(gmat, theta):
        log.append(("a2m_bwd", tuple(gmat.shape), tuple(theta.shape)))
        want = torch.eye(12).repeat(n, 1).view(12 * n, 3, 4)
        assert torch.equal(gmat, want)  # the constant one-hot block
        assert torch.equal(theta.view(n, 12, 6), theta.view(n, 12, 6)[:, :1].expand(n, 12, 6))  # every pose 12 times
        return torch.zeros(theta.shape[0], 6)

    def normal(tr, jac, vol, psf, y, sm, wt, res, min_weight, out=None, ws=None):
        log.append(("normal", tuple(jac.shape), tuple(y.shape), min_weight, out is not None, ws is not None))
        return out

    def update(state, k, stats, theta, **kw):
        log.append(("update", k, kw["lambda0"], kw["tol"]))

    monkeypatch.setattr(K, "axisangle2mat", a2m)
    monkeypatch.setattr(K, "axisangle2mat_backward", a2m_bwd)
    monkeypatch.setattr(K, "svr_normal", normal)
    monkeypatch.setattr(K, "svr_update", update)
    poses = torch.arange(18, dtype=torch.float32).view(n, 6)
    out, info = svort.svr(poses, torch.zeros(n, 1, 5, 7), torch.zeros(1, 1, 4, 4, 4), torch.ones(1, 1, 1), 1.0, n_iter=n_iter,
                          lambda0=0.5, tol=0.25, min_weight=0.75, return_info=True)
    assert tuple(out.shape) == (n, 6) and set(info) == {"cost", "lambda", "accepted", "frozen"}
    assert len(log) == 4 * (n_iter + 1)
    for k in range(n_iter + 1):
        assert log[4 * k:4 * k + 4] == [("a2m", (n, 6)), ("a2m_bwd", (12 * n, 3, 4), (12 * n, 6)),
                                        ("normal", (n, 12, 6), (n, 5, 7), 0.75, True, True), ("update", k, 0.5, 0.25)]
