"""GPU: per-slice Levenberg-Marquardt registration (fsg_svr_normal_f32, fsg_svr_update_f32, svort.svr; the rule is in
include/fsg_hip.h and DESIGN.md section 23) against the restatement tests/util_svr64.py.

Tolerances (none is derived from what the kernels give):
  exact geometry     per slot (K + 16) * 2^-24 * S with K and S from util_svr64.bounds: coordinates, trilinear weights and
                     per-pixel weights are exact in fp32 there, so only product roundings and the order of the sums remain.
  general rotations  per group (H, g, cost) 4 * E_cpu * max|float64|, E_cpu the difference of the fp32-operation restatement to
                     the float64 one, measured on the CPU (util_svr64.E_CPU).  The mask keeps every floor and range decision
                     further than 1e-3 from its threshold and every weight further than 1e-3 from min_weight.
  update kernel      bit-equal to the float64 restatement: + - * / in double, no contraction.
  capability         a tenth of the cost factor and four times the pose errors the fp32-operation restatement reaches on the
                     CPU (util_svr64.CAP32_*).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util_sa_backward_cases as BC
from tests import util_svr64 as U
from tests import util_transform_convert64 as TC
from tests.util_sa_backward64 import backward64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
SENTINEL = -77.25
F32, F64 = np.float32, np.float64
E_BWD = 1.14e-6  # tests/test_sa_backward_gpu.py: E_CPU[(False, "grad_transforms")]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (and libfsg_hip.so); there is no fallback to skip to")
    from fetalsyngen_amd import kernels

    return kernels


@pytest.fixture(scope="module")
def svort(K):
    from fetalsyngen_amd.generator.artifacts import svort

    return svort


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(x):
    return x.detach().cpu().numpy()


def bits(x):
    return host(x).view(np.uint32 if x.dtype == torch.float32 else np.uint64)


def normal(K, c, sw=True, **kw):
    return K.svr_normal(dev(c["tr"]), dev(c["jac"]), dev(c["vol"]), dev(c["psf"]), dev(c["y"]), dev(c["sm"]),
                        dev(c["sw"]) if sw else None, c["res"], c["min_weight"], **kw)


# ---- exact geometry -------------------------------------------------------------------------------------------------------
_EXACT = {}


def exact_case(name, masks, n):
    key = (name, masks, n)
    if key not in _EXACT:
        b = BC.exact_case(name, masks, n=n)
        rng = np.random.default_rng(len(name) + 7 * masks + n)
        c = dict(tr=b["tr"], vol=b["vol"], psf=b["psf"], y=b["g"], sm=b["sm"], res=b["res"],
                 jac=(rng.integers(-16, 17, (n, 12, 6)) / 8.0).astype(F32), sw=(rng.integers(2, 7, b["g"].shape) / 4.0).astype(F32),
                 min_weight=0.5 * float(b["psf"].astype(F64).sum()))
        p = U.case_pixels(c, F64)
        _EXACT[key] = (c, U.stats64(p["terms"]), U.bounds(p))
    return _EXACT[key]


@pytest.mark.parametrize("n", (5, 1))
@pytest.mark.parametrize("masks", (False, True), ids=("nomask", "mask"))
@pytest.mark.parametrize("name", list(BC.EXACT))
def test_exact_geometry_against_float64(K, name, masks, n):
    c, want, (kk, ss) = exact_case(name, masks, n)
    got = host(normal(K, c))
    assert got.shape == (n, 32) and got.dtype == F64
    err, bound = np.abs(got - want), (kk + 16) * EPS * ss
    print("worst error / bound %.4f, pixels per slice %s" % ((err / np.maximum(bound, 1e-300)).max(), want[:, 29]))
    assert np.all(err <= bound)
    assert np.array_equal(got[:, 29], want[:, 29]) and np.all(got[:, 30:] == 0)
    assert want[:, 29].max() > 0 and np.abs(want[:, :21]).max() > 0


# ---- general rotations ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sw", (True, False), ids=("weights", "noweights"))
@pytest.mark.parametrize("name", U.GENERAL)
def test_general_rotations_within_four_times_the_fp32_cost_of_the_formula(K, name, sw):
    c = U.general_case(name)
    assert c["kept"] >= U.MIN_KEPT
    want = U.stats64(U.case_pixels(c, F64, sw)["terms"])
    got = host(normal(K, c, sw))
    for key, sl in U.GROUPS.items():
        scale = np.abs(want[:, sl]).max()
        e = np.abs(got[:, sl] - want[:, sl]).max() / scale
        print(f"{name} {key}: GPU {e:.3e}, E_cpu {U.E_CPU[key]:.3e}")
        assert e <= 4 * U.E_CPU[key], (key, e)
    assert np.array_equal(got[:, 29], want[:, 29])


def test_g_agrees_with_the_backward_kernels(K):
    c = U.capability_case()
    theta = dev(c["start"])
    n = theta.shape[0]
    tr = K.axisangle2mat(theta)
    onehot = torch.eye(12, device=DEV).repeat(n, 1).view(12 * n, 3, 4)
    jac = K.axisangle2mat_backward(onehot, theta.repeat_interleave(12, 0).contiguous()).view(n, 12, 6)
    sw = dev(np.random.default_rng(3).uniform(0.5, 1.5, c["y"].shape).astype(F32))
    vol, psf, y = dev(c["vol"]), dev(c["psf"]), dev(c["y"])
    got = host(K.svr_normal(tr, jac, vol, psf, y, None, sw, c["res"], 0.5))[:, 21:27]
    s = K.slice_acq_forward(tr, vol, None, None, psf, c["ss"], c["res"])
    _, gt = K.slice_acq_backward(tr, vol, None, None, psf, ((s - y) * sw).contiguous(), c["res"], need_vol_grad=False)
    other = host(K.axisangle2mat_backward(gt, theta)).astype(F64)
    # the float64 values behind both routes, for the two bounds
    p = U.pixels(host(tr), host(jac), c["vol"], c["psf"], c["y"], None, host(sw), c["res"], 0.5, F64)
    g64 = U.stats64(p["terms"])[:, 21:27]
    gt64 = backward64(host(tr), c["vol"], None, c["psf"], (p["w"] * p["e"]).astype(F32), None, c["res"], False)["grad_transforms"]
    lever = np.abs(host(jac).astype(F64)).sum(1).max()  # a grad_transforms error reaches g through at most this
    bound = 4 * U.E_CPU["g"] * np.abs(g64).max() + 4 * E_BWD * np.abs(gt64).max() * lever
    print("largest difference", np.abs(got - other).max(), "bound", bound, "max |g|", np.abs(g64).max())
    assert np.abs(got - other).max() <= bound
    assert np.abs(got - g64).max() <= 4 * U.E_CPU["g"] * np.abs(g64).max()


# ---- the update kernel ------------------------------------------------------------------------------------------------------
def _hand_rows():
    """per slice: the trial stats of slots 0..3 (the hand cases of tests/test_svr64_reference.py, one slice each)"""
    from tests.test_svr64_reference import _stats

    H_bad = np.diag([4.0, 2.0, 1.0, 8.0, 16.0, 0.5])
    H_bad[0, 1] = H_bad[1, 0] = 3.0
    H_zero = np.diag([4.0, 0.0, 1.0, 8.0, 16.0, 0.5])
    H_zero[0, 1] = H_zero[1, 0] = 3.0
    nan = _stats(swe2=0.1)
    nan[0, 3] = np.nan
    rows = [
        [_stats(), _stats(swe2=0.5), _stats(swe2=0.5), _stats(swe2=0.3)],          # accept, reject, accept
        [_stats(), _stats(swe2=2.0), _stats(swe2=3.0), _stats(swe2=0.9)],          # reject twice, accept
        [_stats(), nan, _stats(swe2=0.1, m=4.0), _stats(swe2=0.1, m=5.0)],          # NaN, too little overlap, just enough
        [_stats(H=H_bad), _stats(swe2=0.1), _stats(swe2=0.1), _stats(swe2=0.1)],   # pivot: frozen at 0
        [_stats(H=H_zero), _stats(H=H_zero, swe2=0.7), _stats(H=H_zero, swe2=0.2), _stats(swe2=0.1)],
        [_stats(m=0.0, sw=0.0, swe2=0.0), _stats(swe2=0.1), _stats(), _stats()],   # empty slice
        [_stats(sw=0.0), _stats(swe2=0.1), _stats(), _stats()],                     # no weight
    ]
    return np.stack([np.concatenate(r, 0) for r in rows], 0)  # (slices, slots, 32)


def _same_state(st, ref):
    """every field of the device block equals the restatement's (a NaN cost, 0 / 0 of an empty slice, equals a NaN)"""
    for name in ("stats_cur", "lam", "m0", "theta_cur", "frozen_now", "cost", "lambda_hist", "accepted", "frozen"):
        a, b = host(getattr(st, name)), ref[name]
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), name


@pytest.mark.parametrize("opts", (dict(), dict(lambda0=1e9), dict(lambda0=0.25, factor=4.0, tol=0.3, min_overlap=0.45)),
                         ids=("defaults", "lambda_max", "other"))
def test_update_kernel_is_bit_equal_on_the_hand_cases(K, opts):
    seq = _hand_rows()
    n, slots = seq.shape[:2]
    n_iter = slots - 1
    theta0 = (np.random.default_rng(1).uniform(-1, 1, (n, 6))).astype(F32)
    st, ref = K.svr_state(n, n_iter, DEV), U.new_state(n, n_iter)
    st.buf.fill_(-1)  # the block needs no initialisation
    th_d, th_r = dev(theta0), theta0.copy()
    for k in range(slots):
        K.svr_update(st, k, dev(seq[:, k]), th_d, **opts)
        th_r = U.update(ref, k, seq[:, k], th_r, **opts)
        assert np.array_equal(bits(th_d), th_r.view(np.uint32)), k
    _same_state(st, ref)
    if not opts:  # the failed pivot, the empty slice and the slice without weight freeze at slot 0; the zero diagonal does not
        assert ref["frozen"][0].tolist() == [0, 0, 0, 1, 0, 1, 1] and ref["accepted"].sum() >= 5


def test_update_kernel_is_bit_equal_on_recorded_stats(K):
    c = U.capability_case()
    n, n_iter = c["start"].shape[0], 8
    st, ref = K.svr_state(n, n_iter, DEV), U.new_state(n, n_iter)
    th_d, th_r = dev(c["start"]), c["start"].copy()
    for k in range(n_iter + 1):
        stats = U.normal(th_r, c["vol"], c["psf"], c["y"], None, None, c["res"], ft=F32, device_order=True)
        K.svr_update(st, k, dev(stats), th_d)
        th_r = U.update(ref, k, stats, th_r)
        assert np.array_equal(bits(th_d), th_r.view(np.uint32)), k
    _same_state(st, ref)
    assert ref["accepted"].sum() >= 20


# ---- the solver --------------------------------------------------------------------------------------------------------------
def solve(svort, c, poses=None, idx=None, **kw):
    sel = slice(None) if idx is None else idx
    kw.setdefault("n_iter", U.CAP_N_ITER)
    return svort.svr(dev((c["start"] if poses is None else poses)[sel]), dev(c["y"][sel]), dev(c["vol"]), dev(c["psf"]), c["res"],
                     return_info=True, **kw)


def test_capability_recovers_the_poses(svort):
    c = U.capability_case()
    out, info = solve(svort, c)
    cost = host(info["cost"])
    factor = float((cost[0] / cost[-1]).min())
    rot, trans = U.pose_errors(host(out), c["true"])
    print("cost", cost[0], "->", cost[-1], "factor", factor, "(restatement %.3e)" % U.CAP32_COST_FACTOR, "errors", rot, trans,
          "(restatement %.3e %.3e)" % (U.CAP32_ROT_ERR, U.CAP32_TRANS_ERR), "accepted", host(info["accepted"]).sum(0))
    assert factor >= U.CAP32_COST_FACTOR / 10
    assert rot < 4 * U.CAP32_ROT_ERR and trans < 4 * U.CAP32_TRANS_ERR
    assert out.dtype == torch.float32 and tuple(out.shape) == (BC.N, 6)


def test_stats_and_poses_are_deterministic(K, svort):
    c, _, _ = exact_case("psf223_big", True, 5)  # 3 x 2 ragged tiles
    a = normal(K, c)
    b = normal(K, c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = normal(K, c)
    side.synchronize()
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(s))
    perm = np.array([3, 0, 4, 2, 1])
    cp = dict(c, **{k: c[k][perm] for k in ("tr", "jac", "y", "sm", "sw")})
    assert np.array_equal(bits(normal(K, cp)), bits(a)[perm])
    one = dict(c, **{k: c[k][2:3] for k in ("tr", "jac", "y", "sm", "sw")})
    assert np.array_equal(bits(normal(K, one)), bits(a)[2:3])

    cap = U.capability_case()
    p1, i1 = solve(svort, cap)
    p2, _ = solve(svort, cap)
    with torch.cuda.stream(side):
        p3, _ = solve(svort, cap)
    side.synchronize()
    assert np.array_equal(bits(p1), bits(p2)) and np.array_equal(bits(p1), bits(p3))
    pp, ip = solve(svort, cap, idx=perm)
    assert np.array_equal(bits(pp), bits(p1)[perm])
    assert np.array_equal(host(ip["cost"]).view(np.uint64), host(i1["cost"]).view(np.uint64)[:, perm])
    alone, _ = solve(svort, cap, idx=slice(2, 3))
    assert np.array_equal(bits(alone), bits(p1)[2:3])


# ---- edges ---------------------------------------------------------------------------------------------------------------------
def test_slices_wholly_outside_every_face_stay_where_they_are(K, svort):
    c = U.capability_case()
    poses = np.zeros((6, 6), F32)
    poses[:, :3] = np.random.default_rng(2).uniform(-0.05, 0.05, (6, 3))
    for i in range(6):
        poses[i, 3 + i // 2] = 60.0 if i % 2 else -60.0
    y = np.repeat(c["y"][:1], 6, 0)
    out, info = svort.svr(dev(poses), dev(y), dev(c["vol"]), dev(c["psf"]), c["res"], n_iter=3, return_info=True)
    assert np.array_equal(bits(out), poses.view(np.uint32))
    assert host(info["frozen"]).min() == 1 and host(info["accepted"]).max() == 0
    tr = K.axisangle2mat(dev(poses))
    stats = host(K.svr_normal(tr, torch.zeros(6, 12, 6, device=DEV), dev(c["vol"]), dev(c["psf"]), dev(y), None, None, c["res"], 0.5))
    assert np.all(stats == 0)


@pytest.mark.parametrize("what", ("mask", "weight"))
def test_an_empty_mask_or_zero_weights_freeze_every_slice(svort, what):
    c = U.capability_case()
    kw = (dict(slices_mask=torch.zeros(c["y"].shape, dtype=torch.bool, device=DEV)) if what == "mask"
          else dict(slices_weight=torch.zeros(c["y"].shape, device=DEV)))
    out, info = solve(svort, c, n_iter=2, **kw)
    assert np.array_equal(bits(out), c["start"].view(np.uint32))
    assert host(info["frozen"]).min() == 1


def test_one_slice_and_the_matrix_front_end(K, svort):
    c = U.capability_case()
    out, info = solve(svort, c, idx=slice(0, 1))
    rot, trans = U.pose_errors(host(out), c["true"][:1])
    assert rot < 4 * U.CAP32_ROT_ERR and trans < 4 * U.CAP32_TRANS_ERR and host(info["cost"]).shape == (U.CAP_N_ITER + 1, 1)
    mats = svort.SVR(n_iter=U.CAP_N_ITER)(K.axisangle2mat(dev(c["start"])), dev(c["y"]), dev(c["vol"]), dev(c["psf"]), c["res"])
    want = TC.axisangle2mat(c["true"], F64)
    assert tuple(mats.shape) == (BC.N, 3, 4) and np.abs(host(mats) - want).max() < 1e-4


def test_requires_grad_raises(svort):
    c = U.capability_case()
    with pytest.raises(NotImplementedError, match="poses"):
        svort.svr(dev(c["start"]).requires_grad_(True), dev(c["y"]), dev(c["vol"]), dev(c["psf"]), c["res"], n_iter=1)
    with pytest.raises(NotImplementedError, match="vol"):
        svort.svr(dev(c["start"]), dev(c["y"]), dev(c["vol"]).requires_grad_(True), dev(c["psf"]), c["res"], n_iter=1)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_and_workspaces_untouched(K):
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    c, _, _ = exact_case("psf223_big", False, 5)
    n, (h, w), (pd, ph, pw) = 5, c["y"].shape[1:], c["psf"].shape
    t = {k: dev(c[k]) for k in ("tr", "jac", "vol", "psf", "y")}
    need = K.svr_ws_bytes(n, h, w)
    stats = torch.full((n, 32), SENTINEL, dtype=torch.float64, device=DEV)
    ws = torch.full((need // 4 + 2,), SENTINEL, dtype=torch.float32, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def call(mode=0, min_weight=0.5, ws_ptr=None, ws_bytes=need, pd_=pd, st_ptr=None):
        return lib.fsg_svr_normal_f32(p(t["tr"]), p(t["jac"]), p(t["vol"]), p(t["psf"]), pd_, ph, pw, p(t["y"]), None, None,
                                      st_ptr or p(stats), *BC.VS, n, h, w, c["res"], min_weight, mode, ws_ptr or p(ws), ws_bytes,
                                      None)

    assert call(mode=_lib.SA.NEAREST_PSF) == _lib.E_BADARG and call(min_weight=-1.0) == _lib.E_BADARG
    assert call(min_weight=float("nan")) == _lib.E_BADARG and call(ws_bytes=need - 1) == _lib.E_BADARG
    assert call(ws_ptr=C.c_void_p(ws.data_ptr() + 4)) == _lib.E_ALIGN and call(pd_=65) == _lib.E_TOOBIG
    assert call(st_ptr=C.c_void_p(stats.data_ptr() + 4)) == _lib.E_ALIGN
    torch.cuda.synchronize()
    assert bool((stats == SENTINEL).all()) and bool((ws == SENTINEL).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((stats == SENTINEL).any()) and bool((ws[need // 4:] == SENTINEL).all())

    st = K.svr_state(n, 3, DEV)
    st.buf.fill_(-3)
    theta = torch.full((n, 6), SENTINEL, device=DEV)
    for kw in (dict(lambda0=0.0), dict(factor=1.0), dict(tol=-1.0)):
        with pytest.raises(_lib.FsgError):
            K.svr_update(st, 0, stats, theta, **kw)
    with pytest.raises(_lib.FsgError):
        K.svr_update(st, 4, stats, theta)
    with pytest.raises(ValueError):
        K.svr_update(st, 0, stats[:4], theta)
    with pytest.raises(ValueError):
        K.svr_normal(t["tr"], t["jac"][:, :6], t["vol"], t["psf"], t["y"], None, None, c["res"])
    with pytest.raises(ValueError):
        K.svr_normal(t["tr"], t["jac"], t["vol"], t["psf"], t["y"], None, None, c["res"], min_weight=-1.0)
    torch.cuda.synchronize()
    assert bool((st.buf == -3).all()) and bool((theta == SENTINEL).all())
