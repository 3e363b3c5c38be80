"""CPU: the restatement tests/util_tk1_64.py of the first-order regulariser (the rule is in
include/fsg_hip.h, fsg_tk1_apply_f32), the host side of the new entry, the launch sequence of `svort.srr` with `lam`, and the
generator's keywords.  No device is needed: refusals return before a launch, and the sequence tests replace the kernels by
recorders."""
import ctypes
import importlib
import inspect
import re
from dataclasses import fields
from pathlib import Path

import numpy as np
import pytest

from tests import util_srr64 as U
from tests import util_tk1_64 as T

ROOT = Path(__file__).resolve().parents[1]
F32, F64 = np.float32, np.float64
S345 = (3, 4, 5)


def _fields(shape, seed=7):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape), rng.standard_normal(shape), rng.random(shape) < 0.7, rng.uniform(0, 0.3, shape)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- L as a matrix --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", (False, True))
@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("ft", (F64, F32))
def test_dense_l_is_exactly_symmetric_with_zero_row_sums(ft, masked, guided):
    _, _, V, g = _fields(S345)
    mask, guide, delta = (V if masked else None), (g if guided else None), (0.05 if guided else None)
    L = T.dense(S345, mask, guide, delta, ft)
    assert L.dtype == ft and np.array_equal(L, L.T)  # exactly, not to a tolerance
    if guided:
        assert ((L != 0) & (np.abs(L) < 1) & ~np.eye(60, dtype=bool)).any()  # some edge is steeper than delta
    assert np.abs(L.astype(F64).sum(1)).max() <= (0 if not guided else 16 * np.finfo(ft).eps)  # guided: the roundings of the diagonal's six additions
    if masked:
        out = ~V.reshape(-1)
        assert out.any() and not L[out].any() and not L[:, out].any()


@pytest.mark.parametrize("guided", (False, True))
@pytest.mark.parametrize("masked", (False, True))
def test_quadratic_form_is_the_weighted_sum_over_the_edges(masked, guided):
    v, _, V, g = _fields(S345, 11)
    mask, guide, delta = (V if masked else None), (g if guided else None), (0.05 if guided else None)
    Lv = T.apply(v, np.zeros(S345), 1.0, mask, guide, delta)
    vf, gf = v.reshape(-1), g.reshape(-1)
    want = 0.0
    edges = T.edges(S345, mask)
    assert len(edges) == (133 if not masked else len(edges)) and len(edges) > 20  # 3*4*4 + 3*3*5 + 2*4*5 edges of the full grid
    for i, j in edges:
        a = abs(gf[i] - gf[j])
        c = 1.0 if not guided or a <= delta else delta / a
        want += c * (vf[i] - vf[j]) ** 2
    got = float((v * Lv).sum())
    assert abs(got - want) <= 1e-12 * want and want > 0


# ---- hand cases --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", (F64, F32))
@pytest.mark.parametrize("masked,guided", ((False, False), (True, False), (False, True), (True, True)))
def test_vectorised_restatement_equals_the_literal_loop(ft, masked, guided):
    p, t, V, g = _fields(S345, 3)
    mask, guide, delta = (V if masked else None), (g if guided else None), (0.05 if guided else None)
    assert same_bits(T.apply(p, t, 0.3, mask, guide, delta, ft), T.apply_loop(p, t, 0.3, mask, guide, delta, ft))


@pytest.mark.parametrize("ft", (F64, F32))
def test_hand_cases(ft):
    one = np.full((1, 1, 1), 3.0)
    assert same_bits(T.apply(one, one + 4, 0.5, ft=ft), (one + 4).astype(ft))  # a single voxel has no edge
    p, t = np.array([[[1.0, 4.0]]]), np.array([[[10.0, 20.0]]])
    assert T.apply(p, t, 0.5, ft=ft).tolist() == [[[10 + 0.5 * (1 - 4), 20 + 0.5 * (4 - 1)]]]
    # an edge exactly at a == delta has weight 1; just above it, delta / a
    delta = ft(0.25)
    g = np.array([[[0.0, delta]]], ft)
    assert T.apply(p, t, 0.5, guide=g, delta=delta, ft=ft).tolist() == [[[8.5, 21.5]]]
    up = np.nextafter(delta, ft(1))
    g2 = np.array([[[0.0, up]]], ft)
    c = ft(delta / up)
    assert c < 1
    want = [[[float(ft(10) + ft(ft(0.5) * ft(c * ft(-3)))), float(ft(20) + ft(ft(0.5) * ft(c * ft(3))))]]]
    assert T.apply(p, t, 0.5, guide=g2, delta=delta, ft=ft).tolist() == want
    # a mask that isolates a voxel: out = t there, and its neighbours do not see it
    p3, t3, _, _ = _fields((3, 3, 3), 5)
    V = np.zeros((3, 3, 3), bool)
    V[1, 1, 1] = True
    out = T.apply(p3, t3, 0.7, mask=V, ft=ft)
    assert same_bits(out, t3.astype(ft))
    V2 = np.ones((3, 3, 3), bool)
    V2[1, 1, 1] = False
    out2 = T.apply(p3, t3, 0.7, mask=V2, ft=ft)
    p_hole = p3.copy()
    p_hole[1, 1, 1] = 1e6
    assert same_bits(out2, T.apply(p_hole, t3, 0.7, mask=V2, ft=ft)) and out2[1, 1, 1] == ft(t3[1, 1, 1])
    # lam = 0
    assert same_bits(T.apply(p3, t3, 0.0, ft=ft), t3.astype(ft))
    # the order of the six neighbours matters in fp32 and is the stated one
    if ft is F32:
        pc = np.zeros((3, 3, 3), F32)
        pc[1, 1, 0], pc[1, 1, 2], pc[1, 0, 1] = 1e8, -1e8, 1.0  # x-, x+, y-
        got = T.apply(pc, np.zeros((3, 3, 3)), 1.0, ft=F32)[1, 1, 1]
        assert got == F32(F32(F32(-1e8) + F32(1e8)) + F32(-1.0)) == -1.0  # (x- + x+) + y-, not x- + (x+ + y-)


# ---- mutants -------------------------------------------------------------------------------------------------------------------------------
def test_mutant_mask_at_one_end_breaks_symmetry():
    _, _, V, _ = _fields(S345)
    L = T.dense(S345, V, None, None, F64, "mask_one_end")
    assert not np.array_equal(L, L.T)


def test_mutant_guide_at_one_end_breaks_symmetry():
    _, _, _, g = _fields(S345)
    L = T.dense(S345, None, g, 0.05, F64, "guide_one_end")
    assert not np.array_equal(L, L.T)


def test_mutant_wrapped_x_neighbour_differs_from_the_loop_on_1_2_3():
    shape = (1, 2, 3)
    p, t, _, _ = _fields(shape, 2)
    assert same_bits(T.apply(p, t, 1.0), T.apply_loop(p, t, 1.0))
    assert not same_bits(T.apply(p, t, 1.0, mutant="wrap_x"), T.apply_loop(p, t, 1.0))
    L = T.dense(shape, mutant="wrap_x")
    assert np.abs(L.sum(1)).max() == 0 and np.abs(T.dense(shape).sum(1)).max() == 0  # the row sums alone do not see it
    assert L[2, 3] == -1 and T.dense(shape)[2, 3] == 0  # the edge across the row end


# ---- the solve -----------------------------------------------------------------------------------------------------------------------------
def _small_reg(lam):
    from tests.test_srr64_reference import SMALL, _small

    op, y, z = _small(False)
    reg = T.RegOperator(op.tr, op.psf, SMALL, op.ss, 1.0, False, None, op.V, op.w, 0.5, F64, lam=lam)
    return op, reg, y, z


def test_srr_with_lam_reaches_the_dense_solution():
    from tests.test_srr64_reference import SMALL, _dense

    lam = 0.2
    M, _ = _dense(False)
    op, reg, y, z = _small_reg(lam)
    keep = op.V.reshape(-1)
    A = M + lam * T.dense(SMALL, op.V)
    rhs = op.mask(op.rhs_raw(y) + 0.5 * z).reshape(-1)
    want = np.zeros(A.shape[0])
    want[keep] = np.linalg.solve(A[np.ix_(keep, keep)], rhs[keep])
    x, h = U.cg(reg, y, 150, z=z, tol=1e-26)
    assert np.abs(x.reshape(-1) - want).max() <= 1e-8 * np.abs(want).max() and h["frozen"][-1] == 1
    x_plain, _ = U.cg(op, y, 150, z=z, tol=1e-26)
    assert np.abs(x_plain.reshape(-1) - want).max() > 1e-3 * np.abs(want).max()  # the regulariser is not a no-op here


@pytest.mark.parametrize("ft", (F64, F32))
def test_lam_0_reproduces_util_srr64_exactly(ft):
    c = U.solver_case("psf223_vm", False)
    plain = U.cg(U.case_operator(c, False, 0.0, ft), c["y"], 3, ft=ft)
    reg, hist = T.srr(T.case_maker(c, False, ft, lam=0.0), c["y"], 3, relu=False, ft=ft)
    assert same_bits(reg, plain[0]) and all(same_bits(hist[0][k], plain[1][k]) for k in ("rr", "pq", "alpha", "beta", "frozen"))


def test_e_cpu_and_capability_constants_are_what_is_measured():
    m = T.measure_e_cpu()
    assert set(m) == set(T.E_CPU_TK1)
    for key, bound in T.E_CPU_TK1.items():
        assert 0.98 * bound <= m[key] <= bound, (key, m[key], bound)
    got = {name: T.cap_run(name) for name in T.CAP_RUNS}
    assert set(got) == set(T.CAP_RMS)
    for name, bound in T.CAP_RMS.items():
        assert 0.995 * bound <= got[name] <= bound, (name, got[name], bound)
    assert got["piecewise_huber"] < got["piecewise_tk1"] < got["piecewise_none"]
    assert got["piecewise_huber"] < 0.7 * got["piecewise_tk1"] and got["piecewise_huber"] < 0.5 * got["piecewise_none"]


def test_piecewise_phantom_is_the_stated_one():
    vol = T.piecewise_phantom()
    D, H, W = T.BC.VS
    cz, cy, cx = (D - 1) / 2, (H - 1) / 2, (W - 1) / 2
    want = np.zeros(T.BC.VS)
    for z in range(D):
        for y in range(H):
            for x in range(W):
                r2 = ((z - cz) / (0.38 * D)) ** 2 + ((y - cy) / (0.38 * H)) ** 2 + ((x - cx) / (0.38 * W)) ** 2
                v = (1.0 if r2 < 1 else 0.0) + (0.8 if r2 < 0.35 else 0.0)
                if abs(z - cz - 2) < 2.5 and abs(y - cy + 2) < 3 and abs(x - cx) < 2.5:
                    v -= 0.6
                want[z, y, x] = v
    assert vol.shape == tuple(T.BC.VS) and vol.dtype == F32 and np.array_equal(vol, want.astype(F32))
    assert sorted(np.unique(vol).tolist()) == pytest.approx([0.0, 0.4, 1.0, 1.2, 1.8])  # piecewise constant, five levels


# ---- the host side of the entry ----------------------------------------------------------------------------------------------------------
def test_header_build_list_abi_and_exports():
    from fetalsyngen_amd import _build, _lib
    from fetalsyngen_amd import kernels as K

    text = (ROOT / "include" / "fsg_hip.h").read_text()
    assert re.search(r"\bfsg_tk1_apply_f32\s*\(", text) and "fsg_tk1_apply_f32" in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES["fsg_tk1_apply_f32"]
    assert res is ctypes.c_int and len(args) == 11 and args[4] is ctypes.c_float and args[5] is ctypes.c_float
    assert _lib.ABI_VERSION == 8
    assert "fsg_tk1.hip" in _build.SOURCES and (ROOT / "fetalsyngen_amd" / "csrc" / "fsg_tk1.hip").exists()
    assert callable(K.tk1_apply)
    assert list(inspect.signature(K.tk1_apply).parameters) == ["p", "t", "shape", "lam", "mask", "guide", "delta", "out"]


def test_entry_refuses_before_any_launch():
    """no device is needed: every refusal returns before the launch (the addresses are made up)"""
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    D, H, W = 4, 5, 6
    n = D * H * W
    p, t, m, g, out = (ctypes.c_void_p((i + 1) << 24) for i in range(5))
    null = ctypes.c_void_p(0)

    def call(p=p, t=t, m=m, g=g, delta=0.05, lam=0.1, D=D, H=H, W=W, out=out):
        return lib.fsg_tk1_apply_f32(p, t, m, g, delta, lam, D, H, W, out, None)

    for kw in (dict(p=null), dict(t=null), dict(out=null)):
        assert call(**kw) == _lib.E_BADARG, kw
    for dim in "DHW":
        for v in (0, -1):
            assert call(**{dim: v}) == _lib.E_BADARG, (dim, v)
    for lam in (-1e-3, float("inf"), float("nan"), -float("inf")):
        assert call(lam=lam) == _lib.E_BADARG, lam
    for delta in (0.0, -0.05, float("inf"), float("nan")):
        assert call(delta=delta) == _lib.E_BADARG, delta
    assert call(D=2048, H=2048, W=512) == _lib.E_TOOBIG
    # out must not share a byte with p, guide or mask; t is allowed only as out itself
    last = 4 * n - 1
    for other in (p, g):
        for off in (0, last, -last):
            assert call(out=ctypes.c_void_p(other.value + off)) == _lib.E_BADARG, off
    for off in (0, n - 1, -last):
        assert call(out=ctypes.c_void_p(m.value + off)) == _lib.E_BADARG, off
    for off in (4, last, -last, -4):
        assert call(out=ctypes.c_void_p(t.value + off)) == _lib.E_BADARG, off


def test_front_end_refuses_cpu_tensors_and_bad_arguments():
    import torch

    from fetalsyngen_amd import kernels as K

    v = torch.zeros(2, 3, 4)
    with pytest.raises(RuntimeError, match="MI355X"):
        K.tk1_apply(v, v.clone(), (2, 3, 4), 0.1)
    with pytest.raises(RuntimeError, match="MI355X"):
        K.tk1_apply(v, v.clone(), (2, 3, 4), 0.1, out=v.clone())


def test_srr_argument_rules():
    import torch

    from fetalsyngen_amd.generator.artifacts import svort

    args = (torch.zeros(2, 3, 4), torch.zeros(2, 1, 4, 4), torch.ones(1, 1, 1), (4, 4, 4), 1.0)
    for kw in (dict(huber_delta=0.05), dict(huber_delta=0.05, lam=0.0), dict(lam=0.1, n_outer=2), dict(lam=0.1, n_outer=0),
               dict(n_outer=0), dict(lam=-0.1), dict(lam=float("nan")), dict(lam=0.1, huber_delta=0.0),
               dict(lam=0.1, guide=torch.zeros(4, 4, 4))):
        with pytest.raises(ValueError):
            svort.srr(*args, n_iter=1, **kw)
    with pytest.raises(NotImplementedError, match="guide"):
        svort.srr(*args, n_iter=1, lam=0.1, huber_delta=0.05, guide=torch.zeros(4, 4, 4, requires_grad=True))


# ---- the launch sequence (kernels replaced by recorders: no device) ----------------------------------------------------------------------
class _WS:
    def __init__(self, log):
        self.id = sum(1 for e in log if e[0] == "workspace")

    def info(self):
        return {"ws": self.id}


@pytest.fixture
def recorded(monkeypatch):
    import torch

    module = importlib.import_module("fetalsyngen_amd.generator.artifacts.svort.srr")
    log = []
    vs = (4, 4, 4)

    def rec(name, result=None):
        def f(*a, **kw):
            log.append((name, a, kw))
            return result() if result else None
        return f

    def workspace(n, n_iter, device):
        ws = _WS(log)
        log.append(("workspace", (n, n_iter), {}))
        return ws

    monkeypatch.setattr(module.K, "slice_acq_forward", rec("forward", lambda: torch.zeros(2, 4, 4)))
    monkeypatch.setattr(module.K, "slice_acq_adjoint", rec("adjoint", lambda: torch.zeros(vs)))
    monkeypatch.setattr(module.K, "mul", rec("mul", lambda: torch.zeros(2, 4, 4)))
    monkeypatch.setattr(module.K, "cg_workspace", workspace)
    for name in ("cg_init", "cg_q", "cg_step", "cg_dir", "tk1_apply"):
        monkeypatch.setattr(module.K, name, rec(name))
    run = lambda **kw: module.srr(torch.zeros(2, 3, 4), torch.zeros(2, 1, 4, 4), torch.ones(1, 1, 1), vs, 1.0, **kw)  # noqa: E731
    return run, log


def _names(log):
    return [e[0] for e in log]


TODAY = ["workspace", "adjoint", "cg_init"] + ["forward", "adjoint", "cg_q", "cg_step", "cg_dir"] * 2


def test_lam_0_records_todays_sequence(recorded):
    run, log = recorded
    run(n_iter=2)
    assert _names(log) == TODAY
    del log[:]
    run(n_iter=2, lam=0.0, n_outer=1)
    assert _names(log) == TODAY and "tk1_apply" not in _names(log)
    del log[:]
    out, info = run(n_iter=2, return_info=True)
    assert info == {"ws": 0} and out.shape == (1, 1, 4, 4, 4)  # and today's dict: "rounds" comes with lam > 0 only
    del log[:]
    _, info = run(n_iter=2, lam=0.5, return_info=True)
    assert info == {"ws": 0, "rounds": [{"ws": 0}]}


def test_lam_with_two_rounds_records_the_expected_sequence(recorded):
    import torch

    run, log = recorded
    vm = torch.ones(4, 4, 4, dtype=torch.bool)
    out, info = run(n_iter=2, lam=0.25, huber_delta=0.05, n_outer=2, vol_mask=vm, return_info=True)
    it = ["forward", "adjoint", "tk1_apply", "cg_q", "cg_step", "cg_dir"]
    assert _names(log) == (["workspace", "adjoint", "cg_init"] + it * 2  # round 0: x0 = None, so no t0
                           + ["workspace", "forward", "adjoint", "tk1_apply", "cg_init"] + it * 2)
    assert [e[2]["relu"] for e in log if e[0] == "cg_step"] == [False, False, True, True]
    tk = [e for e in log if e[0] == "tk1_apply"]
    # round 0 is plain TK1; round 1 is guided by round 0's x with huber_delta, and starts from it
    assert all(e[2]["guide"] is None and e[2]["delta"] is None for e in tk[:2])
    x_round0 = [e for e in log if e[0] == "cg_init"][0][1][4]
    assert all(e[2]["guide"] is x_round0 and e[2]["delta"] == 0.05 for e in tk[2:])
    init1 = [e for e in log if e[0] == "cg_init"][1]
    assert init1[2]["x0"] is x_round0 and init1[2]["t0"] is tk[2][2]["out"] and tk[2][1][0] is x_round0
    for e in tk:
        assert e[1][2] == (4, 4, 4) and e[1][3] == 0.25 and e[2]["mask"].dtype == torch.bool and e[2]["out"] is e[1][1]
    for e in tk[:2] + tk[3:]:
        q = [c for c in log if c[0] == "cg_q" and c[1][3] is e[1][1]]
        assert len(q) == 1 and q[0][1][2] is e[1][0]  # tk1_apply(p, t) then cg_q(ws, k, p, t)
    assert info["rounds"] == [{"ws": 0}, {"ws": 1}] and info["ws"] == 1
    del log[:]
    run(n_iter=1, lam=0.25, output_relu=False, x0=torch.ones(4, 4, 4))
    assert _names(log) == ["workspace", "adjoint", "forward", "adjoint", "tk1_apply", "cg_init"] + it
    assert [e[2]["relu"] for e in log if e[0] == "cg_step"] == [False]
    del log[:]
    g = torch.ones(4, 4, 4)
    run(n_iter=1, lam=0.25, huber_delta=0.1, guide=g)
    (e,) = [e for e in log if e[0] == "tk1_apply"]
    assert torch.equal(e[2]["guide"], g) and e[2]["delta"] == 0.1


# ---- the generator's keywords (recorders: no device) --------------------------------------------------------------------------------------
def test_srr_class_hands_the_regulariser_on_only_when_set(monkeypatch):
    module = importlib.import_module("fetalsyngen_amd.generator.artifacts.svort.srr")
    seen = {}

    def solve(transforms, slices, psf, vol_shape, res_slice, **kw):
        seen.clear()
        seen.update(kw)
        return "x"

    monkeypatch.setattr(module, "srr", solve)
    params = {"psf": "PSF", "res_s": 1.5, "res_r": 0.5, "volume_shape": (4, 5, 6)}
    sig = inspect.signature(module.SRR.__init__).parameters
    assert (sig["lam"].default, sig["huber_delta"].default, sig["n_outer"].default) == (0.0, None, 1)
    module.SRR(4)(None, None, None, params)
    assert not {"lam", "huber_delta", "n_outer"} & set(seen)
    module.SRR(4, lam=0.1)(None, None, None, params)
    assert seen["lam"] == 0.1 and not {"huber_delta", "n_outer"} & set(seen)
    module.SRR(4, lam=0.1, huber_delta=0.05, n_outer=3)(None, None, None, params)
    assert (seen["lam"], seen["huber_delta"], seen["n_outer"]) == (0.1, 0.05, 3)


def test_reconstructor_and_simulate_motion_hand_the_regulariser_on(monkeypatch):
    import torch

    from fetalsyngen_amd.generator.artifacts import simulate_reco as SR
    from fetalsyngen_amd.generator.artifacts.utils import ReconMergeParams, ReconParams
    from fetalsyngen_amd.generator.augmentation import artifacts as A
    from tests.test_adjoint_det_wiring_host import VS, _data, _recon

    for cls in (SR.PSFReconstructor, A.SimulateMotion):
        sig = inspect.signature(cls.__init__).parameters
        assert (sig["srr_lambda"].default, sig["srr_huber_delta"].default, sig["srr_outer"].default) == (0.0, None, 1)
    with pytest.raises(ValueError):
        _recon(srr_lambda=0.1)  # without srr_iterations there is no solve to regularise
    calls = []

    def solve(transforms, slices, psf, vol_shape, res_slice, **kw):
        calls.append(kw)
        return torch.full((1, 1, *vol_shape), 3.0)

    monkeypatch.setattr(SR, "slice_acquisition_adjoint", lambda *a, **kw: torch.full((1, 1, *VS), 2.0))
    monkeypatch.setattr(SR, "srr", solve)
    monkeypatch.setattr(SR.K, "_upload", lambda host, device: host)
    plain = _recon(srr_iterations=3)
    plain.recon_psf(_data(), want_weight=False)
    assert not {"lam", "huber_delta", "n_outer"} & set(calls[-1])
    assert not {"srr_lambda", "srr_huber_delta", "srr_outer"} & set(plain.get_seeds())
    one = _recon(srr_iterations=3, srr_lambda=0.1)
    one.recon_psf(_data(), want_weight=False)
    assert calls[-1]["lam"] == 0.1 and not {"huber_delta", "n_outer"} & set(calls[-1])
    assert one.get_seeds()["srr_lambda"] == 0.1 and "srr_outer" not in one.get_seeds()
    full = _recon(srr_iterations=3, srr_lambda=0.1, srr_huber_delta=0.05, srr_outer=4)
    full.recon_psf(_data(), want_weight=False)
    assert (calls[-1]["lam"], calls[-1]["huber_delta"], calls[-1]["n_outer"], calls[-1]["n_iter"]) == (0.1, 0.05, 4, 3)
    seeds = full.get_seeds()
    assert (seeds["srr_lambda"], seeds["srr_huber_delta"], seeds["srr_outer"]) == (0.1, 0.05, 4)
    # SRRreconstruction takes them from `params`
    params = {"psf": "P", "interp_psf": True, "res_s": 1.0, "res_r": 1.0, "volume_shape": VS, "lam": 0.2, "n_outer": 1}
    SR.SRRreconstruction(None, None, None, None, params, 2)
    assert calls[-1]["lam"] == 0.2 and calls[-1]["n_outer"] == 1 and "huber_delta" not in calls[-1]

    built = []

    class Recon:
        def __init__(self, **kw):
            built.append(kw)

        def recon_psf(self, data, want_weight=True):
            return torch.zeros(1, 1, *VS), None

        def get_seeds(self):
            return {}

    class Scan:
        def __init__(self, **kw):
            pass

        def scan(self, d):
            return {"resolution_recon": 1.0, "resolution_slice": 1.0, "slice_thickness": 1.0, "gap": 1.0,
                    "positions_host": torch.zeros(3, 2)}

    monkeypatch.setattr(A, "PSFReconstructor", Recon)
    monkeypatch.setattr(A, "Scanner", Scan)
    monkeypatch.setattr(A, "_need_gpu", lambda *a: None)
    monkeypatch.setattr(A.K, "threshold", lambda x, v: (x > v).float())
    recon_params = ReconParams(prob_misreg_slice=0.0, slices_misreg_ratio=0.0, prob_misreg_stack=0.0, txy=0.0, prob_smooth=0.0,
                               prob_rm_slices=0.0, rm_slices_min=0.0, rm_slices_max=0.0, prob_merge=0.0,
                               merge_params=ReconMergeParams(merge_type="gaussian"))
    scanner_params = A.ScannerParams(**{f.name: None for f in fields(A.ScannerParams)})
    vol = torch.zeros(VS)
    base = {f.name for f in fields(ReconParams)} | {"deterministic"}
    for kw, extra in (({}, {}), (dict(srr_iterations=2), dict(srr_iterations=2, srr_mu=0.0)),
                      (dict(srr_iterations=2, srr_lambda=0.1, srr_huber_delta=0.05, srr_outer=2),
                       dict(srr_iterations=2, srr_mu=0.0, srr_lambda=0.1, srr_huber_delta=0.05, srr_outer=2))):
        A.SimulateMotion(1.0, scanner_params, recon_params, **kw)(vol, vol, "cpu", resolution=(1.0, 1.0, 1.0))
        assert set(built[-1]) == base | set(extra) and all(built[-1][k] == v for k, v in extra.items())
