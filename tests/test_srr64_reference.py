"""CPU: the restatement of `svort.srr` (tests/util_srr64.py) checked against what does not depend on it -- the oracle's forward,
adjoint64, a dense solve, hand-worked freeze cases, three mutants -- and the host side of the new entries (header, build list,
refusals before any launch, front-end checks, exports).  DESIGN.md section 22.
"""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests import util_sa_backward_cases as BC
from tests import util_srr64 as U
from tests.util_sa_adjoint_backward64 import adjoint64

ROOT = Path(__file__).resolve().parents[1]
F32, F64 = np.float32, np.float64
MODES = (False, True)


# ---- the operators against their yardsticks ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp_psf", MODES)
@pytest.mark.parametrize("name", U.SOLVER_CASES)
def test_forward_restatement_is_the_oracles_forward(name, interp_psf):
    """the oracle is fp32 in the kernel's order; the restatement in float32 differs by the association of a few products at
    most (8 ulp of the largest value), in float64 by fp32 rounding of sums of <= 360 terms"""
    from oracle.fsg_oracle_sr import slice_acq_forward_cuda

    c = BC.general_case(name, interp_psf)
    ss = c["g"].shape[1:]
    want, wwant = slice_acq_forward_cuda(c["tr"], c["vol"], None, c["sm"], c["psf"], ss, c["res"], True, interp_psf)
    scale = np.abs(want).max()
    for ft, tol in ((F32, 8 * 2.0 ** -24), (F64, 360 * 2.0 ** -24)):
        got, wgot = U.forward(c["tr"], c["vol"], c["psf"], c["sm"], ss, c["res"], interp_psf, ft)
        assert np.abs(got - want).max() <= tol * scale
        assert np.abs(wgot - wwant).max() <= tol * np.abs(wwant).max()
        assert ((got != 0) == (want != 0)).all()


@pytest.mark.parametrize("interp_psf", MODES)
@pytest.mark.parametrize("name", U.SOLVER_CASES)
def test_adjoint_restatement_is_adjoint64(name, interp_psf):
    c = BC.general_case(name, interp_psf)
    for ft in (F64, F32):
        want = adjoint64(c["tr"], c["psf"], c["g"], c["sm"], None, BC.VS, c["res"], interp_psf, False, ft=ft)
        got, wgt = U.adjoint(c["tr"], c["psf"], c["g"], c["sm"], BC.VS, c["res"], interp_psf, ft)
        assert np.array_equal(got, want["vol"]) and np.array_equal(wgt, want["pixel_weight"])


@pytest.mark.parametrize("interp_psf", MODES)
@pytest.mark.parametrize("name", U.SOLVER_CASES)
def test_one_mask_serves_the_whole_solve(name, interp_psf):
    """the decisions depend on the geometry alone; the mask keeps the pixels whose every decision is safe, the 0.5 cut included"""
    c = U.solver_case(name, interp_psf)
    assert c["kept"] >= U.MIN_KEPT
    assert not (c["sm"] & ~c["sm_own"]).any()
    _, wgt = U.adjoint(c["tr"], c["psf"], np.zeros((BC.N, *c["ss"])), None, BC.VS, c["res"], interp_psf)
    assert (np.abs(wgt[c["sm"]] - 0.5) > 1e-3).all()


def _weights(case, seed=5):
    return np.random.default_rng(seed).uniform(0.2, 1.5, case["y"].shape)


@pytest.mark.parametrize("mu", (0.0, 0.5))
@pytest.mark.parametrize("use_V", (False, True))
@pytest.mark.parametrize("use_w", (False, True))
@pytest.mark.parametrize("interp_psf", MODES)
def test_operator_is_symmetric_positive_semidefinite(interp_psf, use_w, use_V, mu):
    c = U.solver_case("psf223_vm", interp_psf)
    op = U.case_operator(c, interp_psf, mu, F64, w=_weights(c) if use_w else None, use_V=use_V)
    rng = np.random.default_rng(11)
    u, v = rng.standard_normal(BC.VS), rng.standard_normal(BC.VS)
    if use_V:  # M is symmetric on the range of V, where the solve lives
        u, v = op.mask(u), op.mask(v)
    a, b = U.dot64(op(u), v), U.dot64(u, op(v))
    assert abs(a - b) <= 1e-12 * abs(a)
    assert U.dot64(u, op(u)) >= 0


# ---- the solve against a dense one ----------------------------------------------------------------------------------------------------
SMALL = (6, 5, 7)


def _small(interp_psf, mutant=None):
    rng = np.random.default_rng(31)
    n, ss = 6, (7, 6)
    tr = np.zeros((n, 3, 4), F32)
    for i in range(n):
        tr[i, :, :3] = BC.rotation(rng, 1.0)
        tr[i, :, 3] = rng.uniform(-1.5, 1.5, 3)
    psf = rng.uniform(0.1, 1.0, (2, 2, 3)).astype(F32)
    V = rng.random(SMALL) < 0.8
    w = rng.uniform(0.2, 1.5, (n, *ss))
    y = rng.standard_normal((n, *ss))
    z = rng.standard_normal(SMALL)
    op = U.Operator(tr, psf, SMALL, ss, 1.0, interp_psf, None, V, w, 0.5, F64, mutant)
    return op, y, z


_DENSE = {}


def _dense(interp_psf):
    """M from 210 applications of the unmutated operator, and the solution of M x = V(b + mu z) by numpy.linalg.solve"""
    if interp_psf not in _DENSE:
        op, y, z = _small(interp_psf)
        nv = int(np.prod(SMALL))
        M = np.zeros((nv, nv))
        for j in range(nv):
            e = np.zeros(nv)
            e[j] = 1
            M[:, j] = op(e.reshape(SMALL)).reshape(-1)
        keep = op.V.reshape(-1)
        rhs = op.mask(op.rhs_raw(y) + 0.5 * z).reshape(-1)
        x = np.zeros(nv)
        x[keep] = np.linalg.solve(M[np.ix_(keep, keep)], rhs[keep])
        _DENSE[interp_psf] = (M, x.reshape(SMALL))
    return _DENSE[interp_psf]


@pytest.mark.parametrize("interp_psf", MODES)
def test_cg_reaches_the_dense_solution_from_either_start(interp_psf):
    M, want = _dense(interp_psf)
    assert np.abs(M - M.T).max() <= 1e-13 * np.abs(M).max()
    assert (~np.asarray(_small(interp_psf)[0].V)).any() and (want[~_small(interp_psf)[0].V] == 0).all()
    op, y, z = _small(interp_psf)
    x0 = np.random.default_rng(3).standard_normal(SMALL)
    for start in (None, x0):
        x, h = U.cg(op, y, 150, x0=start, z=z, tol=1e-26)
        assert np.abs(x - want).max() <= 1e-8 * np.abs(want).max()
        assert h["frozen"][-1] == 1  # it stopped by itself, well before 150


@pytest.mark.parametrize("mutant", ("beta_swapped", "no_P", "no_V_on_q"))
def test_mutants_miss_the_dense_solution(mutant):
    """beta with old and new <r,r> exchanged; the 0.5 cut of P left out (it lives in the adjoint leg: util_srr64); V left off q"""
    _, want = _dense(False)
    op, y, z = _small(False, None if mutant == "beta_swapped" else mutant)
    if mutant == "no_P":
        assert op.P().sum() < U.Operator(op.tr, op.psf, SMALL, op.ss, 1.0, False, mutant=None).P().size  # some pixel is cut
    x, _ = U.cg(op, y, 150, z=z, tol=1e-26, mutant=mutant if mutant == "beta_swapped" else None,
                b=_small(False)[0].rhs_raw(y))  # the right-hand side is the true one: only the operator or the recurrence is wrong
    assert not np.abs(x - want).max() <= 1e-8 * np.abs(want).max()


# ---- the freeze rule by hand --------------------------------------------------------------------------------------------------------
class Diag:
    """M = diag(d) behind Operator's interface (b is given to cg directly)"""

    def __init__(self, d, ft):
        self.d, self.ft, self.vs, self.V, self.mu = np.asarray(d, ft), ft, (len(d),), None, ft(0)

    def mask(self, v):
        return v

    def normal(self, v):
        return (self.d * np.asarray(v, self.ft)).astype(self.ft)

    __call__ = normal


@pytest.mark.parametrize("ft", (F64, F32))
def test_freeze_when_tol_is_reached_at_k_2(ft):
    """diag(1, 4), b = (1, 1): CG is exact after two iterations.  By hand: rr0 = 2, alpha1 = 2/5, r1 = (3/5, -3/5), rr1 = 18/25,
    beta1 = 9/25, p1 = (24/25, -6/25), pq2 = 144/125, alpha2 = 5/8, x = (1, 1/4), rr2 = 0 (up to rounding)"""
    op, b = Diag([1.0, 4.0], ft), np.array([1.0, 1.0], ft)
    x, h = U.cg(op, None, 5, b=b, tol=1e-10, ft=ft)
    x2, h2 = U.cg(op, None, 2, b=b, tol=1e-10, ft=ft)
    eps = 1e-6 if ft is F32 else 1e-14
    assert h["frozen"].tolist() == [0, 0, 1, 1, 1, 1]
    assert np.allclose(h["rr"][:3], [2, 18 / 25, 0], atol=eps) and np.allclose(h["alpha"][1:3], [2 / 5, 5 / 8], rtol=eps)
    assert abs(h["beta"][1] - 9 / 25) <= eps and abs(h["pq"][2] - 144 / 125) <= eps * 2
    assert np.allclose(x, [1, 0.25], atol=eps) and np.array_equal(x, x2)  # what an early return at k = 2 returns, bit for bit
    assert (h["alpha"][3:] == 0).all() and (h["pq"][3:] == 0).all() and (h["rr"][3:] == h["rr"][2]).all()
    assert np.array_equal(h["rr"][:3], h2["rr"]) and np.array_equal(h["alpha"][:3], h2["alpha"])


@pytest.mark.parametrize("ft", (F64, F32))
def test_freeze_on_a_zero_right_hand_side_and_on_pq_0(ft):
    x, h = U.cg(Diag([1.0, 4.0], ft), None, 3, b=np.zeros(2, ft), ft=ft)
    assert h["frozen"].tolist() == [1, 1, 1, 1] and (x == 0).all() and (h["alpha"] == 0).all()
    # M = 0 on the direction: <p, M p> = 0, no step is taken and nothing becomes NaN
    x, h = U.cg(Diag([0.0, 0.0], ft), None, 3, b=np.array([1.0, 2.0], ft), ft=ft)
    assert h["frozen"].tolist() == [0, 1, 1, 1] and (x == 0).all() and h["rr"].tolist() == [5.0] * 4
    assert np.isfinite(h["alpha"]).all() and np.isfinite(h["beta"]).all()
    # a NaN direction freezes too
    x, h = U.cg(Diag([np.nan, 1.0], ft), None, 2, b=np.array([1.0, 2.0], ft), ft=ft)
    assert h["frozen"].tolist() == [0, 1, 1] and (x == 0).all()


def test_dot32_order_is_the_documented_one():
    """against a literal transcription for a size with a tail group and more than one workgroup"""
    rng = np.random.default_rng(2)
    n = 4099
    a, b = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    B = U.cg_blocks(n)
    assert B == 5 and U.cg_blocks(1) == 1 and U.cg_blocks(1024) == 1 and U.cg_blocks(1025) == 2 and U.cg_blocks(1 << 21) == 1024
    T = 256 * B
    acc = [0.0] * T
    for e in range(n):
        acc[(e // 4) % T] += float(a[e]) * float(b[e])
    parts = []
    for blk in range(B):
        waves = []
        for wv in range(4):
            v = acc[blk * 256 + wv * 64: blk * 256 + wv * 64 + 64]
            for o in (32, 16, 8, 4, 2, 1):
                v = [v[i] + v[i ^ o] for i in range(64)]
            waves.append(v[0])
        parts.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    assert np.array_equal(U.dot32_partials(a, b), np.array(parts))
    assert U.dot32(a, b) == sum(parts[1:], parts[0] + 0.0)
    assert abs(U.dot32(a, b) - U.dot64(a, b)) <= 1e-12 * float(np.abs(a.astype(F64) * b).sum())


def test_e_cpu_constants_are_what_is_measured():
    m = U.measure_e_cpu()
    for table, i in ((U.E_CPU, 0), (U.E_CPU_RR, 1), (U.E_CPU_ALPHA, 2)):
        assert set(table) == set(m)
        for key, bound in table.items():
            assert 0.98 * bound <= m[key][i] <= bound, (key, i, m[key][i], bound)


def test_capability_case_in_float64_more_than_halves_the_residual():
    """the figures in util_srr64's docstring"""
    cap = U.capability_case()
    op = U.Operator(cap["tr"], cap["psf"], BC.VS, cap["ss"], cap["res"], False)
    x0 = U.equalised_x0(cap)
    x6, _ = U.cg(op, cap["y"], 6, x0=x0, relu=True)
    r0, r6 = U.data_residual(op, cap["y"], x0), U.data_residual(op, cap["y"], x6)
    assert abs(r0 - 4.5643) < 1e-3 and abs(r6 - 0.021086) < 1e-5 and r6 < 0.5 * r0


# ---- the host side of the new entries ---------------------------------------------------------------------------------------------------
ENTRIES = ("fsg_cg_ws_bytes", "fsg_cg_init_f32", "fsg_cg_q_f32", "fsg_cg_step_f32", "fsg_cg_dir_f32")


def test_header_build_list_and_abi():
    from fetalsyngen_amd import _build, _lib

    text = (ROOT / "include" / "fsg_hip.h").read_text()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", text) and name in _lib.PROTOTYPES
    assert _lib.ABI_VERSION == 8 and _lib.CG_RELU == 1
    assert "fsg_cg.hip" in _build.SOURCES and (ROOT / "fetalsyngen_amd" / "csrc" / "fsg_cg.hip").exists()


def _calls(lib, n, k, K, ws, nbytes, ptrs=None, flags=0):
    b, z, t0, x0, m, r, p, x, q = ptrs or (ctypes.c_void_p((i + 1) << 24) for i in range(9))
    return {
        "init": lambda: lib.fsg_cg_init_f32(b, z, t0, x0, m, 0.5, n, K, r, p, x, ws, nbytes, None),
        "q": lambda: lib.fsg_cg_q_f32(p, q, m, 0.5, 0.0, n, k, K, ws, nbytes, None),
        "step": lambda: lib.fsg_cg_step_f32(p, q, x, r, n, k, K, flags, ws, nbytes, None),
        "dir": lambda: lib.fsg_cg_dir_f32(r, p, 0.0, n, k, K, ws, nbytes, None),
    }


def test_entries_refuse_before_any_launch():
    """no device is needed: every refusal, and n == 0, returns before the first launch (the addresses are made up)"""
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    n, K = 5000, 6
    need = lib.fsg_cg_ws_bytes(n, K)
    s, B = K + 1, U.cg_blocks(n)
    assert need == (16 * s + 16 * B + 12 * s + 7) // 8 * 8
    assert lib.fsg_cg_ws_bytes(n, 0) == 0 and lib.fsg_cg_ws_bytes(n, 4097) == 0 and lib.fsg_cg_ws_bytes(0, 1) > 0
    ws = ctypes.c_void_p(100 << 24)
    null = ctypes.c_void_p(0)
    for name, call in _calls(lib, 0, 1, K, null, 0, ptrs=(null,) * 9).items():
        assert call() == 0, name  # n == 0: success, nothing launched, nothing looked at
    for k, kk in ((0, K), (K + 1, K), (1, 0), (1, 4097), (-1, K)):
        for name, call in _calls(lib, n, k, kk, ws, 1 << 20).items():
            if name == "init" and 1 <= kk <= 4096:
                continue  # init has no k
            assert call() == _lib.E_BADARG, (name, k, kk)
    for name, call in _calls(lib, n, 1, K, ws, need - 1).items():
        assert call() == _lib.E_BADARG, name
    for name, call in _calls(lib, n, 1, K, null, need).items():
        assert call() == _lib.E_BADARG, name
    for name, call in _calls(lib, n, 1, K, ctypes.c_void_p((100 << 24) + 4), need).items():
        assert call() == _lib.E_ALIGN, name
    assert _calls(lib, n, 1, K, ws, need, flags=2)["step"]() == _lib.E_BADARG
    base = [ctypes.c_void_p((i + 1) << 24) for i in range(9)]  # b z t0 x0 m r p x q
    required = {"init": (0, 5, 6, 7), "q": (6, 8), "step": (5, 6, 7, 8), "dir": (5, 6)}
    for name, idx in required.items():
        for i in idx:
            ptrs = list(base)
            ptrs[i] = null
            assert _calls(lib, n, 1, K, ws, need, ptrs=ptrs)[name]() == _lib.E_BADARG, (name, i)
    ptrs = list(base)
    ptrs[2] = null  # x0 without t0
    assert _calls(lib, n, 1, K, ws, need, ptrs=ptrs)["init"]() == _lib.E_BADARG
    # an output that shares a byte with an input, another output or the scalar block
    last = 4 * n - 1
    shares = {"init": ((5, 0), (6, 1), (7, 3), (5, 4), (5, 6), (6, 7)), "q": ((8, 6), (8, 4)), "step": ((7, 6), (5, 8), (7, 5)),
              "dir": ((6, 5),)}
    for name, pairs in shares.items():
        for out, inp in pairs:
            for off in (0, last, -last):
                ptrs = list(base)
                ptrs[out] = ctypes.c_void_p(base[inp].value + off)
                if inp == 4 and off > 0:
                    ptrs[out] = ctypes.c_void_p(base[inp].value + n - 1)  # the mask has n bytes
                assert _calls(lib, n, 1, K, ws, need, ptrs=ptrs)[name]() == _lib.E_BADARG, (name, out, inp, off)
        for out in {o for o, _ in pairs}:
            ptrs = list(base)
            ptrs[out] = ctypes.c_void_p(ws.value + need - 1)
            assert _calls(lib, n, 1, K, ws, need, ptrs=ptrs)[name]() == _lib.E_BADARG, (name, out, "ws")


@pytest.mark.parametrize("K", (1, 2, 12, 4096))
@pytest.mark.parametrize("n", (1, 5, 1024, 1025, 2**20 + 1, 2**20 + 1025))
def test_ws_bytes_is_the_headers_formula(n, K):
    """fsg_cg_ws_bytes against the layout paragraph of include/fsg_hip.h, written out: rr, pq (double[s]), the two partial
    arrays (double[B]), alpha, beta, frozen (4 bytes, [s]), rounded up to 8; s = K + 1 takes both parities, B its clamp"""
    from fetalsyngen_amd import _lib

    s, B = K + 1, min(max(-(-n // 1024), 1), 1024)
    assert B == (1024 if n > 2**20 else {1: 1, 5: 1, 1024: 1, 1025: 2}[n])
    assert _lib.load().fsg_cg_ws_bytes(n, K) == -(-(16 * s + 16 * B + 12 * s) // 8) * 8
    assert _lib.load().fsg_cg_ws_bytes(n, 0) == 0 and _lib.load().fsg_cg_ws_bytes(n, 4096 + 1) == 0


def test_front_ends_refuse_cpu_tensors():
    import torch

    from fetalsyngen_amd import kernels as K
    from fetalsyngen_amd.generator.artifacts import svort

    v = torch.zeros(8)

    class WS:  # a workspace is only ever made on a device; the checks come before it is used
        n, n_iter, nbytes, buf = 8, 2, 0, v
    for call in (lambda: K.cg_init(WS, v, v.clone(), v.clone(), v.clone()), lambda: K.cg_q(WS, 1, v, v.clone()),
                 lambda: K.cg_step(WS, 1, v, v.clone(), v.clone(), v.clone()), lambda: K.cg_dir(WS, 1, v, v.clone())):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()
    with pytest.raises(ValueError):
        K.cg_workspace(8, 0, "cpu")
    with pytest.raises(ValueError):
        K.cg_workspace(8, 4097, "cpu")
    with pytest.raises(RuntimeError, match="MI355X"):
        svort.srr(torch.zeros(2, 3, 4), torch.zeros(2, 1, 4, 4), torch.ones(1, 1, 1), (4, 4, 4), 1.0, n_iter=1)


def test_srr_is_not_differentiable():
    import torch

    from fetalsyngen_amd.generator.artifacts import svort

    args = dict(transforms=torch.zeros(2, 3, 4), slices=torch.zeros(2, 1, 4, 4), psf=torch.ones(1, 1, 1))
    for name in ("transforms", "slices"):
        a = {k: (v.clone().requires_grad_(True) if k == name else v) for k, v in args.items()}
        with pytest.raises(NotImplementedError, match=name):
            svort.srr(a["transforms"], a["slices"], a["psf"], (4, 4, 4), 1.0, n_iter=1)
    with pytest.raises(NotImplementedError, match="x0"):
        svort.srr(args["transforms"], args["slices"], args["psf"], (4, 4, 4), 1.0, n_iter=1, x0=torch.zeros(4, 4, 4, requires_grad=True))


def test_namespace_exports():
    from fetalsyngen_amd import kernels as K
    from fetalsyngen_amd.generator.artifacts import svort
    import importlib

    module = importlib.import_module("fetalsyngen_amd.generator.artifacts.svort.srr")

    assert svort.srr is module.srr and svort.SRR is module.SRR
    for name in ("cg_workspace", "cg_init", "cg_q", "cg_step", "cg_dir"):
        assert callable(getattr(K, name))


# ---- the generator's opt-in (kernels replaced by recorders: no device) -----------------------------------------------------------------
def test_reconstructor_and_simulate_motion_accept_the_new_keywords(monkeypatch):
    import inspect

    import torch

    from fetalsyngen_amd.generator.artifacts import simulate_reco as SR
    from fetalsyngen_amd.generator.augmentation import artifacts as A
    from tests.test_adjoint_det_wiring_host import VS, _data, _recon

    for cls in (SR.PSFReconstructor, A.SimulateMotion):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["srr_iterations"].default == 0 and sig["srr_mu"].default == 0.0
    assert list(inspect.signature(SR.SRRreconstruction).parameters) == [
        "transforms", "slices", "slices_mask", "vol_mask", "params", "n_iter", "mu", "x0", "deterministic"]
    with pytest.raises(ValueError):
        _recon(srr_iterations=-1)
    calls = []

    def adjoint(transforms, psf, slices, *a, slice_ids=None, **kw):
        calls.append(("psf", int(slices.shape[0]), len(slice_ids)))
        return torch.full((1, 1, *VS), 2.0)

    def solve(transforms, slices, psf, vol_shape, res_slice, **kw):
        calls.append(("srr", int(slices.shape[0]), int(transforms.shape[0]), kw["n_iter"], kw["mu"], kw["x0"] is kw["z"],
                      float(kw["x0"].max()), kw["interp_psf"], kw["deterministic"]))
        return torch.full((1, 1, *vol_shape), 3.0)

    monkeypatch.setattr(SR, "slice_acquisition_adjoint", adjoint)
    monkeypatch.setattr(SR, "srr", solve)
    monkeypatch.setattr(SR.K, "_upload", lambda host, device: host)
    plain = _recon(prob_rm_slices=1.0, rm_slices_min=0.5, rm_slices_max=0.5)
    torch.manual_seed(1)
    v0, _ = plain.recon_psf(_data(), want_weight=False)
    assert calls == [("psf", 4, 2)] and float(v0.max()) == 2.0 and "srr_iterations" not in plain.get_seeds()
    del calls[:]
    refined = _recon(prob_rm_slices=1.0, rm_slices_min=0.5, rm_slices_max=0.5, srr_iterations=3, srr_mu=0.25)
    torch.manual_seed(1)
    v3, _ = refined.recon_psf(_data(), want_weight=False)
    # the kept slices are gathered for the solve; x0 and z are the PSF reconstruction; the result replaces it
    assert calls == [("psf", 4, 2), ("srr", 2, 2, 3, 0.25, True, 2.0, True, False)]
    assert float(v3.max()) == 3.0 and refined.get_seeds()["srr_iterations"] == 3


def test_srr_class_maps_psfreconstructions_call_shape(monkeypatch):
    import importlib

    import torch

    module = importlib.import_module("fetalsyngen_amd.generator.artifacts.svort.srr")
    seen = {}

    def solve(transforms, slices, psf, vol_shape, res_slice, **kw):
        seen.update(kw, psf=psf, vol_shape=tuple(vol_shape), res_slice=res_slice)
        return "x"

    monkeypatch.setattr(module, "srr", solve)
    params = {"psf": "PSF", "interp_psf": True, "res_s": 1.5, "res_r": 0.5, "s_thick": 3.0, "volume_shape": (4, 5, 6)}
    vol, w, z, vm, sm = torch.zeros(1, 1, 7, 8, 9), "w", "z", "vm", "sm"
    assert module.SRR(n_iter=4, tol=1e-3, output_relu=False)(None, None, vol, params, p=w, mu=0.2, z=z, vol_mask=vm, slices_mask=sm) == "x"
    assert seen == dict(psf="PSF", vol_shape=(7, 8, 9), res_slice=3.0, interp_psf=True, slices_mask=sm, vol_mask=vm, slices_weight=w,
                        x0=vol, mu=0.2, z=z, n_iter=4, tol=1e-3, output_relu=False)
    module.SRR()(None, None, None, params)
    assert seen["vol_shape"] == (4, 5, 6) and seen["x0"] is None and seen["n_iter"] == 10 and seen["output_relu"] is True
