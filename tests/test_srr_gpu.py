"""GPU: the conjugate-gradient reconstruction `svort.srr` and its vector kernels (fsg_cg.hip; the rule is in include/fsg_hip.h
and DESIGN.md section 22) against the restatement tests/util_srr64.py.

Tolerances (none is derived from what the kernels give):
  vector kernels   bit-equal to the float32 restatement, the double dot products included: the element-wise operations are
                   single fp32 roundings and the sums have one documented order.
  solver           per (mode, n_iter, mu) 4 * E_cpu * max|float64|, E_cpu the difference of the float32 restatement to the float64
                   one over the same cases, measured on the CPU (util_srr64.E_CPU, held by the CPU tests); the factor 4 is section
                   18's, for the kernels ordering the operators' sums differently.  The rr and alpha histories likewise with their
                   own E_cpu.  One slices_mask serves the whole solve: every decision of the geometry keeps its margin (asserted on
                   the CPU).
  capability       the thresholds of the issue: below the residual of x0, and at most 1.05 x the float64 restatement's.
"""
import numpy as np
import pytest
import torch

from tests import util_sa_backward_cases as BC
from tests import util_srr64 as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64


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


def bits(x):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return a.reshape(-1).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want):
    return np.array_equal(bits(got), bits(want))


# ---- the vector kernels, launch by launch ----------------------------------------------------------------------------------------------
SIZES = (1, 255, 256, 257, 1023, 4099, 7920, 1048581)  # the last: past the 1024-workgroup cap, two trips per thread


def _view(n, offset, dtype=torch.float32):
    """n elements, 16-byte aligned (torch's allocations are) or 4 bytes (1 byte for a mask) past that"""
    return torch.zeros(n + 4, dtype=dtype, device=DEV)[1:n + 1] if offset else torch.zeros(n, dtype=dtype, device=DEV)


def _put(n, offset, a, dtype=torch.float32):
    v = _view(n, offset, dtype)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert v.data_ptr() % 16 == ((4 if dtype == torch.float32 else 1) if offset else 0)
    return v


def _scalars_match(ws, ref, k):
    h = {name: getattr(ws, name).cpu().numpy() for name in ("rr", "pq", "alpha", "beta", "frozen")}
    return all(same_bits(h[name][:k + 1], ref[name][:k + 1]) for name in h)


@pytest.mark.parametrize("full", (True, False), ids=("mask_z_x0_relu", "plain"))
@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset4"))
@pytest.mark.parametrize("n", SIZES)
def test_vector_kernels_are_bit_equal_to_the_restatement(K, n, offset, full):
    """two iterations (the second is the last: r is not stored, p is not touched, the relu is fused) with t = d * p for a
    positive d in place of the operator, every array and every scalar compared after every launch"""
    rng = np.random.default_rng(n + 2 * offset + full)
    g = lambda: rng.standard_normal(n).astype(F32)  # noqa: E731
    b, z, x0, t0 = g(), g(), g(), g()
    d = rng.uniform(0.5, 2.0, n).astype(F32)
    mask = (rng.random(n) < 0.8) if full else None
    if mask is not None and n == 1:
        mask[:] = True
    mu = 0.375 if full else 0.0
    kw = dict(mask=mask, mu=mu, z=z, x0=x0, t0=t0) if full else {}
    ref = U.new_ws(2)
    r_, p_, x_ = U.init32(ref, b, **kw)
    ws = K.cg_workspace(n, 2, DEV)
    put = lambda a: _put(n, offset, a)  # noqa: E731
    dm = None if mask is None else _put(n, offset, mask, torch.bool)
    r, p, x = _view(n, offset), _view(n, offset), _view(n, offset)
    if full:
        K.cg_init(ws, put(b), r, p, x, mask=dm, mu=mu, z=put(z), x0=put(x0), t0=put(t0))
    else:
        K.cg_init(ws, put(b), r, p, x)
    assert same_bits(r, r_) and same_bits(p, p_) and same_bits(x, x_)
    assert same_bits(ws.partial_rr, ref["part_rr"])
    for k in (1, 2):
        t_ = (d * p_).astype(F32)
        q_ = U.q32(ref, k, p_, t_, mask, mu)
        q = put(t_)
        K.cg_q(ws, k, p, q, mask=dm, mu=mu)
        assert same_bits(q, q_) and same_bits(ws.partial_pq, ref["part_pq"])
        x_, r_ = U.step32(ref, k, p_, q_, x_, r_, relu=full)
        K.cg_step(ws, k, p, q, x, r, relu=full)
        assert same_bits(x, x_) and same_bits(r, r_) and same_bits(ws.partial_rr, ref["part_rr"])
        p_ = U.dir32(ref, k, r_, p_)
        K.cg_dir(ws, k, r, p)
        assert same_bits(p, p_)
        assert _scalars_match(ws, ref, k)
    if n > 1:  # (one unknown: the first step is exact up to rounding, and the second iteration may be a frozen one)
        assert ref["frozen"].tolist() == [0, 0, 0] and ref["alpha"][2] > 0
    if full:
        assert (x_ >= 0).all() and (n == 1 or (x_ == 0).any())


@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset4"))
@pytest.mark.parametrize("what", ("mask", "z", "x0", "relu"))
def test_vector_kernels_with_one_option_at_a_time(K, what, offset):
    """the options of init and the relu of the last step singly (the test above has all of them or none), one iteration that is
    the last, n with a tail group and several workgroups"""
    n = 4099
    rng = np.random.default_rng(len(what) + offset)
    g = lambda: rng.standard_normal(n).astype(F32)  # noqa: E731
    b, z, x0, t0 = g(), g(), g(), g()
    mask = (rng.random(n) < 0.8) if what == "mask" else None
    mu = 0.625
    kw = dict(mask=mask, mu=mu, z=z if what == "z" else None, x0=x0 if what == "x0" else None, t0=t0 if what == "x0" else None)
    ref = U.new_ws(1)
    r_, p_, x_ = U.init32(ref, b, **kw)
    put = lambda a: None if a is None else _put(n, offset, a)  # noqa: E731
    dm = None if mask is None else _put(n, offset, mask, torch.bool)
    ws = K.cg_workspace(n, 1, DEV)
    r, p, x = _view(n, offset), _view(n, offset), _view(n, offset)
    K.cg_init(ws, put(b), r, p, x, mask=dm, mu=mu, z=put(kw["z"]), x0=put(kw["x0"]), t0=put(kw["t0"]))
    assert same_bits(r, r_) and same_bits(p, p_) and same_bits(x, x_) and same_bits(ws.partial_rr, ref["part_rr"])
    t_ = (F32(1.5) * p_).astype(F32)
    q_ = U.q32(ref, 1, p_, t_, mask, mu)
    q = put(t_)
    K.cg_q(ws, 1, p, q, mask=dm, mu=mu)
    x_, r1_ = U.step32(ref, 1, p_, q_, x_, r_, relu=what == "relu")
    K.cg_step(ws, 1, p, q, x, r, relu=what == "relu")
    p1_ = U.dir32(ref, 1, r1_, p_)
    K.cg_dir(ws, 1, r, p)
    assert same_bits(q, q_) and same_bits(x, x_) and same_bits(r, r_) and same_bits(p, p_)  # the last iteration leaves r and p
    assert same_bits(r1_, r_) and same_bits(p1_, p_) and _scalars_match(ws, ref, 1) and ref["alpha"][1] > 0
    assert ((x_ < 0).any()) == (what != "relu")


def test_a_nan_in_p_freezes_the_solve_and_touches_nothing_else(K):
    n = 4099
    rng = np.random.default_rng(9)
    b = rng.standard_normal(n).astype(F32)
    ws = K.cg_workspace(n, 3, DEV)
    r, p, x = _view(n, False), _view(n, False), _view(n, False)
    K.cg_init(ws, dev(b), r, p, x)
    p[17] = float("nan")
    before = [bits(v).copy() for v in (r, p, x)]
    t1 = (2 * p).contiguous()
    K.cg_q(ws, 1, p, t1)
    assert torch.isnan(t1).sum().item() == 1  # q itself is the launch's output; the NaN stays in its voxel
    K.cg_step(ws, 1, p, t1, x, r, relu=True)
    K.cg_dir(ws, 1, r, p)
    sentinel = torch.full((n,), -3.5, device=DEV)
    for k in (2, 3):
        t = sentinel.clone()
        K.cg_q(ws, k, p, t)
        K.cg_step(ws, k, p, t, x, r, relu=True)
        K.cg_dir(ws, k, r, p)
        assert torch.equal(t, sentinel)  # a frozen launch writes no vector
    frozen, alpha, rr = ws.frozen.cpu().tolist(), ws.alpha.cpu().numpy(), ws.rr.cpu().numpy()
    assert frozen == [0, 1, 1, 1] and (alpha[1:] == 0).all() and np.isfinite(rr).all() and (rr == rr[0]).all()
    assert np.isnan(ws.pq.cpu().numpy()[1])
    # x was 0 everywhere: the relu of the last iteration leaves it 0; r and p are what they were
    assert all(np.array_equal(a, bits(v)) for a, v in zip(before, (r, p, x)))


# ---- the solver against float64 ------------------------------------------------------------------------------------------------------------
_REF = {}


def ref64(name, interp_psf, n_iter, mu):
    """float64 solve of a solver case, computed once and shared (read only)"""
    key = (name, interp_psf, n_iter, mu)
    if key not in _REF:
        c = U.solver_case(name, interp_psf)
        _REF[key] = U.cg(U.case_operator(c, interp_psf, mu, F64), c["y"], n_iter, ft=F64)
    return _REF[key]


def gpu_srr(svort, c, interp_psf, perm=None, **kw):
    tr, y, sm = c["tr"], c["y"], c["sm"]
    if perm is not None:
        tr, y, sm = tr[perm], y[perm], sm[perm]
    kw.setdefault("output_relu", False)
    return svort.srr(dev(tr), dev(y[:, None]), dev(c["psf"]), BC.VS, c["res"], interp_psf=interp_psf, slices_mask=dev(sm[:, None]),
                     vol_mask=dev(c["V"]), **kw)


def _ratios(out, info, want, hist, key):
    """seen / bound for x, rr and alpha"""
    x = out.cpu().numpy().reshape(BC.VS).astype(F64)
    seen = {
        "x": np.abs(x - want).max() / (4 * U.E_CPU[key] * np.abs(want).max()),
        "rr": np.abs(info["rr"].cpu().numpy() - hist["rr"]).max() / (4 * U.E_CPU_RR[key] * np.abs(hist["rr"]).max()),
        "alpha": np.abs(info["alpha"].cpu().numpy()[1:].astype(F64) - hist["alpha"][1:]).max()
        / (4 * U.E_CPU_ALPHA[key] * np.abs(hist["alpha"][1:]).max()),
    }
    return seen


@pytest.mark.parametrize("mu", U.MUS)
@pytest.mark.parametrize("n_iter", U.N_ITERS)
@pytest.mark.parametrize("interp_psf", (False, True), ids=("linear", "nearest_psf"))
@pytest.mark.parametrize("name", U.SOLVER_CASES)
def test_solver_against_float64(svort, name, interp_psf, n_iter, mu):
    c = U.solver_case(name, interp_psf)
    want, hist = ref64(name, interp_psf, n_iter, mu)
    out, info = gpu_srr(svort, c, interp_psf, n_iter=n_iter, mu=mu, deterministic=False, return_info=True)
    assert out.shape == (1, 1, *BC.VS) and out.dtype == torch.float32
    seen = _ratios(out, info, want, hist, (interp_psf, n_iter, mu))
    print(f"srr {name} interp_psf={interp_psf} n_iter={n_iter} mu={mu}: seen/bound " + " ".join(f"{k} {v:.3f}" for k, v in seen.items()))
    assert info["frozen"].cpu().tolist() == hist["frozen"].tolist() == [0] * (n_iter + 1)
    if c["V"] is not None:
        assert (out.cpu().numpy().reshape(BC.VS)[~c["V"]] == 0).all()
    assert all(v <= 1 for v in seen.values()), seen


@pytest.mark.parametrize("interp_psf", (False, True), ids=("linear", "nearest_psf"))
def test_deterministic_solve_replays_bit_for_bit(svort, interp_psf):
    name, n_iter, mu = "psf223_vm", 6, 0.5
    c = U.solver_case(name, interp_psf)
    want, hist = ref64(name, interp_psf, n_iter, mu)
    run = lambda **kw: gpu_srr(svort, c, interp_psf, n_iter=n_iter, mu=mu, return_info=True, **kw)  # noqa: E731
    a, ia = run(deterministic=True)
    b, ib = run(deterministic=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s, _ = run(deterministic=True)
    side.synchronize()
    perm = np.array([3, 0, 4, 2, 1])
    p, _ = run(deterministic=True, perm=perm)
    assert same_bits(a, b) and same_bits(a, s) and same_bits(a, p)
    assert all(same_bits(ia[k], ib[k]) for k in ia)
    key = (interp_psf, n_iter, mu)
    assert all(v <= 1 for v in _ratios(a, ia, want, hist, key).values())
    f, info = run(deterministic=False)
    assert all(v <= 1 for v in _ratios(f, info, want, hist, key).values())


def test_keyed_scope_selects_the_deterministic_adjoint(svort, monkeypatch):
    from fetalsyngen_amd import rng

    c = U.solver_case("psf335", False)
    a = gpu_srr(svort, c, False, n_iter=2, deterministic=True)
    monkeypatch.setattr(rng, "in_keyed_scope", lambda: True)
    b = gpu_srr(svort, c, False, n_iter=2)
    assert same_bits(a, b)


def test_tol_freeze_equals_the_shorter_solve(svort):
    c = U.solver_case("psf223_vm", False)
    run = lambda **kw: gpu_srr(svort, c, False, mu=0.5, deterministic=True, return_info=True, output_relu=True, **kw)  # noqa: E731
    _, info = run(n_iter=6)
    rr = info["rr"].cpu().numpy()
    assert (rr[1:3] > rr[3]).all()  # so that tol = rr[3] is first reached at k = 3
    long, il = run(n_iter=6, tol=float(rr[3]))
    short, _ = run(n_iter=3)
    assert il["frozen"].cpu().tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert same_bits(long, short) and (long >= 0).all() and (long == 0).any()
    assert same_bits(il["rr"][:4], rr[:4]) and (il["alpha"].cpu().numpy()[4:] == 0).all()


@pytest.mark.parametrize("interp_psf", (False, True), ids=("linear", "nearest_psf"))
def test_one_iteration_is_alpha_times_the_adjoint(svort, K, interp_psf):
    c = U.solver_case("psf335", interp_psf)
    out, info = gpu_srr(svort, c, interp_psf, n_iter=1, deterministic=True, return_info=True)
    b = K.slice_acq_adjoint(dev(c["tr"]), dev(c["psf"]), dev(c["y"]), dev(c["sm"]), None, BC.VS, c["res"], interp_psf=interp_psf,
                            deterministic=True)
    want = info["alpha"][1] * b
    assert info["alpha"][1].item() > 0 and torch.equal(out.reshape(BC.VS), want)


def test_a_zero_right_hand_side_returns_x0(svort):
    c = U.solver_case("psf335", False)
    zero = dict(c, y=np.zeros_like(c["y"]))
    out, info = gpu_srr(svort, zero, False, n_iter=3, return_info=True)
    assert info["frozen"].cpu().tolist() == [1, 1, 1, 1] and (out == 0).all()


def test_capability_residual_falls_to_the_float64_level(svort, K):
    """what the package could not do before: six CG iterations from the equalised PSF reconstruction fit the slices"""
    cap = U.capability_case()
    op = U.Operator(cap["tr"], cap["psf"], BC.VS, cap["ss"], cap["res"], False)
    x64, _ = U.cg(op, cap["y"], 6, x0=U.equalised_x0(cap), relu=True)
    want = U.data_residual(op, cap["y"], x64)
    tr, y, psf = dev(cap["tr"]), dev(cap["y"]), dev(cap["psf"])
    x0 = K.slice_acq_adjoint(tr, psf, y, None, None, BC.VS, cap["res"], equalize=True)
    x = svort.srr(tr, y[:, None], psf, BC.VS, cap["res"], x0=x0, n_iter=6)
    r0 = U.data_residual(op, cap["y"], x0.cpu().numpy())
    r6 = U.data_residual(op, cap["y"], x.cpu().numpy().reshape(BC.VS))
    print(f"capability: residual {r0:.5f} at x0, {r6:.6f} after 6 iterations on the device, {want:.6f} in float64")
    assert r6 < r0 and r6 <= 1.05 * want


def test_requires_grad_raises(svort):
    c = U.solver_case("psf335", False)
    tr = dev(c["tr"]).requires_grad_(True)
    with pytest.raises(NotImplementedError):
        svort.srr(tr, dev(c["y"][:, None]), dev(c["psf"]), BC.VS, c["res"], n_iter=1)
    with torch.no_grad():
        svort.srr(tr, dev(c["y"][:, None]), dev(c["psf"]), BC.VS, c["res"], n_iter=1)


# ---- the generator's opt-in ------------------------------------------------------------------------------------------------------------
S48 = (48, 48, 48)
SCANNER_KW = dict(resolution_slice_fac_min=0.5, resolution_slice_fac_max=2, resolution_slice_max=1.5, slice_thickness_min=1.5,
                  slice_thickness_max=3.5, gap_min=1.5, gap_max=5.5, min_num_stack=2, max_num_stack=6, max_num_slices=250,
                  noise_sigma_min=0, noise_sigma_max=0.1, TR_min=1, TR_max=2, prob_void=0.2, prob_gamma=0.1, gamma_std=0.05,
                  slice_size=None, restrict_transform=False, txy=3.0, resolution_recon=np.float64(0.5))
MERGE_KW = dict(perlin_res_list=[1, 2], perlin_octaves_list=[1, 2, 4], perlin_persistence=0.5, perlin_lacunarity=2,
                gauss_ngaussians_min=2, gauss_ngaussians_max=4, perlin_increase_size=0.25)
RECON_KW = dict(prob_misreg_slice=0.0, slices_misreg_ratio=0.0, prob_misreg_stack=0.0, txy=0.0, prob_merge=0.0, prob_smooth=0.0,
                prob_rm_slices=1.0, rm_slices_min=0.1, rm_slices_max=0.4)
KEY = 0x5EED5EED5EED5EED


@pytest.fixture(scope="module")
def scanned(K):
    """Scanner.scan of a 48^3 phantom (shared, read only) and the simulate_reco module"""
    from fetalsyngen_amd.generator.artifacts import simulate_reco as SR
    from fetalsyngen_amd.phantom import make_seed_volumes

    seg = torch.from_numpy(make_seed_volumes(S48, 1)[0]).to(DEV).float()
    img = ((seg % 7 + 1) / 8) * (seg > 0)
    np.random.seed(13)
    torch.manual_seed(13)
    d = {"resolution": np.float64(0.5), "volume": img[None, None], "mask": (seg > 0).float()[None, None], "seg": seg[None, None],
         "threshold": 0.1}
    return SR, SR.Scanner(**SCANNER_KW).scan(d)


def _recon(SR, data, **kw):
    from fetalsyngen_amd.generator.artifacts.utils import ReconMergeParams

    np.random.seed(3)
    torch.manual_seed(3)
    rec = SR.PSFReconstructor(**RECON_KW, merge_params=ReconMergeParams(merge_type="perlin", **MERGE_KW), **kw)
    vol, _ = rec.recon_psf(data, want_weight=False)
    return vol, rec.get_seeds()


def test_reconstructor_with_srr_iterations(scanned):
    SR, data = scanned
    plain, seeds0 = _recon(SR, data)
    refined, seeds3 = _recon(SR, data, srr_iterations=3, srr_mu=0.1)
    assert refined.shape == plain.shape == (1, 1, *data["volume_shape"]) and torch.isfinite(refined).all()
    assert not torch.equal(refined, plain) and (refined >= 0).all()
    assert "srr_iterations" not in seeds0 and seeds3["srr_iterations"] == 3
    assert seeds0["rm_slices_on"] and {k: v for k, v in seeds3.items() if k != "srr_iterations"} == seeds0  # no draw added or moved
    params = {"psf": data["psf_rec"], "interp_psf": True, "res_s": data["resolution_slice"], "res_r": data["resolution_recon"],
              "volume_shape": data["volume_shape"]}
    mats = data["transforms_gt"].to(DEV).float().contiguous()
    x0 = SR.PSFreconstruction(mats, data["stacks"], None, None, params)
    out = SR.SRRreconstruction(mats, data["stacks"], None, None, params, 3, mu=0.1, x0=x0)
    assert out.shape == x0.shape and torch.isfinite(out).all() and not torch.equal(out, x0)


def test_srr_iterations_0_is_todays_reconstruction_and_3_replays(scanned):
    from fetalsyngen_amd import rng as R

    SR, data = scanned
    got = {}
    for name, kw in (("today", {}), ("zero", dict(srr_iterations=0)), ("three", dict(srr_iterations=3)), ("again", dict(srr_iterations=3))):
        with R.keyed_scope(KEY, R.STAGE_STREAMS["simulate_motion"]):
            got[name] = _recon(SR, data, **kw)
    assert same_bits(got["today"][0], got["zero"][0]) and got["today"][1] == got["zero"][1]
    assert same_bits(got["three"][0], got["again"][0]) and not same_bits(got["three"][0], got["today"][0])


def test_keyed_sample_with_srr_replays_bit_for_bit():
    from tests.test_keyed_motion_replay_gpu import MOTION_ONLY, _equal_samples, _key
    from tests.util_cases import default_artifacts, make_generator
    from fetalsyngen_amd.data.datasets import SeedBank
    from fetalsyngen_amd.phantom import make_seed_volumes

    seg, seeds = make_seed_volumes(S48, 1)
    seg_d = torch.from_numpy(seg).to(DEV)
    bank = SeedBank(seeds, DEV)
    arts = default_artifacts(prob=1.0, merge_type="perlin")
    for name, on in MOTION_ONLY.items():
        if name != "boundaries":
            arts[name].prob = 1.0 if on else 0.0
    b = arts["boundaries"]
    b.prob_no_mask, b.prob_halo, b.prob_fuzzy = 1.0, 0.5, 0.5
    arts["simulate_motion"].srr_iterations = 3
    gen = make_generator(S48, DEV, rng="keyed", prob=1.0, artifacts=arts, nonlin_scale=(0.08, 0.2), bf_scale=(0.05, 0.2))
    gen.register_label_twin(seg_d, seg_d.to(torch.uint8))
    k = _key(6)
    a = gen._pipeline(None, seg_d, bank, {}, scale01=False, key=k)
    b2 = gen._pipeline(None, seg_d, bank, {}, scale01=False, key=k)
    assert a[3]["artifacts"]["simulate_motion"]["srr_iterations"] == 3
    assert _equal_samples(a, b2)
