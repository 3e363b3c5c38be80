"""GPU: the first-order regulariser `kernels.tk1_apply` (fsg_tk1.hip; the rule is in include/fsg_hip.h and DESIGN.md section 24)
and `svort.srr` with `lam`, against the restatement tests/util_tk1_64.py.

Tolerances (none is derived from what the kernels give):
  tk1_apply      bit-equal to the float32 restatement, guided or not: + - * /, abs and a comparison, one rounding each, the
                 division correctly rounded.
  solver         per (mode, huber) 4 * E_cpu * max|float64|, E_cpu the difference of the float32 restatement to the float64 one
                 over the same cases, measured on the CPU (util_tk1_64.E_CPU_TK1, held by the CPU tests, and measured afresh
                 here); the factor 4 is section 18's.
  capability     the RMS error against the phantom at most 1.05 x the float64 restatement's (util_tk1_64.CAP_RMS), and the
                 ordering Huber < TK1 < none.
"""
import numpy as np
import pytest
import torch

from tests import util_sa_backward_cases as BC
from tests import util_srr64 as U
from tests import util_tk1_64 as T

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


def _put(shape, offset, a, dtype=torch.float32):
    """`a` in device storage that is 16-byte aligned (torch's allocations are) or 4 bytes (1 byte for a mask) past that"""
    n = int(np.prod(shape))
    v = torch.zeros(n + 4, dtype=dtype, device=DEV)[1:n + 1] if offset else torch.zeros(n, dtype=dtype, device=DEV)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    assert v.data_ptr() % 16 == ((4 if dtype == torch.float32 else 1) if offset else 0)
    return v.view(shape)


# ---- the kernel against the float32 restatement ------------------------------------------------------------------------------------------
# the smallest that can go wrong: no neighbour at all / along one axis only, rows that are no multiple of 4 so that groups straddle
# row ends (4,3,67), a row that crosses a 256-thread workgroup (2,3,259), rows of whole groups (2,3,8), and the solver's volume
SHAPES = ((1, 1, 1), (1, 1, 5), (1, 5, 1), (5, 1, 1), (2, 2, 2), (3, 4, 5), (2, 3, 8), (4, 3, 67), (2, 3, 259), BC.VS)
MASKS = ("none", "random", "all", "empty", "isolated")
_IN = {}


def _inputs(shape):
    """p, t, guide and the masks of a shape, computed once and shared (read only)"""
    if shape not in _IN:
        rng = np.random.default_rng(sum(shape))
        iso = np.zeros(shape, bool)
        iso.reshape(-1)[::3] = True  # along x every third voxel; rows shift the pattern unless W % 3 == 0
        masks = {"none": None, "random": rng.random(shape) < 0.7, "all": np.ones(shape, bool), "empty": np.zeros(shape, bool),
                 "isolated": iso}
        _IN[shape] = dict(p=rng.standard_normal(shape).astype(F32), t=rng.standard_normal(shape).astype(F32),
                          g=rng.uniform(0, 0.3, shape).astype(F32), masks=masks)
    return _IN[shape]


@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset4"))
@pytest.mark.parametrize("inplace", (False, True), ids=("out", "inplace"))
@pytest.mark.parametrize("guided", (False, True), ids=("tk1", "huber"))
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tk1_apply_is_bit_equal_to_the_restatement(K, shape, mask, guided, inplace, offset):
    c = _inputs(shape)
    m, lam, delta = c["masks"][mask], 0.3, 0.05
    want = T.apply(c["p"], c["t"], lam, m, c["g"] if guided else None, delta if guided else None, F32)
    p, t = _put(shape, offset, c["p"]), _put(shape, offset, c["t"])
    g = _put(shape, offset, c["g"]) if guided else None
    md = None if m is None else _put(shape, offset, m, torch.bool)
    out = t if inplace else _put(shape, offset, np.full(shape, 7.0, F32))
    got = K.tk1_apply(p, t, shape, lam, mask=md, guide=g, delta=delta if guided else None, out=out)
    assert got is out and same_bits(got, want)
    assert same_bits(p, c["p"]) and (inplace or same_bits(t, c["t"]))
    if mask in ("empty",) or shape == (1, 1, 1):
        assert same_bits(got, c["t"])
    if guided and shape == BC.VS and m is None:
        assert not same_bits(got, T.apply(c["p"], c["t"], lam, None, None, None, F32))  # the weights did something


def test_default_out_is_a_new_tensor_and_the_hand_case(K):
    p, t = dev(np.array([[[1.0, 4.0]]], F32)), dev(np.array([[[10.0, 20.0]]], F32))
    out = K.tk1_apply(p, t, (1, 1, 2), 0.5)
    assert out.data_ptr() != t.data_ptr() and out.cpu().tolist() == [[[8.5, 21.5]]] and t.cpu().tolist() == [[[10.0, 20.0]]]
    g = dev(np.array([[[0.0, 0.25]]], F32))
    assert K.tk1_apply(p, t, (1, 1, 2), 0.5, guide=g, delta=0.25).cpu().tolist() == [[[8.5, 21.5]]]  # a == delta: weight 1
    assert K.tk1_apply(p, t, (1, 1, 2), 0.5, guide=g, delta=0.125).cpu().tolist() == [[[9.25, 20.75]]]  # weight 1/2
    assert same_bits(K.tk1_apply(p, t, (1, 1, 2), 0.0), t)


def test_refusals_leave_the_output_untouched(K):
    from fetalsyngen_amd import _lib

    shape = (3, 4, 5)
    c = _inputs(shape)
    p, t, g, m = dev(c["p"]), dev(c["t"]), dev(c["g"]), dev(c["masks"]["random"])
    out = torch.full(shape, 7.0, device=DEV)
    bad = [dict(lam=-0.1), dict(lam=float("nan")), dict(lam=float("inf")), dict(guide=g, delta=0.0), dict(guide=g, delta=-1.0),
           dict(guide=g, delta=float("nan")), dict(guide=g, delta=float("inf"))]
    for kw in bad:
        kw = dict(dict(lam=0.1, mask=m), **kw)
        lam = kw.pop("lam")
        with pytest.raises(_lib.FsgError) as e:
            K.tk1_apply(p, t, shape, lam, out=out, **kw)
        assert e.value.code == _lib.E_BADARG
    big = torch.full((61,), 7.0, device=DEV)
    # out over p, out over the guide, out one element into p, out one element into t (only out == t is in place)
    for args, kw in (((p, t), dict(out=p)), ((p, t), dict(out=g, guide=g, delta=0.05)), ((big[:60], t), dict(out=big[1:])),
                     ((p, big[:60]), dict(out=big[1:]))):
        with pytest.raises(_lib.FsgError) as e:
            K.tk1_apply(*args, shape, 0.1, **kw)
        assert e.value.code == _lib.E_BADARG
    assert (big == 7.0).all()
    with pytest.raises(ValueError):
        K.tk1_apply(p, t, (3, 4, 4), 0.1, out=out)  # element count
    with pytest.raises(TypeError):
        K.tk1_apply(p.double(), t, shape, 0.1, out=out)
    with pytest.raises(ValueError):
        K.tk1_apply(p, t, shape, 0.1, guide=g, out=out)  # guide without delta
    with pytest.raises(ValueError):
        K.tk1_apply(p.view(-1)[::2], t, shape, 0.1, out=out)  # not contiguous
    torch.cuda.synchronize()
    assert (out == 7.0).all() and same_bits(p, c["p"]) and same_bits(g, c["g"]) and same_bits(t, c["t"])


def test_tk1_apply_replays_bit_for_bit_and_on_a_side_stream(K):
    c = _inputs(BC.VS)
    p, t, g, m = dev(c["p"]), dev(c["t"]), dev(c["g"]), dev(c["masks"]["random"])
    run = lambda: K.tk1_apply(p, t, BC.VS, 0.3, mask=m, guide=g, delta=0.05)  # noqa: E731
    a, b = run(), run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = run()
    side.synchronize()
    assert same_bits(a, b) and same_bits(a, s)


# ---- the solver --------------------------------------------------------------------------------------------------------------------------
_REF = {}


def ref(name, interp_psf, huber, ft):
    """the restatement's solve of a solver case, computed once and shared (read only)"""
    key = (name, interp_psf, huber, ft)
    if key not in _REF:
        _REF[key] = T.solve_case(name, interp_psf, huber, ft)
    return _REF[key]


def gpu_srr(svort, c, interp_psf, perm=None, **kw):
    tr, y, sm = c["tr"], c["y"], c["sm"]
    if perm is not None:
        tr, y, sm = tr[perm], y[perm], sm[perm]
    return svort.srr(dev(tr), dev(y[:, None]), dev(c["psf"]), BC.VS, c["res"], interp_psf=interp_psf, slices_mask=dev(sm[:, None]),
                     vol_mask=dev(c["V"]), **kw)


def _huber(on):
    return dict(huber_delta=T.HUBER_DELTA, n_outer=T.N_OUTER) if on else {}


@pytest.mark.parametrize("huber", (False, True), ids=("tk1", "huber2"))
@pytest.mark.parametrize("interp_psf", (False, True), ids=("linear", "nearest_psf"))
@pytest.mark.parametrize("name", U.SOLVER_CASES)
def test_solver_against_float64(svort, name, interp_psf, huber):
    c = U.solver_case(name, interp_psf)
    assert c["kept"] >= U.MIN_KEPT
    want = ref(name, interp_psf, huber, F64)
    fresh = np.abs(ref(name, interp_psf, huber, F32).astype(F64) - want).max() / np.abs(want).max()
    out, info = gpu_srr(svort, c, interp_psf, n_iter=T.N_ITER, lam=T.LAM, deterministic=False, return_info=True, **_huber(huber))
    x = out.cpu().numpy().reshape(BC.VS).astype(F64)
    seen = np.abs(x - want).max() / np.abs(want).max()
    print(f"srr lam={T.LAM} {name} interp_psf={interp_psf} huber={huber}: seen {seen:.3e}, E_cpu {T.E_CPU_TK1[(interp_psf, huber)]:.3e}"
          f" (this case afresh {fresh:.3e})")
    assert out.shape == (1, 1, *BC.VS) and out.dtype == torch.float32 and (x >= 0).all()
    assert len(info["rounds"]) == (T.N_OUTER if huber else 1) and same_bits(info["rr"], info["rounds"][-1]["rr"])
    assert all(r["frozen"].cpu().tolist() == [0] * (T.N_ITER + 1) for r in info["rounds"])
    if c["V"] is not None:
        assert (x[~c["V"]] == 0).all()
    assert fresh <= T.E_CPU_TK1[(interp_psf, huber)]  # the committed constant covers what is measured now
    assert seen <= 4 * T.E_CPU_TK1[(interp_psf, huber)]


@pytest.mark.parametrize("huber", (False, True), ids=("tk1", "huber2"))
def test_deterministic_solve_with_lam_replays_bit_for_bit(svort, huber):
    c = U.solver_case("psf223_vm", False)
    run = lambda **kw: gpu_srr(svort, c, False, n_iter=T.N_ITER, lam=T.LAM, deterministic=True, **_huber(huber), **kw)  # noqa: E731
    a, b = run(), run()
    p = run(perm=np.array([3, 0, 4, 2, 1]))
    assert same_bits(a, b) and same_bits(a, p)
    want = ref("psf223_vm", False, huber, F64)
    assert np.abs(a.cpu().numpy().reshape(BC.VS) - want).max() <= 4 * T.E_CPU_TK1[(False, huber)] * np.abs(want).max()


def test_lam_0_is_the_call_without_the_keyword(svort):
    c = U.solver_case("psf223_vm", False)
    a, ia = gpu_srr(svort, c, False, n_iter=3, mu=0.5, deterministic=True, return_info=True)
    b, ib = gpu_srr(svort, c, False, n_iter=3, mu=0.5, deterministic=True, return_info=True, lam=0.0, n_outer=1)
    assert same_bits(a, b) and all(same_bits(ia[k], ib[k]) for k in ("rr", "pq", "alpha", "beta", "frozen"))
    r = gpu_srr(svort, c, False, n_iter=3, mu=0.5, deterministic=True, lam=T.LAM)
    assert not same_bits(a, r)


def test_requires_grad_on_guide_raises(svort):
    c = U.solver_case("psf335", False)
    args = (dev(c["tr"]), dev(c["y"][:, None]), dev(c["psf"]), BC.VS, c["res"])
    guide = torch.zeros(BC.VS, device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError, match="guide"):
        svort.srr(*args, n_iter=1, lam=0.1, huber_delta=0.05, guide=guide)
    with torch.no_grad():
        svort.srr(*args, n_iter=1, lam=0.1, huber_delta=0.05, guide=guide)


def test_an_explicit_guide_is_round_1_of_the_reweighting(svort):
    c = U.solver_case("psf335", False)
    kw = dict(n_iter=2, lam=T.LAM, deterministic=True, output_relu=False)
    x1 = gpu_srr(svort, c, False, **kw)
    two = gpu_srr(svort, c, False, huber_delta=T.HUBER_DELTA, n_outer=2, **kw)
    by_hand = gpu_srr(svort, c, False, huber_delta=T.HUBER_DELTA, guide=x1, x0=x1, **kw)
    assert same_bits(two, by_hand) and not same_bits(two, x1)


# ---- capability ---------------------------------------------------------------------------------------------------------------------------
def _cap_rms(svort, name):
    case, lam, n_iter, delta, n_outer = T.CAP_RUNS[name]
    c = T.capability_cases()[case]
    kw = dict(huber_delta=delta, n_outer=n_outer) if delta is not None else {}
    x = svort.srr(dev(c["tr"]), dev(c["y"][:, None]), dev(c["psf"]), BC.VS, c["res"], n_iter=n_iter, lam=lam, **kw)
    return T.rms(x.cpu().numpy(), c["vol"])


def test_capability_smooth_phantom_from_nothing(svort):
    """what the package could not do before: x0 = None and no target, and the voxels no slice touches are filled in"""
    got = _cap_rms(svort, "smooth_tk1")
    c = T.capability_cases()["smooth"]
    none = T.rms(svort.srr(dev(c["tr"]), dev(c["y"][:, None]), dev(c["psf"]), BC.VS, c["res"], n_iter=6).cpu().numpy(), c["vol"])
    print(f"capability, smooth phantom, 6 iterations: RMS {got:.4f} with lam = 0.1 (float64 {T.CAP_RMS['smooth_tk1']}), {none:.4f} with lam = 0")
    assert got <= 1.05 * T.CAP_RMS["smooth_tk1"] and got < none / 3


def test_capability_piecewise_phantom_huber_beats_tk1_beats_none(svort):
    got = {name: _cap_rms(svort, name) for name in ("piecewise_none", "piecewise_tk1", "piecewise_huber")}
    print("capability, piecewise-constant phantom, 24 iterations in all: RMS " + ", ".join(
        f"{k[10:]} {v:.4f} (float64 {T.CAP_RMS[k]})" for k, v in got.items()))
    for name, v in got.items():
        assert v <= 1.05 * T.CAP_RMS[name], (name, v)
    assert got["piecewise_huber"] < got["piecewise_tk1"] < got["piecewise_none"]


# ---- the generator's opt-in ------------------------------------------------------------------------------------------------------------
def test_reconstructor_with_srr_lambda(K):
    from fetalsyngen_amd import rng as R
    from tests.test_srr_gpu import KEY, S48, SCANNER_KW, _recon
    from fetalsyngen_amd.generator.artifacts import simulate_reco as SR
    from fetalsyngen_amd.phantom import make_seed_volumes

    seg = torch.from_numpy(make_seed_volumes(S48, 1)[0]).to(DEV).float()
    img = ((seg % 7 + 1) / 8) * (seg > 0)
    np.random.seed(13)
    torch.manual_seed(13)
    d = {"resolution": np.float64(0.5), "volume": img[None, None], "mask": (seg > 0).float()[None, None], "seg": seg[None, None],
         "threshold": 0.1}
    data = SR.Scanner(**SCANNER_KW).scan(d)
    got = {}
    new = dict(srr_lambda=0.1, srr_huber_delta=0.05, srr_outer=2)
    for name, kw in (("plain", dict(srr_iterations=3)), ("tk1", dict(srr_iterations=3, srr_lambda=0.1)),
                     ("huber", dict(srr_iterations=3, **new)), ("again", dict(srr_iterations=3, **new))):
        with R.keyed_scope(KEY, R.STAGE_STREAMS["simulate_motion"]):
            got[name] = _recon(SR, data, **kw)
    vols = {k: v[0] for k, v in got.items()}
    assert all(torch.isfinite(v).all() and (v >= 0).all() and v.shape == (1, 1, *data["volume_shape"]) for v in vols.values())
    assert not same_bits(vols["tk1"], vols["plain"]) and not same_bits(vols["huber"], vols["tk1"])  # it changes the volume
    assert same_bits(vols["huber"], vols["again"])  # and replays bit for bit in a keyed scope
    assert got["tk1"][1] == dict(got["plain"][1], srr_lambda=0.1)  # the seeds differ only by the new keys: no draw added or moved
    assert got["huber"][1] == dict(got["plain"][1], **new)
