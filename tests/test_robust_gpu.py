"""GPU: the outlier weights (fsg_robust_estep_f32, fsg_robust_update_f32, fsg_robust_weights_f32, svort.robust_weights and
srr(n_robust=); the rule is in include/fsg_hip.h and DESIGN.md section 25) against the restatement tests/util_robust64.py.

Tolerances (none is derived from what the kernels give):
  p, rows, scalars, ws   per group 4 * E_cpu relative to max|float64|, E_cpu the difference of the fp32-operation restatement
                         to the float64 one, measured on the CPU (util_robust64.E_CPU).  expf differs from numpy's by an ulp,
                         so no bit-equality with the restatement is asked.  Every comparison case keeps every slice potential
                         1e-3 away from mu1 and mu2 in float64 (checked on the CPU), so no slice weight sits on its jump.
  determinism            bit-equal: twice, on a side stream, 16-byte loads against scalars, a slice alone against the batch.
  capability             the flagged set of the float64 run, and the RMS within 4 * CAP32_RMS_DIFF of the float64 RMS
                         (5.27e-8 relative is what the fp32-operation restatement of the whole run differs by on the CPU).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util_robust64 as U
from tests import util_sa_backward_cases as BC
from tests import util_tk1_64 as TK

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77.25
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


def host(x):
    return x.detach().cpu().numpy()


def run_em(K, y, s, mask=None, sw=None, n_em=5, min_weight=0.5, **opts):
    """the launch sequence one slot at a time, with the rows and the two floats of every slot -> a dict in em()'s keys"""
    n, h, w = y.shape
    st = K.robust_state(n, n_em, DEV, (h, w))
    rows_hist, scal_hist = [], []
    for t in range(n_em + 1):
        K.robust_estep(st, t, y, s, mask, sw, min_weight)
        K.robust_update(st, t, **opts)
        rows_hist.append(host(st.rows).copy())
        scal_hist.append(tuple(float(v) for v in host(st.scal)))
    out = {k: host(v).copy() for k, v in st.info().items()}
    out.update(rows_hist=rows_hist, scal_hist=scal_hist, consts=host(st.consts).copy(), state=st,
               slice=host(K.robust_weights(st, y, s, mask, sw, min_weight, level="slice")),
               both=host(K.robust_weights(st, y, s, mask, sw, min_weight, level="both")))
    return out


def case_on_device(name):
    c = U.synthetic_case(name)
    return dev(c["y"]), dev(c["s"]), dev(c["mask"]), dev(c["sw"])


# ---- against float64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.SYNTH))
def test_em_within_four_times_the_fp32_cost_of_the_formula(K, name):
    want = U.run_case(name, F64)
    if U.SYNTH[name][0] > 1:
        U.assert_margin(want)
    got = run_em(K, *case_on_device(name))
    assert np.array_equal(got["frozen"], want["frozen"]) and not want["frozen"].any()
    for t in range(6):
        assert np.array_equal(got["rows_hist"][t][:, 0], want["rows_hist"][t][:, 0])  # the pixel counts
        assert np.array_equal(got["rows_hist"][t][:, 4:], want["rows_hist"][t][:, 4:])  # min y, max y
    assert np.array_equal(got["consts"], want["consts"])
    err = U.compare(got, want)
    for g in U.GROUPS:
        print(f"{name} {g}: GPU {err[g]:.3e}, E_cpu {U.E_CPU[g]:.3e}")
    for g in U.GROUPS:
        assert err[g] <= 4 * U.E_CPU[g], (g, err[g])
    assert np.array_equal(got["slice"] != 0, want["slice"] != 0)
    assert np.abs(got["slice"] - want["slice"]).max() <= 4 * U.E_CPU["ws"]
    assert np.array_equal(got["both"][~want["part"]], np.zeros((~want["part"]).sum(), F32))


def test_front_end_gives_the_same_weights_and_histories(K, svort):
    y, s, mask, sw = case_on_device("n5_37x29_mw")
    ref = run_em(K, y, s, mask, sw)
    for level in ("slice", "both"):
        out, info = svort.robust_weights(y[:, None], s[:, None], slices_mask=mask[:, None], sim_weight=sw, level=level,
                                         return_info=True)
        assert out.shape == (5, 37, 29) and out.dtype == torch.float32 and out.device.type == "cuda"
        assert np.array_equal(host(out), ref[level])
        assert set(info) == {"sigma", "c", "mu1", "mu2", "frozen", "ws", "u"}
        for k in info:
            assert np.array_equal(host(info[k]), ref[k]), k


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
def test_bit_equal_twice_and_on_a_side_stream(K, svort):
    y, s, mask, sw = case_on_device("n5_37x29_mw")
    kw = dict(slices_mask=mask, sim_weight=sw, level="both", return_info=True)
    a, ia = svort.robust_weights(y, s, **kw)
    b, ib = svort.robust_weights(y, s, **kw)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c, ic = svort.robust_weights(y, s, **kw)
    side.synchronize()
    for o, i in ((b, ib), (c, ic)):
        assert np.array_equal(host(o).view(np.uint32), host(a).view(np.uint32))
        for k in ia:
            assert np.array_equal(host(i[k]).view(np.uint8), host(ia[k]).view(np.uint8)), k


def test_sixteen_byte_loads_and_scalars_give_the_same_bits(K):
    y, s, mask, sw = case_on_device("n5_36x32_mw")
    assert all(t.data_ptr() % 16 == 0 for t in (y, s, sw)) and mask.data_ptr() % 4 == 0 and (36 * 32) % 4 == 0

    def shifted(t):  # the same values one element further: no pointer is 16-byte aligned, the mask not 4-byte
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        buf[1:] = t.reshape(-1)
        return buf[1:].view(t.shape)

    a = run_em(K, y, s, mask, sw)
    b = run_em(K, shifted(y), shifted(s), shifted(mask), shifted(sw))
    assert b["state"] is not a["state"]
    for k in ("sigma", "c", "mu1", "mu2", "ws", "u", "slice", "both"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    for ra, rb in zip(a["rows_hist"], b["rows_hist"]):
        assert np.array_equal(ra, rb)


def test_a_slice_alone_has_the_row_it_has_in_the_batch(K):
    y, s, mask, sw = case_on_device("n5_37x29_mw")
    batch = K.robust_state(5, 2, DEV, (37, 29))
    for t in range(2):
        K.robust_estep(batch, t, y, s, mask, sw)
        if t == 0:
            K.robust_update(batch, 0)
            scal = batch.scal.clone()
    K.robust_update(batch, 1)
    want = host(batch.rows)
    for k in (0, 1, 4):
        one = K.robust_state(1, 2, DEV, (37, 29))
        args = (y[k:k + 1].clone(), s[k:k + 1].clone(), mask[k:k + 1].clone(), sw[k:k + 1].clone())
        K.robust_estep(one, 0, *args)
        K.robust_update(one, 0)
        one.scal.copy_(scal)  # the batch's kappa and inv2var: given the two scalars a row is a function of the slice alone
        K.robust_estep(one, 1, *args)
        K.robust_update(one, 1)
        assert np.array_equal(host(one.rows)[0].view(np.uint64), want[k].view(np.uint64)), k
    assert want[:, 3].max() > 0


# ---- degenerate cases ------------------------------------------------------------------------------------------------------------------
def _finite(r):
    return all(np.isfinite(r[k]).all() for k in ("sigma", "c", "mu1", "mu2", "ws", "u", "consts", "slice", "both")) and all(
        np.isfinite(x).all() for x in r["rows_hist"])


def test_flat_image_freezes_with_unit_weights(K):
    y = torch.full((3, 13, 11), 1.5, device=DEV)
    s = torch.rand((3, 13, 11), device=DEV)
    r = run_em(K, y, s)
    assert r["frozen"].tolist() == [1] * 6 and _finite(r) and r["scal_hist"][-1] == (0.0, 0.0)
    assert np.array_equal(r["ws"], np.ones((6, 3))) and np.array_equal(r["slice"], np.ones((3, 13, 11), F32))
    assert np.array_equal(r["both"], np.ones((3, 13, 11), F32)) and r["consts"].tolist() == [0, 0, 0, 0]


def test_all_false_mask_freezes_with_zero_weights(K):
    c = U.synthetic_case("n5_13x11")
    r = run_em(K, dev(c["y"]), dev(c["s"]), torch.zeros((5, 13, 11), dtype=torch.bool, device=DEV), None)
    assert r["frozen"].tolist() == [1] * 6 and _finite(r)
    assert not r["ws"].any() and not r["slice"].any() and not r["both"].any() and not r["rows_hist"][-1].any()


def test_slice_under_min_pixels_nan_and_inf_pixels(K):
    c = U.synthetic_case("n5_13x11")
    mask = np.ones((5, 13, 11), bool)
    mask[2] = False
    mask[2, 0, :3] = True  # three pixels: under min_pixels = 4
    want = U.em(c["y"], c["s"], mask)
    got = run_em(K, dev(c["y"]), dev(c["s"]), dev(mask), None)
    assert _finite(got) and not got["frozen"].any()
    assert not got["ws"][:, 2].any() and not got["slice"][2].any() and got["rows_hist"][-1][2, 0] == 3
    assert got["slice"][0, 2, 3] == 0 and got["slice"][4, 5, 1] == 0 and got["both"][0, 2, 3] == 0  # the NaN and the Inf pixel
    assert got["rows_hist"][0][0, 0] == 13 * 11 - 1 and got["rows_hist"][0][4, 0] == 13 * 11 - 1
    assert np.array_equal(got["slice"] != 0, want["slice"] != 0)


def test_one_slice_keeps_its_weight(K):
    r = run_em(K, *case_on_device("n1_13x11"))
    assert r["ws"][:, 0].tolist() == [1.0] * 6 and not r["frozen"].any() and _finite(r)
    assert np.array_equal(r["mu1"][1:], r["mu2"][1:]) and r["mu1"][-1] == r["u"][0]  # u is the last slot's


# ---- refusals over sentinels -------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(K):
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    y, s, mask, sw = case_on_device("n5_13x11_mw")
    st = K.robust_state(5, 5, DEV, (13, 11))
    out = torch.full((5, 13, 11), SENTINEL, device=DEV)
    st.buf.fill_(0x5A5A5A5A5A5A5A5A)
    st.part.fill_(0x5A5A5A5A5A5A5A5A)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    sb, wb = st.nbytes, st.part.numel() * 8
    bad = [
        lib.fsg_robust_estep_f32(p(y), p(s), p(mask), p(sw), -1.0, 5, 13, 11, 0, 5, p(st.buf), sb, p(st.part), wb, None),
        lib.fsg_robust_estep_f32(p(y), p(s), p(mask), p(sw), 0.5, 5, 13, 11, 6, 5, p(st.buf), sb, p(st.part), wb, None),
        lib.fsg_robust_estep_f32(p(y), p(s), p(mask), p(sw), 0.5, 5, 13, 11, 0, 5, p(st.buf), sb, p(st.part), wb - 1, None),
        lib.fsg_robust_estep_f32(p(y), p(s), p(mask), p(sw), 0.5, 5, 13, 11, 0, 5, p(st.buf), sb, p(st.buf), wb, None),
        lib.fsg_robust_update_f32(p(st.buf), sb, p(st.part), wb, 5, 13, 11, 0, 5, 0.0, 0.04, 0.025, 4, None),
        lib.fsg_robust_update_f32(p(st.buf), sb, p(st.part), wb, 5, 13, 11, 0, 5, 0.9, float("nan"), 0.025, 4, None),
        lib.fsg_robust_update_f32(p(st.buf), sb - 1, p(st.part), wb, 5, 13, 11, 0, 5, 0.9, 0.04, 0.025, 4, None),
        lib.fsg_robust_weights_f32(p(y), p(s), p(mask), p(sw), 0.5, 5, 13, 11, 5, 2, p(st.buf), sb, p(out), None),
        lib.fsg_robust_weights_f32(p(y), p(s), p(mask), p(sw), 0.5, 5, 13, 11, 5, 0, p(st.buf), sb, p(y), None),
        lib.fsg_robust_weights_f32(p(y), p(s), p(mask), p(sw), 0.5, 5, 13, 11, 0, 0, p(st.buf), sb, p(out), None),
    ]
    torch.cuda.synchronize()
    assert bad == [_lib.E_BADARG] * len(bad)
    assert bool((out == SENTINEL).all()) and bool((st.buf == 0x5A5A5A5A5A5A5A5A).all()) and bool((st.part == 0x5A5A5A5A5A5A5A5A).all())
    assert np.array_equal(host(y), U.synthetic_case("n5_13x11_mw")["y"], equal_nan=True)


def test_requires_grad_raises(svort):
    y, s, _, _ = case_on_device("n5_13x11")
    with pytest.raises(NotImplementedError, match="simulated"):
        svort.robust_weights(y, s.clone().requires_grad_(True))
    with torch.no_grad():
        svort.robust_weights(y, s.clone().requires_grad_(True))


# ---- the capability run on the device ------------------------------------------------------------------------------------------------
def test_capability_srr_with_two_rejection_rounds(svort):
    c = U.capability_case()
    args = (dev(c["tr"]), dev(c["y"][:, None]), dev(c["psf"]), BC.VS, c["res"])
    kw = dict(n_iter=U.CAP_ITERS, lam=U.CAP_LAM, deterministic=True)
    plain = TK.rms(host(svort.srr(*args, **kw)), c["vol"])
    x, info = svort.srr(*args, n_robust=2, return_info=True, **kw)
    got = TK.rms(host(x), c["vol"])
    assert len(info["robust"]) == 2 and set(info) >= {"rr", "alpha", "rounds", "robust"}
    flagged = [sorted(np.flatnonzero(host(r["ws"])[-1] < 0.5).tolist()) for r in info["robust"]]
    want = U.cap_robust(2, "slice")[1][0]
    d = abs(got - want) / want
    print(f"capability on the device: RMS {got:.6f} (float64 {want:.6f}, relative difference {d:.3e}, bound "
          f"{4 * U.CAP32_RMS_DIFF:.3e}), unweighted {plain:.4f}, flagged {flagged}")
    assert flagged == [list(U.CAP_FLAGGED)] * 2
    assert got <= 0.5 * plain and got <= 1.5 * U.CAP_RMS["oracle"]
    assert d <= 4 * U.CAP32_RMS_DIFF
