"""GPU: the slice intensity matching (fsg_imatch_sums_f32, fsg_imatch_scale_f32, fsg_imatch_bias_f32, fsg_imatch_apply_f32,
svort.intensity_match and srr(n_match=); the rule is in include/fsg_hip.h and DESIGN.md section 28) against the restatement
tests/util_imatch64.py.

Tolerances (none is derived from what the kernels give):
  rows, scale, bias, corrected   per group 4 * E_cpu relative to max|float64|, E_cpu the difference of the fp32-operation
                         restatement to the float64 one, measured on the CPU (util_imatch64.E_CPU).  expf and logf differ from
                         numpy's by an ulp, so bit equality is asked only of the counts, of min y and max y and of membership.
                         Every comparison case keeps d and s of every pixel 1e-3 * floor away from the floor in float64 (checked
                         on the CPU), so no pixel sits on the jump and none is left out of a comparison.  The cases reach the
                         largest radius (48): n2_131x33_r48 / _r33 put a column tile between two others with tap windows
                         across both borders, n2_14x600_r48 a row-pass workgroup between two others.
  determinism            bit-equal: twice, on a side stream, 16-byte loads against shifted pointers, a slice alone against the
                         batch (its row of sums), the scale with and without the bias field.
  capability             the RMS against the phantom within 4 * CAP32_RMS_DIFF of the float64 RMS (1.30e-7 relative is what the
                         fp32-operation restatement of the whole run differs by on the CPU), and matched below unmatched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util_imatch64 as U
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


def run_match(K, y, s, mask=None, sw=None, pw=None, b0=None, sigma=0.0, min_weight=0.5, log_floor=0.01, min_pixels=4):
    """the launch sequence kernel by kernel -> a dict in match()'s keys"""
    n, h, w = y.shape
    st = K.imatch_state(n, DEV, (h, w))
    K.imatch_sums(st, y, s, mask, sw, min_weight, pw, b0)
    K.imatch_scale(st, log_floor, min_pixels)
    b1 = K.imatch_bias(st, y, s, sigma, mask, sw, min_weight, pw, b0) if sigma > 0 else None
    b1_copy = None if b1 is None else host(b1).copy()
    corrected, bias = K.imatch_apply(st, y, b1, b0)
    out = {k: host(v).copy() for k, v in st.info().items()}
    out.update(corrected=host(corrected), bias=host(bias), b1=b1_copy, state=st, frozen=int(out["frozen"][0]), ok=out["ok"] != 0)
    return out


def case_on_device(name):
    c = U.case(name)
    return dict(y=dev(c["y"]), s=dev(c["s"]), mask=dev(c["mask"]), sw=dev(c["sw"]), pw=dev(c["pw"]), b0=dev(c["b0"]), sigma=c["sigma"])


def check_against(got, want, name):
    assert got["frozen"] == want["frozen"] and np.array_equal(got["ok"], want["ok"])
    assert np.array_equal(got["rows"][:, 0], want["rows"][:, 0])  # the pixel counts
    assert np.array_equal(got["rows"][:, 3:], want["rows"][:, 3:])  # min y, max y
    assert got["consts"][0] == want["consts"][0] and got["consts"][3] == want["consts"][3]  # R and the number of ok slices
    err = U.compare(got, want)
    for g in U.GROUPS:
        print(f"{name} {g}: GPU {err[g]:.3e}, E_cpu {U.E_CPU[g]:.3e}")
    for g in U.GROUPS:
        assert err[g] <= 4 * U.E_CPU[g], (g, err[g])
    for k in ("scale", "raw", "mean", "consts", "rows"):
        assert np.isfinite(got[k]).all(), k


# ---- against float64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.CASES))
def test_match_within_four_times_the_fp32_cost_of_the_formula(K, name):
    want = U.run_case(name, F64)
    U.assert_margin(want)
    got = run_match(K, **case_on_device(name))
    check_against(got, want, name)
    assert np.array_equal(np.isnan(got["corrected"]), np.isnan(U.case(name)["y"]))  # a NaN in y stays one, at that pixel only
    if name == "n1_1x1":
        assert got["frozen"] == 1 and got["scale"].tolist() == [1.0] and got["corrected"][0, 0, 0] == U.case(name)["y"][0, 0, 0]
    else:
        assert got["frozen"] == 0 and got["ok"].all()
        assert abs(got["scale"].astype(F64).mean() - 1) < 1e-6  # the gauge
    if U.CASES[name][4] > 0 and name != "n1_1x1":
        # the background is counted for the scale and not for the bias
        bg = want["part"] & ~want["inb"]
        assert bg.sum() > 0 and (U.case(name)["s"][bg] < want["consts"][1]).all() and want["inb"].sum() > 0


def test_a_pixel_whose_taps_all_miss_omega_b_gets_no_increment(K):
    name = "n5_37x29_r1"  # radius 1: the inside of the 6 x 6 background corner sees no pixel of Omega_b
    c, want = U.case(name), U.run_case(name, F64)
    assert not want["inb"][:, :6, :6].any() and want["inb"][:, 7:, 7:].any()
    got = run_match(K, **case_on_device(name))
    inc = got["b1"] - c["b0"]
    assert np.array_equal(inc[:, :5, :5], np.zeros((5, 5, 5), F32))  # exactly: Q2 == 0
    assert np.array_equal(want["inc"][:, :5, :5], np.zeros((5, 5, 5)))
    assert np.abs(inc[:, 8:, 8:]).max() > 1e-3


def test_a_slice_wholly_outside_the_mask_keeps_scale_one_and_its_bias(K):
    c = U.case("n5_36x32")
    mask = c["mask"].copy()
    mask[2] = False
    kw = dict(mask=mask, sim_weight=c["sw"], weights=c["pw"], bias0=c["b0"], sigma=2.0)
    want = U.match(c["y"], c["s"], ft=F64, **kw)
    U.assert_margin(want)
    d = case_on_device("n5_36x32")
    got = run_match(K, d["y"], d["s"], dev(mask), d["sw"], d["pw"], d["b0"], 2.0)
    check_against(got, want, "slice 2 masked out")
    assert got["ok"].tolist() == [True, True, False, True, True] and got["scale"][2] == 1 and got["rows"][2].tolist() == [0] * 5
    assert np.array_equal(got["bias"][2], c["b0"][2])
    e = np.exp(-c["b0"][2].astype(F64)) * c["y"][2]
    keep = np.isfinite(e)
    assert np.abs(got["corrected"][2][keep] - e[keep]).max() <= 4 * U.E_CPU["corrected"] * np.abs(e[keep]).max()


def test_flat_slices_and_an_empty_mask_freeze(K):
    y = torch.full((3, 13, 11), 1.5, device=DEV)
    s = torch.rand((3, 13, 11), device=DEV) + 0.5
    b0 = 0.1 * torch.rand((3, 13, 11), device=DEV)
    for mask in (None, torch.zeros((3, 13, 11), dtype=torch.bool, device=DEV)):
        r = run_match(K, y, s, mask, b0=b0, sigma=2.0)
        assert r["frozen"] == 1 and not r["ok"].any() and r["scale"].tolist() == [1, 1, 1] and r["consts"].tolist() == [0, 0, 0, 0]
        assert np.array_equal(r["bias"], host(b0)) and np.isfinite(r["corrected"]).all() and not r["mean"].any()
        e = np.exp(-host(b0).astype(F64)) * 1.5
        assert np.abs(r["corrected"] - e).max() <= 4 * U.E_CPU["corrected"] * e.max()


# ---- determinism -------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_bit_equal_twice_and_on_a_side_stream(K, svort):
    d = case_on_device("n5_37x29")
    kw = dict(weights=d["pw"], slices_mask=d["mask"], sim_weight=d["sw"], bias_sigma=2.0, return_info=True)
    a = svort.intensity_match(d["y"], d["s"], **kw)
    b = svort.intensity_match(d["y"], d["s"], **kw)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = svort.intensity_match(d["y"], d["s"], **kw)
    side.synchronize()
    for o in (b, c):
        for i in range(3):
            assert np.array_equal(_bits(host(o[i])), _bits(host(a[i]))), i
        for k in a[3]:
            assert np.array_equal(_bits(host(o[3][k])), _bits(host(a[3][k]))), k


def test_sixteen_byte_loads_and_shifted_pointers_give_the_same_bits(K):
    d = case_on_device("n5_36x32")
    assert all(d[k].data_ptr() % 16 == 0 for k in ("y", "s", "sw", "pw", "b0")) and d["mask"].data_ptr() % 4 == 0

    def shifted(t):  # the same values one element further: no pointer is 16-byte aligned, the mask not 4-byte
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        buf[1:] = t.reshape(-1)
        return buf[1:].view(t.shape)

    a = run_match(K, **d)
    b = run_match(K, **{k: (v if k == "sigma" else shifted(v)) for k, v in d.items()})
    for k in ("rows", "raw", "scale", "mean", "consts", "bias", "corrected", "b1"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_a_slice_alone_has_the_row_it_has_in_the_batch(K):
    d = case_on_device("n5_37x29_r1")
    want = run_match(K, **d)["rows"]
    for k in (0, 2, 4):
        one = run_match(K, *(d[a][k:k + 1].clone() for a in ("y", "s", "mask", "sw", "pw", "b0")), sigma=0.0)
        assert np.array_equal(_bits(one["rows"][0]), _bits(want[k])), k
    assert want[:, 1].min() > 0


def test_the_scale_is_the_same_with_and_without_the_bias_field(K):
    d = case_on_device("n5_36x32")
    a, b = run_match(K, **d), run_match(K, **dict(d, sigma=0.0))
    for k in ("rows", "raw", "scale", "consts"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(b["bias"], U.case("n5_36x32")["b0"]) and not np.array_equal(a["bias"], b["bias"])


# ---- the front end -------------------------------------------------------------------------------------------------------------------
def test_front_end_shapes_dtypes_info_and_the_kernel_sequence(K, svort):
    d = case_on_device("n5_36x32")
    ref = run_match(K, **d)
    kw = dict(weights=d["pw"][:, None], slices_mask=d["mask"][:, None], sim_weight=d["sw"], bias0=d["b0"].double(), bias_sigma=2.0)
    for y, s in ((d["y"][:, None], d["s"][:, None]), (d["y"], d["s"].double())):
        corrected, scale, bias, info = svort.intensity_match(y, s, return_info=True, **kw)
        for t, shape in ((corrected, (5, 36, 32)), (scale, (5,)), (bias, (5, 36, 32))):
            assert tuple(t.shape) == shape and t.dtype == torch.float32 and t.device.type == "cuda"
        assert set(info) == {"scale", "ok", "frozen", "raw", "rows", "mean", "consts"}
        assert info["ok"].dtype == torch.int32 and info["frozen"].dtype == torch.int32 and info["raw"].dtype == torch.float64
        for k, v in (("corrected", corrected), ("scale", scale), ("bias", bias), ("rows", info["rows"]), ("mean", info["mean"])):
            assert np.array_equal(_bits(host(v)), _bits(ref[k])), k
    out = svort.intensity_match(d["y"], d["s"])  # scale only, no info
    assert len(out) == 3 and not out[2].any() and bool((out[1] > 0).all())
    assert np.array_equal(host(out[0]), host(out[1])[:, None, None] * U.case("n5_36x32")["y"], equal_nan=True)
    with pytest.raises(NotImplementedError, match="simulated"):
        svort.intensity_match(d["y"], d["s"].clone().requires_grad_(True))


def test_refusals_write_nothing(K):
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    d = case_on_device("n5_37x29")
    y, s, mask, sw, pw = d["y"], d["s"], d["mask"], d["sw"], d["pw"]
    st = K.imatch_state(5, DEV, (37, 29))
    planes = st.reserve_planes()
    out = torch.full((5, 37, 29), SENTINEL, device=DEV)
    out2 = torch.full((5, 37, 29), SENTINEL, device=DEV)
    fill = 0x5A5A5A5A5A5A5A5A
    st.buf.fill_(fill), st.part.fill_(fill), planes.fill_(SENTINEL)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    sb, wb, pb = st.nbytes, st.part.numel() * 8, planes.numel() * 4
    bias = lambda **k: lib.fsg_imatch_bias_f32(p(y), p(s), p(mask), p(sw), k.get("mw", 0.5), p(pw), None, k.get("sigma", 2.0), 5, 37,  # noqa: E731
                                               29, p(st.buf), k.get("sb", sb), p(k.get("planes", planes)), k.get("pb", pb),
                                               p(k.get("ws", st.part)), k.get("wb", wb), p(k.get("out", out)), None)
    bad = [
        lib.fsg_imatch_sums_f32(p(y), p(s), p(mask), p(sw), -1.0, p(pw), None, 5, 37, 29, p(st.part), wb, None),
        lib.fsg_imatch_sums_f32(p(y), p(s), p(mask), p(sw), 0.5, p(pw), None, 5, 37, 29, p(st.part), wb - 1, None),
        lib.fsg_imatch_sums_f32(p(y), p(s), p(mask), p(sw), 0.5, p(pw), None, 5, 37, 29, p(y), wb, None),
        lib.fsg_imatch_scale_f32(p(st.buf), sb, p(st.part), wb, 5, 37, 29, float("nan"), 4, None),
        lib.fsg_imatch_scale_f32(p(st.buf), sb - 1, p(st.part), wb, 5, 37, 29, 0.01, 4, None),
        lib.fsg_imatch_scale_f32(p(st.buf), sb, p(st.buf), wb, 5, 37, 29, 0.01, 4, None),
        bias(sigma=0.0), bias(sigma=-1.0), bias(sigma=float("nan")), bias(sigma=16.5), bias(pb=pb - 1), bias(sb=sb - 1),
        bias(wb=wb - 1), bias(out=y), bias(planes=out), bias(mw=float("nan")),
        lib.fsg_imatch_apply_f32(p(y), None, 2, 5, 37, 29, p(st.buf), sb, p(out), p(out2), None),
        lib.fsg_imatch_apply_f32(p(y), None, 0, 5, 37, 29, p(st.buf), sb, p(out), p(out), None),
        lib.fsg_imatch_apply_f32(p(y), None, 0, 5, 37, 29, p(st.buf), sb, p(out), p(y), None),
        lib.fsg_imatch_apply_f32(p(y), None, 0, 5, 37, 29, p(st.buf), sb - 1, p(out), p(out2), None),
    ]
    torch.cuda.synchronize()
    assert bad == [_lib.E_BADARG] * len(bad)
    assert bool((out == SENTINEL).all()) and bool((out2 == SENTINEL).all()) and bool((planes == SENTINEL).all())
    assert bool((st.buf == fill).all()) and bool((st.part == fill).all())
    assert np.array_equal(host(y), U.case("n5_37x29")["y"], equal_nan=True)


# ---- the capability run on the device ------------------------------------------------------------------------------------------------
def test_capability_srr_with_three_matching_rounds(svort):
    Cc = U.capability_case()
    c = Cc["base"]
    args = (dev(c["tr"]), dev(Cc["y"][:, None]), dev(c["psf"]), BC.VS, c["res"])
    kw = dict(n_iter=6, lam=0.1, deterministic=True)
    plain = TK.rms(host(svort.srr(*args, **kw)), c["vol"])
    x, info = svort.srr(*args, n_match=U.CAP_ROUNDS, match=dict(bias_sigma=U.CAP_SIGMA), return_info=True, **kw)
    got = TK.rms(host(x), c["vol"])
    assert len(info["match"]) == 3 and set(info["match"][0]) == {"scale", "ok", "frozen"} and tuple(info["match_bias"].shape) == (42, 13, 11)
    assert all(int(m["frozen"][0]) == 0 and bool(m["ok"].all()) for m in info["match"])
    want, unmatched = U.cap_run(U.CAP_ROUNDS)[0], U.cap_run(0)[0]
    d = abs(got - want) / want
    print(f"capability on the device: RMS {got:.6f} (float64 {want:.6f}, relative difference {d:.3e}, bound "
          f"{4 * U.CAP32_RMS_DIFF:.3e}), unmatched {plain:.6f} (float64 {unmatched:.6f})")
    assert want < unmatched and got < plain
    assert d <= 4 * U.CAP32_RMS_DIFF
