"""CPU: the restatement of the outlier weights (tests/util_robust64.py) held to a literal loop, the update
rule by hand, the capability case in float64 with three mutants, and the host side of the new entries (header, build list,
refusals before any launch, front-end checks, the launch sequence of `svort.srr` with and without rejection rounds)."""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import util_robust64 as U

ROOT = Path(__file__).resolve().parents[1]
F32, F64 = np.float32, np.float64


# ---- the pixel pass against a literal loop ------------------------------------------------------------------------------------
def test_p_and_rows_follow_a_literal_loop_on_a_ragged_slice():
    c = U.synthetic_case("n5_37x29_mw")
    y, s, mask, sw = c["y"], c["s"], c["mask"], c["sw"]
    kappa, inv2var = F32(0.37), F32(11.5)
    _, e, part = U.pixels(y, s, mask, sw, 0.5, F32)
    tm, p = U.terms(e, part, kappa, inv2var, False, F32)
    got = U.rows_device(tm, y, part)
    n, h, w = y.shape
    assert (n, h, w) == (5, 37, 29) and h * w > U.CHUNK and (h * w) % 4  # two workgroups a slice, a ragged last thread
    for k in (0, 3):
        want = np.zeros(4)
        for b in range(2):
            red = np.zeros((4, 4), F32)
            for wave in range(4):
                lanes = np.zeros((64, 4), F32)
                for lane in range(64):
                    acc = np.zeros(4, F32)
                    for j in range(4):
                        i = b * 1024 + (wave * 64 + lane) * 4 + j
                        if i >= h * w:
                            continue
                        yy, xx = divmod(i, w)
                        ev = F32(y[k, yy, xx] - s[k, yy, xx])
                        if not (mask[k, yy, xx] and sw[k, yy, xx] > 0 and sw[k, yy, xx] >= F32(0.5) and np.isfinite(ev)):
                            assert p[k, yy, xx] == 0
                            continue
                        e2 = F32(ev * ev)
                        x = np.exp(F32(e2 * inv2var))
                        pv = F32(0) if np.isinf(x) else F32(F32(1) / F32(F32(1) + F32(kappa * x)))
                        assert pv == p[k, yy, xx]
                        q = F32(F32(1) - pv)
                        acc = acc + np.array([1, pv, F32(pv * e2), F32(q * q)], F32)
                    lanes[lane] = acc
                for o in (32, 16, 8, 4, 2, 1):
                    src = np.where(np.arange(64) + o < 64, np.arange(64) + o, np.arange(64))
                    lanes = lanes + lanes[src]
                red[wave] = lanes[0]
            part_sum = red[0].copy()
            for wave in range(1, 4):
                part_sum = part_sum + red[wave]
            want = want + part_sum.astype(F64)
        assert np.array_equal(got[k, :4], want)
        assert got[k, 4] == y[k][part[k]].min() and got[k, 5] == y[k][part[k]].max()
    assert not np.array_equal(got[:, 1:4], U.rows64(tm, y, part)[:, 1:4])  # and the order matters on these values
    assert not part[0, 2, 3] and not part[n - 1, 5, 1] and not part[0, 1, 1]  # the NaN, the Inf and the NaN weight


def test_overflowing_exponential_gives_zero():
    e2 = np.array([0.0, 1.0, 1e4], F32)
    p = U.posterior(e2, F32(0.5), F32(50.0), F32)
    assert p[0] == F32(1) / F32(1.5) and p[2] == 0 and 0 < p[1] < 1e-20
    assert U.posterior(e2, F32(0.0), F32(50.0), F32)[2] == 0  # kappa == 0 does not turn the overflow into a NaN


def test_e_cpu_constants_are_what_is_measured():
    m = U.measure_e_cpu()  # asserts the margin of every comparison case
    assert set(m) == set(U.E_CPU)
    for key, bound in U.E_CPU.items():
        assert 0.98 * bound <= m[key] <= bound, (key, m[key], bound)


@pytest.mark.parametrize("name", [n for n in U.SYNTH if U.SYNTH[n][0] > 1])
def test_comparison_cases_keep_every_potential_away_from_mu1_and_mu2(name):
    S = U.run_case(name)
    assert U.MARGIN <= S["margin"] < math.inf
    ws = S["ws"][-1]
    assert ws[1] == 0 and ((ws > 0.01) & (ws < 0.99)).any()  # a rejected slice and a fractional weight are both compared


# ---- the update rule by hand ---------------------------------------------------------------------------------------------------
def _rows(N, sp, spe2, sq2, mn=0.0, mx=2.0):
    n = len(N)
    r = np.zeros((n, 6))
    r[:, 0], r[:, 1], r[:, 2], r[:, 3] = N, sp, spe2, sq2
    r[:, 4], r[:, 5] = mn, mx
    return r


def test_update_slot_zero_gives_sigma_c0_and_kappa():
    S = U.new_state(2, 2)
    U.update(S, 0, _rows([100, 50], [100, 50], [4.0, 2.0], [0, 0]), c0=0.8, sigma_floor=0.01)
    var = 6.0 / 150
    assert S["consts"].tolist() == [2.0, 0.5, 0.02, 0.0]
    assert S["sigma"][0] == math.sqrt(var) and S["c"][0] == 0.8 and S["ws"][0].tolist() == [1, 1] and not S["frozen"][0]
    assert S["kappa"] == float(F32((0.2 / 0.8) * 0.5 * math.sqrt(U.TWO_PI * var))) and S["inv2var"] == float(F32(1 / (2 * var)))


def test_update_all_slices_equal_takes_the_so_zero_path():
    """so == 0 and v2 == 0: mu2 = (max u + mu1) / 2 = mu1, v2 = (mu2 - mu1)^2 / 4 = 0 -> the floor; ws = 1 from the quotient"""
    S = U.new_state(4, 2)
    r = _rows([100] * 4, [90] * 4, [1.0] * 4, [4.0] * 4)
    U.update(S, 0, r)
    U.update(S, 1, r, slice_floor=0.025)
    assert S["u"].tolist() == [0.2] * 4 and S["mu1"][1] == 0.2 and S["mu2"][1] == 0.2
    assert S["ws"][1].tolist() == [1.0] * 4 and S["c"][1] == 0.9 and not S["frozen"][1]


def test_update_both_floors_active():
    r = _rows([100, 100, 100], [99, 99, 50], [1e-6, 1e-6, 1e-6], [0.01, 1.0, 25.0])
    S = U.new_state(3, 2)
    U.update(S, 0, r, sigma_floor=0.05)
    assert S["sigma"][0] == 0.05 * 2.0  # S2 / S0 = 1e-8 is below (0.05 * 2)^2
    S["ws"][0] = [1.0, 0.5, 0.0]  # old weights that give both classes mass
    U.update(S, 1, r, sigma_floor=0.05, slice_floor=0.5)
    u = [0.01, 0.1, 0.5]
    assert np.allclose(S["u"], u, rtol=1e-15)
    mu1, mu2 = (u[0] + 0.5 * u[1]) / 1.5, (0.5 * u[1] + u[2]) / 1.5
    assert S["mu1"][1] == pytest.approx(mu1, rel=1e-14) and S["mu2"][1] == pytest.approx(mu2, rel=1e-14) and S["sigma"][1] == 0.1
    # both spreads (0.04 and 0.19) are under the floor 0.5: two normals of the same width, mix = 1.5 / 3
    g1, g2 = math.exp(-(u[1] - mu1) ** 2 / 0.5), math.exp(-(u[1] - mu2) ** 2 / 0.5)
    assert S["ws"][1][0] == 1 and S["ws"][1][2] == 0 and S["ws"][1][1] == pytest.approx(g1 / (g1 + g2), rel=1e-12)
    assert S["c"][1] == pytest.approx((99 + 0.5 * 99) / 150, rel=1e-15)  # the OLD weights in S0 / Nw


def test_update_slice_under_min_pixels_is_zero_for_good():
    S = U.new_state(3, 2)
    r = _rows([100, 3, 100], [90, 3, 80], [1.0, 0.1, 2.0], [1.0, 0.0, 9.0])
    for t in range(3):
        U.update(S, t, r, min_pixels=4)
    assert S["ws"][:, 1].tolist() == [0, 0, 0] and S["u"][1] == 0
    assert S["c"][1] == (90.0 + 80.0) / 200.0  # the slice is in no sum
    assert S["ws"][1].tolist() == [1.0, 0.0, 0.0]  # u = 0.1 < mu1 = 0.2 < mu2 = 0.25 < 0.3


def test_update_freezes_on_a_flat_image_and_on_an_empty_mask():
    for r in (_rows([100, 100], [100, 100], [1.0, 1.0], [0, 0], mn=1.0, mx=1.0),  # R == 0
              _rows([0, 0], [0, 0], [0, 0], [0, 0])):  # all-false mask: no pixel at all
        S = U.new_state(2, 2)
        for t in range(3):
            U.update(S, t, r, min_pixels=0)
        assert S["frozen"].tolist() == [1, 1, 1] and S["kappa"] == 0 and S["inv2var"] == 0
        assert S["ws"].tolist() == [[1.0 if r[0, 0] else 0.0] * 2] * 3
        for k in ("sigma", "c", "mu1", "mu2", "ws", "u", "consts"):
            assert np.isfinite(S[k]).all()


def test_em_leaves_nan_and_inf_pixels_out_and_handles_one_slice():
    c = U.synthetic_case("n1_13x11")
    S = U.em(c["y"], c["s"])
    assert not S["part"][0, 2, 3] and not S["part"][0, 5, 1] and S["part"].sum() == 13 * 11 - 2
    assert S["rows"][0, 0] == 13 * 11 - 2 and np.isfinite(S["rows"]).all() and np.isfinite(S["both"]).all()
    assert S["ws"][:, 0].tolist() == [1.0] * 6 and not S["frozen"].any()  # n == 1: u == mu1 == mu2, the weight stays 1
    assert S["slice"][0, 2, 3] == 0 and S["slice"][0, 0, 0] == 1


# ---- the capability case in float64 ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cap():
    base = U.cap_baselines()
    return dict(base=base, slice=U.cap_robust(2, "slice"))


def _capable(rms, flagged, base):
    return (set(U.CAP_VOID) <= flagged and not (flagged - set(U.CAP_VOID) - set(U.CAP_MOVED))
            and rms <= 0.5 * base["unweighted"] and rms <= 1.5 * base["oracle"])


def test_capability_rejection_recovers_the_oracle(cap):
    base, (r1, r2) = cap["base"], cap["slice"]
    print("float64:", base, "slice", r1[0], r2[0], sorted(r2[1]))
    for r in (r1, r2):
        assert set(U.CAP_VOID) <= r[1] and not (r[1] - set(U.CAP_VOID) - set(U.CAP_MOVED))  # the voids and no clean slice
    assert r2[0] <= 0.5 * base["unweighted"] and r2[0] <= 1.5 * base["oracle"]
    assert _capable(r2[0], r2[1], base)
    assert tuple(sorted(r2[1])) == U.CAP_FLAGGED
    for key, got in (("clean", base["clean"]), ("unweighted", base["unweighted"]), ("oracle", base["oracle"]),
                     ("slice_1", r1[0]), ("slice_2", r2[0])):
        assert 0.98 * U.CAP_RMS[key] <= got <= U.CAP_RMS[key], (key, got)
    c = r1[2]["c"]
    assert abs(c[1] - U.CAP_C[0]) <= 1e-5 and abs(c[-1] - U.CAP_C[1]) <= 1e-5


def test_capability_pixel_times_slice_weights(cap):
    r1, r2 = U.cap_robust(2, "both")
    assert _capable(r2[0], r2[1], cap["base"])
    for key, got in (("both_1", r1[0]), ("both_2", r2[0])):
        assert 0.98 * U.CAP_RMS[key] <= got <= U.CAP_RMS[key], (key, got)


def test_mutant_without_the_sigma_floor_fails(cap):
    """the pixel posteriors switch off the pixels where the short solve is still biased: 0.172 measured after two rounds"""
    r = U.cap_robust(2, "both", mutant="no_sigma_floor")
    print("no_sigma_floor:", [x[0] for x in r], [sorted(x[1]) for x in r])
    assert not _capable(r[1][0], r[1][1], cap["base"])
    assert not set(U.CAP_VOID) <= r[0][1]  # and slice 20 is missed in the first round


def test_mutant_with_the_new_slice_weights_in_the_pixel_sums_fails(cap):
    """With the sigma floor active this mutant moves the inlier fraction c and not the RMS (0.0341 / 0.0300 either way), so it
    is held to the recorded c of the first round's EM, which the rule reproduces to 1e-5 and the mutant misses by 0.02."""
    c = U.cap_first_em(mutant="new_ws_in_sums")["c"]
    print("new_ws_in_sums: c", c)
    assert abs(c[1] - U.CAP_C[0]) > 1e-2
    assert abs(cap["slice"][0][2]["c"][1] - U.CAP_C[0]) <= 1e-5


def test_mutant_without_the_mu2_rule_fails(cap):
    """without u > mu2 -> 0 the quotient of the densities rises again beyond mu2 (the outlier class is the wider one only from
    the second sweep on): nothing is flagged"""
    r = U.cap_robust(1, "slice", mutant="no_mu2_rule")
    print("no_mu2_rule:", r[0][0], sorted(r[0][1]))
    assert not _capable(r[0][0], r[0][1], cap["base"])


def test_fp32_restatement_gives_the_recorded_capability_difference(cap):
    r32 = U.cap_robust(2, "slice", F32)
    r64 = cap["slice"]
    d = abs(r32[1][0] - r64[1][0]) / r64[1][0]
    print("fp32:", r32[1][0], "diff", d)
    assert tuple(sorted(r32[1][1])) == U.CAP_FLAGGED
    assert 0.9 * U.CAP32_RMS_DIFF <= d <= U.CAP32_RMS_DIFF


# ---- the host side of the new entries ---------------------------------------------------------------------------------------
ENTRIES = ("fsg_robust_ws_bytes", "fsg_robust_state_bytes", "fsg_robust_estep_f32", "fsg_robust_update_f32",
           "fsg_robust_weights_f32")


def test_header_build_list_and_abi():
    from fetalsyngen_amd import _build, _lib

    text = (ROOT / "include" / "fsg_hip.h").read_text()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", text) and name in _lib.PROTOTYPES
    assert _lib.ABI_VERSION == 8 and (_lib.ROBUST_SLICE, _lib.ROBUST_BOTH) == (0, 1)
    assert "fsg_robust.hip" in _build.SOURCES and (ROOT / "fetalsyngen_amd" / "csrc" / "fsg_robust.hip").exists()
    for phrase in ("permuting the slices permutes the result only up to rounding", "It needs no initialisation",
                   "No NaN is ever stored", "double consts[4]"):
        assert phrase in text, phrase


N_, H_, W_, T_ = 5, 37, 29, 5


def _addr(**kw):
    a = dict(y=1 << 24, s=2 << 24, sw=3 << 24, sm=4 << 24, state=5 << 24, ws=6 << 24, out=7 << 24, n=N_, h=H_, w=W_, t=0, T=T_,
             min_weight=0.5, state_bytes=None, ws_bytes=None, c0=0.9, sigma_floor=0.04, slice_floor=0.025, min_pixels=4, level=0)
    a.update(kw)
    return a


def _estep(lib, **kw):
    a, p = _addr(**kw), ctypes.c_void_p
    sb = lib.fsg_robust_state_bytes(N_, T_) if a["state_bytes"] is None else a["state_bytes"]
    wb = lib.fsg_robust_ws_bytes(N_, H_, W_) if a["ws_bytes"] is None else a["ws_bytes"]
    return lib.fsg_robust_estep_f32(p(a["y"]), p(a["s"]), p(a["sm"]), p(a["sw"]), a["min_weight"], a["n"], a["h"], a["w"], a["t"],
                                    a["T"], p(a["state"]), sb, p(a["ws"]), wb, None)


def _update(lib, **kw):
    a, p = _addr(**kw), ctypes.c_void_p
    sb = lib.fsg_robust_state_bytes(N_, T_) if a["state_bytes"] is None else a["state_bytes"]
    wb = lib.fsg_robust_ws_bytes(N_, H_, W_) if a["ws_bytes"] is None else a["ws_bytes"]
    return lib.fsg_robust_update_f32(p(a["state"]), sb, p(a["ws"]), wb, a["n"], a["h"], a["w"], a["t"], a["T"], a["c0"],
                                     a["sigma_floor"], a["slice_floor"], a["min_pixels"], None)


def _weights(lib, **kw):
    a, p = _addr(**kw), ctypes.c_void_p
    sb = lib.fsg_robust_state_bytes(N_, T_) if a["state_bytes"] is None else a["state_bytes"]
    return lib.fsg_robust_weights_f32(p(a["y"]), p(a["s"]), p(a["sm"]), p(a["sw"]), a["min_weight"], a["n"], a["h"], a["w"], a["T"],
                                      a["level"], p(a["state"]), sb, p(a["out"]), None)


def test_entries_refuse_before_any_launch():
    """no device is needed: every refusal returns before the first launch (the addresses are made up)"""
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    BAD, BIG, ALIGN = _lib.E_BADARG, _lib.E_TOOBIG, _lib.E_ALIGN
    nan, inf = float("nan"), float("inf")
    assert lib.fsg_robust_ws_bytes(5, 37, 29) == 5 * 2 * 32 and lib.fsg_robust_ws_bytes(1, 13, 11) == 32
    assert lib.fsg_robust_ws_bytes(0, 4, 4) == 0 and lib.fsg_robust_ws_bytes(1, 0, 4) == 0 and lib.fsg_robust_ws_bytes(4, 65536, 65536) == 0
    s = T_ + 1
    sb = lib.fsg_robust_state_bytes(N_, T_)
    assert sb == (8 * (4 + 6 * N_ + N_ + 4 * s + s * N_) + 4 * (2 + s) + 7) // 8 * 8
    assert lib.fsg_robust_state_bytes(0, 5) == 0 and lib.fsg_robust_state_bytes(5, 0) == 0 and lib.fsg_robust_state_bytes(5, 4097) == 0
    pix = N_ * H_ * W_ * 4
    for call in (_estep, _weights):
        for key in ("y", "s", "state"):
            assert call(lib, **{key: 0}) == BAD, key
        for kw in (dict(n=0), dict(h=0), dict(w=-1), dict(T=0), dict(T=4097), dict(min_weight=-0.5), dict(min_weight=nan),
                   dict(state_bytes=sb - 1)):
            assert call(lib, **kw) == BAD, kw
        for kw in (dict(n=65536, state_bytes=1 << 40, ws_bytes=1 << 40), dict(h=65536, w=65536, ws_bytes=1 << 40)):
            assert call(lib, **kw) == BIG, kw
        for kw in (dict(y=(1 << 24) + 2), dict(s=(2 << 24) + 1), dict(sw=(3 << 24) + 2), dict(state=(5 << 24) + 4)):
            assert call(lib, **kw) == ALIGN, kw
    for kw in (dict(ws=0), dict(t=-1), dict(t=T_ + 1), dict(ws_bytes=5 * 2 * 32 - 1), dict(ws=(5 << 24) + 8), dict(ws=(1 << 24) + pix - 4),
               dict(ws=(2 << 24) + 16), dict(ws=(3 << 24) + 16), dict(ws=(4 << 24) + 8)):
        assert _estep(lib, **kw) == BAD, kw
    assert _estep(lib, ws=(6 << 24) + 4) == ALIGN
    for kw in (dict(state=0), dict(ws=0), dict(n=0), dict(h=0), dict(t=-1), dict(t=T_ + 1), dict(T=0), dict(state_bytes=sb - 1),
               dict(ws_bytes=5 * 2 * 32 - 1), dict(c0=0.0), dict(c0=1.5), dict(c0=nan), dict(sigma_floor=-0.1), dict(sigma_floor=nan),
               dict(sigma_floor=inf), dict(slice_floor=-1.0), dict(slice_floor=nan), dict(min_pixels=-1), dict(ws=(5 << 24) + 64)):
        assert _update(lib, **kw) == BAD, kw
    assert _update(lib, n=65536, state_bytes=1 << 40, ws_bytes=1 << 40) == BIG
    assert _update(lib, state=(5 << 24) + 4) == ALIGN and _update(lib, ws=(6 << 24) + 4) == ALIGN
    for kw in (dict(out=0), dict(level=2), dict(level=-1), dict(out=(1 << 24) + 16), dict(out=(2 << 24) + pix - 4), dict(out=(3 << 24) + 4),
               dict(out=(4 << 24) + 4), dict(out=(5 << 24) + 8)):
        assert _weights(lib, **kw) == BAD, kw
    assert _weights(lib, out=(7 << 24) + 2) == ALIGN
    # a slice's pixels are counted in int, 1024 to a workgroup: the last workgroup's first index has to fit
    edge = 2 ** 31 - 1 - 1024
    for call in (_estep, _update, _weights):
        assert call(lib, n=1, h=1, w=edge + 1, state_bytes=1 << 40, ws_bytes=1 << 40) == BIG, call.__name__
    fn = lib.fsg_robust_ws_bytes
    assert fn(1, 1, edge) > 0 and fn(1, edge, 1) > 0 and fn(1, 1, edge + 1) == 0 and fn(1, 2, edge // 2 + 1) == 0


@pytest.mark.parametrize("T", (1, 2, 12, 4096))
@pytest.mark.parametrize("n", (1, 5, 1024, 1025))
def test_state_bytes_is_the_headers_formula(n, T):
    """fsg_robust_state_bytes against the layout paragraph of include/fsg_hip.h, written out; s = T + 1 takes both parities,
    so the rounding to 8 is exercised"""
    from fetalsyngen_amd import _lib

    lib, s = _lib.load(), T + 1
    assert lib.fsg_robust_state_bytes(n, T) == (8 * (4 + 6 * n + n + 4 * s + s * n) + 4 * (2 + s) + 7) // 8 * 8
    assert lib.fsg_robust_state_bytes(n, 0) == 0 and lib.fsg_robust_state_bytes(n, 4096 + 1) == 0


def test_front_ends_refuse_cpu_tensors_and_bad_arguments():
    import torch

    from fetalsyngen_amd import kernels as K
    from fetalsyngen_amd.generator.artifacts import svort

    st = K.robust_state(3, 4, "cpu", (13, 11))  # the layout is checked against fsg_robust_state_bytes on any device
    assert st.ws.shape == (5, 3) and st.rows.shape == (3, 6) and st.sigma.shape == (5,) and st.scal.shape == (2,)
    assert st.part.numel() * 8 == 3 * 32
    assert set(st.info()) == {"sigma", "c", "mu1", "mu2", "frozen", "ws", "u"}
    y = torch.zeros(3, 13, 11)
    with pytest.raises(RuntimeError, match="MI355X"):
        K.robust_estep(st, 0, y, y.clone())
    with pytest.raises(RuntimeError, match="MI355X"):
        K.robust_weights(st, y, y.clone())
    with pytest.raises(ValueError, match="level"):
        K.robust_weights(st, y, y.clone(), level="pixel")
    with pytest.raises(ValueError, match="follows robust_estep"):
        K.robust_update(K.robust_state(3, 4, "cpu"), 0)
    for n, k in ((0, 3), (2, 0), (2, 4097)):
        with pytest.raises(ValueError):
            K.robust_state(n, k, "cpu")
    with pytest.raises(RuntimeError, match="MI355X"):
        svort.robust_weights(y, y.clone())
    for kw in (dict(n_em=0), dict(c0=0.0), dict(c0=float("nan")), dict(sigma_floor=-1.0), dict(slice_floor=float("nan")),
               dict(min_pixels=-1), dict(level="pixel"), dict(min_weight=-0.5)):
        with pytest.raises(ValueError):
            svort.robust_weights(y, y.clone(), **kw)


def test_robust_weights_and_srr_refuse_inputs_that_require_grad():
    import torch

    from fetalsyngen_amd.generator.artifacts import svort

    y = torch.zeros(3, 13, 11)
    for name in ("slices", "simulated", "sim_weight"):
        a = dict(slices=y, simulated=y.clone(), sim_weight=y.clone())
        a[name] = a[name].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match=name):
            svort.robust_weights(a["slices"], a["simulated"], sim_weight=a["sim_weight"])
    with pytest.raises(ValueError, match="n_robust"):
        svort.srr(torch.zeros(3, 3, 4), y, torch.ones(1, 1, 1), (4, 4, 4), 1.0, robust=dict(n_em=3))
    with pytest.raises(ValueError, match="n_robust"):
        svort.srr(torch.zeros(3, 3, 4), y, torch.ones(1, 1, 1), (4, 4, 4), 1.0, n_robust=-1)
    with pytest.raises(ValueError, match="unknown robust option"):
        svort.srr(torch.zeros(3, 3, 4), y, torch.ones(1, 1, 1), (4, 4, 4), 1.0, n_robust=1, robust=dict(sigma=0.1))


def test_namespace_exports():
    import importlib

    from fetalsyngen_amd import kernels as K
    from fetalsyngen_amd.generator.artifacts import svort

    module = importlib.import_module("fetalsyngen_amd.generator.artifacts.svort.outlier")
    assert svort.robust_weights is module.robust_weights
    for name in ("robust_state", "robust_estep", "robust_update", "robust_weights", "RobustState"):
        assert callable(getattr(K, name))
    s = svort.SRR(n_iter=3)
    assert s.reg == {}
    s = svort.SRR(n_iter=3, n_robust=2, robust=dict(level="both"))
    assert s.reg == {"n_robust": 2, "robust": {"level": "both"}}


# ---- the launch sequence of srr ---------------------------------------------------------------------------------------------------
def _record(monkeypatch, log):
    import torch

    from fetalsyngen_amd import kernels as K

    D = (4, 4, 4)

    def fwd(tr, v, vm, sm, ps, ss, res, need_weight=False, **kw):
        log.append("fwd_w" if need_weight else "fwd")
        out = torch.zeros(tr.shape[0], *ss)
        return (out, torch.ones_like(out)) if need_weight else out

    def adj(tr, ps, s, *a, **kw):
        log.append("adj")
        return torch.zeros(D)

    def mul(a, b):
        log.append("mul")
        return a

    class Ws:
        def info(self):
            return dict(rr=None, pq=None, alpha=None, beta=None, frozen=None)

    class St:
        n_em = 2

        def info(self):
            return dict(sigma=None, c=None, mu1=None, mu2=None, frozen=None, ws=None, u=None)

    monkeypatch.setattr(K, "slice_acq_forward", fwd)
    monkeypatch.setattr(K, "slice_acq_adjoint", adj)
    monkeypatch.setattr(K, "mul", mul)
    monkeypatch.setattr(K, "cg_workspace", lambda n, k, dev: Ws())
    monkeypatch.setattr(K, "cg_init", lambda *a, **kw: log.append("init"))
    monkeypatch.setattr(K, "cg_q", lambda *a, **kw: log.append("q"))
    monkeypatch.setattr(K, "cg_step", lambda ws, k, p, q, x, r, relu=False: log.append("step_relu" if relu else "step"))
    monkeypatch.setattr(K, "cg_dir", lambda *a, **kw: log.append("dir"))
    monkeypatch.setattr(K, "_need_gpu", lambda *a: None)
    monkeypatch.setattr(K, "robust_state", lambda n, n_em, dev, ss=None: St())
    monkeypatch.setattr(K, "robust_estep", lambda st, t, *a: log.append(("estep", t)))
    monkeypatch.setattr(K, "robust_update", lambda st, t, **kw: log.append(("update", t, kw["sigma_floor"])))
    monkeypatch.setattr(K, "robust_weights", lambda st, y, *a, **kw: (log.append(("weights", kw["level"])), torch.ones_like(y))[1])


def _solve(n_iter, relu_last):
    # the flag goes to every step of the solve; fsg_cg_step_f32 honours it in the last one only
    return ["adj", "init"] + ["fwd", "adj", "q", "step_relu" if relu_last else "step", "dir"] * n_iter


def test_srr_launch_sequence_is_todays_without_rejection_rounds(monkeypatch):
    import torch

    from fetalsyngen_amd.generator.artifacts import svort

    log = []
    _record(monkeypatch, log)
    out, info = svort.srr(torch.zeros(3, 3, 4), torch.zeros(3, 1, 5, 7), torch.ones(1, 1, 1), (4, 4, 4), 1.0, n_iter=3,
                          return_info=True)
    assert log == _solve(3, True)
    assert set(info) == {"rr", "pq", "alpha", "beta", "frozen"} and tuple(out.shape) == (1, 1, 4, 4, 4)


def test_srr_launch_sequence_with_one_rejection_round(monkeypatch):
    import torch

    from fetalsyngen_amd.generator.artifacts import svort

    log = []
    _record(monkeypatch, log)
    out, info = svort.srr(torch.zeros(3, 3, 4), torch.zeros(3, 1, 5, 7), torch.ones(1, 1, 1), (4, 4, 4), 1.0, n_iter=3,
                          return_info=True, n_robust=1, robust=dict(n_em=2, sigma_floor=0.1, level="both"))
    em = ["fwd_w"] + [x for t in range(3) for x in (("estep", t), ("update", t, 0.1))] + [("weights", "both")]
    # the second solve is weighted: y * w for the right-hand side, and a multiplication between A and A^T in every iteration
    second = ["mul", "adj", "init"] + ["fwd", "mul", "adj", "q", "step_relu", "dir"] * 3
    assert log == _solve(3, False) + em + second
    assert set(info) == {"rr", "pq", "alpha", "beta", "frozen", "robust"} and len(info["robust"]) == 1
    assert set(info["robust"][0]) == {"sigma", "c", "mu1", "mu2", "frozen", "ws", "u"}
