"""CPU: the restatement of the slice intensity matching (tests/util_imatch64.py) held to closed forms, the
gauge and the freeze rules by hand, the capability case in float64, and the host side of the new entries (header, build list,
byte counts, refusals before any launch, front-end checks, the launch sequence of `svort.srr` with and without matching
rounds)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests import util_imatch64 as U

ROOT = Path(__file__).resolve().parents[1]
F32, F64 = np.float32, np.float64


# ---- closed forms ------------------------------------------------------------------------------------------------------------------
def test_constant_slices_against_a_constant_simulation_give_the_exact_ratio():
    y = np.stack([np.full((6, 5), 1.0, F32), np.full((6, 5), 2.0, F32)])
    s = np.full((2, 6, 5), 3.0, F32)
    for ft in (F64, F32):
        S = U.match(y, s, ft=ft)
        assert S["raw"].tolist() == [3.0, 1.5] and S["consts"].tolist() == [1.0, 0.01, 2.25, 2.0] and not S["frozen"]
        assert S["scale"].tolist() == [float(ft(3.0 / 2.25)), float(ft(1.5 / 2.25))]
        # both slices come out as the simulation over the gauge
        assert np.allclose(S["corrected"], 3.0 / 2.25, rtol=2e-7, atol=0)
    one = U.match(y[:1], s[:1])  # one constant slice: the ratio is exact, and R == 0 freezes the call
    assert one["raw"].tolist() == [3.0] and one["frozen"] == 1 and one["scale"].tolist() == [1.0]
    assert np.array_equal(one["corrected"], y[:1])


def test_a_smooth_bias_is_recovered_away_from_the_border():
    h, w, sigma = 41, 37, 2.0
    yy, xx = np.meshgrid(np.arange(h, dtype=F64), np.arange(w, dtype=F64), indexing="ij")
    s = np.stack([1.5 + 0.5 * np.sin(yy / 5 + k) * np.cos(xx / 7) for k in range(3)])
    b = np.stack([0.004 * (k + 1) * (yy - h / 2) - 0.003 * (xx - w / 2) for k in range(3)])  # a ramp: the blur's fixed point
    gain = np.array([0.8, 1.0, 1.3])
    y = (s * np.exp(b) / gain[:, None, None]).astype(F32)
    S = U.match(y, s.astype(F32), sigma=sigma)
    Rr = U.taps(sigma)[0]
    inner = (slice(None), slice(Rr, h - Rr), slice(Rr, w - Rr))
    off = (S["bias"] - b)[inner]
    # y and s are rounded to fp32 (6e-8 each): bias = b + a constant per slice to that accuracy
    assert np.abs(off - off.mean((1, 2), keepdims=True)).max() < 3e-7
    ratio = (S["corrected"] / s)[inner]
    assert np.abs(ratio / ratio.mean((1, 2), keepdims=True) - 1).max() < 3e-7  # inside a slice one gain remains
    assert np.abs((S["bias"] * S["inb"]).sum((1, 2))).max() < 1e-9  # the weighted mean of every field is 0
    flat = U.match(y, s.astype(F32), sigma=0.0)
    r2 = (flat["corrected"] / s)[inner]
    assert np.abs(r2 / r2.mean((1, 2), keepdims=True) - 1).max() > 0.05  # scale only leaves the ramp in


def test_the_gauge_gives_mean_one_and_ignores_a_common_gain():
    c = U.case("n5_37x29")
    kw = dict(mask=c["mask"], sim_weight=c["sw"], weights=c["pw"], sigma=2.0)
    a = U.match(c["y"], c["s"], **kw)
    assert abs(a["scale"][a["ok"]].mean() - 1) < 1e-15 and a["consts"][3] == 5
    assert a["consts"][2] == pytest.approx(a["raw"].mean(), rel=1e-15)
    b = U.match(2 * c["y"], c["s"], **kw)
    assert np.allclose(b["scale"], a["scale"], rtol=1e-14) and b["consts"][2] == pytest.approx(a["consts"][2] / 2, rel=1e-14)
    keep = np.isfinite(a["corrected"])
    assert np.allclose(b["corrected"][keep], 2 * a["corrected"][keep], rtol=1e-6)


def test_slices_that_do_not_qualify_keep_scale_one_and_their_bias():
    c = U.case("n5_36x32")
    mask = c["mask"].copy()
    mask[1] = False
    mask[1, 0, :3] = True  # three pixels: under min_pixels
    y = c["y"].copy()
    y[3] = -np.abs(y[3])  # A <= 0: no gain to speak of
    S = U.match(y, c["s"], mask, c["sw"], weights=c["pw"], bias0=c["b0"], sigma=2.0)
    assert S["ok"].tolist() == [True, False, True, False, True] and not S["frozen"] and S["consts"][3] == 3
    assert S["scale"][1] == 1 and S["scale"][3] == 1 and 0 < S["rows"][1, 0] <= 3 and S["raw"][1] == 0 and S["raw"][3] == 0
    for k in (1, 3):
        assert np.array_equal(S["bias"][k], c["b0"][k].astype(F64)) and not S["inb"][k].any() and S["mean"][k] == 0
    assert abs(S["scale"][[0, 2, 4]].mean() - 1) < 1e-15


def test_freeze_rules():
    c = U.case("n5_37x29")
    flat = U.match(np.full((3, 7, 5), 1.5, F32), np.full((3, 7, 5), 2.0, F32), sigma=2.0)  # R == 0
    empty = U.match(c["y"], c["s"], np.zeros(c["y"].shape, bool), sigma=2.0)  # no pixel
    few = U.match(c["y"], c["s"], min_pixels=10 ** 6, sigma=2.0)  # no slice qualifies
    neg = U.match(-np.abs(c["y"]), np.abs(c["s"]), sigma=2.0)  # every A < 0
    for S in (flat, empty, few, neg):
        assert S["frozen"] == 1 and not S["ok"].any() and S["scale"].tolist() == [1.0] * len(S["scale"])
        assert S["consts"].tolist() == [0, 0, 0, 0] and not S["inb"].any() and not np.asarray(S["bias"]).any()
        for k in ("rows", "raw", "scale", "mean", "consts"):
            assert np.isfinite(S[k]).all()
    assert np.array_equal(flat["corrected"], np.full((3, 7, 5), 1.5))
    huge = U.scale(np.array([[10, 1e-30, 1.0, 0, 1], [10, 1e30, 1e-30, 0, 1]]))  # raw = 1e-30 and 1e60: raw / g leaves fp32
    assert huge["frozen"] == 1 and huge["scale"].tolist() == [1, 1]
    inf = U.scale(np.array([[10, 1e30, 1e-300, 0, 1], [10, 2.0, 1.0, 0, 1]]))  # a quotient that leaves double: that slice is out
    assert inf["frozen"] == 0 and inf["ok"].tolist() == [False, True] and inf["raw"].tolist() == [0, 2] and inf["scale"].tolist() == [1, 1]


def test_nan_and_inf_reach_no_sum_and_stay_where_they_are():
    c = U.case("n5_37x29")
    S = U.match(c["y"], c["s"], c["mask"], c["sw"], weights=c["pw"], sigma=2.0)
    h = 37
    for k, i, j in ((0, h - 1, 3), (4, h - 2, 1), (0, h - 2, 4), (0, h - 1, 1)):  # NaN y, Inf y, NaN s, NaN weight
        assert not S["part"][k, i, j]
    assert all(np.isfinite(S[k]).all() for k in ("rows", "raw", "scale", "mean", "consts", "bias"))
    assert np.array_equal(np.isnan(S["corrected"]), np.isnan(c["y"])) and np.isinf(S["corrected"][4, h - 2, 1])


def test_blur_follows_a_literal_loop_and_skips_taps_outside_the_slice():
    rng = np.random.default_rng(5)
    p = rng.standard_normal((2, 5, 7)).astype(F32)
    Rr, g = U.taps(4.0)
    assert Rr == 12 and g[0] == 1 and g.dtype == F32
    got = U.blur(p, g, Rr, 2, F32)
    for k, i, j in ((0, 0, 0), (1, 4, 6), (0, 2, 3)):
        acc = F32(0)
        for t in range(-Rr, Rr + 1):
            if 0 <= j + t < 7:
                acc = F32(F64(g[abs(t)]) * F64(p[k, i, j + t]) + F64(acc))
        assert got[k, i, j] == acc
    q = U.blur(np.ones((1, 5, 7), F64), g, Rr, 1, F64)  # the weight plane: the sum of the taps inside the slice
    assert q[0, 0, 0] == pytest.approx(float(g[:5].astype(F64).sum()), rel=1e-15)


def test_means_follow_the_column_passs_tiles():
    rng = np.random.default_rng(6)
    t = rng.standard_normal((2, 65, 33)).astype(F32)
    om = rng.uniform(0.2, 1, t.shape).astype(F32)
    inb = rng.random(t.shape) < 0.8
    num, den = U.means_device(t, om, inb)
    assert num.shape == (2,) and np.allclose(num, np.where(inb, t, 0).astype(F64).sum((1, 2)), rtol=0, atol=1e-4)
    assert np.allclose(den, np.where(inb, om, 0).astype(F64).sum((1, 2)), rtol=1e-6)
    # tile (1, 1) is the single pixel (64, 32): its partial is that pixel
    only = np.zeros(t.shape, bool)
    only[:, 64, 32] = True
    assert np.array_equal(U.means_device(t, om, only)[0], t[:, 64, 32].astype(F64))


def test_e_cpu_constants_are_what_is_measured():
    m = U.measure_e_cpu()  # asserts the margin of every comparison case
    assert set(m) == set(U.E_CPU)
    for key, bound in U.E_CPU.items():
        assert 0.98 * bound <= m[key] <= bound, (key, m[key], bound)


# ---- the capability case in float64 ---------------------------------------------------------------------------------------------
def test_capability_matching_beats_the_unmatched_solve():
    t = U.cap_table()
    print("float64:", t)
    assert set(t) == set(U.CAP_RMS)
    for key, got in t.items():
        assert 0.98 * U.CAP_RMS[key] <= got <= U.CAP_RMS[key], (key, got)
    assert t["matched_3"] < t["corrupted"] and t["matched_1"] < t["corrupted"] and t["scale_only_3"] < t["corrupted"]
    assert t["matched_3"] < t["scale_only_3"]  # the bias field earns its launches


def test_fp32_restatement_gives_the_recorded_capability_difference():
    r32, r64 = U.cap_run(U.CAP_ROUNDS, ft=F32)[0], U.cap_run(U.CAP_ROUNDS)[0]
    d = abs(r32 - r64) / r64
    print("fp32:", r32, "diff", d)
    assert 0.9 * U.CAP32_RMS_DIFF <= d <= U.CAP32_RMS_DIFF


# ---- the host side of the new entries ---------------------------------------------------------------------------------------
ENTRIES = ("fsg_imatch_ws_bytes", "fsg_imatch_state_bytes", "fsg_imatch_plane_bytes", "fsg_imatch_sums_f32", "fsg_imatch_scale_f32",
           "fsg_imatch_bias_f32", "fsg_imatch_apply_f32")


def test_header_build_list_and_abi():
    from fetalsyngen_amd import _build, _lib

    text = (ROOT / "include" / "fsg_hip.h").read_text()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", text) and name in _lib.PROTOTYPES
    assert _lib.ABI_VERSION == 8 and _lib.load().fsg_abi_version() == 8
    assert (_lib.IMATCH_SCALE_ONLY, _lib.IMATCH_WITH_BIAS, _lib.IMATCH_ROW) == (0, 1, 5) and _lib.IMATCH_MAX_RADIUS >= 48
    assert _lib.IMATCH_MAX_RADIUS == U.MAX_RADIUS
    assert "fsg_imatch.hip" in _build.SOURCES and (ROOT / "fetalsyngen_amd" / "csrc" / "fsg_imatch.hip").exists()
    for phrase in ("a tap outside the slice is skipped", "It needs no initialisation", "No NaN is ever stored", "double consts[4]",
                   "NOT normalised"):
        assert phrase in text, phrase


@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (5, 37, 29), (5, 36, 32), (2, 65, 33), (3, 64, 32), (7, 1024, 1), (1025, 3, 1025)])
def test_byte_counts_are_the_headers_formulas(n, h, w):
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    assert lib.fsg_imatch_state_bytes(n) == (8 * (4 + 5 * n + n + n) + 4 * (n + n + 1) + 7) // 8 * 8
    chunks, tiles = -(-(h * w) // 1024), -(-h // 64) * -(-w // 32)
    assert lib.fsg_imatch_ws_bytes(n, h, w) == 32 * n * chunks + 8 * n * tiles
    assert lib.fsg_imatch_plane_bytes(n, h, w) == 12 * n * h * w
    assert lib.fsg_imatch_state_bytes(0) == 0 and lib.fsg_imatch_state_bytes(65536) == 0
    for fn in (lib.fsg_imatch_ws_bytes, lib.fsg_imatch_plane_bytes):
        assert fn(0, h, w) == 0 and fn(n, 0, w) == 0 and fn(n, h, -1) == 0 and fn(4, 65536, 65536) == 0 and fn(65536, 1, 1) == 0


N_, H_, W_ = 5, 37, 29


def _addr(**kw):
    a = dict(y=1 << 24, s=2 << 24, sw=3 << 24, sm=4 << 24, pw=5 << 24, b0=6 << 24, state=7 << 24, ws=8 << 24, planes=9 << 24,
             bias=10 << 24, corrected=11 << 24, n=N_, h=H_, w=W_, min_weight=0.5, sigma=2.0, log_floor=0.01, min_pixels=4, mode=0,
             state_bytes=None, ws_bytes=None, plane_bytes=None)
    a.update(kw)
    return a


def _sizes(lib, a):
    sb = lib.fsg_imatch_state_bytes(N_) if a["state_bytes"] is None else a["state_bytes"]
    wb = lib.fsg_imatch_ws_bytes(N_, H_, W_) if a["ws_bytes"] is None else a["ws_bytes"]
    pb = lib.fsg_imatch_plane_bytes(N_, H_, W_) if a["plane_bytes"] is None else a["plane_bytes"]
    return sb, wb, pb


def _sums(lib, **kw):
    a, p = _addr(**kw), ctypes.c_void_p
    _, wb, _ = _sizes(lib, a)
    return lib.fsg_imatch_sums_f32(p(a["y"]), p(a["s"]), p(a["sm"]), p(a["sw"]), a["min_weight"], p(a["pw"]), p(a["b0"]), a["n"], a["h"],
                                   a["w"], p(a["ws"]), wb, None)


def _scale(lib, **kw):
    a, p = _addr(**kw), ctypes.c_void_p
    sb, wb, _ = _sizes(lib, a)
    return lib.fsg_imatch_scale_f32(p(a["state"]), sb, p(a["ws"]), wb, a["n"], a["h"], a["w"], a["log_floor"], a["min_pixels"], None)


def _bias(lib, **kw):
    a, p = _addr(**kw), ctypes.c_void_p
    sb, wb, pb = _sizes(lib, a)
    return lib.fsg_imatch_bias_f32(p(a["y"]), p(a["s"]), p(a["sm"]), p(a["sw"]), a["min_weight"], p(a["pw"]), p(a["b0"]), a["sigma"],
                                   a["n"], a["h"], a["w"], p(a["state"]), sb, p(a["planes"]), pb, p(a["ws"]), wb, p(a["bias"]), None)


def _apply(lib, **kw):
    a, p = _addr(**kw), ctypes.c_void_p
    sb, _, _ = _sizes(lib, a)
    return lib.fsg_imatch_apply_f32(p(a["y"]), p(a["b0"]), a["mode"], a["n"], a["h"], a["w"], p(a["state"]), sb, p(a["bias"]),
                                    p(a["corrected"]), None)


def test_entries_refuse_before_any_launch():
    """no device is needed: every refusal returns before the first launch (the addresses are made up)"""
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    BAD, BIG, ALIGN = _lib.E_BADARG, _lib.E_TOOBIG, _lib.E_ALIGN
    nan, inf = float("nan"), float("inf")
    pix = N_ * H_ * W_ * 4
    big = dict(state_bytes=1 << 40, ws_bytes=1 << 40, plane_bytes=1 << 40)
    for call in (_sums, _bias):
        for key in ("y", "s"):
            assert call(lib, **{key: 0}) == BAD, key
        for kw in (dict(n=0), dict(h=0), dict(w=-1), dict(min_weight=-0.5), dict(min_weight=nan), dict(ws=0), dict(ws_bytes=0)):
            assert call(lib, **kw) == BAD, kw
        for kw in (dict(n=65536, **big), dict(h=65536, w=65536, **big)):
            assert call(lib, **kw) == BIG, kw
        for kw in (dict(y=(1 << 24) + 2), dict(s=(2 << 24) + 1), dict(sw=(3 << 24) + 2), dict(pw=(5 << 24) + 2), dict(b0=(6 << 24) + 1),
                   dict(ws=(8 << 24) + 4)):
            assert call(lib, **kw) == ALIGN, kw
        for kw in (dict(ws=(1 << 24) + pix - 4), dict(ws=(2 << 24) + 16), dict(ws=(3 << 24) + 16), dict(ws=(4 << 24) + 8),
                   dict(ws=(5 << 24) + 8), dict(ws=(6 << 24) + 8)):  # the workspace over each of the six inputs
            assert call(lib, **kw) == BAD, kw
    for kw in (dict(state=0), dict(ws=0), dict(n=0), dict(h=0), dict(state_bytes=0), dict(ws_bytes=8), dict(log_floor=-0.1),
               dict(log_floor=nan), dict(log_floor=inf), dict(min_pixels=-1), dict(ws=(7 << 24) + 64)):
        assert _scale(lib, **kw) == BAD, kw
    assert _scale(lib, n=65536, **big) == BIG
    assert _scale(lib, state=(7 << 24) + 4) == ALIGN and _scale(lib, ws=(8 << 24) + 4) == ALIGN
    sb = lib.fsg_imatch_state_bytes(N_)
    for kw in (dict(state=0), dict(planes=0), dict(bias=0), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=nan), dict(sigma=inf),
               dict(sigma=(_lib.IMATCH_MAX_RADIUS + 0.5) / 3), dict(state_bytes=sb - 1), dict(plane_bytes=3 * pix - 1),
               dict(bias=(1 << 24) + 16), dict(bias=(6 << 24) + 4), dict(planes=(2 << 24) + 16), dict(planes=(10 << 24) + 16),
               dict(state=(9 << 24) + 8), dict(state=(4 << 24) + 8), dict(ws=(9 << 24) + 8), dict(ws=(7 << 24) + 8)):
        assert _bias(lib, **kw) == BAD, kw
    assert _bias(lib, h=65536, w=1, n=1, **big) == BIG
    for kw in (dict(state=(7 << 24) + 4), dict(planes=(9 << 24) + 8), dict(bias=(10 << 24) + 2)):
        assert _bias(lib, **kw) == ALIGN, kw
    for kw in (dict(y=0), dict(state=0), dict(bias=0), dict(corrected=0), dict(n=0), dict(w=0), dict(mode=2), dict(mode=-1),
               dict(state_bytes=sb - 1), dict(corrected=(10 << 24) + 4), dict(corrected=(1 << 24) + 4), dict(bias=(6 << 24) + 4),
               dict(bias=(7 << 24) + 8), dict(corrected=(7 << 24) + 8), dict(corrected=(6 << 24) + pix - 4)):
        assert _apply(lib, **kw) == BAD, kw
    assert _apply(lib, n=65536, **big) == BIG
    # a slice's pixels are counted in int, 1024 to a workgroup: the last workgroup's first index has to fit
    edge = 2 ** 31 - 1 - 1024
    for call in (_sums, _scale, _bias, _apply):
        assert call(lib, n=1, h=1, w=edge + 1, **big) == BIG, call.__name__
    for fn in (lib.fsg_imatch_ws_bytes, lib.fsg_imatch_plane_bytes):
        assert fn(1, 1, edge) > 0 and fn(1, edge, 1) > 0 and fn(1, 1, edge + 1) == 0 and fn(1, 2, edge // 2 + 1) == 0
    for kw in (dict(y=(1 << 24) + 2), dict(bias=(10 << 24) + 1), dict(corrected=(11 << 24) + 2), dict(state=(7 << 24) + 4)):
        assert _apply(lib, **kw) == ALIGN, kw


def test_state_views_tile_the_block_in_the_headers_order():
    from fetalsyngen_amd import kernels as K

    n = 5
    st = K.imatch_state(n, "cpu", (13, 11))
    off = 0
    for name, dtype, shape in (("consts", "float64", (4,)), ("rows", "float64", (n, 5)), ("raw", "float64", (n,)), ("mean", "float64", (n,)),
                               ("scale", "float32", (n,)), ("ok", "int32", (n,)), ("frozen", "int32", (1,))):
        v = getattr(st, name)
        assert (str(v.dtype), tuple(v.shape)) == ("torch." + dtype, shape) and v.is_contiguous(), name
        assert v.data_ptr() - st.buf.data_ptr() == off, name
        off += v.numel() * v.element_size()
    assert -(-off // 8) * 8 == st.nbytes == st.buf.numel() * 8
    assert st.part.numel() * 8 == n * 32 + n * 8 and st.reserve_planes().numel() * 4 == 12 * n * 13 * 11


def test_front_ends_refuse_cpu_tensors_and_bad_arguments():
    import torch

    from fetalsyngen_amd import kernels as K
    from fetalsyngen_amd.generator.artifacts import svort

    st = K.imatch_state(3, "cpu", (13, 11))
    assert set(st.info()) == {"scale", "ok", "frozen", "raw", "rows", "mean", "consts"}
    y = torch.zeros(3, 13, 11)
    with pytest.raises(RuntimeError, match="MI355X"):
        K.imatch_sums(st, y, y.clone())
    with pytest.raises(RuntimeError, match="MI355X"):
        K.imatch_bias(st, y, y.clone(), 2.0)
    with pytest.raises(RuntimeError, match="MI355X"):
        K.imatch_apply(st, y)
    with pytest.raises(ValueError, match="follows imatch_sums"):
        K.imatch_scale(K.imatch_state(3, "cpu"))
    with pytest.raises(ValueError):
        K.imatch_state(0, "cpu")
    with pytest.raises(RuntimeError, match="MI355X"):
        svort.intensity_match(y, y.clone())
    for kw in (dict(bias_sigma=-1.0), dict(bias_sigma=float("nan")), dict(bias_sigma=K.IMATCH_MAX_RADIUS / 3 + 0.2), dict(log_floor=-0.1),
               dict(log_floor=float("inf")), dict(min_pixels=-1), dict(min_weight=-0.5)):
        with pytest.raises(ValueError):
            svort.intensity_match(y, y.clone(), **kw)
    for name in ("slices", "simulated", "weights", "sim_weight", "bias0"):
        a = dict(slices=y, simulated=y.clone(), weights=y.clone(), sim_weight=y.clone(), bias0=y.clone())
        a[name] = a[name].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match=name):
            svort.intensity_match(a.pop("slices"), a.pop("simulated"), **a)
    tr, psf = torch.zeros(3, 3, 4), torch.ones(1, 1, 1)
    with pytest.raises(ValueError, match="n_match"):
        svort.srr(tr, y, psf, (4, 4, 4), 1.0, match=dict(bias_sigma=3))
    with pytest.raises(ValueError, match="n_match"):
        svort.srr(tr, y, psf, (4, 4, 4), 1.0, n_match=-1)
    with pytest.raises(ValueError, match="unknown match option"):
        svort.srr(tr, y, psf, (4, 4, 4), 1.0, n_match=1, match=dict(sigma=3))


def test_namespace_exports():
    import importlib

    from fetalsyngen_amd import kernels as K
    from fetalsyngen_amd.generator.artifacts import svort

    module = importlib.import_module("fetalsyngen_amd.generator.artifacts.svort.intensity")
    assert svort.intensity_match is module.intensity_match
    assert module.DEFAULTS == dict(min_weight=0.5, bias_sigma=None, log_floor=0.01, min_pixels=4)
    for name in ("imatch_state", "imatch_sums", "imatch_scale", "imatch_bias", "imatch_apply", "ImatchState"):
        assert callable(getattr(K, name))
    assert svort.SRR(n_iter=3).reg == {}
    assert svort.SRR(n_iter=3, n_match=2, match=dict(bias_sigma=15)).reg == {"n_match": 2, "match": {"bias_sigma": 15}}


# ---- the launch sequence of srr ---------------------------------------------------------------------------------------------------
def _record(monkeypatch, log):
    import torch

    from fetalsyngen_amd import kernels as K

    D = (4, 4, 4)

    def fwd(tr, v, vm, sm, ps, ss, res, need_weight=False, **kw):
        log.append("fwd_w" if need_weight else "fwd")
        out = torch.zeros(tr.shape[0], *ss)
        return (out, torch.ones_like(out)) if need_weight else out

    class Ws:
        def info(self):
            return dict(rr=None, pq=None, alpha=None, beta=None, frozen=None)

    class Rb:
        n_em = 1

        def info(self):
            return dict(sigma=None, c=None, mu1=None, mu2=None, frozen=None, ws=None, u=None)

    class Im:
        scale = None

        def info(self):
            return dict(scale=None, ok=None, frozen=None, raw=None, rows=None, mean=None, consts=None)

    def apply(st, y, bias=None, bias0=None):
        log.append(("apply", bias is not None, bias0 is not None))
        return y.clone(), torch.zeros_like(y)

    monkeypatch.setattr(K, "slice_acq_forward", fwd)
    monkeypatch.setattr(K, "slice_acq_adjoint", lambda tr, ps, s, *a, **kw: (log.append("adj"), torch.zeros(D))[1])
    monkeypatch.setattr(K, "mul", lambda a, b: (log.append("mul"), a)[1])
    monkeypatch.setattr(K, "cg_workspace", lambda n, k, dev: Ws())
    monkeypatch.setattr(K, "cg_init", lambda *a, **kw: log.append("init"))
    monkeypatch.setattr(K, "cg_q", lambda *a, **kw: log.append("q"))
    monkeypatch.setattr(K, "cg_step", lambda ws, k, p, q, x, r, relu=False: log.append("step_relu" if relu else "step"))
    monkeypatch.setattr(K, "cg_dir", lambda *a, **kw: log.append("dir"))
    monkeypatch.setattr(K, "_need_gpu", lambda *a: None)
    monkeypatch.setattr(K, "robust_state", lambda n, n_em, dev, ss=None: Rb())
    monkeypatch.setattr(K, "robust_estep", lambda st, t, *a: log.append(("estep", t)))
    monkeypatch.setattr(K, "robust_update", lambda st, t, **kw: log.append(("update", t)))
    monkeypatch.setattr(K, "robust_weights", lambda st, y, *a, **kw: (log.append("weights"), torch.ones_like(y))[1])
    monkeypatch.setattr(K, "imatch_state", lambda n, dev, ss=None: Im())
    monkeypatch.setattr(K, "imatch_sums", lambda st, y, s, sm, wg, mw, om, b0: log.append(("sums", om is not None, b0 is not None)))
    monkeypatch.setattr(K, "imatch_scale", lambda st, lf, mp: log.append(("scale", lf)))
    monkeypatch.setattr(K, "imatch_bias", lambda st, y, s, sigma, *a: (log.append(("bias", sigma)), torch.zeros_like(y))[1])
    monkeypatch.setattr(K, "imatch_apply", apply)


def _solve(n_iter, relu_last, weighted=False):
    it = ["fwd"] + (["mul"] if weighted else []) + ["adj", "q", "step_relu" if relu_last else "step", "dir"]
    return (["mul"] if weighted else []) + ["adj", "init"] + it * n_iter


def _srr(**kw):
    import torch

    from fetalsyngen_amd.generator.artifacts import svort

    return svort.srr(torch.zeros(3, 3, 4), torch.zeros(3, 1, 5, 7), torch.ones(1, 1, 1), (4, 4, 4), 1.0, n_iter=2, return_info=True, **kw)


def test_srr_without_matching_rounds_issues_the_parents_launch_sequence(monkeypatch):
    log = []
    _record(monkeypatch, log)
    out, info = _srr()
    assert log == _solve(2, True)
    assert set(info) == {"rr", "pq", "alpha", "beta", "frozen"} and tuple(out.shape) == (1, 1, 4, 4, 4)
    del log[:]
    out, info = _srr(n_robust=1, robust=dict(n_em=1))
    em = ["fwd_w", ("estep", 0), ("update", 0), ("estep", 1), ("update", 1), "weights"]
    assert log == _solve(2, False) + em + _solve(2, True, weighted=True)
    assert set(info) == {"rr", "pq", "alpha", "beta", "frozen", "robust"}


def test_srr_launch_sequence_with_matching_rounds(monkeypatch):
    log = []
    _record(monkeypatch, log)
    out, info = _srr(n_match=2, match=dict(bias_sigma=3.0, log_floor=0.02))
    first = ["fwd_w", ("sums", False, False), ("scale", 0.02), ("bias", 3.0), ("apply", True, False)]
    second = ["fwd_w", ("sums", False, True), ("scale", 0.02), ("bias", 3.0), ("apply", True, True)]  # the bias is carried
    assert log == _solve(2, False) + first + _solve(2, False) + second + _solve(2, True)
    assert set(info) == {"rr", "pq", "alpha", "beta", "frozen", "match", "match_bias"} and len(info["match"]) == 2
    assert set(info["match"][0]) == {"scale", "ok", "frozen"} and tuple(info["match_bias"].shape) == (3, 5, 7)
    del log[:]
    out, info = _srr(n_match=1, n_robust=2, robust=dict(n_em=1))  # scale only, under the round's robust weights
    em = [("estep", 0), ("update", 0), ("estep", 1), ("update", 1), "weights"]
    match = [("sums", True, False), ("scale", 0.01), ("apply", False, False)]
    assert log == (_solve(2, False) + ["fwd_w"] + em + match + _solve(2, False, weighted=True) + ["fwd_w"] + em
                   + _solve(2, True, weighted=True))
    assert len(info["robust"]) == 2 and len(info["match"]) == 1
