"""CPU restatement of the slice intensity matching of `svort.intensity_match` (the rule is in
include/fsg_hip.h, fsg_imatch_*).  Test infrastructure, numpy only.

    pixels(...)      c = exp(-bias0) * y, omega and Omega, the pixels that take part
    rows(...)        the five per-slice sums: in float64, or from fp32 terms in the device's order (util_robust64.rows_device)
    scale(...)       the scalar pass: R, floor, raw, the gauge g, scale, ok, frozen; double arithmetic as the device's
    bias(...)        Omega_b, P and Q, the row pass and the column pass (taps -Rr..Rr increasing, one fma each, taps outside the
                     slice skipped), inc, b1, the means (fp32: the column pass's tiles, threads, shuffle tree), bias
    match(...)       the whole call.  ft = float64: every pixel operation in float64, scale not rounded; ft = float32: pixel
                     operations in float32 one rounding each (fmaf through one float64 product and sum), the sums in the
                     device's order, scale and the mean rounded to float32: what the device computes, expf and logf apart.

Margins: membership of Omega_b is a jump at d = floor and s = floor, so a comparison between two arithmetics needs every d and s
of Omega away from the floor.  match() records the smallest relative distance (`margin`); `assert_margin` demands 1e-3.

E_CPU: max |match(float32) - match(float64)| relative to max |float64|, per group (rows, scale, bias, corrected) over CASES;
CAP32_RMS_DIFF the same for the capability RMS.  Measured on the CPU (python -m tests.util_imatch64 prints them and the
capability table of DESIGN.md section 28), written below rounded up in the third digit with the measured value beside each.

The capability case: section 25's geometry (util_robust64.capability_case: 42 slices of 13 x 11 in three orthogonal stacks) with
its clean slices, slice k multiplied by exp(0.25 z_k) and by exp(b_k), b_k = 0.3 (p u + q v + r u v) over u, v in [-1, 1] along the
two slice axes, z normal and p, q, r uniform in [-1, 1] from default_rng(11).  Solves: lam = 0.1, 6 CG iterations from 0.
"""
import math

import numpy as np

from tests import util_robust64 as RB
from tests import util_srr64 as SR
from tests import util_tk1_64 as TK

F32, F64 = np.float32, np.float64
TH, TW, TROWS, WAVE = 64, 32, 8, 64  # the column pass's tile, its thread rows, the wave
MAX_RADIUS = 48
FLT_MIN = float(np.finfo(F32).tiny)
DEFAULTS = dict(min_weight=0.5, log_floor=0.01, min_pixels=4)
MARGIN = 1e-3


def _fl(x, ft):
    return np.asarray(x).astype(ft)


# ---- the pixel pass --------------------------------------------------------------------------------------------------------------
def pixels(y, s, mask=None, sim_weight=None, min_weight=0.5, weights=None, bias0=None, ft=F64):
    """-> y, s, c, omega (ft) and Omega (bool), all (n,h,w)"""
    y32, s32 = np.asarray(y, F32), np.asarray(s, F32)  # the device's inputs are fp32 whatever the arithmetic after
    with np.errstate(all="ignore"):
        yy, ss = y32.astype(ft), s32.astype(ft)
        c = yy if bias0 is None else _fl(_fl(np.exp(-np.asarray(bias0, F32).astype(ft)), ft) * yy, ft)
        part = np.isfinite(y32) & np.isfinite(s32) & np.isfinite(c.astype(F32))
        if mask is not None:
            part &= np.asarray(mask, bool).reshape(yy.shape)
        if sim_weight is not None:
            sw = np.asarray(sim_weight, F32)
            part &= (sw > 0) & (sw >= F32(min_weight))
        om = np.ones_like(yy)
        if weights is not None:
            pw = np.asarray(weights, F32)
            part &= (pw > 0) & np.isfinite(pw)
            om = pw.astype(ft)
    return yy, ss, c, om, part


def rows(yy, ss, c, om, part, ft=F64):
    """(n,5): N, A = sum omega c s, B = sum omega c c, min y, max y"""
    with np.errstate(all="ignore"):
        t = _fl(om * c, ft)
        terms = np.stack([np.ones_like(c), _fl(t * ss, ft), _fl(t * c, ft), np.zeros_like(c)], -1)
    terms = np.where(part[..., None], terms, ft(0)).astype(ft)
    r = RB.rows_device(terms, yy, part) if ft is F32 else RB.rows64(terms, yy, part)
    return r[:, [0, 1, 2, 4, 5]]


# ---- the scalar pass -------------------------------------------------------------------------------------------------------------
def scale(r, log_floor=0.01, min_pixels=4, single=True, mutant=None):
    """single: scale rounded to float32 (the device); False: kept in double (the float64 reference).  mutant: one of
    util_robust64.ORDER_MUTANTS, the slices the sums over the slices visit and their order (util_robust64.slice_order)."""
    r = np.asarray(r, F64).copy()
    n = r.shape[0]
    bad = ~(np.isfinite(r[:, 1]) & np.isfinite(r[:, 2]))
    r[bad, 1:3] = 0.0
    N, A, B = r[:, 0], r[:, 1], r[:, 2]
    own = (N >= min_pixels) & (N > 0) & ~bad & (A > 0) & (B > 0)
    with np.errstate(all="ignore"):
        q = A / np.where(own, B, 1.0)
    own &= np.isfinite(q)
    raw = np.where(own, q, 0.0)
    order = RB.slice_order(n, mutant)
    have = np.zeros(n, bool)
    have[order] = True
    have &= N > 0
    R = (r[have, 4].max() - r[have, 3].min()) if have.any() else math.nan
    floor = log_floor * R
    tot = nok = 0.0
    for k in (j for j in order if own[j]):
        tot, nok = tot + raw[k], nok + 1.0
    g = tot / nok if nok else math.nan
    frozen = not (math.isfinite(R) and R > 0 and math.isfinite(floor) and nok > 0 and math.isfinite(g) and g > 0)
    sc = np.ones(n)
    if not frozen:
        with np.errstate(all="ignore"):
            q = np.where(own, raw / g, 1.0)
            sc = q.astype(F32).astype(F64) if single else q
        frozen = bool((~(np.isfinite(sc) & (sc > 0)))[own].any())
    if frozen:
        return dict(rows=r, raw=raw, scale=np.ones(n), ok=np.zeros(n, bool), frozen=1, consts=np.zeros(4), mean=np.zeros(n))
    return dict(rows=r, raw=raw, scale=sc, ok=own, frozen=0, consts=np.array([R, floor, g, nok]), mean=np.zeros(n))


# ---- the bias field --------------------------------------------------------------------------------------------------------------
def taps(sigma):
    Rr = int(math.ceil(3.0 * sigma))
    return Rr, np.array([math.exp(-(t * t) / (2.0 * sigma * sigma)) for t in range(Rr + 1)], F64).astype(F32)


def _fma(a, b, c, ft):
    # fp32: the product of two floats is exact in double, the sum is rounded once in double and once to float
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(ft)


def blur(plane, g, Rr, axis, ft):
    """taps t = -Rr..Rr in increasing t from +0, one fma per tap, taps outside the slice skipped"""
    acc = np.zeros(plane.shape, ft)
    L = plane.shape[axis]
    for t in range(-Rr, Rr + 1):
        lo, hi = max(0, -t), min(L, L - t)  # the pixels j with 0 <= j + t < L
        if lo >= hi:
            continue
        dst, src = [slice(None)] * plane.ndim, [slice(None)] * plane.ndim
        dst[axis], src[axis] = slice(lo, hi), slice(lo + t, hi + t)
        dst, src = tuple(dst), tuple(src)
        acc[dst] = _fma(np.full((), g[abs(t)], ft), plane[src], acc[dst], ft)
    return acc


def means_device(term, om, inb):
    """sum of fp32 `term` and `om` over Omega_b in the column pass's order: a thread's rows, the shuffle tree, waves, tiles"""
    n, h, w = term.shape
    ty, tx = -(-h // TH), -(-w // TW)
    pad = np.zeros((2, n, ty * TH, tx * TW), F32)
    pad[0, :, :h, :w] = np.where(inb, term, 0)
    pad[1, :, :h, :w] = np.where(inb, om, 0)
    v = pad.reshape(2, n, ty, TH // TROWS, TROWS, tx, TW).transpose(0, 1, 2, 5, 3, 4, 6)  # [.., tile_y, tile_x, m, ly, lx]
    acc = np.zeros(v.shape[:4] + (TROWS, TW), F32)
    for m in range(TH // TROWS):
        acc = acc + v[:, :, :, :, m]
    lanes = acc.reshape(2, n, ty, tx, TROWS * TW // WAVE, WAVE)
    idx = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[..., np.where(idx + o < WAVE, idx + o, idx)]
    red = lanes[..., 0]
    part = red[..., 0]
    for q in range(1, red.shape[-1]):
        part = part + red[..., q]
    part = part.reshape(2, n, ty * tx)
    out = np.zeros((2, n))
    for b in range(ty * tx):
        out = out + part[:, :, b].astype(F64)
    return out[0], out[1]


def bias(S, ss, c, om, part, sigma, bias0=None, ft=F64, weighted=True):
    """S: scale()'s dict.  -> b1, bias, mean, Omega_b, margin"""
    Rr, g = taps(sigma)
    floor = ft(S["consts"][1])
    sc = S["scale"].astype(ft)[:, None, None]
    with np.errstate(all="ignore"):
        d = _fl(sc * c, ft)
        cand = part & S["ok"][:, None, None]
        inb = cand & (d > floor) & (ss > floor)
        r = _fl(np.log(_fl(d / np.where(inb, ss, 1), ft)), ft)
        inb &= np.isfinite(r)
        fl64 = float(S["consts"][1])
        dist = np.minimum(np.abs(d.astype(F64) - fl64), np.abs(ss.astype(F64) - fl64))[cand]
        margin = float(dist.min() / fl64) if dist.size and fl64 > 0 else math.inf
        P = np.where(inb, _fl(om * r, ft) if weighted else r, ft(0)).astype(ft)
        Q = np.where(inb, om, ft(0)).astype(ft)
        P2 = blur(blur(P, g, Rr, 2, ft), g, Rr, 1, ft)
        Q2 = blur(blur(Q, g, Rr, 2, ft), g, Rr, 1, ft)
        inc = np.where(Q2 >= FLT_MIN, _fl(P2 / np.where(Q2 >= FLT_MIN, Q2, 1), ft), ft(0)).astype(ft)
        b1 = inc if bias0 is None else _fl(np.asarray(bias0, F32).astype(ft) + inc, ft)
        term = _fl(om * b1, ft)
        if ft is F32:
            num, den = means_device(term, om, inb)
        else:
            num, den = np.where(inb, term, 0).sum((1, 2)), np.where(inb, om, 0).sum((1, 2))
        mean = np.where(S["ok"] & (den > 0), num / np.where(den > 0, den, 1.0), 0.0)
        m = mean.astype(F32).astype(ft) if ft is F32 else mean
        out = np.where(S["ok"][:, None, None], _fl(b1 - m[:, None, None], ft), b1).astype(ft)
    return dict(b1=b1, bias=out, mean=mean, inb=inb, margin=margin, inc=inc)


def match(y, s, mask=None, sim_weight=None, min_weight=0.5, weights=None, bias0=None, sigma=0.0, log_floor=0.01, min_pixels=4,
          ft=F64):
    """-> dict: corrected, scale, bias (ft), rows, raw, ok, frozen, consts, mean, part, inb, margin"""
    yy, ss, c, om, part = pixels(y, s, mask, sim_weight, min_weight, weights, bias0, ft)
    S = scale(rows(yy, ss, c, om, part, ft), log_floor, min_pixels, single=ft is F32)
    S.update(part=part, inb=np.zeros(part.shape, bool), margin=math.inf)
    if sigma > 0:
        B = bias(S, ss, c, om, part, sigma, bias0, ft, weighted=weights is not None)
        S.update(bias=B["bias"], mean=B["mean"], inb=B["inb"], margin=B["margin"], inc=B["inc"])
    else:
        S["bias"] = np.zeros(yy.shape, ft) if bias0 is None else np.asarray(bias0, F32).astype(ft)
    with np.errstate(all="ignore"):
        S["corrected"] = _fl(S["scale"].astype(ft)[:, None, None] * _fl(_fl(np.exp(-S["bias"]), ft) * yy, ft), ft)
    return S


def assert_margin(S):
    assert S["margin"] >= MARGIN, f"a pixel lies {S['margin']:.2e} of the floor from the floor"


# ---- synthetic comparison cases --------------------------------------------------------------------------------------------------
CASES = {  # name: (n, h, w, seed, sigma, with bias0)
    "n5_37x29": (5, 37, 29, 41, 2.0, False),  # scalar loads
    "n5_36x32": (5, 36, 32, 42, 2.0, True),  # h * w a multiple of 4: the 16-byte loads
    "n3_5x7": (3, 5, 7, 43, 4.0, False),  # radius 12, above both extents
    "n5_37x29_r1": (5, 37, 29, 44, 0.3, True),  # radius 1
    "n1_1x1": (1, 1, 1, 45, 2.0, False),  # one pixel: R == 0, the matching freezes
    "n2_65x257": (2, 65, 257, 46, 2.0, False),  # one pixel more than the column tile, and than the row pass's 256; radius 6
    "n5_37x29_scale": (5, 37, 29, 47, 0.0, True),  # scale only
    # the largest radius, 48: three column tiles (rows 0..63, 64..127, 128..130), the middle one with slice data in both halos,
    # and the tap windows of rows 80..111 cross both borders; the row pass fills its 33 + 96 halo entries over zeros on both sides
    "n2_131x33_r48": (2, 131, 33, 48, 16.0, True),
    # radius 48 along the row: three row-pass workgroups (columns 0..255, 256..511, 512..599), the middle one with slice data in
    # both halos, its 352 LDS entries filled in two trips; 19 column tiles across
    "n2_14x600_r48": (2, 14, 600, 49, 16.0, False),
    "n2_131x33_r33": (2, 131, 33, 50, 11.0, False),  # radius 33: the smallest whose window spans a whole tile and both borders
}
_CASES = {}


def case(name):
    """s a smooth field in [0.6, 2]; y = s * exp(field_k) / gain_k + noise, field_k a smooth ramp, gain_k in [0.7, 1.4]; a
    background corner (6 x 6, or the first row of the small slices) where s and y are 1e-3: counted for the scale, under the floor
    for the bias; 10 % of the pixels masked, sim weights in (0.3, 1.2) with zeros and a NaN, robust weights in (0.2, 1] with
    zeros; one NaN and one Inf pixel in y and one NaN in s."""
    if name in _CASES:
        return _CASES[name]
    n, h, w, seed, sigma, with_b0 = CASES[name]
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=F64), np.arange(w, dtype=F64), indexing="ij")
    s = np.stack([1.3 + 0.7 * np.sin(yy / (3.0 + k) + k) * np.cos(xx / (4.0 + 0.5 * k)) for k in range(n)])
    u, v = (yy / max(h - 1, 1)) * 2 - 1, (xx / max(w - 1, 1)) * 2 - 1
    field = np.stack([0.25 * (rng.uniform(-1, 1) * u + rng.uniform(-1, 1) * v + rng.uniform(-1, 1) * u * v) for _ in range(n)])
    gain = rng.uniform(0.7, 1.4, n)
    y = s * np.exp(field) / gain[:, None, None] + 0.01 * rng.standard_normal(s.shape)
    if h * w > 1:
        bh, bw = (6, 6) if h >= 13 else (1, w)
        s[:, :bh, :bw], y[:, :bh, :bw] = 1e-3, 1e-3 * rng.uniform(0.5, 1.5, (n, bh, bw))
    y, s = y.astype(F32), s.astype(F32)
    mask = sw = pw = b0 = None
    if h * w > 1:
        mask = rng.random(s.shape) < 0.9
        sw = rng.uniform(0.3, 1.2, s.shape).astype(F32)
        sw[rng.random(s.shape) < 0.05] = 0
        pw = rng.uniform(0.2, 1.0, s.shape).astype(F32)
        pw[rng.random(s.shape) < 0.05] = 0
        sw[0, h - 1, 1] = np.nan
        y[0, h - 1, 3], y[n - 1, h - 2, 1], s[0, h - 2, 4] = np.nan, np.inf, np.nan
    if with_b0:
        b0 = (0.1 * np.stack([rng.uniform(-1, 1) * u + rng.uniform(-1, 1) * v for _ in range(n)])).astype(F32)
    _CASES[name] = dict(y=y, s=s, mask=mask, sw=sw, pw=pw, b0=b0, sigma=sigma)
    return _CASES[name]


def run_case(name, ft=F64, **kw):
    c = case(name)
    a = dict(mask=c["mask"], sim_weight=c["sw"], weights=c["pw"], bias0=c["b0"], sigma=c["sigma"])
    a.update(kw)
    return match(c["y"], c["s"], ft=ft, **a)


def _rel(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    keep = np.isfinite(b)
    if not keep.any():
        return 0.0
    return float(np.abs(a[keep] - b[keep]).max() / max(np.abs(b[keep]).max(), 1e-300))


def compare(got, want):
    """relative differences per group between two match() results (or a device result in the same keys)"""
    assert np.array_equal(np.isfinite(np.asarray(got["corrected"], F64)), np.isfinite(np.asarray(want["corrected"], F64)))
    return dict(rows=_rel(np.asarray(got["rows"])[:, 1:3], np.asarray(want["rows"])[:, 1:3]),
                scale=max(_rel(got["scale"], want["scale"]), _rel(got["raw"], want["raw"]), _rel(got["consts"], want["consts"])),
                bias=max(_rel(got["bias"], want["bias"]), _rel(got["mean"], want["mean"])),
                corrected=_rel(got["corrected"], want["corrected"]))


GROUPS = ("rows", "scale", "bias", "corrected")
# group: bound, measured beside it (max over CASES)
E_CPU = {
    "rows": 6.45e-08,  # 6.448e-08
    "scale": 1.26e-07,  # 1.256e-07
    "bias": 2.71e-06,  # 2.702e-06
    "corrected": 2.99e-07,  # 2.982e-07
}

# the groups in which a size case of tests/util_recon_counts.py (three slices, scale only) exceeds the figure above, measured by
# the same procedure (util_recon_counts.measure_size_e_cpu); the tests of those cases use the larger of the two, times 4
E_CPU_SIZES = {
    "rows": 1.23e-07,  # 1.224e-07, set by imatch_size_case((2, 513)): 1026 pixels, the second chunk holds two
    "scale": 2.62e-07,  # 2.614e-07, set by imatch_size_case((2, 513))
}
# the same for the one case of 257 slices of 5 x 7 with the bias field (util_recon_counts.imatch_means_case, sigma 4)
E_CPU_N257 = {
    "scale": 1.53e-07,  # 1.524e-07, set by imatch_means_case(): the gauge is a sum of 255 gains
}


def measure_e_cpu():
    worst = dict.fromkeys(GROUPS, 0.0)
    for name in CASES:
        a, b = run_case(name, F32), run_case(name, F64)
        assert_margin(b)
        assert a["frozen"] == b["frozen"] and np.array_equal(a["ok"], b["ok"]) and np.array_equal(a["inb"], b["inb"])
        for g, v in compare(a, b).items():
            worst[g] = max(worst[g], v)
    return worst


# ---- the capability case ---------------------------------------------------------------------------------------------------------
CAP_SIGMA, CAP_ROUNDS, CAP_SEED = 4.0, 3, 11
_CAP = {}


def capability_case():
    if _CAP:
        return _CAP
    c = RB.capability_case()
    n, (h, w) = c["y_clean"].shape[0], c["ss"]
    rng = np.random.default_rng(CAP_SEED)
    gain = np.exp(0.25 * rng.standard_normal(n))
    yy, xx = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing="ij")
    co = rng.uniform(-1, 1, (n, 3))
    field = 0.3 * (co[:, 0, None, None] * yy + co[:, 1, None, None] * xx + co[:, 2, None, None] * yy * xx)
    factor = gain[:, None, None] * np.exp(field)
    clean = c["y_clean"].astype(F64)
    g = gain.mean()  # the oracle under the rule's gauge: what remains is one common gain, the volume's
    _CAP.update(base=c, clean=c["y_clean"], y=(clean * factor).astype(F32), oracle=((clean * factor).astype(F32) / (factor / g)).astype(F32),
                gain=gain, field=field)
    return _CAP


def cap_run(n_match, sigma=CAP_SIGMA, ft=F64):
    """srr(lam, 6 iterations, n_match=, match=dict(bias_sigma=sigma)) restated -> (rms against the phantom, x, last match)"""
    C = capability_case()
    c = C["base"]
    y, b, S = C["y"], None, None
    for rb in range(n_match + 1):
        x = RB.cap_solve(c, y, None, relu=rb == n_match, ft=ft)
        if rb < n_match:
            s, wgt = SR.forward(c["tr"], x, c["psf"], None, c["ss"], c["res"], False, ft)
            S = match(C["y"], s.astype(F32), None, wgt.astype(F32), bias0=b, sigma=sigma, ft=ft)
            y, b = S["corrected"].astype(F32), S["bias"].astype(F32)
    return TK.rms(x, c["vol"]), x, S


def cap_table():
    C = capability_case()
    c = C["base"]
    out = dict(clean=TK.rms(RB.cap_solve(c, C["clean"]), c["vol"]), corrupted=cap_run(0)[0],
               oracle=TK.rms(RB.cap_solve(c, C["oracle"]), c["vol"]))
    for r in range(1, CAP_ROUNDS + 1):
        out[f"matched_{r}"] = cap_run(r)[0]
    out["scale_only_3"] = cap_run(CAP_ROUNDS, sigma=0.0)[0]
    return out


# float64 RMS against the phantom: rounded up in the third digit, measured beside it
CAP_RMS = {
    "clean": 0.0275,  # 0.027404
    "corrupted": 0.130,  # 0.129554
    "oracle": 0.0273,  # 0.027210
    "matched_1": 0.0701,  # 0.070045
    "matched_2": 0.0619,  # 0.061831
    "matched_3": 0.0637,  # 0.063663
    "scale_only_3": 0.0719,  # 0.071806
}
CAP32_RMS_DIFF = 1.30e-07  # 1.297e-07: |RMS(float32 restatement) - RMS(float64)| / RMS(float64), three rounds, sigma 4


if __name__ == "__main__":
    for g, v in measure_e_cpu().items():
        print("E_CPU", g, f"{v:.3e}")
    for name in CASES:
        b = run_case(name)
        print(name, "margin", f"{b['margin']:.3e}", "frozen", b["frozen"], "scale", np.round(b["scale"], 4), "Omega_b", int(b["inb"].sum()),
              "of", int(b["part"].sum()))
    for k, v in cap_table().items():
        print("capability", k, f"{v:.6f}")
    r32, r64 = cap_run(CAP_ROUNDS, ft=F32), cap_run(CAP_ROUNDS)
    print("capability fp32", r32[0], "float64", r64[0], "diff", abs(r32[0] - r64[0]) / r64[0])
