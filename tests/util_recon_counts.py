"""Inputs, comparisons and mutants for the reconstruction units at slice counts past a wave (64) and a workgroup (256) and at
the slice sizes where the streaming passes change path.  Test infrastructure, numpy only; the
restatements are tests/util_robust64.py, util_imatch64.py, util_svr64.py and util_svr_group64.py.

    COUNTS                     the slice counts every unit is run at
    robust_case(n)             n slices of 5 x 7, every slice with its own seeded scale, offset and noise level, five classes of
                               slice (clean, 3 or 8 outlier pixels, two depths of corruption), slices that take no part in the
                               first trip, in the last trip and at index 256
    robust_freeze_case()       n = 300, one residual in slice 270 whose square leaves fp32: S2 is not finite, the run freezes
    imatch_case(n)             the same for the intensity matching; imatch_bad_case(): slice 270's scale leaves fp32
    tiled(case, n)             a 5-slice case repeated to n slices
    SIZES, robust_size_case / imatch_size_case   three slices of every size at which the streaming passes change path
    robust_fields / imatch_fields / differing    what point 1 compares bit for bit, and the names of the fields that differ
    ws_check                   the slice weights of a slot: exact on the early-out branches, WS_BOUND on the quotient
    svr_update_run, compose_mutant               util_svr64.update over every slot, and the workgroup mutants of the per-slice kernels
    robust_point1, imatch_point1                 point 1's comparison between the true restatement and a mutant of it

Margins: the seeds below are chosen on the CPU so that the float64 run of every case keeps util_robust64's and
util_imatch64's margin (`python -m tests.util_recon_counts` searches them and prints the E_cpu of the new size cases).
"""
import math

import numpy as np

from tests import util_imatch64 as IM
from tests import util_robust64 as RB
from tests import util_svr64 as SV
from tests import util_svr_group64 as GU

F32, F64 = np.float32, np.float64
COUNTS = (63, 64, 65, 128, 129, 255, 256, 257, 300)
H, W = 5, 7
N_EM = 3
LATE = 270  # the slice of the two n = 300 cases that alone meets the condition: trip 4 of the wave walk, second thread stride
# |ws(device) - ws(restatement)| on the quotient branch.  w = g1 / (g1 + g2), g_i = exp(a_i) / sqrt(2 pi v_i) * mix_i; the
# arguments a_i and every other operand are bit-equal on both sides.  exp in double is documented to 1 ulp on the device (the
# HIP math API's table of double-precision functions) and to 1 ulp in the C library numpy calls, so the two exponentials differ
# by at most 2 ulp = 4 u relative, u = 2^-53.  Two values that differ by eps relative differ by at most eps + 2 u after one more
# correctly rounded operation (each side rounds once): 6 u after the division by the root, 8 u after the product with the
# mixing weight; the sum of two positive terms 8 u + 2 u = 10 u; the quotient 8 u + 10 u + 2 u = 20 u, and w <= 1.
WS_BOUND = 20 * 2.0 ** -53


def not_ok_slices(n):
    """slices with fewer than min_pixels pixels: one in the first trip, the last slice (the ragged last trip) and index 256.
    At n = 65, 129 and 257 the last slice is the whole ragged trip, so it also holds the largest y of the batch: the range R
    is then the figure through which a dropped trip shows."""
    return sorted({7, n - 1} | ({256} if n > 256 else set()))


def _field():
    yy, xx = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
    return 1.0 + 0.5 * np.sin(yy / 2.0) * np.cos(xx / 3.0)


def _few_pixels_mask(n):
    mask = np.ones((n, H, W), bool)
    for k in not_ok_slices(n):
        mask[k] = False
        mask[k, 0, :3] = True  # three pixels: under min_pixels = 4
    return mask


# ---- robust ------------------------------------------------------------------------------------------------------------------
OUTLIER_PIXELS = (0, 3, 18, 30, 8)  # per class of slice; u is about sqrt(count / 35)
RB_SEEDS = {63: 1063, 64: 3064, 65: 1065, 128: 1128, 129: 1129, 255: 6255, 256: 1256, 257: 1257, 300: 7300}
_RB = {}


def _robust_case(n, seed):
    rng = np.random.default_rng(seed)
    scale, offset, level = rng.uniform(0.6, 1.6, n), rng.uniform(-0.3, 0.3, n), rng.uniform(0.01, 0.03, n)
    s = scale[:, None, None] * _field() + offset[:, None, None]
    y = s + rng.standard_normal(s.shape) * level[:, None, None]
    cls = np.zeros(n, int)
    idx = rng.permutation(n)
    nb, nc, nd = n // 3, max(n // 10, 2), max(n // 20, 1)  # a third with a few outlier pixels, a tenth corrupted
    cls[idx[:nb]] = 1
    cls[idx[nb:nb + nc]] = 2 + (np.arange(nc) % 2)
    cls[idx[nb + nc:nb + nc + nd]] = 4
    for k in range(n):
        for i in rng.permutation(H * W)[:OUTLIER_PIXELS[cls[k]]]:
            y[k, i // W, i % W] += rng.choice([-1.0, 1.0]) * rng.uniform(0.8, 1.2)
    y[n - 1, 0, :3] = s[n - 1, 0, :3] + 3.0  # the last slice is not ok and holds max y: a walk that drops it changes R
    return dict(y=y.astype(F32), s=s.astype(F32), mask=_few_pixels_mask(n), sw=None, cls=cls)


def robust_case(n):
    if n not in _RB:
        _RB[n] = _robust_case(n, RB_SEEDS[n])
    return _RB[n]


def robust_em(c, ft=F64, mutant=None, n_em=N_EM):
    return RB.em(c["y"], c["s"], c["mask"], c["sw"], n_em=n_em, ft=ft, mutant=mutant)


def robust_freeze_case():
    """robust_case(300) with one pixel of slice LATE at 1e30: e is finite, e * e is not in fp32, so the slice's sum p e^2 is
    Inf at slot 0, S2 is not finite and the run freezes; every other slice alone would not freeze it"""
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in robust_case(300).items()}
    c["y"][LATE, 2, 3] = F32(1e30)
    return c


def robust_fields(S, t, scal=None):
    """the figures of slot t that are built from + - * /, sqrt and fmax in double: a device state (host arrays by name, scal
    the two floats) or a restatement's dict"""
    kf, vf = (S["kappa"], S["inv2var"]) if scal is None else scal
    return dict(u=np.asarray(S["u"], F64), consts=np.asarray(S["consts"], F64), sigma=F64(S["sigma"][t]), c=F64(S["c"][t]),
                mu1=F64(S["mu1"][t]), mu2=F64(S["mu2"][t]), frozen=np.int32(S["frozen"][t]), scal=np.array([kf, vf], F32))


def differing(a, b):
    """names of the fields of two dicts of arrays whose bits differ"""
    out = []
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            out.append(k)
    return out


def ws_check(got, S, t, min_pixels=4):
    """the slice weights `got` of slot t against the restatement S after update(S, t, ...): exactly 0 for a slice that is not
    ok, exactly 1 / 0 on the two early-out branches (and 1 for every ok slice at slot 0 and in a frozen slot), within WS_BOUND
    on the quotient branch.  -> (number of slices on the quotient branch, largest difference there)"""
    got, want = np.asarray(got, F64), S["ws"][t]
    N, u = S["rows"][:, 0], S["u"]
    ok = (N >= min_pixels) & (N > 0)
    exact = ~ok
    if t == 0 or S["frozen"][t]:
        exact = np.ones_like(ok)
    else:
        exact = exact | (u < S["mu1"][t]) | (u > S["mu2"][t])
    assert np.array_equal(got[exact], want[exact]) and set(np.unique(want[exact])) <= {0.0, 1.0}
    assert not got[~ok].any()
    d = np.abs(got[~exact] - want[~exact])
    worst = float(d.max()) if d.size else 0.0
    assert worst <= WS_BOUND, worst
    return int((~exact).sum()), worst


def robust_rows32(c, kappa=0.0, inv2var=0.0, first=True):
    """a slot's rows from fp32 terms in the device's order, as the estep leaves them"""
    yy, e, part = RB.pixels(c["y"], c["s"], c["mask"], c["sw"], 0.5, F32)
    tm, _ = RB.terms(e, part, kappa, inv2var, first, F32)
    return RB.rows_device(tm, yy, part)


def robust_point1(c, mutant, n_em=N_EM):
    """Point 1's comparison with the true restatement in the device's place and a mutant of it in the restatement's: slot by
    slot the mutant is given the rows, ws[t-1], frozen[t-1] and consts of the true run -> the set of fields whose bits differ
    in some slot, with "ws" where ws_check fails.  Empty for mutant None."""
    n = c["y"].shape[0]
    A, B, out = RB.new_state(n, n_em), RB.new_state(n, n_em), set()
    for t in range(n_em + 1):
        rows = robust_rows32(c, A["kappa"], A["inv2var"], t == 0)
        RB.update(A, t, rows)
        if t > 0:
            B["ws"][t - 1], B["frozen"][t - 1], B["consts"] = A["ws"][t - 1], A["frozen"][t - 1], A["consts"].copy()
        RB.update(B, t, rows, mutant=mutant)
        out |= set(differing(robust_fields(A, t), robust_fields(B, t)))
        try:
            ws_check(A["ws"][t], B, t)
        except AssertionError:
            out.add("ws")
    return out, A


# ---- imatch ------------------------------------------------------------------------------------------------------------------
_IMC = {}


# chosen so that the gauge's sum over the slices is sensitive to its order: adding the gains in decreasing index gives other bits
IM_SEEDS = {63: 8063, 64: 7064, 65: 7065, 128: 7128, 129: 7129, 255: 7255, 256: 7256, 257: 7257, 300: 7300}


def imatch_case(n, seed=None):
    """s = scale_k * field + offset_k in [0.45, 2.7], y = s / gain_k + noise; robust weights in (0.2, 1] with zeros; the slices
    of not_ok_slices(n) keep three pixels"""
    if n not in _IMC:
        rng = np.random.default_rng(IM_SEEDS[n] if seed is None else seed)
        scale, offset, gain = rng.uniform(0.6, 1.6, n), rng.uniform(0.15, 0.3, n), rng.uniform(0.7, 1.4, n)
        s = scale[:, None, None] * _field() + offset[:, None, None]
        y = s / gain[:, None, None] + 0.01 * rng.standard_normal(s.shape)
        pw = rng.uniform(0.2, 1.0, s.shape).astype(F32)
        pw[rng.random(s.shape) < 0.05] = 0
        pw[n - 1, 0, :3] = 1
        y[n - 1, 0, :3] = 6.0  # the last slice is not ok and holds max y: a walk that drops it changes R
        c = dict(y=y.astype(F32), s=s.astype(F32), mask=_few_pixels_mask(n), sw=None, pw=pw, b0=None)
        if seed is not None:
            return c
        _IMC[n] = c
    return _IMC[n]


def imatch_bad_case():
    """imatch_case(300) with slice LATE at y = 1e18, s = 1e-30: A = sum y s and B = sum y y are finite and positive in fp32,
    raw = A / B is about 1e-48, and (float)(raw / g) is 0: the scale leaves fp32 and the matching freezes"""
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in imatch_case(300).items()}
    c["y"][LATE], c["s"][LATE] = F32(1e18), F32(1e-30)
    c["pw"][LATE] = 1
    return c


MEANS_SIGMA = 4.0  # radius 12, above both extents of a 5 x 7 slice


def imatch_means_case():
    """imatch_case(257) with slice 256 given back its pixels, so that the one slice of im_means_kernel's second workgroup has
    a mean"""
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in imatch_case(257).items()}
    c["mask"][256] = True
    return c


def imatch_run(c, ft=F64, sigma=0.0):
    return IM.match(c["y"], c["s"], c["mask"], c["sw"], weights=c["pw"], bias0=c["b0"], sigma=sigma, ft=ft)


def imatch_fields(S):
    """what the scalar pass leaves, from a device state (host arrays by name) or scale()'s dict"""
    return dict(raw=np.asarray(S["raw"], F64), ok=np.asarray(S["ok"]).astype(np.int32), consts=np.asarray(S["consts"], F64),
                frozen=np.int32(np.asarray(S["frozen"]).reshape(-1)[0]), scale=np.asarray(S["scale"]).astype(F32),
                mean=np.asarray(S["mean"], F64))


def imatch_rows32(c):
    yy, ss, cc, om, part = IM.pixels(c["y"], c["s"], c["mask"], c["sw"], 0.5, c["pw"], c["b0"], F32)
    return IM.rows(yy, ss, cc, om, part, F32)


def imatch_point1(c, mutant):
    """point 1's comparison for im_scale_kernel between the true scalar pass and a mutant -> (fields that differ, the true pass)"""
    rows = imatch_rows32(c)
    A = IM.scale(rows)
    return set(differing(imatch_fields(A), imatch_fields(IM.scale(rows, mutant=mutant)))), A


def tiled(c, n):
    """the arrays of a case repeated along the slices to n: slice k is slice k % (the case's count)"""
    out = {}
    for k, v in c.items():
        if isinstance(v, np.ndarray) and v.ndim >= 1:
            m = v.shape[0]
            out[k] = np.ascontiguousarray(v[np.arange(n) % m])
        else:
            out[k] = v
    return out


# ---- slice sizes of the streaming passes -------------------------------------------------------------------------------------
SIZES = {  # (h, w): what h * w reaches
    (1, 1): "cnt 1",
    (1, 2): "cnt 2",
    (1, 6): "cnt == 2 in the second group of four",
    (32, 32): "one chunk exactly full, 16-byte path",
    (2, 513): "a second chunk of one thread with cnt == 2",
    (4, 257): "16-byte path, one thread in the second chunk",
    (3, 1025): "four chunks: the fold order over more than two",
}
SIZE_N_EM = 1
RB_SIZE_SEEDS = {(1, 1): 1, (1, 2): 1, (1, 6): 3, (32, 32): 1, (2, 513): 1, (4, 257): 1, (3, 1025): 1}
_SZ = {}


def _smooth(n, h, w):
    yy, xx = np.meshgrid(np.arange(h, dtype=F64), np.arange(w, dtype=F64), indexing="ij")
    return np.stack([1.3 + 0.6 * np.sin(yy / (3.0 + k) + k) * np.cos(xx / (40.0 + 5.0 * k)) for k in range(n)])


def robust_size_case(shape, seed=None):
    """three slices of `shape`: outlier pixels in 64 % of slice 1 and in 30 % of slice 2, none in slice 0; from 1024 pixels on
    a mask and sim weights with zeros.  Run with SIZE_N_EM = 1: slot 0 is the pass with p = 1, slot 1 the pass with the
    posterior, and with three slices a later slot puts mu2 on the potential of the one rejected slice (no margin)."""
    key = ("rb", shape, seed)
    if key not in _SZ:
        h, w = shape
        rng = np.random.default_rng(100 * h + w + 1000 * (RB_SIZE_SEEDS[shape] if seed is None else seed))
        s = _smooth(3, h, w) * rng.uniform(0.8, 1.2, 3)[:, None, None]
        y = s + rng.standard_normal(s.shape) * np.array([0.02, 0.03, 0.025])[:, None, None]
        for k, frac in ((1, 0.64), (2, 0.3)):
            for i in rng.permutation(h * w)[:int(round(h * w * frac))]:
                y[k, i // w, i % w] += rng.choice([-1.0, 1.0])
        mask = sw = None
        if h * w >= 1024:
            mask = rng.random(s.shape) < 0.9
            sw = rng.uniform(0.3, 1.2, s.shape).astype(F32)
            sw[rng.random(s.shape) < 0.05] = 0
        _SZ[key] = dict(y=y.astype(F32), s=s.astype(F32), mask=mask, sw=sw)
    return _SZ[key]


def imatch_size_case(shape):
    """three slices of `shape`, y = s / gain_k + noise; from 1024 pixels on a mask, sim weights, robust weights and a bias0"""
    key = ("im", shape)
    if key not in _SZ:
        h, w = shape
        rng = np.random.default_rng(9000 + 100 * h + w)
        s = _smooth(3, h, w)
        y = s / rng.uniform(0.7, 1.4, 3)[:, None, None] + 0.01 * rng.standard_normal(s.shape)
        mask = sw = pw = b0 = None
        if h * w >= 1024:
            mask = rng.random(s.shape) < 0.9
            sw = rng.uniform(0.3, 1.2, s.shape).astype(F32)
            sw[rng.random(s.shape) < 0.05] = 0
            pw = rng.uniform(0.2, 1.0, s.shape).astype(F32)
            b0 = (0.1 * rng.uniform(-1, 1, s.shape)).astype(F32)
        _SZ[key] = dict(y=y.astype(F32), s=s.astype(F32), mask=mask, sw=sw, pw=pw, b0=b0)
    return _SZ[key]


def measure_size_e_cpu():
    """the utils' measure_e_cpu procedure on the new size cases -> (robust per group, imatch per group, the case of each worst)"""
    rb, im, who = dict.fromkeys(RB.GROUPS, 0.0), dict.fromkeys(IM.GROUPS, 0.0), {}
    for shape in SIZES:
        c = robust_size_case(shape)
        if shape[0] * shape[1] >= 4:  # the smaller ones freeze: no slice is ok
            a, b = robust_em(c, F32, n_em=SIZE_N_EM), robust_em(c, F64, n_em=SIZE_N_EM)
            RB.assert_margin(b)
            assert np.array_equal(a["frozen"], b["frozen"]) and not b["frozen"].any()
            for g, v in RB.compare(a, b).items():
                if v > rb[g]:
                    rb[g], who["rb_" + g] = v, shape
        c = imatch_size_case(shape)
        a, b = imatch_run(c, F32), imatch_run(c, F64)
        IM.assert_margin(b)
        assert a["frozen"] == b["frozen"] and np.array_equal(a["ok"], b["ok"])
        for g, v in IM.compare(a, b).items():
            if v > im[g]:
                im[g], who["im_" + g] = v, shape
    return rb, im, who


def rb_e_cpu(g):
    """E_cpu of a robust group for the size cases: no size case exceeds util_robust64.E_CPU"""
    return RB.E_CPU[g]


def im_e_cpu(g, beside=None):
    """E_cpu of an imatch group for the new cases: the larger of util_imatch64.E_CPU and what a new case set beside it (the
    size cases: E_CPU_SIZES; the 257 slices with the bias field: E_CPU_N257)"""
    return max(IM.E_CPU[g], (IM.E_CPU_SIZES if beside is None else beside).get(g, 0.0))


# ---- svr_update, svr_compose, svr_group_reduce -------------------------------------------------------------------------------
def hand_sequences(n):
    """the seven hand sequences of tests/test_svr_gpu._hand_rows tiled to n slices, (n, slots, 32), and a theta per slice"""
    from tests.test_svr_gpu import _hand_rows

    seq = _hand_rows()
    seq = np.ascontiguousarray(seq[np.arange(n) % seq.shape[0]])
    theta0 = np.random.default_rng(n).uniform(-1, 1, (n, 6)).astype(F32)
    return seq, theta0


STATE_FIELDS = ("stats_cur", "lam", "m0", "theta_cur", "frozen_now", "cost", "lambda_hist", "accepted", "frozen")


def svr_update_run(seq, theta0, mutant=None):
    """every slot of util_svr64.update over a state block filled with -1 -> (state, theta_trial).  The workgroup mutants of a
    thread-per-slice kernel: "drop_256" never runs the second workgroup (its slices keep the fill), "drop_ragged" leaves out the
    slices of the ragged last wave, "trip0_again" gives slices 64..127 the inputs of slices 0..63.  "reverse" has no meaning
    for a kernel without a sum over the slices and changes nothing."""
    n, slots = seq.shape[:2]
    src = RB.slice_order(n, mutant if mutant == "trip0_again" else None)
    st = SV.new_state(n, slots - 1)
    th = theta0[src].copy()
    for k in range(slots):
        th = SV.update(st, k, seq[src, k], th)
    out = {name: st[name] for name in STATE_FIELDS}
    out["theta_trial"] = th
    if mutant in ("drop_256", "drop_ragged"):
        keep = np.zeros(n, bool)
        keep[RB.slice_order(n, mutant)] = True
        for v in out.values():
            dead = np.frombuffer(b"\xff" * v.dtype.itemsize, dtype=v.dtype)[0]  # the fill, bytes 0xFF
            if v.shape[0] == n:
                v[~keep] = dead
            else:
                v[:, ~keep] = dead
    return out


def compose_inputs(n, G, seed=0):
    """base transforms, group ids from {-1, 0, 1, 2, 7} (G = 3) with slice 42 in a live group, or one group per slice, and the
    groups' poses"""
    rng = np.random.default_rng(500 + n + seed)
    theta = np.concatenate((rng.uniform(-0.5, 0.5, (n, 3)), rng.uniform(-5, 5, (n, 3))), 1)
    from tests import util_transform_convert64 as TC

    base = TC.axisangle2mat(theta, F64).astype(F32)
    if G == n:
        group = rng.permutation(n).astype(np.int32)
    else:
        group = rng.choice(np.array([-1, 0, 1, 2, 7], np.int32), n).astype(np.int32)
        if n > 42:
            group[42] = 1
    phi = np.concatenate((rng.uniform(-0.3, 0.3, (G, 3)), rng.uniform(-1.5, 1.5, (G, 3))), 1).astype(F32)
    return base, group, phi


def compose_mutant(gmat, gjac, base, group):
    """compose with the transform of slice s taken from the thread layout of a 252-thread workgroup: the threads of slice 42
    that own columns 4 and 5 of its Jacobian do not exist, so those columns stay zero"""
    tr, jac = GU.compose(gmat, gjac, base, group, F32)
    if base.shape[0] > 42:
        jac[42, :, 4:] = 0
    return tr, jac


def reduce_inputs(n, G, seed=0):
    """n rows of stats over 16 decades; G groups of 0..5 members: group 1 empty, a repeated member, the indices -1 and n"""
    rng = np.random.default_rng(900 + G + seed)
    stats = rng.standard_normal((n, 32)) * 10.0 ** rng.integers(-8, 8, (n, 32))
    members, offsets = [], [0]
    for g in range(G):
        m = [] if g == 1 else rng.integers(0, n, int(rng.integers(1, 6))).tolist()
        if g == 0:
            m = [4, -1, 0, n, 2, 4]
        if g == G - 1:
            m = m + [n - 1, 256, 255]
        members += m
        offsets.append(len(members))
    return stats, np.array(members, np.int32), np.array(offsets, np.int32)


# ---- the search that chose the seeds, and the measurements ------------------------------------------------------------------
def _search():
    for n in COUNTS:
        for seed in range(1000 + n, 20000 + n, 1000):
            c = _robust_case(n, seed)
            S = robust_em(c)
            ws = S["ws"][-1]
            if S["margin"] >= 2 * RB.MARGIN and not S["frozen"].any() and ((ws > 0.01) & (ws < 0.99)).any():
                print("robust", n, "seed", seed, "margin %.2e" % S["margin"], "rejected", int((ws == 0).sum()), "fractional",
                      int(((ws > 0.01) & (ws < 0.99)).sum()))
                break
    for n in COUNTS:
        for seed in range(7000 + n, 27000 + n, 1000):
            rows = imatch_rows32(imatch_case(n, seed))
            if differing(imatch_fields(IM.scale(rows)), imatch_fields(IM.scale(rows, mutant="reverse"))):
                print("imatch", n, "seed", seed)
                break
    for shape in SIZES:
        if shape[0] * shape[1] < 4:
            continue
        for seed in range(1, 20):
            S = robust_em(robust_size_case(shape, seed), n_em=SIZE_N_EM)
            if S["margin"] >= 2 * RB.MARGIN and not S["frozen"].any() and S["ws"][-1][1] == 0:
                print("robust size", shape, "seed", seed, "margin %.2e" % S["margin"], "ws", S["ws"][-1])
                break


if __name__ == "__main__":
    import sys

    if "--search" in sys.argv:
        _search()
    rb, im, who = measure_size_e_cpu()
    for g, v in rb.items():
        print("robust E_cpu", g, f"{v:.3e}", "recorded", RB.E_CPU[g], who.get("rb_" + g))
    for g, v in im.items():
        print("imatch E_cpu", g, f"{v:.3e}", "recorded", IM.E_CPU[g], who.get("im_" + g))
    for n in COUNTS:
        print(n, "robust margin %.2e" % robust_em(robust_case(n))["margin"], "imatch margin",
              imatch_run(imatch_case(n), sigma=4.0)["margin"] if n == 257 else math.inf)
