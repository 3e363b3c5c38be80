"""Float64 numpy restatement of seed generation: meta-label fusion and 1-D Gaussian-mixture EM.

This is the yardstick the GPU tests of `fetalsyngen_amd.seedgen` compare against.  It is itself pinned to
scikit-learn's `GaussianMixture` on the CPU (tests/test_em64_reference.py: a committed fixture, and live
when sklearn imports).  The algorithm, restated from the published description of EM for mixtures (Dempster,
Laird, Rubin 1977) with sklearn's conventions for the one-dimensional "full" covariance case:

  E-step   lp[i, c] = log w_c - 0.5 log(2 pi var_c) - 0.5 (x_i - mu_c)^2 / var_c
           lse[i]   = logsumexp_c lp[i, c];  r[i, c] = exp(lp[i, c] - lse[i])
  M-step   nk_c = sum_i r[i, c] + 10 eps;  mu_c = sum_i r x / nk_c;
           var_c = sum_i r (x - mu_c)^2 / nk_c + reg_covar;  w_c = nk_c / n
  bound    lb = mean_i lse[i]  (with the parameters the E-step used)
  stop     |lb - lb_prev| < tol (lb_prev = -inf before the first iteration), at most max_iter iterations
  labels   argmax_c lp[i, c] under the final parameters (ties -> lowest c), components renumbered by ascending mean
"""
from __future__ import annotations

import numpy as np

EPS10 = 10 * np.finfo(np.float64).eps
REG_COVAR = 1e-6
LOG_2PI = float(np.log(2 * np.pi))

FETA2META = {1: 1, 4: 1, 2: 2, 6: 2, 5: 3, 7: 3, 3: 3}
DHCP2META = {1: 1, 5: 1, 2: 2, 7: 2, 9: 2, 3: 3, 6: 3, 8: 3}


def meta_table(annotation) -> np.ndarray:
    """256-entry label -> meta-label table of an annotation scheme ("feta", "dhcp" or a {label: meta} dict)."""
    mapping = {"feta": FETA2META, "dhcp": DHCP2META}.get(annotation, annotation) if isinstance(annotation, str) else annotation
    if not isinstance(mapping, dict):
        raise ValueError(f"unknown annotation {annotation!r}")
    table = np.zeros(256, np.uint8)
    for lab, meta in mapping.items():
        table[int(lab)] = int(meta)
    if annotation == "dhcp":
        table[4] = 0  # label 4 is cleared before the fusion; it then counts as background
    return table


def meta_labels(image, segmentation, annotation="feta") -> np.ndarray:
    """uint8 meta-label volume: NaN -> 0 in both inputs; meta = table[label]; background (label 0, for dhcp also
    label 4) with a non-zero image value -> 4.  A float segmentation value that is not an integer in 0..255 (2.5, -1,
    256, +-inf) equals no label and is not background either: meta 0 whatever the image holds (the reference's rule is
    the comparisons `segmentation == label` and `(segmentation == 0) & (image != 0)`).  -0.0 is 0."""
    img = np.nan_to_num(np.asarray(image, np.float32), nan=0.0, posinf=np.inf, neginf=-np.inf)
    seg = np.asarray(segmentation)
    is_label = np.ones(seg.shape, bool)
    if seg.dtype.kind == "f":
        seg = np.where(np.isnan(seg), 0, seg)
        is_label = (seg >= 0) & (seg <= 255) & (seg == np.trunc(seg))
        seg = np.where(is_label, seg, 0)
    seg = seg.astype(np.uint8)
    if annotation == "dhcp":
        seg = np.where(seg == 4, 0, seg).astype(np.uint8)
    meta = meta_table(annotation)[seg]
    meta[(seg == 0) & (img != 0)] = 4
    meta[~is_label] = 0
    return meta


def packed(image, meta, m) -> np.ndarray:
    """Intensities of meta-label m in C (voxel) order, NaN counted as 0."""
    img = np.asarray(image, np.float32)
    img = np.where(np.isnan(img), np.float32(0), img)
    return img[np.asarray(meta) == m]


def log_prob(x, w, mu, var) -> np.ndarray:
    x = np.asarray(x, np.float64)[:, None]
    w, mu, var = (np.asarray(a, np.float64)[None, :] for a in (w, mu, var))
    with np.errstate(divide="ignore"):
        return np.log(w) - 0.5 * (LOG_2PI + np.log(var)) - 0.5 * (x - mu) ** 2 / var


def logsumexp(lp) -> np.ndarray:
    m = lp.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(lp - m).sum(axis=1, keepdims=True)))[:, 0]


def m_step(x, r):
    x = np.asarray(x, np.float64)
    nk = r.sum(axis=0) + EPS10
    mu = (r * x[:, None]).sum(axis=0) / nk
    var = (r * (x[:, None] - mu[None, :]) ** 2).sum(axis=0) / nk + REG_COVAR
    return nk / x.size, mu, var


def init_from_means(x, means):
    """One-hot responsibilities of the nearest initial centre (ties -> lowest index), then an M-step."""
    x = np.asarray(x, np.float64)
    means = np.asarray(means, np.float64)
    near = np.abs(x[:, None] - means[None, :]).argmin(axis=1)
    r = np.zeros((x.size, means.size))
    r[np.arange(x.size), near] = 1.0
    return m_step(x, r)


def lower_bound(x, w, mu, var) -> float:
    return float(logsumexp(log_prob(x, w, mu, var)).mean())


def fit(x, w, mu, var, tol=1e-3, max_iter=100, trace=False):
    """EM from the given parameters.  -> dict(weights, means, variances, lower_bound, n_iter, converged[, lbs])."""
    x = np.asarray(x, np.float64)
    w, mu, var = (np.array(a, np.float64) for a in (w, mu, var))
    lb, converged, n_iter, lbs = -np.inf, False, 0, []
    for n_iter in range(1, int(max_iter) + 1):
        prev = lb
        lp = log_prob(x, w, mu, var)
        lse = logsumexp(lp)
        w, mu, var = m_step(x, np.exp(lp - lse[:, None]))
        lb = float(lse.mean())
        lbs.append(lb)
        if abs(lb - prev) < tol:
            converged = True
            break
    out = dict(weights=w, means=mu, variances=var, lower_bound=lb, n_iter=n_iter, converged=converged,
               lse_absmax=float(np.abs(lse).max()))  # of the last E-step: the scale of the device's float32 bound terms
    if trace:
        out["lbs"] = np.array(lbs)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# The same algorithm with float32 rounding where the kernels document it (csrc/fsg_seedgen.hip section (b), DESIGN.md
# section 10).  Not a second yardstick: it shows, without a GPU, which inputs are well-conditioned -- on which a float32
# evaluation of the per-sample terms stays close to `fit` -- so that a device result that does not is a wrong kernel.
# ----------------------------------------------------------------------------------------------------------------------
def derive32(w, mu, var):
    """The four floats per component the E-step reads: a = log w - 0.5 log(2 pi var), b = 0.5 / var, mu_hi + mu_lo = mu."""
    w, mu, var = (np.asarray(a, np.float64) for a in (w, mu, var))
    with np.errstate(divide="ignore"):
        a = (np.log(w) - 0.5 * np.log(2 * np.pi * var)).astype(np.float32)
    hi = mu.astype(np.float32)
    return a, (0.5 / var).astype(np.float32), hi, (mu - hi.astype(np.float64)).astype(np.float32)


def _m_step_pivoted(S0, S1, S2, pivot, n):
    """M-step from float64 sums of r, r (x - pivot), r (x - pivot)^2 taken about the previous mean."""
    nk = S0 + EPS10
    dlt = (S1 - pivot * EPS10) / nk           # new mean - pivot;  pivot + dlt = sum r x / nk
    ss = np.maximum((S2 - 2.0 * dlt * S1) + dlt * dlt * S0, 0.0)
    return nk / n, pivot + dlt, ss / nk + REG_COVAR


def _diff32(x32, hi, lo):
    return (x32[:, None] - hi[None, :]) - lo[None, :]   # float32 throughout: x - mu rounded once, relative to the difference


def init_from_means32(x, means):
    """`init_from_means` as the device does it: nearest centre by |(x - mu_hi) - mu_lo| in float32 (ties -> lowest
    index), one-hot sums in float64 about the centres."""
    x32 = np.asarray(x, np.float32)
    means = np.asarray(means, np.float64)
    _a, _b, hi, lo = derive32(np.ones_like(means), means, np.ones_like(means))
    near = (-np.abs(_diff32(x32, hi, lo))).argmax(axis=1)
    r = np.zeros((x32.size, means.size))
    r[np.arange(x32.size), near] = 1.0
    dd = x32.astype(np.float64)[:, None] - means[None, :]
    return _m_step_pivoted(r.sum(axis=0), (r * dd).sum(axis=0), (r * dd * dd).sum(axis=0), means, x32.size)


def fit32(x, w, mu, var, tol=1e-3, max_iter=100):
    """`fit` with the device's rounding: d, lp = a - d d b, exp, the sum over components, log and r = exp * (1 / sum) in
    float32; every sum over samples in float64, about the previous mean."""
    x32 = np.asarray(x, np.float32)
    x64 = x32.astype(np.float64)
    w, mu, var = (np.array(a, np.float64) for a in (w, mu, var))
    k = mu.size
    lb, converged, n_iter, lse = -np.inf, False, 0, np.zeros(1)
    for n_iter in range(1, int(max_iter) + 1):
        prev = lb
        a, b, hi, lo = derive32(w, mu, var)
        d = _diff32(x32, hi, lo)
        dd32 = d * d
        # a - (d d) b in one rounding (the compiler contracts it to a fused multiply-add; the float64 product is exact)
        lp = (a.astype(np.float64)[None, :] - dd32.astype(np.float64) * b.astype(np.float64)[None, :]).astype(np.float32)
        mx = lp.max(axis=1)
        with np.errstate(under="ignore"):
            e = np.exp(lp - mx[:, None])
        s = np.zeros(x32.size, np.float32)
        for c in range(k):
            s = s + e[:, c]
        lse = (mx + np.log(s)).astype(np.float64)
        r = (e * (np.float32(1.0) / s)[:, None]).astype(np.float64)
        dd = x64[:, None] - mu[None, :]
        rd = r * dd
        w, mu, var = _m_step_pivoted(r.sum(axis=0), rd.sum(axis=0), (rd * dd).sum(axis=0), mu, x32.size)
        lb = float(lse.mean())
        if abs(lb - prev) < tol:
            converged = True
            break
    return dict(weights=w, means=mu, variances=var, lower_bound=lb, n_iter=n_iter, converged=converged,
                lse_absmax=float(np.abs(lse).max()))


def param_error(got, ref, floor=1e-9) -> float:
    """Largest error of `got` against `ref`: relative where |ref| >= floor, absolute below it (an empty component has
    weight ~2e-15 / n and mean 0; without the floor its last bits would decide the result)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    big = np.abs(ref) >= floor
    return float(np.max(np.where(big, err / np.where(big, np.abs(ref), 1.0), err)))


def lb_bound(lse_absmax) -> float:
    """Bound on |device lower bound - reference|: every sample's mx + logf(sum) is a float32 value built from float32
    terms of at most that size, then averaged in float64."""
    return 16.0 * 2.0**-24 * float(lse_absmax)


def next_lower_bound(x, fitted) -> float:
    """The bound one more iteration would report (used to decide whether a stop was a close call)."""
    return lower_bound(x, fitted["weights"], fitted["means"], fitted["variances"])


def predict(x, w, mu, var, sort=True):
    """-> (labels, gap): argmax of the weighted log-densities, renumbered by ascending mean when `sort`; gap is the
    difference between the two largest weighted log-densities of every sample."""
    lp = log_prob(x, w, mu, var)
    lab = lp.argmax(axis=1)
    top = np.sort(lp, axis=1)
    gap = top[:, -1] - top[:, -2] if lp.shape[1] > 1 else np.full(lp.shape[0], np.inf)
    if sort:
        lab = mean_rank(mu)[lab]
    return lab.astype(np.uint8), gap


def mean_rank(mu) -> np.ndarray:
    """rank[c] = position of component c when the components are ordered by ascending mean (stable)."""
    order = np.argsort(np.asarray(mu, np.float64), kind="stable")
    rank = np.empty(order.size, np.int64)
    rank[order] = np.arange(order.size)
    return rank


def quantile_init(x, k):
    """The fixed initialisation of the parity cases: quantile means, equal weights, var(x) / k^2."""
    x = np.asarray(x, np.float64)
    q = (np.arange(k) + 0.5) / k
    return np.full(k, 1.0 / k), np.quantile(x, q), np.full(k, x.var() / k**2)
