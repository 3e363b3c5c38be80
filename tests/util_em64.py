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
    label 4) with a non-zero image value -> 4."""
    img = np.nan_to_num(np.asarray(image, np.float32), nan=0.0, posinf=np.inf, neginf=-np.inf)
    seg = np.asarray(segmentation)
    if seg.dtype.kind == "f":
        seg = np.where(np.isnan(seg), 0, seg)
    seg = seg.astype(np.uint8)
    if annotation == "dhcp":
        seg = np.where(seg == 4, 0, seg).astype(np.uint8)
    meta = meta_table(annotation)[seg]
    meta[(seg == 0) & (img != 0)] = 4
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
    out = dict(weights=w, means=mu, variances=var, lower_bound=lb, n_iter=n_iter, converged=converged)
    if trace:
        out["lbs"] = np.array(lbs)
    return out


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
