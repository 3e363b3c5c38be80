"""numpy float64 restatement of the fsg_voxel_pick_* contract (include/fsg_hip.h): sequential prefix sum over the eligible
weights, `searchsorted(side="right")`, ordered de-duplication.  Shared by the CPU checks of the restatement itself and by the
GPU tests of the kernels."""
import numpy as np

MODES = {">": 0, "==": 1, "!=": 2}


def eligible_mask(pred, op, value, weight=None):
    p = np.asarray(pred).reshape(-1).astype(np.float32)
    v = np.float32(value)
    ok = p > v if op == ">" else (p == v if op == "==" else p != v)
    if weight is not None:
        with np.errstate(invalid="ignore"):
            ok = ok & (np.asarray(weight, dtype=np.float32).reshape(-1) > 0)  # NaN and negative weights count as 0
    return ok


def prefix(pred, op, value, weight=None):
    """(flat indices of the eligible voxels in raster order, their inclusive float64 prefix sums)."""
    ok = eligible_mask(pred, op, value, weight)
    idx = np.flatnonzero(ok)
    w = np.ones(idx.size, np.float64) if weight is None else np.asarray(weight, dtype=np.float32).reshape(-1)[idx].astype(np.float64)
    return idx, np.cumsum(w, dtype=np.float64)


def candidates(pred, op, value, u, weight=None):
    """Flat index of every candidate (one per entry of `u`), or an empty array when nothing is eligible."""
    idx, cdf = prefix(pred, op, value, weight)
    if idx.size == 0:
        return np.zeros(0, np.int64)
    t = np.asarray(u, dtype=np.float64) * cdf[-1]
    return idx[np.minimum(np.searchsorted(cdf, t, side="right"), idx.size - 1)].astype(np.int64)


def pick(pred, op, value, k, u, weight=None):
    """The `out` array of the contract: k + 2 int64."""
    out = np.full(int(k) + 2, -1, np.int64)
    idx, _cdf = prefix(pred, op, value, weight)
    kept = []
    for c in candidates(pred, op, value, u, weight).tolist():
        if c not in kept:
            kept.append(c)
            if len(kept) == k:
                break
    out[0], out[1] = idx.size, len(kept)
    out[2:2 + len(kept)] = kept
    return out


def boundary_distance(pred, op, value, u, weight=None):
    """|u * total - nearest prefix boundary| / total for every entry of `u` (boundaries: 0 and every S_e)."""
    _idx, cdf = prefix(pred, op, value, weight)
    t = np.asarray(u, dtype=np.float64) * cdf[-1]
    b = np.concatenate([[0.0], cdf])
    j = np.clip(np.searchsorted(b, t), 1, b.size - 1)
    return np.minimum(np.abs(t - b[j - 1]), np.abs(b[j] - t)) / cdf[-1]


# ---- the cases the CPU and the GPU tests share ----------------------------------------------------------------------
RANDOM_SEED = 20  # test_pick64_reference checks that the restatement leaves out none of the 64 candidates for this seed
RANDOM_N, RANDOM_M = 40 * 4096 + 1, 64


def random_case(seed=RANDOM_SEED):
    """float32 uniform weights (sums are not exact), every voxel passes the predicate, 64 uniforms."""
    rng = np.random.default_rng(seed)
    pred = np.ones(RANDOM_N, np.float32)
    weight = rng.random(RANDOM_N, dtype=np.float32)
    u = rng.random(RANDOM_M)
    return pred, weight, u


def dyadic_weights(n, seed):
    """Weights on a 2^-10 grid in [0, 4): every partial sum of up to 2^40 of them is exact in float64, in any order."""
    return (np.random.default_rng(seed).integers(0, 4096, n) / 1024.0).astype(np.float32)
