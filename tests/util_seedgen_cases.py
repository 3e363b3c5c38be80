"""The edge cases of seed generation, one list for the CPU file (tests/test_em64_edges_reference.py: are they well-conditioned?)
and the GPU file (tests/test_seedgen_edges_gpu.py: do the kernels get them right?).  Every draw comes from a fixed
`np.random.default_rng` seed.  Sizes sit on either side of a wave (64), a workgroup pass (256) and a tile (4096 samples or voxels).
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

TILE = 4096
SIZES = (1, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 1)
KS = (1, 2, 11, 13, 16)
ITERS = (1, 20)
MODES = (0, 1)
# the mixture of size n is drawn from seed MIX_SEED[n] (default: its position in SIZES).  Seeds 4 (n = 65) and 5 (n = 255) gave
# vectors on which a float32 evaluation drifts from the float64 one by more than a quarter of the caps (ill-conditioned inputs, see
# the CPU file); 46 and 45 are the nearest seeds with the same number of mixture components that do not.
MIX_SEED = {65: 46, 255: 45}

# name, float32 samples, component count, centres of init mode 1 (taken from the samples), (w, mu, var) of init mode 0
EmCase = namedtuple("EmCase", "name x k mu0 init0")


def mixture(n, seed, offset=0.0, centres=(400.0, 900.0, 1500.0, 2300.0), sds=(50.0, 90.0, 70.0, 160.0)):
    """n float32 draws from a mixture of 2..4 Gaussians (the count follows from the seed)."""
    rng = np.random.default_rng(seed)
    ncomp = min(2 + seed % 3, len(centres))
    p = np.array([0.4, 0.3, 0.2, 0.1][:ncomp])
    comp = rng.choice(ncomp, size=n, p=p / p.sum())
    return (offset + np.array(centres)[comp] + np.array(sds)[comp] * rng.standard_normal(n)).astype(np.float32)


def sample_centres(x, k):
    """k centres that are samples of x: those at the (c + 0.5) / k positions of the sorted vector (duplicates when x has fewer
    than k distinct values -- as k-means++ gives when every sample already coincides with a centre)."""
    xs = np.sort(np.asarray(x, np.float64))
    return xs[np.minimum(((np.arange(k) + 0.5) / k * xs.size).astype(np.int64), xs.size - 1)]


def given_init(x, k):
    """Init mode 0: equal weights, the sample centres, var(x) / k^2 (at least 1: constant data has no variance to share out)."""
    x = np.asarray(x, np.float64)
    return np.full(k, 1.0 / k), sample_centres(x, k), np.full(k, max(x.var() / k**2, 1.0))


def _case(name, x, k, mu0=None):
    x = np.ascontiguousarray(x, np.float32)
    w, mu, var = given_init(x, k)
    mu0 = mu if mu0 is None else np.asarray(mu0, np.float64)
    return EmCase(f"{name}_k{k}", x, k, mu0, (w, mu0.copy(), var))


def offset_vector():
    """Unnormalised integer-scaled T2w: intensities near 30 000, components 0.1 .. 0.5 wide."""
    return mixture(8192, 4, offset=30000.0, centres=(-3.0, 0.0, 4.0), sds=(0.1, 0.3, 0.5))


def integer_vector(k, seed=16):
    """Integer-valued floats < 2^24 with centres among them, plus five samples at the exact midpoint of every pair of
    neighbouring centres an even distance apart: x - mu is exact in float32, those samples are exactly equidistant."""
    rng = np.random.default_rng(seed)
    comp = rng.choice(3, size=6000, p=[0.5, 0.3, 0.2])
    x = np.rint(np.array([3.0e6, 6.0e6, 1.1e7])[comp] + np.array([3.0e5, 4.0e5, 6.0e5])[comp] * rng.standard_normal(6000))
    x = np.clip(x, 1, 2**24 - 1)
    mu0 = sample_centres(x, k)
    mids = [(a + b) / 2 for a, b in zip(mu0, mu0[1:]) if a != b and (a + b) % 2 == 0]
    assert mids, "no pair of centres an even distance apart"
    return np.concatenate([x, np.repeat(mids, 5)]).astype(np.float32), mu0


def apart_vector(seed=17):
    """Three integer clusters 1 000 wide and 4e6 apart, with five samples exactly midway between neighbouring centres.  After the
    initial M-step every responsibility of the next E-step is exactly 0 or 1 (exp underflows, in float32 and float64 alike), so
    the weights after one iteration still show the one-hot counts of the initial M-step -- to which the ties belong."""
    rng = np.random.default_rng(seed)
    mu0 = np.array([9.0e6, 5.0e6, 1.0e6])     # not in mean order: "lowest index" and "lowest mean" differ
    x = np.concatenate([c + rng.integers(-1000, 1001, size=n) for c, n in zip(mu0, (1000, 1500, 2000))] + [mu0, [7.0e6] * 5, [3.0e6] * 5])
    return x.astype(np.float32), mu0


@lru_cache(maxsize=None)
def em_cases():
    cases = []
    for i, n in enumerate(SIZES):
        x = mixture(n, MIX_SEED.get(n, i))
        cases += [_case(f"mix{n}", x, k) for k in KS]
    cases += [_case("constant", np.full(1000, 512.0), k) for k in (1, 2, 5)]
    two = np.where(np.arange(1000) % 3 == 0, 900.0, 100.0)
    cases += [_case("two_valued", two, k) for k in (2, 3, 5)]
    cases += [_case("few", np.array([700.0, 710.0, 1300.0]), k) for k in (2, 3, 5, 16)]
    cases += [_case("offset", offset_vector(), k) for k in (2, 3, 5)]
    for k in (2, 5, 16):
        x, mu0 = integer_vector(k)
        cases.append(_case("integers", x, k, mu0[::-1] if k == 5 else mu0))  # k = 5: lowest index is not lowest mean
    x, mu0 = apart_vector()
    cases.append(_case("integers_apart", x, 3, mu0))
    return tuple(cases)


# ----------------------------------------------------------------------------------------------------------------------
# assignment: parameters given, so the labels of a float64 evaluation are the answer outside its own near-ties
# ----------------------------------------------------------------------------------------------------------------------
AssignCase = namedtuple("AssignCase", "name x w mu var base")


@lru_cache(maxsize=None)
def assign_cases():
    x1 = mixture(4097, 21)
    x16 = mixture(3 * 4096 + 1, 22)
    perm = np.random.default_rng(23).permutation(16)  # component order is not mean order
    mu16 = sample_centres(x16, 16)[perm]
    w16 = (np.arange(16) + 8.0)[perm]
    xe = mixture(4095, 24, centres=(500.0, 900.0), sds=(40.0, 20.0))
    xo = offset_vector()
    return (
        AssignCase("k1", x1, np.ones(1), np.zeros(1), np.ones(1), 7),
        AssignCase("k16_top_base", x16, w16 / w16.sum(), mu16, np.full(16, np.float64(x16).var() / 16**2), 256 - 16),
        # two exactly equal means: the narrow and the wide component at 500 rank by index, below the one at 900
        AssignCase("equal_means", xe, np.array([0.3, 0.3, 0.4]), np.array([500.0, 900.0, 500.0]), np.array([2500.0, 400.0, 100.0]), 30),
        AssignCase("offset", xo, np.array([0.3, 0.4, 0.3]), 30000.0 + np.array([4.0, -3.0, 0.0]), np.array([0.25, 0.01, 0.09]), 40),
    )


# ----------------------------------------------------------------------------------------------------------------------
# volumes for fusion and compaction
# ----------------------------------------------------------------------------------------------------------------------
FUSION_SIZES = (1, 255, 256, 257, 4095, 4096, 4097, 8193)
SEG_SALT = (2.5, -1.0, 256.0, 1e9, np.inf, -np.inf, -0.0, np.nan, 0.0, 2.0)
IMG_SALT = (np.inf, -np.inf, -0.0, np.nan, 0.0, 3.5)
CUSTOM = {255: 1, 7: 2, 9: 0, 3: 3, 12: 4}  # uses label 255, maps label 9 to nothing

FusionCase = namedtuple("FusionCase", "name image seg annotation")


def planted(n, seed, labels=tuple(range(10))):
    """A flat volume in the style of `_planted` of test_seedgen_gpu.py: labels of both schemes, NaN in both inputs, background
    with and without signal, label 4 (dhcp: cleared, then background) over zero and non-zero intensities."""
    rng = np.random.default_rng(seed)
    seg = rng.choice(np.array(labels, np.float32), size=n)
    img = (rng.random(n) * 100 + 1).astype(np.float32)
    img[rng.random(n) < 0.2] = 0.0
    img[rng.random(n) < 0.05] = np.nan
    seg[rng.random(n) < 0.05] = np.nan
    if n == 1:
        seg[:], img[:] = 2.0, 5.0
    return img, seg


@lru_cache(maxsize=None)
def fusion_cases():
    cases = []
    both = ("feta", "dhcp")
    for i, n in enumerate(FUSION_SIZES):
        img, seg = planted(n, 100 + i)
        shape = (n,) if i % 2 == 0 else (1, 1, n)
        cases += [FusionCase(f"flat{n}_{a}", img.reshape(shape), seg.reshape(shape), a) for a in both]
    rng = np.random.default_rng(120)
    img = (rng.random(8192) * 50 + 1).astype(np.float32)
    for m, lab in ((1, 1.0), (2, 2.0), (3, 3.0), (4, 0.0)):   # a full 4096 in one 16-bit half of a workgroup's counters
        cases += [FusionCase(f"all_meta{m}_{a}", img, np.full(8192, lab, np.float32), a) for a in both]
    img, seg = planted(4097, 121, labels=(0, 1, 4, 5, 3))      # feta: no GM label; background carries no signal
    img = np.where(np.nan_to_num(seg) == 0, np.float32(0), img)
    cases.append(FusionCase("absent_2_and_4_feta", img, seg, "feta"))
    img, seg = planted(4097, 122)
    pairs = [(s, v) for s in SEG_SALT for v in IMG_SALT]       # every salted label over every salted intensity
    at = np.random.default_rng(123).permutation(4097)[: len(pairs)]
    seg[at], img[at] = np.array(pairs, np.float32).T
    cases += [FusionCase(f"salted_{a}", img, seg, a) for a in both]
    img, seg = planted(4097, 124, labels=(0, 3, 7, 9, 12, 255, 200))
    cases.append(FusionCase("custom_annotation", img, seg, "custom"))
    return tuple(cases)


def annotation_of(case):
    return dict(CUSTOM) if case.annotation == "custom" else case.annotation


def as_uint8(seg):
    """The uint8 form of a segmentation, or None when it holds values a uint8 volume cannot (the salted one)."""
    s = np.nan_to_num(np.asarray(seg, np.float32), nan=0.0, posinf=-1.0, neginf=-1.0)
    if ((s < 0) | (s > 255) | (s != np.trunc(s))).any():
        return None
    return s.astype(np.uint8)


# ----------------------------------------------------------------------------------------------------------------------
# a whole subject at the edges: 24^3, feta labels
# ----------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def edge_subject():
    """(image, uint8 dseg): CSF (meta 1) ordinary -- 3 456 voxels of a three-component mixture; GM (meta 2) three voxels; WM
    (meta 3) constant at 512; no background with signal (meta 4 absent)."""
    shape = (24, 24, 24)
    seg = np.zeros(shape, np.uint8)
    img = np.zeros(shape, np.float32)
    seg[2:14, 2:14, :] = 1
    seg[2:8, 2:14, :] = 4                       # both fuse into CSF
    img[seg > 0] = mixture(int((seg > 0).sum()), 31)
    seg[16:20, 3:9, 5:15] = 5                   # WM, constant
    img[16:20, 3:9, 5:15] = 512.0
    for at, v in (((21, 20, 3), 700.0), ((21, 20, 4), 710.0), ((22, 5, 17), 1300.0)):
        seg[at], img[at] = 2, v                 # GM: three voxels
    return img, seg
