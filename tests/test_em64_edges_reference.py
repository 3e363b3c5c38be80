"""CPU: the edge cases of seed generation (tests/util_seedgen_cases.py) seen from the float64 yardstick alone.

tests/test_seedgen_edges_gpu.py holds the kernels to `util_em64` on these cases within the project's caps (1e-5 means and
weights, 1e-4 variances, the lower bound within 16 * 2^-24 * max |lse|).  That is only a check of the kernels if the cases are
well-conditioned: if the float32 evaluation the kernels document (`util_em64.fit32`, plain numpy) already stays within a quarter
of those bounds of the float64 one.  This file asserts that for every case, every init mode and both iteration counts -- every
case in the list passes; two mixture seeds that did not were replaced by neighbouring seeds (MIX_SEED in the case list), no bound
was widened.  It also pins the yardstick's meta-label rule to the two comparisons the reference fuses labels with, on volumes
salted with non-labels, and counts the samples near a decision boundary in the assignment cases.
"""
import numpy as np
import pytest

from tests import util_em64 as E
from tests import util_seedgen_cases as SC

DELTA = 1e-4        # as in test_em64_reference.py
MAX_SHARE = 1e-3
CAP_MEAN = CAP_WEIGHT = 1e-5
CAP_VAR = 1e-4
EM_CASES = {c.name: c for c in SC.em_cases()}


# ------------------------------------------------------------------------------------------------------------ meta-labels
def two_comparisons(image, seg, annotation):
    """The reference's fusion, written out: meta[seg == label] = meta-label for every entry of the scheme, then
    meta[(seg == 0) & (image != 0)] = 4 -- after NaN -> 0 in both inputs and, for dhcp, label 4 -> 0."""
    img = np.asarray(image, np.float32).astype(np.float64)
    seg = np.asarray(seg).astype(np.float64)
    img[np.isnan(img)] = 0.0
    seg[np.isnan(seg)] = 0.0
    mapping = {"feta": E.FETA2META, "dhcp": E.DHCP2META}.get(annotation, annotation) if isinstance(annotation, str) else annotation
    if annotation == "dhcp":
        seg[seg == 4] = 0.0
    meta = np.zeros(seg.shape, np.uint8)
    for label, m in mapping.items():
        meta[seg == label] = m
    meta[(seg == 0) & (img != 0)] = 4
    return meta


@pytest.mark.parametrize("case", SC.fusion_cases(), ids=lambda c: c.name)
def test_meta_labels_are_the_two_comparisons(case):
    ann = SC.annotation_of(case)
    want = two_comparisons(case.image, case.seg, ann)
    assert np.array_equal(E.meta_labels(case.image, case.seg, ann), want)
    u8 = SC.as_uint8(case.seg)
    if u8 is not None:
        assert np.array_equal(E.meta_labels(case.image, u8, ann), want)
    else:
        assert case.name.startswith("salted")


def test_meta_labels_of_the_salt_spelled_out():
    seg = np.array([2.5, -1.0, 256.0, 1e9, np.inf, -np.inf, -0.0, -0.0, np.nan, np.nan, 0.0, 0.0, 0.0, 0.0, 2.0, 255.0], np.float32)
    img = np.array([3.5, 3.5, 3.5, 3.5, 3.5, 3.5, 3.5, 0.0, np.inf, np.nan, np.inf, -np.inf, -0.0, np.nan, np.inf, 1.0], np.float32)
    assert E.meta_labels(img, seg, "feta").tolist() == [0, 0, 0, 0, 0, 0, 4, 0, 4, 0, 4, 4, 0, 0, 2, 0]
    assert E.meta_labels(img, seg, SC.CUSTOM).tolist() == [0, 0, 0, 0, 0, 0, 4, 0, 4, 0, 4, 4, 0, 0, 0, 1]
    # what is packed for the fits: NaN counts as 0, the infinities stay
    assert E.packed(img, E.meta_labels(img, seg, "feta"), 4).tolist() == [3.5, np.inf, np.inf, -np.inf]


def test_the_fusion_cases_cover_what_they_are_named_for():
    by = {c.name: c for c in SC.fusion_cases()}
    for m in range(1, 5):
        for a in ("feta", "dhcp"):
            c = by[f"all_meta{m}_{a}"]
            assert (E.meta_labels(c.image, c.seg, a) == m).all() and c.image.size == 2 * SC.TILE
    c = by["absent_2_and_4_feta"]
    counts = [int((E.meta_labels(c.image, c.seg, "feta") == m).sum()) for m in range(1, 5)]
    assert counts[1] == 0 and counts[3] == 0 and counts[0] > 0 and counts[2] > 0
    c = by["salted_feta"]
    for s in SC.SEG_SALT:
        for v in SC.IMG_SALT:
            same = lambda a, b: (np.isnan(a) & np.isnan(b)) | ((a == b) & (np.signbit(a) == np.signbit(b)))  # noqa: E731
            assert (same(c.seg, np.float32(s)) & same(c.image, np.float32(v))).any(), (s, v)
    c = by["custom_annotation"]
    assert (c.seg == 255).any() and (c.seg == 9).any()
    assert sorted(c.image.size for c in SC.fusion_cases() if c.name.startswith("flat") and c.annotation == "feta") == list(SC.FUSION_SIZES)


# ------------------------------------------------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("name", list(EM_CASES))
def test_every_em_case_is_well_conditioned(name):
    """A condition on the inputs, not on the product: a case that fails is replaced by a neighbouring size or seed."""
    c = EM_CASES[name]
    for mode in SC.MODES:
        if mode == 0:
            init64 = init32 = c.init0
        else:
            init64, init32 = E.init_from_means(c.x, c.mu0), E.init_from_means32(c.x, c.mu0)
            e = [E.param_error(a, b) for a, b in zip(init32, init64)]
            assert e[0] <= CAP_WEIGHT / 4 and e[1] <= CAP_MEAN / 4 and e[2] <= CAP_VAR / 4, (name, "initial M-step", e)
        for iters in SC.ITERS:
            ref = E.fit(c.x, *init64, tol=0.0, max_iter=iters)
            got = E.fit32(c.x, *init32, tol=0.0, max_iter=iters)
            em, ew, ev = (E.param_error(got[p], ref[p]) for p in ("means", "weights", "variances"))
            elb, bound = abs(got["lower_bound"] - ref["lower_bound"]), E.lb_bound(ref["lse_absmax"])
            print(f"{name} mode {mode} iters {iters}: means {em:.2e} weights {ew:.2e} variances {ev:.2e} |lb diff| {elb:.2e} (bound {bound:.2e})")
            assert em <= CAP_MEAN / 4 and ew <= CAP_WEIGHT / 4 and ev <= CAP_VAR / 4, (name, mode, iters, em, ew, ev)
            assert elb <= bound / 4, (name, mode, iters, elb, bound)


def test_the_em_cases_cover_the_sizes_and_component_counts():
    names = set(EM_CASES)
    assert {f"mix{n}_k{k}" for n in SC.SIZES for k in SC.KS} <= names
    assert {f"two_valued_k{k}" for k in (2, 3, 5)} | {f"few_k{k}" for k in (2, 3, 5, 16)} <= names
    for c in SC.em_cases():
        assert c.x.dtype == np.float32 and c.x.size <= 20000 and c.mu0.size == c.k and np.isin(c.mu0, c.x.astype(np.float64)).all(), c.name
    assert any(np.unique(c.x).size < c.k for c in SC.em_cases()) and any(c.x.size < c.k for c in SC.em_cases())
    off = EM_CASES["offset_k3"].x
    assert off.min() > 29000 and off.size == 8192


@pytest.mark.parametrize("name", [n for n in EM_CASES if n.startswith("integers")])
def test_integer_cases_have_exact_one_hot_counts(name):
    """Integer-valued samples and centres below 2^24: x - mu is exact in float32, a sample midway between two centres is an
    exact tie (-> the lower index), so the float32 initial M-step counts exactly what the float64 one counts."""
    c = EM_CASES[name]
    assert (c.x == np.rint(c.x)).all() and c.x.max() < 2**24 and (c.mu0 == np.rint(c.mu0)).all()
    dist = np.abs(c.x.astype(np.float64)[:, None] - c.mu0[None, :])
    srt = np.sort(dist, axis=1)
    assert (srt[:, 0] == srt[:, 1]).sum() >= 5, "no sample is exactly equidistant from its two nearest centres"
    w64, w32 = E.init_from_means(c.x, c.mu0)[0], E.init_from_means32(c.x, c.mu0)[0]
    n64, n32 = w64 * c.x.size, w32 * c.x.size
    assert np.abs(n64 - np.rint(n64)).max() < 1e-9 and np.array_equal(np.rint(n64), np.rint(n32))
    assert np.array_equal(np.rint(n64), np.bincount(dist.argmin(axis=1), minlength=c.k))
    if name.startswith("integers_apart"):
        # clusters so far apart that one EM iteration leaves the responsibilities exactly one-hot: the counts of the initial
        # M-step can be read from the weights after it (the device shows no parameters between the two)
        one = E.fit(c.x, *E.init_from_means(c.x, c.mu0), tol=0.0, max_iter=1)
        assert np.array_equal(np.rint(one["weights"] * c.x.size), np.rint(n64))
        assert np.abs(one["weights"] * c.x.size - np.rint(n64)).max() < 1e-9


# ---------------------------------------------------------------------------------------------------------- boundary voxels
@pytest.mark.parametrize("case", SC.assign_cases(), ids=lambda c: c.name)
def test_few_samples_sit_on_a_decision_boundary(case):
    _labels, gap = E.predict(case.x, case.w, case.mu, case.var)
    share = float((gap < DELTA).mean())
    print(f"{case.name}: share of samples with gap < {DELTA}: {share:.2e}")
    assert share <= MAX_SHARE
    assert 0 <= case.base and case.base + case.mu.size <= 256


def test_equal_means_rank_by_component_index():
    c = {a.name: a for a in SC.assign_cases()}["equal_means"]
    assert c.mu[0] == c.mu[2] and E.mean_rank(c.mu).tolist() == [0, 2, 1]
    labels, _gap = E.predict(c.x, c.w, c.mu, c.var)
    assert set(np.unique(labels).tolist()) == {0, 1, 2}  # the wide and the narrow component at 500 both own samples


@pytest.mark.parametrize("mode", SC.MODES)
def test_degenerate_cases_have_exactly_stated_labels(mode):
    """Constant data and duplicate centres are exempt from the boundary count (every gap is 0 or huge); their labels are
    stated instead.  An empty component has mean 0 (sum r x / (0 + 10 eps)), so it ranks below every live one."""
    def labels_of(name):
        c = EM_CASES[name]
        init = c.init0 if mode == 0 else E.init_from_means(c.x, c.mu0)
        f = E.fit(c.x, *init, tol=0.0, max_iter=20)
        return c, E.predict(c.x, f["weights"], f["means"], f["variances"])[0]

    for k in (2, 5):
        c, lab = labels_of(f"constant_k{k}")
        # mode 0: k identical components, the tie goes to the lowest, all means equal -> rank 0.
        # mode 1: component 0 takes every sample, the k - 1 empty ones sit at mean 0 below it -> rank k - 1
        assert (lab == (0 if mode == 0 else k - 1)).all()
    c, lab = labels_of("two_valued_k3")
    assert c.mu0.tolist() == [100.0, 100.0, 900.0]
    # mode 0: the twins at 100 tie -> component 0, rank 0; mode 1: component 1 is empty (rank 0), component 0 ranks 1
    assert np.array_equal(lab, np.where(c.x == 900.0, 2, 0 if mode == 0 else 1))
    c, lab = labels_of("few_k16")
    assert c.x.size < c.k and np.array_equal(np.argsort(lab, kind="stable"), np.argsort(c.x, kind="stable"))
