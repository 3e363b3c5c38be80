"""CPU: the reference of the intensity kernels and GMM heads (tests/util_intensity64.py) is right, and the inputs the GPU tests
(tests/test_intensity_kernels_edges.py) feed the kernels can tell a right kernel from a wrong one.

  * normals64 against oracle/fsg_keyed_draws.device_normals (float32 numpy with libm, tied to the Random123 vectors by
    tests/test_keyed_draws.py) at the keys, streams and offsets of the GPU test, within the GPU test's own bar of 4e-5: an honest
    float32 evaluation meets the bar, so the bar is not tighter than the format;
  * gmm32 against oracle/fsg_oracle.gmm_image bit for bit; add_noise32 against torch float32; gamma64 / bias64 against torch
    float64 expressions written out here;
  * label_sums_bound: the kernel's accumulation order restated in float32 stays inside it on every input of the GPU test, and a
    restatement that drops one value per workgroup leaves it;
  * a mutation per reference (lanes swapped, counter words swapped, label off by one, a part left out, a selection column
    moved): the mutant disagrees with the reference on the GPU test's inputs.
"""
import numpy as np
import pytest
import torch

from fetalsyngen_amd import tables as T
from oracle import fsg_keyed_draws as KD
from oracle import fsg_oracle as O
from tests import util_intensity64 as R

F = np.float32


def bits(a):
    return np.asarray(a, F).view(np.uint32)


# ---- normals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", R.RANDN_KEYS, ids=lambda k: f"{k[0]:#x}-{k[1]:#x}")
def test_normals64_against_float32_numpy(key):
    seed, stream = key
    worst = 0.0
    for n in R.RANDN_N:
        if n > 2 ** 20 and key != R.RANDN_KEYS[2]:
            continue  # the large offsets once: the key with both high words in use
        idx = R.sample_indices(n)
        got = KD.device_normals(seed, stream, n)[idx]
        ref = R.normals64(seed, stream, idx)
        assert np.abs(ref).max() <= 5.77
        worst = max(worst, float(np.abs(got - ref).max()))
    print(f"BOUND normals64 vs float32 numpy {key}: max err {worst:.3e}, {worst / R.NORMALS_ATOL:.3f} of the bar")
    assert worst <= R.NORMALS_ATOL


def test_normals64_moments_and_layout():
    z = R.normals64(2 ** 63 + 5, 2 ** 40 + 3, np.arange(2 ** 18))
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.var() - 1) < 5 * np.sqrt(2 / z.size)
    # arbitrary indices: any subset, any order, equals the dense field
    idx = np.array([2 ** 18 - 1, 0, 5, 4, 7, 6, 1023], dtype=np.int64)
    assert np.array_equal(R.normals64(2 ** 63 + 5, 2 ** 40 + 3, idx), z[idx])
    # a block index beyond 2^32 uses the second counter word
    hi = np.array([4 * 2 ** 32 + 1], dtype=np.uint64)
    assert R.normals64(1, 2, hi)[0] != R.normals64(1, 2, hi & np.uint64(0xFFFFFFFF))[0]


@pytest.mark.parametrize("key", R.RANDN_KEYS, ids=lambda k: f"{k[0]:#x}-{k[1]:#x}")
def test_normals_mutations_show(key):
    """Swapped lanes, a swapped counter, the high words of key or stream dropped: each is beyond the bar on the indices the GPU
    test compares (where the mutation changes anything at all: the all-zero key has no high words to drop)."""
    seed, stream = key
    for n in (5, 1023):
        idx = R.sample_indices(n)
        ref = R.normals64(seed, stream, idx)
        far = lambda other: np.abs(other - ref).max() > 100 * R.NORMALS_ATOL  # noqa: E731
        assert far(R.normals64(seed, stream, idx, lanes=(1, 0, 2, 3)))
        assert far(R.normals64(seed, stream, idx, lanes=(0, 1, 3, 2)))
        if n > 5 or stream:
            assert far(R.normals64(seed, stream, idx, swap_counter=True))
        if seed >> 32:
            assert far(R.normals64(seed & 0xFFFFFFFF, stream, idx))
        if stream >> 32:
            assert far(R.normals64(seed, stream & 0xFFFFFFFF, idx))
        assert far(R.normals64(seed, stream + 1, idx)) and far(R.normals64(seed ^ 1, stream, idx))
        assert far(R.normals64(seed, stream, idx + 4))  # the neighbouring block


# ---- GMM ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntab", [1, 50, 256])
def test_gmm32_against_oracle(ntab):
    mus, sigmas = R.gmm_tables(ntab)
    for n in (1, 9, 257, 1025):
        lab = R.gmm_labels(n, ntab, False).astype(np.int64) % ntab  # in range: what the oracle's gather accepts
        z = R.gmm_noise(n)
        want = O.gmm_image(torch.from_numpy(lab.astype(np.uint8)), torch.from_numpy(mus), torch.from_numpy(sigmas), torch.from_numpy(z))
        got = R.gmm32(lab, mus, sigmas, ntab, z)
        assert np.array_equal(bits(got), bits(want.numpy())), (ntab, n)
        assert not np.signbit(got).any()


def test_gmm32_edges_and_mutations():
    for ntab in (1, 50, 256):
        mus, sigmas = R.gmm_tables(ntab)
        for i64 in (False, True):
            n = 257
            lab, z = R.gmm_labels(n, ntab, i64), R.gmm_noise(n)
            ref = R.gmm32(lab, mus, sigmas, ntab, z)
            wide = np.asarray(lab, dtype=np.int64)
            beyond = np.clip(wide, 0, 255) >= ntab
            assert (bits(ref[beyond]) == 0).all() and (beyond.any() or ntab == 256)  # beyond the table: +0, sign bit clear
            assert (ref[z == F(-60.0)] == 0).all() and not np.signbit(ref).any()
            if ntab > 1:
                assert not np.array_equal(ref, R.gmm32(lab, mus, sigmas, ntab, z, label_offset=1))
                assert not np.array_equal(ref, R.gmm32(lab, mus, sigmas, ntab - 1, z))  # the table one entry short
            if i64 and ntab > 4:
                # the defect this suite was written against: narrowing to 32 bits before the clamp
                narrowed = wide.astype(np.int32).astype(np.int64)
                assert not np.array_equal(ref, R.gmm32(narrowed, mus, sigmas, ntab, z))
                assert 2 ** 32 + 3 in wide and -2 ** 40 in wide and 2 ** 63 - 1 in wide
    # the clamp at 255 is visible only with a full table
    mus, sigmas = R.gmm_tables(256)
    assert R.gmm32(np.array([2 ** 63 - 1, 256]), mus, sigmas, 256, np.zeros(2, F)).tolist() == [mus[255], mus[255]]
    assert R.gmm32(np.array([-1, -2 ** 40]), mus, sigmas, 256, np.ones(2, F)).tolist() == [sigmas[0], sigmas[0]]


def test_parts_and_codes_labels():
    rs = np.random.RandomState(4)
    lab = R.gmm_labels(1024, 50, False)
    for nparts in (1, 2, 3, 4):
        parts = R.split_parts(lab, nparts, rs)
        assert np.array_equal(R.parts_label(parts), lab)
        if nparts > 1:
            assert not np.array_equal(R.parts_label(parts[:-1]), lab)  # mutation: a part left out
            holes = [parts[0], None] + parts[2:] + [parts[1]]           # an absent volume in the middle
            assert np.array_equal(R.parts_label(holes), lab)
    a, b = np.array([200, 7], np.uint8), np.array([100, 0], np.uint8)
    assert R.parts_label([a, None, b]).tolist() == [44, 7]              # byte-wise: modulo 256
    tuples = rs.randint(0, 60, (37, 25)).astype(np.uint8)
    tuples[:, 24] = 0                                                   # the zero column
    codes = rs.randint(0, 37, 4096)
    for sel in ((0, 5, 9, 13), (3, 3, 24, 24), (24, 24, 24, 24), (7, 7, 7, 7)):
        want = np.array([(int(tuples[c, sel[0]]) + int(tuples[c, sel[1]]) + int(tuples[c, sel[2]]) + int(tuples[c, sel[3]])) % 256
                         for c in codes], np.uint8)
        assert np.array_equal(R.codes_label(codes, tuples, sel), want)
    assert not R.codes_label(codes, tuples, (24, 24, 24, 24)).any()
    assert not np.array_equal(R.codes_label(codes, tuples, (0, 5, 9, 13)), R.codes_label(codes, tuples, (0, 5, 9, 14)))


# ---- pointwise stages ---------------------------------------------------------------------------------------------------------------------
def test_add_noise32_against_torch():
    for n in (1, 5, 257):
        rs = np.random.RandomState(n)
        x, z = (rs.rand(n) * 255).astype(F), R.gmm_noise(n)
        for std in (0.0, 0.5, 40.0):
            t = torch.from_numpy(x) + torch.tensor(std, dtype=torch.float32) * torch.from_numpy(z)
            want = torch.where(t < 0, torch.zeros_like(t), t).numpy()
            got = R.add_noise32(x, std, z)
            assert np.array_equal(bits(got), bits(want)), (n, std)
            if std and n > 1:
                assert not np.array_equal(got, R.add_noise32(x, std, np.roll(z, 1)))  # mutation: the neighbour's normal
    assert bits(R.add_noise32([1.0], 40.0, [-60.0]))[0] == 0


def same64(a, b):
    """Two float64 evaluations of one formula by numpy and by torch: their pow / exp may differ in the last bits of a double
    (64 ulp = 1.4e-14 relative allowed, eight orders below the GPU test's tolerance)."""
    return bool((np.abs(a - b) <= 64 * 2.0 ** -53 * np.abs(b)).all())


def test_gamma64_bias64_against_torch():
    for g in (np.exp(-0.5), 1.0, np.exp(0.5)):
        x = R.gamma_inputs(257)
        gf = float(F(g))
        want = 300.0 * (torch.from_numpy(x).double() / 300.0) ** gf
        assert same64(R.gamma64(x, g), want.numpy())
        assert R.gamma64(np.zeros(3, F), g).tolist() == [0, 0, 0]
        neg = R.gamma64(np.array([-1.0, -255.0], F), g)
        assert np.isnan(neg).all() if g != 1.0 else neg.tolist() == [-1.0, -255.0]
        if g != 1.0:
            assert np.abs(R.gamma64(x, g) - R.gamma64(x, g * (1 + 1e-3))).max() > 0.01  # mutation: far beyond ATOL
    rs = np.random.RandomState(3)
    shape, bshape = (5, 4, 7), (2, 3, 4)
    x, bias = (rs.rand(*shape) * 255).astype(F), (rs.randn(*bshape) * 0.3).astype(F)
    tabs, new = T.zoom_tables(bshape, np.array(shape) / np.array(bshape))
    assert new == shape
    b = torch.from_numpy(bias).double()
    for axis, tab in enumerate(tabs):  # x, then y, then z: w_lo * a + w_hi * b through the table entries
        lo, hi = torch.from_numpy(tab["lo"].astype(np.int64)), torch.from_numpy(tab["hi"].astype(np.int64))
        view = [1, 1, 1]
        view[axis] = -1
        wl, wh = torch.from_numpy(tab["w_lo"].astype(np.float64)).view(view), torch.from_numpy(tab["w_hi"].astype(np.float64)).view(view)
        b = wl * b.index_select(axis, lo) + wh * b.index_select(axis, hi)
    want = torch.from_numpy(x).double() * torch.exp(b)
    got = R.bias64(x, bias, tabs)
    assert same64(got, want.numpy())
    assert np.abs(got - R.bias64(x, bias[::-1].copy(), tabs)).max() > 1.0  # mutation: the grid mirrored on one axis


# ---- label statistics -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", R.STATS_PATTERNS)
def test_label_sums_bound(pattern):
    worst = [0.0, 0.0]
    for n in R.STATS_N:
        for nlabels in (1, 50, 256):
            for signed in (0, 1):
                l, v = R.stats_inputs(n, pattern, nlabels, signed)
                cnt, s1, s2 = R.label_sums64(l, v, nlabels)
                b1, b2 = R.label_sums_bound(l, v, nlabels)
                assert cnt.sum() == (l < nlabels).sum() and (b1[cnt > 0] > 0).all() and (b1[cnt == 0] == 0).all()
                g1, g2 = R.label_sums32(l, v, nlabels, np.random.RandomState(n))
                assert (np.abs(g1 - s1) <= b1).all() and (np.abs(g2 - s2) <= b2).all(), (n, nlabels, signed)
                for k, (g, s, b) in enumerate(((g1, s1, b1), (g2, s2, b2))):
                    if (b > 0).any():
                        worst[k] = max(worst[k], float((np.abs(g - s)[b > 0] / b[b > 0]).max()))
                if cnt.sum() > 1:
                    d1, d2 = R.label_sums32(l, v, nlabels, np.random.RandomState(n), drop_one_per_block=True)
                    assert (np.abs(d1 - s1) > b1).any() and (np.abs(d2 - s2) > b2).any(), (n, nlabels, signed)
    print(f"BOUND label_sums float32 restatement [{pattern}]: {worst[0]:.3f} / {worst[1]:.3f} of the bounds (sum / sum of squares)")


def test_label_stats_inputs_reach_the_peel_loop():
    """What the GPU test relies on: 64 distinct labels in one wave, one label in every lane, labels >= nlabels beside valid ones,
    partial last waves and workgroups."""
    l, _v = R.stats_inputs(4097, "lanes64", 256, 0)
    assert all(len(set(l[w:w + 64])) == 64 for w in range(0, 4096, 64))
    l, _v = R.stats_inputs(4097, "one", 50, 0)
    assert len(set(l)) == 1
    l, _v = R.stats_inputs(4097, "all256", 256, 0)
    assert len(set(l)) == 256
    for nlabels in (1, 50, 256):
        l, _v = R.stats_inputs(255, "mixed", nlabels, 0)
        first = l[:64].astype(int)
        assert 255 in first and (first < nlabels).any() and ((first >= nlabels).any() or nlabels == 256)
    l, _v = R.stats_inputs(3 * 4096 + 1, "runs", 50, 0)
    assert (l >= 50).any() and (np.diff(l.astype(int)) == 0).mean() > 0.9
    # a label shifted by one is visible in the counts
    l, v = R.stats_inputs(4097, "runs", 50, 0)
    assert not np.array_equal(R.label_sums64(l, v, 50)[0], R.label_sums64((l.astype(int) + 1) % 256, v, 50)[0])


def test_minmax_identities():
    k = R.minmax_identities(2, 1)
    assert k.view(np.uint32).tolist() == [0x7F800000, 0x7F800000, 0xFF800000 ^ 0x7FFFFFFF]


# ---- the wrappers' table check (no GPU: the check comes before anything that needs one) -----------------------------------------------------
def test_gmm_wrappers_refuse_mismatched_tables():
    """kernels.gmm_sample_parts and kernels.sample_head are told ONE table length and read both tables that far: a shorter
    `sigmas` would be read past its end.  ValueError on the host, before the device check and any launch."""
    from fetalsyngen_amd import kernels as K

    part = torch.zeros(2, 2, 4, dtype=torch.uint8)
    for nm, ns in ((50, 49), (49, 50), (0, 0), (257, 257), (1, 2)):
        mus, sigmas = torch.zeros(nm), torch.zeros(ns)
        with pytest.raises(ValueError, match="mus/sigmas"):
            K.gmm_sample_parts([part], mus, sigmas)
        with pytest.raises(ValueError, match="mus/sigmas"):
            K.sample_head([part], mus, sigmas, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # equal lengths: on to the device check, as before
        K.gmm_sample_parts([part], torch.zeros(50), torch.zeros(50))
