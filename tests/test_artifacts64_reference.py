"""CPU: the float64 reference of the artifact / reduction kernels (tests/util_artifacts64.py) is right.

  * against the recorded output of the reference for one operation alone (tests/golden/sr_units.npz: MoG a / b / c, Perlin
    p1..p3, the scanner's gamma / noise / void stacks, replaying the draws of `Scanner`), at the tolerances of
    tests/test_oracle_sr.py and tests/test_sr_stages.py, and against oracle/fsg_oracle_sr.py on random small inputs;
  * brute-force distance == ball convolution == repeated cross dilations == the separable form;
  * each `*_bound` is not tighter than an honest float32 evaluation in the reference's operation order (>= 10^5 elements per
    operation), and not vacuous: with one input moved by 4 ulp the float32 result leaves it;
  * the near-tie census of the random `boundary_mask` case stays under its cap.
"""
import numpy as np
import pytest
import torch

from oracle import fsg_oracle_sr as S
from tests import util_artifacts64 as R
from tests.util_artifact_cases import NEAR_TIE_CAP, boundary_random_inputs, mog_cases, perlin_octaves

F = np.float32


def ulps(x, k):
    """x moved by k float32 ulps."""
    x = np.asarray(x, F).copy()
    return (x.view(np.int32) + np.int32(k)).view(F)


def lattice(res, seed):
    g = np.random.RandomState(seed).randn(res[0] + 1, res[1] + 1, res[2] + 1, 3)
    g /= np.linalg.norm(g, axis=-1, keepdims=True)
    g[-1], g[:, -1], g[:, :, -1] = g[0], g[:, 0], g[:, :, 0]
    return g.astype(F)


def lins(shape, res):
    return [torch.linspace(0, res[i], shape[i]).numpy() for i in range(3)]


# ---- recorded reference output ------------------------------------------------------------------------------------------
def test_mog_pinned(golden):
    g = golden("sr_units")
    c = g["mog_centers"]
    for sig, tag in ((np.full((3, 3), 4.0), "mog_a"), (g["mog_sig"], "mog_b"),
                     (np.array([[6.0] * 3, [2.0] * 3, [11.0] * 3]), "mog_c")):
        np.testing.assert_allclose(R.mog64((24, 20, 28), c, sig), g[tag], atol=1e-6)


@pytest.mark.parametrize("tag", ["p1", "p2", "p3"])
def test_perlin_pinned(golden, tag):
    g = golden("sr_units")
    cfg = g[f"perlin_{tag}_cfg"]
    shape, res, octv, inc = tuple(int(v) for v in cfg[:3]), int(cfg[3]), int(cfg[4]), float(cfg[5])
    torch.manual_seed(17)
    octs, f, a = [], 1, 1.0
    for _ in range(octv):
        r = (f * res,) * 3
        octs.append((S.perlin_lattice(r).numpy(), lins(shape, r), r, a))
        f, a = f * 2, a * 0.5
    raw, mn, mx = R.perlin_fractal64(shape, octs)
    assert mn == raw.min() and mx == raw.max()
    np.testing.assert_allclose(R.perlin_normalise64(raw, inc), g[f"perlin_{tag}"], atol=2e-6)


def test_scanner_corruptions_pinned(golden):
    """The draws of Scanner.random_gamma / add_noise / signal_void (simulate_reco.py:210-298) replayed from the seeds of the
    fixture; tolerances of tests/test_sr_stages.py."""
    g = golden("sr_units")
    np.random.seed(21)
    torch.manual_seed(22)
    assert np.random.rand() < 1.0
    gamma = np.exp(0.05 * np.random.randn(1)[0])
    s = 300.0 * (R.f64(g["slices_in"]) / 300.0) ** gamma
    mn, mx = R.minmax64(s.astype(F))
    np.testing.assert_allclose(R.scale64(s.astype(F), mn, mx, 0), g["slices_gamma"], atol=2e-5)
    sigma = np.random.uniform(0.0, 0.1)
    s1 = g["slices_gamma"]
    mask = s1.reshape(-1) > F(0.1)  # Scanner.slice_noise_threshold
    z = np.zeros((2, mask.size), F)
    z[0, mask] = torch.randn(int(mask.sum())).numpy()
    z[1, mask] = torch.randn(int(mask.sum())).numpy()
    np.testing.assert_allclose(R.rician64(s1, 0.1, sigma, z[0].reshape(s1.shape), z[1].reshape(s1.shape)), g["slices_noise"],
                               atol=2e-6)
    s2 = g["slices_noise"]
    n, h, w = s2.shape[0], s2.shape[-2], s2.shape[-1]
    idx = torch.rand(n) < 0.5
    nv = int(idx.sum())
    assert nv > 0
    y, x = torch.linspace(-(h - 1) / 2, (h - 1) / 2, h), torch.linspace(-(w - 1) / 2, (w - 1) / 2, w)
    yc, xc = (torch.rand(nv) - 0.5) * (h - 1), (torch.rand(nv) - 0.5) * (w - 1)
    th = 2 * np.pi * torch.rand((nv, 1, 1))
    a = 30 + torch.rand_like(th) * 90
    A = torch.rand_like(th) * 0.5 + 0.5
    sx = torch.rand_like(th) * 30 + 39
    sy = a ** 2 / sx
    par = torch.stack([yc, xc, torch.cos(th).view(-1), torch.sin(th).view(-1), A.view(-1), (-0.5 / sx ** 2).view(-1),
                       (-0.5 / sy ** 2).view(-1)], 1).float().numpy()
    out = R.void64(s2.reshape(n, h, w), torch.nonzero(idx).view(-1).tolist(), par, y.numpy(), x.numpy())
    np.testing.assert_allclose(out.reshape(s2.shape), g["slices_void"], atol=2e-6)


# ---- the oracle on random small inputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_against_oracle(seed):
    rs = np.random.RandomState(seed)
    shape = (int(rs.randint(2, 9)), int(rs.randint(2, 9)), int(rs.randint(2, 40)))
    k = int(rs.randint(1, 6))
    c, sg = (rs.rand(k, 3) * 30 - 5).astype(F), (0.5 + rs.rand(k, 3) * 6).astype(F)
    np.testing.assert_allclose(R.mog64(shape, c, sg), S.mog3d(shape, c, sg).numpy(), atol=1e-6)
    res = (int(rs.randint(1, 4)), int(rs.randint(1, 4)), int(rs.randint(1, 4)))
    g = lattice(res, seed)
    np.testing.assert_allclose(R.perlin_octave64(shape, res, g, lins(shape, res)),
                               S.perlin_octave(shape, res, torch.from_numpy(g)).numpy(), atol=2e-6)
    r1 = (res[0],) * 3
    lat = [torch.from_numpy(lattice((r1[0] * 2 ** q,) * 3, seed + q)) for q in range(3)]
    octs = [(lat[q].numpy(), lins(shape, (r1[0] * 2 ** q,) * 3), (r1[0] * 2 ** q,) * 3, 0.5 ** q) for q in range(3)]
    norm, raw = S.fractal_noise(shape, r1[0], 3, 0.5, 2, 0.1, lattices=lat)
    v, _mn, _mx = R.perlin_fractal64(shape, octs)
    np.testing.assert_allclose(v, raw.numpy(), atol=4e-6)
    np.testing.assert_allclose(R.perlin_normalise64(raw.numpy(), 0.1), norm.numpy(), atol=2e-6)
    s = (rs.rand(5, 6, 7) * (rs.rand(5, 6, 7) > 0.3)).astype(F)
    z1, z2 = rs.randn(5, 6, 7).astype(F), rs.randn(5, 6, 7).astype(F)
    np.testing.assert_allclose(R.rician64(s, 0.25, 0.07, z1, z2), S.rician(s, 0.25, 0.07, z1, z2).numpy(), atol=1e-6)
    m = (rs.rand(*shape) > 0.5).astype(F)
    np.testing.assert_allclose(R.box_sum64(m, 3) / 27.0, S.box_mean3(m).numpy(), atol=1e-6)


# ---- distances ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1, 2, 3, 4])
def test_distance_forms_agree(r):
    rs = np.random.RandomState(r)
    for mask in (rs.rand(9, 7, 11) < 0.02, rs.rand(9, 7, 11) < 0.3, np.zeros((9, 7, 11), bool)):
        mask = mask.copy()
        if mask.any() or r == 0:
            mask[0, 0, 0] = mask.any()
        e, l = R.distance_brute64(mask, r, "euclid2"), R.distance_brute64(mask, r, "l1")
        assert np.array_equal(e <= r * r, R.ball_dilate64(mask, r))
        assert np.array_equal(l <= r, R.cross_dilate64(mask, r))
        assert np.array_equal(R.distance_separable64(mask, r, "euclid2"), e)
        assert np.array_equal(R.distance_separable64(mask, r, "l1"), l)


# ---- the bounds: not tighter than honest float32, not vacuous -----------------------------------------------------------------
def mog32(shape, c, s):
    return S.mog3d(shape, c, s).numpy()


def test_mog_bound():
    rs = np.random.RandomState(4)
    shape = (24, 20, 210)  # 100800 voxels
    c, s = (rs.rand(7, 3) * [210, 20, 24]).astype(F), (0.5 + rs.rand(7, 3) * 30).astype(F)
    ref, b = R.mog64(shape, c, s), R.mog_bound(shape, c, s)
    assert (np.abs(mog32(shape, c, s) - ref) <= b).all()
    c2 = c.copy()
    c2[1, 0] = ulps(c[1, 0], 4)
    assert (np.abs(mog32(shape, c2, s) - ref) > b).any()


def test_perlin_bound():
    shape, res = (24, 20, 210), (3, 2, 16)
    g = lattice(res, 8)
    ln = lins(shape, res)
    ref, b = R.perlin_octave64(shape, res, g, ln), R.perlin_octave_bound(shape, res, g, ln)
    got = S.perlin_octave(shape, res, torch.from_numpy(g)).numpy()
    assert (np.abs(got - ref) <= b).all()
    assert b.max() < 256 * R.U32  # the fade's own error times a corner difference of O(1) dominates; no tolerance in disguise
    ln2 = [ln[0], ln[1], ulps(ln[2], 4)]  # the oracle builds its own axes: the moved input goes through the restatement
    assert (np.abs(R.perlin_octave64(shape, res, g, ln2).astype(F) - ref) > b).any()


def blend32(a, b, w, w_mm=None, inc=0.0, seg=None, std=None, b_mm=None, a_mm=None):
    a, b, w = F(a), F(b), F(w)
    if w_mm is not None:
        w = np.clip((w + F(inc) - F(w_mm[0])) / (F(w_mm[1]) - F(w_mm[0])), F(0), F(1))
    if seg is not None:
        w = (seg > 0).astype(F) * w
    if std is not None:
        sc = max(abs(F(b_mm[0])), abs(F(b_mm[1])))
        b = np.clip(a + F(std) * (b / sc), F(0), F(a_mm[1]) * F(2))
    return (F(1) - w) * a + w * b, w


@pytest.mark.parametrize("wm", [0, 1])
@pytest.mark.parametrize("bm", [0, 1])
def test_blend_bound(wm, bm):
    rs = np.random.RandomState(wm * 2 + bm)
    n = 100003
    a, b = (rs.rand(n) * 200).astype(F), (rs.randn(n) * 50).astype(F)
    w = (rs.rand(n) * 1.6 - 0.3).astype(F) if wm else rs.rand(n).astype(F)
    seg = (rs.rand(n) > 0.2).astype(F)
    kw = dict(seg=seg)
    if wm:
        kw.update(w_mm=R.minmax64(w), increase=0.15)
    if bm:
        kw.update(noise_std=7.5, b_mm=R.minmax64(b), a_mm=R.minmax64(a))
    (ro, rw), (bo, bw) = R.blend64(a, b, w, **kw), R.blend_bound(a, b, w, **kw)
    go, gw = blend32(a, b, w, kw.get("w_mm"), kw.get("increase", 0.0), seg, kw.get("noise_std"), kw.get("b_mm"), kw.get("a_mm"))
    assert (np.abs(go - ro) <= bo).all() and (np.abs(gw - rw) <= bw).all()
    go2, _ = blend32(ulps(a, 4), b, w, kw.get("w_mm"), kw.get("increase", 0.0), seg, kw.get("noise_std"), kw.get("b_mm"),
                     kw.get("a_mm"))
    assert (np.abs(go2 - ro) > bo).any()


def test_rician_void_sums_scale_bounds():
    rs = np.random.RandomState(9)
    s = (rs.rand(6, 130, 131) * (rs.rand(6, 130, 131) > 0.3)).astype(F)
    z1, z2 = rs.randn(*s.shape).astype(F), rs.randn(*s.shape).astype(F)
    ref, b = R.rician64(s, 0.2, 0.07, z1, z2), R.rician_bound(s, 0.2, 0.07, z1, z2)
    f32 = lambda s_, z_: np.where(s_ > F(0.2), np.sqrt((s_ + z_ * F(0.07)) ** 2 + (z2 * F(0.07)) ** 2), s_)  # noqa: E731
    assert f32(s, z1).dtype == F and (np.abs(f32(s, z1) - ref) <= b).all()
    assert (np.abs(f32(ulps(s, 4), z1) - ref) > b).any()

    ids = [4, 0, 3]
    par = np.array([[3.5, -7.25, np.cos(0.7), np.sin(0.7), 0.8, -0.5 / 45.0 ** 2, -0.5 / 80.0 ** 2],
                    [-200.0, 10.0, np.cos(2.9), np.sin(2.9), 0.55, -0.5 / 60.0 ** 2, -0.5 / 30.0 ** 2],
                    [0.0, 0.0, 1.0, 0.0, 1.0, -0.5 / 39.0 ** 2, -0.5 / 39.0 ** 2]], F)
    yl, xl = np.linspace(-64.5, 64.5, 130).astype(F), np.linspace(-65, 65, 131).astype(F)
    ref, b = R.void64(s, ids, par, yl, xl), R.void_bound(s, ids, par, yl, xl)

    def void32(sl):
        out = sl.copy()
        for t, i in enumerate(ids):
            p = par[t]
            y, x = yl[:, None] - p[0], xl[None, :] - p[1]
            xr, yr = p[2] * x - p[3] * y, p[3] * x + p[2] * y
            out[i] *= F(1) - p[4] * np.exp(p[5] * (xr * xr) + p[6] * (yr * yr))
        return out

    assert void32(s).dtype == F and (np.abs(void32(s) - ref) <= b).all()
    assert (b[[1, 2, 5]] == 0).all() and (np.abs(void32(ulps(s, 4)) - ref) > b).any()

    big = (rs.rand(3, 320 * 320) * 1000).astype(F)
    ref, b = R.slice_sums64(big), R.slice_sums_bound(big)
    assert (np.abs(big.astype(np.float64).sum(1).astype(F) - ref) <= b).all()
    assert (np.abs(ulps(big.astype(np.float64).sum(1).astype(F), 4) - ref) > b).all()  # the rounded sum moved by 4 ulp leaves it

    x = (rs.randn(100003) * 300 + 20).astype(F)
    mn, mx = R.minmax64(x)
    for mode in (0, 1, 2):
        ref, b = R.scale64(x, mn, mx, mode), R.scale_bound(x, mn, mx, mode)
        got = x / F(mx) if mode == 0 else ((x - F(mn)) / (F(mx) - F(mn)) * (F(255) if mode == 2 else F(1)))
        assert got.dtype == F and (np.abs(got - ref) <= b).all()
        x4 = ulps(x, 4)
        got4 = x4 / F(mx) if mode == 0 else ((x4 - F(mn)) / (F(mx) - F(mn)) * (F(255) if mode == 2 else F(1)))
        assert (np.abs(got4 - ref) > b).any()
    assert (R.scale64(x[:1], x[0], x[0], 1) == 0).all() and (R.scale_bound(x[:1], x[0], x[0], 1) == 0).all()


# ---- the same two properties on the cases the GPU tests run -------------------------------------------------------------------------
def test_mog_bound_on_gpu_cases():
    """Every case of the GPU test: the float32 evaluation of the oracle stays within the bound.  Non-vacuity where a value is
    above the flush term: the first blob's sigmas moved by 4 ulp leave the bound on the 61 tail and on random cases; on the tails at
    170 and 176 the values are below 2e-37 and the bound is the absolute flush term 2^-126 itself."""
    left = {}
    for name, (shape, c, s) in mog_cases().items():
        ref, b = R.mog64(shape, c, s), R.mog_bound(shape, c, s)
        assert (np.abs(mog32(shape, c, s) - ref) <= b).all(), name
        s2 = s.copy()
        s2[0] = ulps(s[0], 4)
        left[name] = bool((np.abs(mog32(shape, c, s2) - ref) > b).any())
    assert left["tail61.0"] and any(v for k, v in left.items() if k.startswith("(")), left


def perlin32(shape, octs):
    """The fractal sum in float32 numpy, in the reference's operation order (utils.py:255-327, :375-384)."""
    v = np.zeros(shape, F)
    for g, lins, r, amp in octs:
        g = np.asarray(g, F)
        lin = [np.asarray(t, F) for t in lins]
        cell = [np.floor(t) for t in lin]
        L = np.meshgrid(*[t - c_ for t, c_ in zip(lin, cell)], indexing="ij")
        idx = [[np.minimum(c_.astype(np.int64) + d, r[a]) for d in (0, 1)] for a, c_ in enumerate(cell)]

        def corner(dx, dy, dz):
            gi = g[idx[0][dx][:, None, None], idx[1][dy][None, :, None], idx[2][dz][None, None, :]]
            return gi[..., 0] * (L[0] - F(dx)) + gi[..., 1] * (L[1] - F(dy)) + gi[..., 2] * (L[2] - F(dz))

        t = [x * x * x * (x * (x * F(6) - F(15)) + F(10)) for x in L]
        n00 = corner(0, 0, 0) * (F(1) - t[0]) + t[0] * corner(1, 0, 0)
        n10 = corner(0, 1, 0) * (F(1) - t[0]) + t[0] * corner(1, 1, 0)
        n01 = corner(0, 0, 1) * (F(1) - t[0]) + t[0] * corner(1, 0, 1)
        n11 = corner(0, 1, 1) * (F(1) - t[0]) + t[0] * corner(1, 1, 1)
        m0, m1 = n00 * (F(1) - t[1]) + t[1] * n10, n01 * (F(1) - t[1]) + t[1] * n11
        v = v + F(amp) * (m0 * (F(1) - t[2]) + t[2] * m1)
    assert v.dtype == F
    return v


@pytest.mark.parametrize("noct", [1, 8])
def test_perlin_fractal_bound_on_gpu_cases(noct):
    for n2 in (1, 63, 64, 65, 128, 129, 255, 256, 257):
        shape = (3, 5, n2)
        octs = [(g.numpy(), [v.numpy() for v in lins], r, a) for g, lins, r, a in perlin_octaves(shape, noct, n2)]
        ref, _mn, _mx = R.perlin_fractal64(shape, octs)
        b = R.perlin_fractal_bound(shape, octs)
        assert (np.abs(perlin32(shape, octs) - ref) <= b).all(), n2
        if n2 > 1:  # one axis table moved by 4 ulp: the float32 evaluation leaves the bound
            g, lins, r, a = octs[-1]
            moved = octs[:-1] + [(g, [lins[0], lins[1], ulps(lins[2], 4)], r, a)]
            assert (np.abs(perlin32(shape, moved) - ref) > b).any(), n2


# ---- exact operations: the restatements agree with numpy / torch idiom ---------------------------------------------------------
def test_voxel_set_and_ewise_restatements():
    rs = np.random.RandomState(2)
    v = (rs.rand(5, 6, 7) * (rs.rand(5, 6, 7) > 0.5)).astype(F)
    v[0, 0, 0], v[0, 0, 1] = np.nan, -0.0
    t = torch.from_numpy(v)
    assert np.array_equal(R.pred64(v, "!=", 0.0), (t != 0).numpy()) and R.pred64(v, "!=", 0.0)[0, 0, 0]
    assert not R.pred64(v, "!=", 0.0)[0, 0, 1] and R.pred64(v, "==", 0.0)[0, 0, 1]
    nz = torch.nonzero(t > 0).numpy()
    assert np.array_equal(R.rank_coords64(v, ">", 0.0, np.arange(len(nz))), nz)
    assert np.array_equal(R.compact64(v, v, ">", 0.0), t[t > 0].numpy())
    a, b = torch.randn(1000), torch.randn(1000)
    for op, want in (("add", a + b), ("mul", a * b), ("max", torch.maximum(a, b)), ("gt", (a > 0.25).float()),
                     ("le", (a <= 0.25).float()), ("eq", (a == float(a[3])).float()), ("mul_gt", a * (b > 0.25).float()),
                     ("sub_gt", ((a - b) > 0.25).float())):
        val = float(a[3]) if op == "eq" else 0.25
        assert np.array_equal(R.ewise64(op, a.numpy(), b.numpy(), val), want.numpy()), op
    assert np.array_equal(R.scatter64((2, 3), [0, 5, 5, -1, 6]), np.array([[1, 0, 0], [0, 0, 1]], F))
    x = np.array([np.nan, 3.0, -0.0, 0.0, -7.5], F)
    assert R.minmax64(x) == (-7.5, 3.0) and R.minmax64(x[:1]) == (np.inf, -np.inf)
    from oracle.fsg_keyed_draws import device_uniforms

    a = (rs.rand(1003) > 0.3).astype(F) * 2
    assert np.array_equal(R.bernoulli64(a, 0.4, 12345, 7), np.where(device_uniforms(12345, 7, 1003) < F(0.4), a, 0).astype(F))


# ---- boundary mask ----------------------------------------------------------------------------------------------------------
def test_boundary_reference_and_near_tie_census():
    """k = rint(p n - 1) in the reference's float32 (product rounded, then the subtraction) equals the float64 restatement
    away from the near-ties; n_dilate = 6 keeps p n below 8, where half an ulp of the product is 2^-22 = NEAR_TIE and the
    subtraction is exact, so the two can differ on near-ties only.  Their share stays under the cap."""
    kw = boundary_random_inputs()
    out, m, near = R.boundary64(**kw)
    assert near.mean() < NEAR_TIE_CAP
    p = np.where(kw["mask_modif"] - kw["mask"] > 0, kw["mog"], F(0))
    k32 = np.maximum(np.rint(p * F(6) - F(1)), 0)
    m32 = kw["mask_modif"] * (kw["dist"] <= np.maximum(k32 - 1, 0))
    assert np.array_equal(m32[~near], m[~near].astype(F))
    assert np.array_equal((kw["image"] * m32)[~near], out[~near].astype(F))
    # ties to even on exactly representable products (n = 12): p n - 1 = 0.5 -> 0, 3.5 -> 4, 6.5 -> 6
    one = np.ones(3, F)
    _o, m, near = R.boundary64(None, 0 * one, one, np.array([0.125, 0.375, 0.625], F), np.array([0, 4, 5], F), 12)
    assert near.all() and m.tolist() == [1.0, 0.0, 1.0]
