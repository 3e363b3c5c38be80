"""GPU: seed generation (csrc/fsg_seedgen.hip, fetalsyngen_amd/seedgen.py) at its edges, against the float64 restatement
tests/util_em64.py; the seed-code builder's one-voxel form against the torch formulation.

The cases are those of tests/util_seedgen_cases.py; tests/test_em64_edges_reference.py shows on the CPU that every one of them is
well-conditioned (a float32 evaluation as the kernels document it stays within a quarter of the bounds below), so a miss here is
a wrong kernel, not rounding.

Tolerances, by the rule of tests/test_seedgen_gpu.py.  Parameters: relative error where |reference| >= 1e-9, absolute error below
that floor (an empty component: weight ~2e-15 / n, mean 0); the bound is 4x the largest error measured on the MI355X over all
cases, init modes 0 and 1 and iteration counts 1 and 20, never above the caps 1e-5 (means, weights) / 1e-4 (variances).
Measured on gfx950 over the 77 cases: mode 0, 1 iteration: means 1.04e-8, weights 8.33e-8, variances 2.003e-6; mode 1, 1
iteration: 2.41e-8, 2.31e-7, 2.01e-7; mode 0, 20 iterations: 1.13e-7, 2.037e-6, 1.818e-6; mode 1, 20 iterations: 1.463e-7, 1.335e-6,
2.011e-6 (beside the fixture cases of test_seedgen_gpu.py: 1.144e-6, 2.416e-6, 2.761e-6).  Lower bound: |lb - reference| <=
16 * 2^-24 * max_i |lse_i| (every sample's mx + logf(sum) is a float32 value built from float32 terms of at most that size, then
averaged in float64); measured: at most 0.118 of that bound (a one-sample job; 0.026 over the jobs of 63 samples and more).  In
the whole-subject test: means 2.03e-8, weights 6.74e-7, variances 3.76e-7, |lb diff| 8.86e-8.  0 labels differ from the reference
in every assignment and whole-subject case.  Labels may differ from the reference only where its own gap between the two largest
weighted log-densities is below DELTA = 1e-4.
"""
import numpy as np
import pytest
import torch

from tests import util_em64 as E
from tests import util_seedgen_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DELTA = 1e-4
# largest errors seen on the MI355X (error measure of util_em64.param_error), and the largest |lb diff| as a share of its bound
MEASURED_MEAN, MEASURED_WEIGHT, MEASURED_VAR, MEASURED_LB = 1.463e-7, 2.037e-6, 2.011e-6, 0.118
TOL_MEAN = min(4 * MEASURED_MEAN, 1e-5)
TOL_WEIGHT = min(4 * MEASURED_WEIGHT, 1e-5)
TOL_VAR = min(4 * MEASURED_VAR, 1e-4)


@pytest.fixture(scope="module")
def sg():
    from fetalsyngen_amd import seedgen

    return seedgen


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_jobs(sg, xd, jobs, order=None):
    """jobs: dicts of `_Batch.add` arguments.  -> (the `_Fit`, params (nj, 3, 16), lower bounds, status) in the order given."""
    from fetalsyngen_amd import _lib

    batch = sg._Batch(_lib.load())
    for j in jobs:
        batch.add(**j)
    fit = sg._Fit(xd, batch, order)
    return (fit,) + fit.results()


def job(xoff, n, k, max_iter, mode, tol, init=None, mu=None):
    w, m, v = init if init is not None else (None, mu, None)
    return dict(xoff=xoff, n=n, k=k, max_iter=max_iter, mode=mode, tol=tol, w=w, mu=m, var=v)


# --------------------------------------------------------------------------------------------------------------------- a
def fuse_poisoned(sg, img, seg, annotation, pad=64):
    """`fsg_seed_meta_pack` into outputs poisoned beforehand (and `pad` slots longer than the volume)."""
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    table, clear = sg.meta_table(annotation)
    imgd, segd, tabd = dev(img), dev(seg), dev(table)
    n = imgd.numel()
    meta = torch.full(imgd.shape, 255, dtype=torch.uint8, device=DEV)
    counts = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    px = torch.full((n + pad,), float("nan"), dtype=torch.float32, device=DEV)
    pidx = torch.full((n + pad,), -1, dtype=torch.int32, device=DEV)
    work = torch.empty(max(int(lib.fsg_seed_meta_work_bytes(n)), 16), dtype=torch.uint8, device=DEV)
    u8 = segd.dtype == torch.uint8
    _lib.check(lib.fsg_seed_meta_pack(sg._p(segd) if u8 else None, None if u8 else sg._p(segd), sg._p(imgd), n, sg._p(tabd), clear,
                                      sg._p(meta), sg._p(counts), sg._p(px), sg._p(pidx), sg._p(work), sg._stream(imgd)), "fsg_seed_meta_pack")
    torch.cuda.synchronize()
    return meta.cpu().numpy(), counts.cpu().numpy().tolist(), px.cpu().numpy(), pidx.cpu().numpy()


FUSION = [(c, t) for c in SC.fusion_cases() for t in ("float32", "uint8") if t == "float32" or SC.as_uint8(c.seg) is not None]


@pytest.mark.parametrize("case,seg_dtype", FUSION, ids=[f"{c.name}-{t}" for c, t in FUSION])
def test_fusion_and_compaction_are_bit_exact(sg, case, seg_dtype):
    ann = SC.annotation_of(case)
    seg = case.seg if seg_dtype == "float32" else SC.as_uint8(case.seg)  # (the salted segmentation has no uint8 form)
    ref = E.meta_labels(case.image, seg, ann)
    meta, counts, px, pidx = fuse_poisoned(sg, case.image, seg, ann)
    assert np.array_equal(meta, ref)
    assert counts == [int((ref == m).sum()) for m in range(1, 5)]
    flat = np.arange(ref.size).reshape(ref.shape)
    off = 0
    for m in range(1, 5):
        assert np.array_equal(px[off: off + counts[m - 1]], E.packed(case.image, ref, m)), f"packed intensities of meta-label {m}"
        assert np.array_equal(pidx[off: off + counts[m - 1]], flat[ref == m]), f"packed indices of meta-label {m}"
        off += counts[m - 1]
    assert np.isnan(px[off:]).all() and (pidx[off:] == -1).all(), "a slot past the totals was written"
    # the public entry point hands out the same
    meta2, counts2, px2, pidx2 = sg.meta_pack(dev(case.image), dev(seg), ann)
    assert np.array_equal(meta2.cpu().numpy(), ref) and counts2 == counts
    assert np.array_equal(px2[:off].cpu().numpy(), px[:off]) and np.array_equal(pidx2[:off].cpu().numpy(), pidx[:off])


# --------------------------------------------------------------------------------------------------------------- b, c, d
@pytest.fixture(scope="module")
def parity(sg):
    """Every EM case x init mode x iteration count, once: {(name, mode, iters): (case, device fit, reference fit)}."""
    out = {}
    for c in SC.em_cases():
        xd = dev(c.x)
        for mode in SC.MODES:
            init = c.init0 if mode == 0 else E.init_from_means(c.x, c.mu0)
            for iters in SC.ITERS:
                ref = E.fit(c.x, *init, tol=0.0, max_iter=iters)
                j = job(0, c.x.size, c.k, iters, mode, 0.0, init=c.init0) if mode == 0 else job(0, c.x.size, c.k, iters, 1, 0.0, mu=c.mu0)
                _fit, params, lb, status = run_jobs(sg, xd, [j])
                got = dict(weights=params[0, 0, :c.k], means=params[0, 1, :c.k], variances=params[0, 2, :c.k], lower_bound=float(lb[0]),
                           n_iter=int(status[0, 0]), converged=bool(status[0, 1]), done=bool(status[0, 2]))
                out[(c.name, mode, iters)] = (c, got, ref)
    return out


def test_initial_m_step_counts_exactly(sg, parity):
    """Init mode 1 on integer data: the one-hot counts of the initial M-step, read from the weights after the one iteration that
    cannot change them (`integers_apart`), are integers and the reference's; a tie belongs to the lower index."""
    c, got, _ref = parity[("integers_apart_k3", 1, 1)]
    counts = got["weights"] * c.x.size
    want = np.rint(E.init_from_means(c.x, c.mu0)[0] * c.x.size)
    print(f"integers_apart: counts {counts.tolist()} (reference {want.tolist()})")
    assert np.abs(counts - np.rint(counts)).max() < 1e-9 and np.array_equal(np.rint(counts), want)
    assert want.tolist() == [1006.0, 1506.0, 2001.0]  # 1 000 / 1 500 / 2 000 draws + the centre itself; both ties to the lower index


@pytest.mark.parametrize("mode", SC.MODES)
@pytest.mark.parametrize("iters", SC.ITERS)
def test_fixed_iteration_parity(parity, mode, iters):
    worst = dict(means=0.0, weights=0.0, variances=0.0)
    at = dict(worst)
    for (name, m, it), (c, got, ref) in parity.items():
        if (m, it) != (mode, iters):
            continue
        assert got["n_iter"] == iters and not got["converged"] and got["done"], name
        e = {p: E.param_error(got[p], ref[p]) for p in worst}
        print(f"{name} mode {mode} iters {iters}: means {e['means']:.2e} weights {e['weights']:.2e} variances {e['variances']:.2e}")
        for p in worst:
            if e[p] > worst[p]:
                worst[p], at[p] = e[p], name
    print(f"mode {mode} iters {iters}: WORST means {worst['means']:.3e} ({at['means']}) weights {worst['weights']:.3e} ({at['weights']}) "
          f"variances {worst['variances']:.3e} ({at['variances']})")
    assert worst["means"] <= TOL_MEAN and worst["weights"] <= TOL_WEIGHT and worst["variances"] <= TOL_VAR, (worst, at)


@pytest.mark.parametrize("mode", SC.MODES)
@pytest.mark.parametrize("iters", SC.ITERS)
def test_lower_bound(parity, mode, iters):
    worst, at, bad = 0.0, "", []
    for (name, m, it), (_c, got, ref) in parity.items():
        if (m, it) != (mode, iters):
            continue
        diff, bound = abs(got["lower_bound"] - ref["lower_bound"]), E.lb_bound(ref["lse_absmax"])
        print(f"{name} mode {mode} iters {iters}: |lb diff| {diff:.3e} bound {bound:.3e} share {diff / bound:.3f}")
        if diff / bound > worst:
            worst, at = diff / bound, name
        if not diff <= bound:
            bad.append((name, diff, bound))
    print(f"mode {mode} iters {iters}: WORST |lb diff| / bound {worst:.3f} ({at})")
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------------------- e
def batch_plan():
    """One x, fourteen jobs: sizes on either side of a wave and a tile, k from 1 to 16, all three init modes, jobs that converge
    early beside jobs that run out of iterations, a job without samples in the middle and jobs that never start."""
    sizes = (1, 255, 4096, 4097, 3 * 4096 + 1)
    xs = [SC.mixture(n, 60 + i) for i, n in enumerate(sizes)]
    off = dict(zip(sizes, np.cumsum([0] + [x.size for x in xs[:-1]]).tolist()))   # odd offsets: no job but the first is aligned
    seg = dict(zip(sizes, xs))
    x = np.concatenate(xs)

    def j(n, k, max_iter, mode, tol):
        s = seg[n]
        if mode == 1:
            return job(off[n], n, k, max_iter, 1, tol, mu=SC.sample_centres(s, k))
        return job(off[n], n, k, max_iter, mode, tol, init=SC.given_init(s, k))

    big = 3 * 4096 + 1
    jobs = [j(1, 1, 1, 1, 0.0), j(255, 2, 40, 0, 1e-3), j(4096, 7, 40, 1, 1e-3), j(4097, 16, 3, 1, 0.0), j(big, 2, 40, 0, 1e-2),
            j(big, 16, 40, 1, 0.0), j(4096, 2, 1, 2, 0.0), job(off[255], 0, 1, 1, 1, 0.0), j(255, 7, 3, 0, 0.0), j(4097, 1, 40, 1, 1e-3),
            j(1, 2, 1, 0, 0.0), j(big, 7, 40, 0, 1e-3), j(4097, 2, 40, 1, 1e-3), j(255, 16, 3, 2, 0.0)]
    return x, jobs


def test_batch_independence(sg):
    x, jobs = batch_plan()
    xd = dev(x)
    nj = len(jobs)
    orders = [list(range(nj)), list(range(nj))[::-1], np.random.default_rng(5).permutation(nj).tolist()]
    runs = [run_jobs(sg, xd, jobs, order)[1:] for order in orders]
    alone = [run_jobs(sg, xd, [jb])[1:] for jb in jobs]
    params, lb, status = runs[0]
    for i, jb in enumerate(jobs):
        print(f"job {i}: n {jb['n']} k {jb['k']} mode {jb['mode']} max_iter {jb['max_iter']} tol {jb['tol']}: status {status[i].tolist()} lb {lb[i]}")
        for tag, (p2, lb2, st2) in (("reversed", runs[1]), ("shuffled", runs[2])):
            assert params[i].tobytes() == p2[i].tobytes() and lb[i].tobytes() == lb2[i].tobytes() and status[i].tobytes() == st2[i].tobytes(), (i, tag)
        p1, lb1, st1 = alone[i]
        assert params[i].tobytes() == p1[0].tobytes() and lb[i].tobytes() == lb1[0].tobytes() and status[i].tobytes() == st1[0].tobytes(), (i, "alone")
    n_iter, conv, done = status[:, 0], status[:, 1], status[:, 2]
    assert done.all()
    never = [i for i, jb in enumerate(jobs) if jb["mode"] == 2 or jb["n"] == 0]
    assert len(never) == 3 and (n_iter[never] == 0).all() and np.isneginf(lb[never]).all()
    for i in never:  # untouched: what the host handed in
        assert np.array_equal(params[i, 0, :jobs[i]["k"]], np.broadcast_to(jobs[i]["w"] if jobs[i]["w"] is not None else 1.0 / jobs[i]["k"], (jobs[i]["k"],)))
    early = [i for i in range(nj) if conv[i] and 1 < n_iter[i] < jobs[i]["max_iter"]]
    ran_out = [i for i in range(nj) if not conv[i] and n_iter[i] == jobs[i]["max_iter"] and i not in never]
    assert len(early) >= 3 and len(ran_out) >= 3, (early, ran_out)
    assert len(set(n_iter.tolist())) >= 5 and n_iter.max() == 40, n_iter.tolist()  # the early returns ran beside live jobs
    # and the batch computed the right thing: every live job against the reference from its own initialisation
    for i in early + ran_out:
        jb = jobs[i]
        xs = x[jb["xoff"]: jb["xoff"] + jb["n"]]
        init = (jb["w"], jb["mu"], jb["var"]) if jb["mode"] == 0 else E.init_from_means(xs, jb["mu"])
        ref = E.fit(xs, *init, tol=jb["tol"], max_iter=jb["max_iter"])
        assert ref["n_iter"] == n_iter[i] and ref["converged"] == bool(conv[i]), (i, ref["n_iter"], n_iter[i])
        k = jb["k"]
        assert E.param_error(params[i, 1, :k], ref["means"]) <= TOL_MEAN and E.param_error(params[i, 0, :k], ref["weights"]) <= TOL_WEIGHT
        assert E.param_error(params[i, 2, :k], ref["variances"]) <= TOL_VAR and abs(lb[i] - ref["lower_bound"]) <= E.lb_bound(ref["lse_absmax"])


# --------------------------------------------------------------------------------------------------------------------- f
def test_assignment_of_several_winners(sg):
    cases = SC.assign_cases()
    offs = np.cumsum([0] + [c.x.size for c in cases]).tolist()
    x = np.concatenate([c.x for c in cases])
    given = [job(offs[i], c.x.size, c.mu.size, 1, 2, 0.0, init=(c.w, c.mu, c.var)) for i, c in enumerate(cases)]
    # four more jobs on the same samples that win nothing
    losers = [job(offs[1], cases[1].x.size, 5, 2, 1, 0.0, mu=SC.sample_centres(cases[1].x, 5)),
              job(offs[0], cases[0].x.size, 3, 2, 0, 0.0, init=SC.given_init(cases[0].x, 3)),
              job(offs[3], cases[3].x.size, 2, 1, 2, 0.0, init=SC.given_init(cases[3].x, 2)),
              job(offs[2], cases[2].x.size, 16, 1, 0, 0.0, init=SC.given_init(cases[2].x, 16))]
    jobs = [losers[0], given[2], losers[1], given[0], given[3], losers[2], losers[3], given[1]]
    winner_rows = {2: 1, 0: 3, 3: 4, 1: 7}  # assignment case -> row of `jobs`
    xd = dev(x)
    fit = run_jobs(sg, xd, jobs, order=[3, 0, 7, 5, 1, 6, 2, 4])[0]
    nvox = x.size + 1500
    pidx = np.random.default_rng(9).permutation(nvox)[: x.size].astype(np.int32)  # packed sample -> voxel, with gaps
    vols = [torch.zeros(nvox, dtype=torch.uint8, device=DEV) for _ in range(8)]
    wins = [(winner_rows[i], vols[winner_rows[i]], cases[i].base) for i in (3, 0, 1, 2)]  # not in job order
    fit.assign(dev(pidx), wins)
    for i, c in enumerate(cases):
        vol = vols[winner_rows[i]].cpu().numpy()
        mine = pidx[offs[i]: offs[i + 1]]
        want, gap = E.predict(c.x, c.w, c.mu, c.var)
        diff = vol[mine] != (want.astype(np.int64) + c.base)
        print(f"{c.name}: {int(diff.sum())} of {c.x.size} labels differ; {int((gap < DELTA).sum())} samples with gap < {DELTA}")
        assert not (diff & ~(gap < DELTA)).any(), c.name
        rest = np.ones(nvox, bool)
        rest[mine] = False
        assert (vol[rest] == 0).all(), f"{c.name}: a voxel outside the winner's own range was written"
    assert (cases[1].base, cases[1].mu.size) == (240, 16) and int(vols[7].max()) == 255
    for r in set(range(8)) - set(winner_rows.values()):
        assert int(vols[r].max()) == 0, f"volume of job {r}, which won nothing, was written"


# --------------------------------------------------------------------------------------------------------------------- g
def test_whole_subject_at_the_edges(sg):
    """One absent, one 3-voxel, one constant and one ordinary meta-label through `generate_seeds` at 16 subclasses, against a host
    restatement from the product's own k-means++ draws (a pure host function) and the float64 EM."""
    key, kmax, n_init = 3, 16, 2
    img, seg = SC.edge_subject()
    meta = E.meta_labels(img, seg, "feta")
    counts = [int((meta == m).sum()) for m in range(1, 5)]
    assert counts[1] == 3 and counts[3] == 0 and np.unique(img[meta == 3]).size == 1 and counts[0] > 1000
    imgd, segd = dev(img), dev(seg)
    seeds, fits = sg.generate_seeds(imgd, segd, max_subclasses=kmax, annotation="feta", key=key, n_init=n_init, return_fits=True)
    again, fits2 = sg.generate_seeds(imgd, segd.float(), max_subclasses=kmax, annotation="feta", key=key, n_init=n_init, return_fits=True)
    assert sorted(seeds) == list(range(1, kmax + 1)) and sorted(fits) == sorted(fits2)
    for k in seeds:
        assert sorted(seeds[k]) == [1, 2, 3, 4]
        for m in seeds[k]:
            assert torch.equal(seeds[k][m], again[k][m]), (k, m)
    for mk, f in fits.items():
        assert all(np.asarray(f[p]).tobytes() == np.asarray(fits2[mk][p]).tobytes() for p in f), mk
    for m in range(1, 5):
        x = E.packed(img, meta, m)
        for k in range(1, kmax + 1):
            v = seeds[k][m].cpu().numpy()
            assert v.dtype == np.uint8 and v.shape == img.shape
            assert np.array_equal(v != 0, meta == m), f"support of ({k}, {m})"   # the absent meta-label: all zero
            if x.size == 0:
                assert (m, k) not in fits
                continue
            inside = v[meta == m]
            assert inside.min() >= 10 * m and inside.max() <= 10 * m + k - 1
            if k == 1:
                assert (inside == 10 * m).all()
                continue
            sub = [img[v == 10 * m + c].mean() for c in range(k) if (v == 10 * m + c).any()]
            assert all(a <= b for a, b in zip(sub, sub[1:])), f"subclass means of ({k}, {m}) not ascending"
            sample = x[sg.subsample_index(x.size)]
            refs = [E.fit(x, *E.init_from_means(x, sg.kmeanspp_means(sample, k, key, m, i))) for i in range(n_init)]
            f = fits[(m, k)]
            ref = refs[f["init"]]
            srt = np.argsort(ref["means"], kind="stable")
            e = {p: E.param_error(f[p], ref[p][srt]) for p in ("means", "weights", "variances")}
            lbd, bound = abs(f["lower_bound"] - ref["lower_bound"]), E.lb_bound(ref["lse_absmax"])
            print(f"m={m} k={k}: init {f['init']} n_iter {f['n_iter']} ({ref['n_iter']}) means {e['means']:.2e} weights {e['weights']:.2e} "
                  f"variances {e['variances']:.2e} |lb diff| {lbd:.2e} (bound {bound:.2e})")
            assert f["n_iter"] == ref["n_iter"] and f["converged"] == ref["converged"], (m, k)
            assert e["means"] <= TOL_MEAN and e["weights"] <= TOL_WEIGHT and e["variances"] <= TOL_VAR, (m, k, e)
            assert lbd <= bound, (m, k)
            # near-ties between initialisations may flip the choice; a worse fit may not win
            assert ref["lower_bound"] >= max(r["lower_bound"] for r in refs) - 2 * bound, (m, k)
            want, gap = E.predict(x, ref["weights"], ref["means"], ref["variances"])
            diff = inside != want.astype(np.int64) + 10 * m
            assert not (diff & ~(gap < DELTA)).any(), f"({k}, {m}): a label differs where the reference's gap is >= {DELTA}"


def test_fit_gmm1d_with_one_component(sg):
    c = {c.name: c for c in SC.em_cases()}["mix4097_k1"]
    got = sg.fit_gmm1d(dev(c.x), 1, n_init=2, key=1)
    x = c.x.astype(np.float64)
    assert got["converged"] and got["n_iter"] == 2 and got["weights"].shape == (1,)
    assert abs(got["weights"][0] - 1.0) <= TOL_WEIGHT and abs(got["means"][0] / x.mean() - 1.0) <= TOL_MEAN
    assert abs(got["variances"][0] / (x.var() + 1e-6) - 1.0) <= TOL_VAR


# --------------------------------------------------------------------------------------------------------------------- h
def _code_parts(shape, nparts, seed, misaligned=False):
    """nparts uint8 device volumes with at most 40 distinct columns; `misaligned`: each one a contiguous slice of a larger
    buffer starting at element 1, so its data pointer is one byte past a 4-byte boundary."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    column = rng.integers(0, 40, size=n)
    table = rng.integers(0, 256, size=(nparts, 40)).astype(np.uint8)
    parts = []
    for j in range(nparts):
        if misaligned:
            buf = torch.zeros(n + 1, dtype=torch.uint8, device=DEV)
            part = buf[1:].view(shape)
            part.copy_(dev(table[j][column].reshape(shape)))
            assert part.is_contiguous() and part.data_ptr() % 4 == 1
        else:
            part = dev(table[j][column].reshape(shape))
        parts.append(part)
    return parts


@pytest.mark.parametrize("nparts", [1, 4, 5, 64])
@pytest.mark.parametrize("shape,misaligned", [((5, 7, 9), False), ((3, 5, 4), False), ((4, 4, 8), True)])
def test_seed_codes_one_voxel_form(shape, misaligned, nparts):
    from fetalsyngen_amd import seedcodes as S

    parts = _code_parts(shape, nparts, 40 + nparts, misaligned)
    stride = nparts + 1
    got, want = S.build_device(parts, stride), S.build(parts, stride)
    assert got is not None and got[1].shape == want[1].shape and want[1].shape[0] < 100
    assert (got[1][:, nparts] == 0).all()
    pair = got[0].reshape(-1).to(torch.int64) * 4096 + want[0].reshape(-1).to(torch.int64)
    assert torch.unique(pair).numel() == want[1].shape[0]
    rs = np.random.RandomState(7)
    for _ in range(6):
        sel = rs.randint(0, stride, 4).tolist()
        assert torch.equal(S.labels_of(*got, sel), S.labels_of(*want, sel))
