"""The brick table of a uint8 label volume (csrc/fsg_label_bricks.hip) and the fused warp that uses it (csrc/fsg_warp_lean.hip,
HAS_MAP): a label gather whose source voxel lies in an 8x8x8 brick of one label is dropped by the buffer range check and the
table's entry is the label.

  * CPU: the registry (attach / detach / re-attach / detach of an unknown volume) and the domain rule at the cap.
  * GPU: the table builder against numpy; the warp with a table against the same launch under FSG_TUNE_NO_LABEL_BRICKS, bit for
    bit, image and labels, every launch form the table serves; a table that must be ignored (another shape, over the cap) and
    one that must be used are told apart by a table that LIES (every brick "uniform, label 9"); keyed FetalSynthGen samples
    against the pinned oracle; the table's lifetime behind the generator's twin cache.
"""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

DEV = "cuda:0"
F = np.float32


def _lib():
    from fetalsyngen_amd import _lib as L

    return L, L.load()


def nbricks(shape):
    return int(np.prod([(n + 7) // 8 for n in shape]))


def ref_table(lab):
    """numpy: per 8x8x8 brick (partial at the upper faces) its label if uniform and not 255, else 255."""
    b = [(n + 7) // 8 for n in lab.shape]
    out = np.empty(b, dtype=np.uint8)
    for i in range(b[0]):
        for j in range(b[1]):
            for k in range(b[2]):
                blk = lab[8 * i:8 * i + 8, 8 * j:8 * j + 8, 8 * k:8 * k + 8]
                u = blk.flat[0]
                out[i, j, k] = u if (blk == u).all() and u != 255 else 255
    return out


# ---- CPU -----------------------------------------------------------------------------------------------------------------
def test_registry_semantics():
    L, lib = _lib()
    P = C.c_void_p
    start = lib.fsg_label_bricks_count()
    vol_a, vol_b, map_a, map_b = 0x10000, 0x20000, 0x30000, 0x30010
    assert lib.fsg_label_bricks_detach(P(vol_a)) == 0                      # unknown volume
    assert lib.fsg_label_bricks_attach(P(vol_a), 8, 8, 8, P(map_a)) == 0
    assert lib.fsg_label_bricks_count() == start + 1
    assert lib.fsg_label_bricks_attach(P(vol_a), 16, 8, 8, P(map_b)) == 0   # re-attach replaces
    assert lib.fsg_label_bricks_count() == start + 1
    assert lib.fsg_label_bricks_attach(P(vol_b), 8, 8, 8, P(map_a)) == 0
    assert lib.fsg_label_bricks_count() == start + 2
    assert lib.fsg_label_bricks_detach(P(vol_a)) == 1
    assert lib.fsg_label_bricks_detach(P(vol_a)) == 0
    assert lib.fsg_label_bricks_count() == start + 1
    assert lib.fsg_label_bricks_detach(P(vol_b)) == 1
    assert lib.fsg_label_bricks_count() == start
    # bad arguments leave the registry as it was
    assert lib.fsg_label_bricks_attach(P(0), 8, 8, 8, P(map_a)) == L.E_BADARG
    assert lib.fsg_label_bricks_attach(P(vol_a), 8, 8, 8, P(0)) == L.E_BADARG
    assert lib.fsg_label_bricks_attach(P(vol_a), 0, 8, 8, P(map_a)) == L.E_BADARG
    assert lib.fsg_label_bricks_attach(P(vol_a), 8, 8, 8, P(map_a + 4)) == L.E_ALIGN
    assert lib.fsg_label_bricks_count() == start


def test_registry_is_bounded():
    L, lib = _lib()
    P = C.c_void_p
    start, vols = lib.fsg_label_bricks_count(), []
    try:
        rc = 0
        for i in range(200):
            rc = lib.fsg_label_bricks_attach(P(0x100000 + 64 * i), 8, 8, 8, P(0x30000))
            if rc != 0:
                break
            vols.append(0x100000 + 64 * i)
        assert rc == L.E_TOOBIG and len(vols) >= 8
        assert lib.fsg_label_bricks_attach(P(vols[0]), 16, 16, 16, P(0x30000)) == 0  # a known volume is still replaced
    finally:
        for v in vols:
            lib.fsg_label_bricks_detach(P(v))
    assert lib.fsg_label_bricks_count() == start


def test_usable_at_the_cap():
    L, lib = _lib()
    assert L.LABEL_BRICKS_CAP == 32768
    assert lib.fsg_label_bricks_usable(256, 256, 256) == 1   # 32 768 bricks
    assert lib.fsg_label_bricks_usable(256, 256, 257) == 0   # 33 792
    assert lib.fsg_label_bricks_usable(8 * 32768, 8, 8) == 1
    assert lib.fsg_label_bricks_usable(8 * 32768 + 1, 8, 8) == 0  # 32 769
    assert lib.fsg_label_bricks_usable(0, 8, 8) == 0
    prev = lib.fsg_label_bricks_set_cap(10)
    try:
        assert prev == 32768
        assert lib.fsg_label_bricks_usable(80, 8, 8) == 1 and lib.fsg_label_bricks_usable(81, 8, 8) == 0
        assert lib.fsg_label_bricks_set_cap(32769) == L.E_BADARG and lib.fsg_label_bricks_set_cap(-1) == L.E_BADARG
        assert lib.fsg_label_bricks_usable(81, 8, 8) == 0
    finally:
        lib.fsg_label_bricks_set_cap(0)
    assert lib.fsg_label_bricks_usable(256, 256, 256) == 1


# ---- GPU -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (and libfsg_hip.so); there is no fallback to skip to")
    from fetalsyngen_amd import kernels

    return kernels


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def build_table(K, d_lab):
    L, lib = _lib()
    table = torch.full((nbricks(d_lab.shape),), 77, dtype=torch.uint8, device=DEV)
    L.check(lib.fsg_label_bricks_u8(C.c_void_p(d_lab.data_ptr()), *d_lab.shape, C.c_void_p(table.data_ptr()), K._stream(d_lab)),
            "fsg_label_bricks_u8")
    return table


def builder_volumes(shape):
    n0, n1, n2 = shape
    last = (min(7, n0 - 1), min(7, n1 - 1), min(7, n2 - 1))
    vols = {"one label": np.full(shape, 5, np.uint8), "checkerboard": (np.indices(shape).sum(0) & 1).astype(np.uint8)}
    v = np.full(shape, 3, np.uint8); v[0, 0, 0] = 4; vols["odd first corner"] = v
    v = np.full(shape, 3, np.uint8); v[last] = 4; vols["odd last corner"] = v
    for name, at in (("x", (n0 - 1, 0, 0)), ("y", (0, n1 - 1, 0)), ("z", (0, 0, n2 - 1)), ("xyz", (n0 - 1, n1 - 1, n2 - 1))):
        v = np.zeros(shape, np.uint8); v[at] = 1; vols[f"odd voxel at the upper {name} face"] = v
    v = np.zeros(shape, np.uint8)
    v[:, :, : n2 // 2] = 254
    v[: max(n0 // 2, 1)] = 255
    vols["labels 0, 254, 255"] = v
    vols["all 255"] = np.full(shape, 255, np.uint8)
    return vols


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(8, 8, 8), (24, 20, 40), (17, 9, 33), (9, 1, 65)])
def test_table_builder_equals_numpy(K, shape):
    for name, lab in builder_volumes(shape).items():
        got = build_table(K, dev(lab)).cpu().numpy().reshape([(n + 7) // 8 for n in shape])
        assert np.array_equal(got, ref_table(lab)), f"{shape} {name}"


def affine(rot, scale):
    from fetalsyngen_amd.utils.generation import make_affine_matrix

    return make_affine_matrix(list(rot), [0.01, -0.02, 0.015], list(scale)).astype(F)


def ellipsoids(shape):
    g = np.indices(shape).astype(np.float64)
    r = sum(((g[a] - (shape[a] - 1) / 2) / (shape[a] / 2)) ** 2 for a in range(3))
    return ((r < 0.8).astype(np.uint8) + (r < 0.45) + (r < 0.2) * 2 + (r < 0.05) * 250).astype(np.uint8)  # labels 0 1 2 4 254


def label_volumes(shape, rs):
    v255 = np.zeros(shape, np.uint8)
    v255[:8, :8, :8] = 255   # a uniform brick of label 255: "mixed" in the table, gathered
    v255[8:16, :, :] = 254
    return {"all-uniform": np.full(shape, 3, np.uint8), "all-mixed": rs.randint(0, 8, shape).astype(np.uint8),
            "nested ellipsoids": ellipsoids(shape), "uniform brick of 255": v255}


CASES = {  # rotation, scale, flip, coarse field, shift
    "identity": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), False, None, 0.0),
    "identity, flipped": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), True, None, 0.0),
    "20 degrees about two axes, flip, field": ((0.35, -0.35, 0.0), (1.05, 0.95, 1.02), True, (3, 2, 4), 0.3),
    "scaled past every face": ((0.1, -0.1, 0.1), (1.9, 1.8, 2.0), False, (2, 2, 3), 0.3),
}


class Launches:
    """One deformation on one label volume: every launch form the brick table serves."""

    def __init__(self, K, shape, case, lab, seed):
        from fetalsyngen_amd import tables as T

        rot, scale, flip, fdim, shift = CASES[case]
        rs = np.random.RandomState(seed)
        c = (np.array(shape) - 1) / 2
        A = np.eye(3, dtype=F) if case.startswith("identity") else affine(rot, scale)
        fs = ft = None
        if fdim is not None:
            fs = dev((rs.randn(*fdim, 3) * 2.0).astype(F))
            ft = K.DeviceTables(T.zoom_tables(fdim, np.array(shape) / np.array(fdim))[0], DEV)
        self.K, self.spec = K, K.DeformSpec(shape, A, c, c.astype(F) + F(shift), flip, fs, ft, device=DEV)
        self.spec.prepare_rows(None, None)
        self.mm6 = K.coords_minmax(self.spec)
        self.img, self.lab = dev((rs.rand(*shape) * 255).astype(F)), dev(lab)

    def run(self):
        K, w = self.K, dict(src_nn=self.lab)
        out = [K.warp(self.spec, self.mm6, src_lin=self.img, nn_out=torch.float32, gamma=1.13, **w),
               K.warp(self.spec, self.mm6, src_lin=self.img, **w),
               K.warp(self.spec, self.mm6, **w),
               K.warp(self.spec, self.mm6, nn_out=torch.float32, **w)]
        L, lib = _lib()
        prev = lib.fsg_set_tuning(0)
        try:  # the instantiations without the hardware log / exp
            lib.fsg_set_tuning(prev | L.TUNE.PRECISE_MATH)
            out.append(K.warp(self.spec, self.mm6, src_lin=self.img, nn_out=torch.float32, gamma=1.13, **w))
            out.append(K.warp(self.spec, self.mm6, src_lin=self.img, gamma=0.9, **w))
        finally:
            lib.fsg_set_tuning(prev)
        torch.cuda.synchronize()
        return [t for pair in out for t in pair if t is not None]

    def run_without_tables(self):
        L, lib = _lib()
        prev = lib.fsg_set_tuning(0)
        try:
            lib.fsg_set_tuning(prev | L.TUNE.NO_LABEL_BRICKS)
            return self.run()
        finally:
            lib.fsg_set_tuning(prev)


def attached(d_lab, table, shape=None):
    L, lib = _lib()
    L.check(lib.fsg_label_bricks_attach(C.c_void_p(d_lab.data_ptr()), *(shape or d_lab.shape), C.c_void_p(table.data_ptr())), "attach")


def detach(d_lab):
    _lib()[1].fsg_label_bricks_detach(C.c_void_p(d_lab.data_ptr()))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(24, 20, 40), (17, 12, 33)])
def test_warp_with_the_table_equals_the_warp_without(K, shape):
    rs = np.random.RandomState(5)
    dropped = 0
    for ci, case in enumerate(CASES):
        for name, lab in label_volumes(shape, rs).items():
            run = Launches(K, shape, case, lab, seed=ci)
            want = run.run_without_tables()
            table = build_table(K, run.lab)
            assert np.array_equal(table.cpu().numpy().reshape([(n + 7) // 8 for n in shape]), ref_table(lab))
            dropped += int((table != 255).sum())
            attached(run.lab, table)
            try:
                got = run.run()
            finally:
                detach(run.lab)
            assert len(got) == len(want) == 10
            for k, (g, w) in enumerate(zip(got, want)):
                assert g.dtype == w.dtype and torch.equal(g, w), f"{shape} {case} / {name}: output {k}"
    assert dropped > 0


@pytest.mark.gpu
def test_a_table_is_used_only_for_its_volume_shape_and_within_the_cap(K):
    """A table that lies -- every brick "uniform, label 9" -- shows whether the warp reads it: attached for this volume and shape
    the labels come out 9; attached for another shape, over the (lowered) cap, or under FSG_TUNE_NO_LABEL_BRICKS it is ignored."""
    L, lib = _lib()
    shape = (24, 20, 40)
    lab = label_volumes(shape, np.random.RandomState(1))["nested ellipsoids"]
    run = Launches(K, shape, "identity", lab, seed=0)
    want = run.run_without_tables()
    liar = torch.full((nbricks(shape),), 9, dtype=torch.uint8, device=DEV)
    try:
        attached(run.lab, liar)
        got = run.run()
        assert torch.equal(got[0], want[0])                                      # the image does not depend on it
        assert all(bool((g == 9).all()) for g in (got[1], got[3], got[4], got[5]))  # u8 -> f32, u8 -> u8, the label-only forms
        assert all(torch.equal(g, w) for g, w in zip(run.run_without_tables(), want))
        attached(run.lab, liar, shape=(24, 20, 48))                             # re-attached under another shape: ignored
        assert all(torch.equal(g, w) for g, w in zip(run.run(), want))
        attached(run.lab, liar)
        prev = lib.fsg_label_bricks_set_cap(nbricks(shape) - 1)                  # over the cap: today's instantiation
        try:
            assert all(torch.equal(g, w) for g, w in zip(run.run(), want))
            lib.fsg_label_bricks_set_cap(nbricks(shape))
            assert bool((run.run()[1] == 9).all())
        finally:
            lib.fsg_label_bricks_set_cap(prev)
    finally:
        detach(run.lab)
    assert all(torch.equal(g, w) for g, w in zip(run.run(), want))


KW = dict(nonlin_scale=(0.08, 0.2), bf_scale=(0.05, 0.2))


@pytest.mark.gpu
def test_keyed_samples_with_the_table_equal_the_oracle(K):
    from fetalsyngen_amd import sharding
    from fetalsyngen_amd.data.datasets import SeedBank
    from fetalsyngen_amd.phantom import make_seed_volumes
    from tests.util_cases import make_generator
    from tests.util_keyed_overrides import oracle_sample

    L, lib = _lib()
    shape = (64, 56, 72)
    seg, seeds = make_seed_volumes(shape)
    gen = make_generator(shape, DEV, rng="keyed", prob=1.0, **KW)
    kc = gen.keyed_context(shape)
    bank, seg_d = SeedBank(seeds, DEV), torch.from_numpy(seg).to(DEV)
    start = lib.fsg_label_bricks_count()
    for i in range(3):  # the twin, and its table, exist from the second sighting of the volume on
        key = sharding.sample_key(31, i)
        out, seg_o, _img, _params = gen._pipeline(None, seg_d, bank, {}, scale01=True, key=key)
        assert lib.fsg_label_bricks_count() == start + (i >= 1)
        prev = lib.fsg_set_tuning(0)
        try:
            lib.fsg_set_tuning(prev | L.TUNE.NO_LABEL_BRICKS)
            out_n, seg_n, _i, _p = gen._pipeline(None, seg_d, bank, {}, scale01=True, key=key)
        finally:
            lib.fsg_set_tuning(prev)
        assert torch.equal(out, out_n) and torch.equal(seg_o, seg_n), f"sample {i}"
        _d, _ex, r = oracle_sample(kc, K, shape, key, seg, seeds, dict(prob=1.0, **KW))
        assert np.array_equal(seg_o.cpu().numpy().astype(np.uint8), r["seg"].numpy().astype(np.uint8)), f"sample {i}: labels"
        np.testing.assert_allclose(out.cpu().numpy(), r["scaled"].numpy(), rtol=0, atol=2e-5, err_msg=f"sample {i}")
    del gen, kc, seg_d, out, seg_o, out_n, seg_n
    gc.collect()
    assert lib.fsg_label_bricks_count() == start


@pytest.mark.gpu
def test_table_lifetime_follows_the_twin(K):
    from fetalsyngen_amd import sharding
    from fetalsyngen_amd.data.datasets import SeedBank
    from fetalsyngen_amd.phantom import make_seed_volumes
    from tests.util_cases import make_generator

    L, lib = _lib()
    shape = (40, 32, 48)
    seg, seeds = make_seed_volumes(shape)
    gen = make_generator(shape, DEV, rng="keyed", prob=1.0, **KW)
    bank, seg_d = SeedBank(seeds, DEV), torch.from_numpy(seg).to(DEV)
    start = lib.fsg_label_bricks_count()
    key = sharding.sample_key(7, 0)

    def sample():
        return gen._pipeline(None, seg_d, bank, {}, scale01=True, key=key)[1].clone()

    def sample_without_tables():
        prev = lib.fsg_set_tuning(0)
        try:
            lib.fsg_set_tuning(prev | L.TUNE.NO_LABEL_BRICKS)
            return sample()
        finally:
            lib.fsg_set_tuning(prev)

    first = sample()
    assert lib.fsg_label_bricks_count() == start
    assert torch.equal(sample(), first) and lib.fsg_label_bricks_count() == start + 1
    # an in-place torch write: the next samples follow the new labels, the stale table goes with its twin
    seg_d[seg_d == seg_d.max()] = 0
    seg_d[:8, :8, :8] = 1
    want = sample_without_tables()
    assert not torch.equal(want, first)
    assert lib.fsg_label_bricks_count() == start
    for _ in range(3):
        assert torch.equal(sample(), want)
    assert lib.fsg_label_bricks_count() == start + 1
    gen.invalidate_label_twins()
    gc.collect()
    assert lib.fsg_label_bricks_count() == start
    for _ in range(2):
        assert torch.equal(sample(), want)
    assert lib.fsg_label_bricks_count() == start + 1
    del seg_d  # the caller's volume dies: its twin and the table with it
    gc.collect()
    assert lib.fsg_label_bricks_count() == start
