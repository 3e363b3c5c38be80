"""Real-image samples on the fused and keyed path: the dual-source warp, the keyed prior sample, `load_image` with seeds,
batches, gates, fallbacks and refusals.  Tolerances are the project's: labels and the warped image bit-exact
(tests/test_hip_parity.py::test_image_is_deformed_with_the_same_field), the synthetic image within RTOL / 2e-5 on [0,1]."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_hip_parity import RTOL, _spec_from_golden
from tests.util_cases import make_generator
from tests.util_real_image import DEV, KW, SHAPE, export_draws, oracle_with_image, phantom_image

pytestmark = pytest.mark.gpu
ATOL01 = 2e-5


@pytest.fixture(scope="module")
def K():
    from fetalsyngen_amd import kernels

    return kernels


@pytest.fixture(scope="module")
def subjects():
    """Three phantom subjects at SHAPE: (segmentation, seed volumes, image) on the host, built once."""
    from fetalsyngen_amd.phantom import make_seed_volumes

    return [(*make_seed_volumes(SHAPE, v), phantom_image(SHAPE, v)) for v in range(3)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _random_spec(K, shape, flip, seed=3):
    from fetalsyngen_amd import tables as T

    rs = np.random.RandomState(seed)
    fs = (rs.randn(5, 4, 6, 3) * 2.0).astype(np.float32)
    ht, new = T.zoom_tables(fs.shape[:3], np.array(shape) / np.array(fs.shape[:3]))
    assert new == shape
    ang = 0.15
    A = np.array([[np.cos(ang), -np.sin(ang), 0.02], [np.sin(ang), np.cos(ang), 0.01], [0.03, 0, 1.04]], dtype=np.float32)
    centre = (np.array(shape) - 1) / 2
    return K.DeformSpec(shape, A, centre, centre.astype(np.float32), flip, _dev(fs), K.DeviceTables(ht, DEV), device=DEV)


def _dual_direct(K, spec, mm, a, b, l, nn_out, gamma=None, bias=None, bias_tabs=None):
    """fsg_warp_dual_f32 called directly, its return code asserted: K.warp(src_img=) answers FSG_E_ALIGN with the two launches
    it stands for, so only this shows that the dual-source kernel is what ran on the shapes of these tests."""
    from fetalsyngen_amd import _lib

    out_lin, out_img, out_nn = torch.empty_like(a), torch.empty_like(b), None
    din = dout = _lib.LABEL_F32
    if l is not None:
        odt = l.dtype if nn_out is None else nn_out
        out_nn = torch.empty(l.shape, dtype=odt, device=l.device)
        din = _lib.LABEL_U8 if l.dtype == torch.uint8 else _lib.LABEL_F32
        dout = _lib.LABEL_U8 if odt == torch.uint8 else _lib.LABEL_F32
    epi = K._epilogue(gamma, bias, bias_tabs, spec.shape)
    rc = _lib.load().fsg_warp_dual_f32(C.byref(spec.c), K._p(mm), K._p(a), K._p(out_lin), K._p(b), K._p(out_img), b.numel(), K._p(l),
                                       K._p(out_nn), din, dout, C.byref(epi), K._stream(mm))
    assert rc == 0, rc
    return out_lin, out_nn, out_img


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("labels", ["f32", "u8", "u8_to_f32"])
def test_dual_source_warp_equals_two_launches(K, flip, labels):
    """K.warp(src_lin=a, src_nn=l, src_img=b) against K.warp(src_lin=a, src_nn=l) + K.warp(src_lin=b), bit for bit: fast and
    general (FSG_TUNE_PRECISE_MATH) variants, a last dimension that is no multiple of the 32-lane tile and a grid of several
    workgroups, gamma + bias on out_lin only."""
    from fetalsyngen_amd import _lib, tables as T

    shape = (21, 19, 45)
    spec = _random_spec(K, shape, flip)
    rs = np.random.RandomState(1)
    a, b = _dev((rs.rand(*shape) * 255).astype(np.float32)), _dev((rs.rand(*shape) * 90 + 5).astype(np.float32))
    lab = rs.randint(0, 9, shape)
    l = _dev(lab.astype(np.float32)) if labels == "f32" else _dev(lab.astype(np.uint8))
    nn_out = torch.float32 if labels == "u8_to_f32" else None
    bias = _dev((rs.randn(3, 2, 4) * 0.2).astype(np.float32))
    bt, _new = T.zoom_tables(bias.shape, np.array(shape) / np.array(bias.shape))
    bias_tabs = K.DeviceTables(bt, DEV)
    spec.prepare_rows(bias, bias_tabs)
    mm = K.coords_floormin(spec)
    lib = _lib.load()
    for precise in (False, True):
        prev = lib.fsg_set_tuning(_lib.TUNE.PRECISE_MATH if precise else 0)
        try:
            lin, nn, img = K.warp(spec, mm, src_lin=a, src_nn=l, src_img=b, gamma=0.9, bias=bias, bias_tabs=bias_tabs, nn_out=nn_out)
            lin2, nn2 = K.warp(spec, mm, src_lin=a, src_nn=l, gamma=0.9, bias=bias, bias_tabs=bias_tabs, nn_out=nn_out)
            img2, _ = K.warp(spec, mm, src_lin=b)
            lin3, none, img3 = K.warp(spec, mm, src_lin=a, src_img=b, gamma=0.9, bias=bias, bias_tabs=bias_tabs)  # no labels
            direct = _dual_direct(K, spec, mm, a, b, l, nn_out, 0.9, bias, bias_tabs)  # the one-launch kernel itself, rc == 0
            direct3 = _dual_direct(K, spec, mm, a, b, None, None, 0.9, bias, bias_tabs)
        finally:
            lib.fsg_set_tuning(prev)
        assert np.array_equal(lin.cpu().numpy(), lin2.cpu().numpy()), precise
        assert np.array_equal(nn.cpu().numpy(), nn2.cpu().numpy()) and nn.dtype == nn2.dtype, precise
        assert np.array_equal(img.cpu().numpy(), img2.cpu().numpy()), precise  # ... so out_img carries no epilogue
        assert none is None and torch.equal(lin3, lin2) and torch.equal(img3, img2)
        assert torch.equal(direct[0], lin2) and torch.equal(direct[1], nn2) and torch.equal(direct[2], img2), precise
        assert direct3[1] is None and torch.equal(direct3[0], lin2) and torch.equal(direct3[2], img2), precise
        assert not torch.equal(img, lin)


def test_dual_source_warp_with_nonzero_margins(K, golden):
    """The golden field whose floor(min) margins are not zero (test_floormin_shortcut_has_the_exact_floor's case 1)."""
    g = golden("deform_image")
    assert list(g["margins_1"][:3]) != [0, 0, 0]
    spec, shape = _spec_from_golden(K, g, 1)
    rs = np.random.RandomState(2)
    a, b = _dev((rs.rand(*shape) * 255).astype(np.float32)), _dev((rs.rand(*shape) * 50).astype(np.float32))
    l = _dev(rs.randint(0, 5, shape).astype(np.uint8))
    spec.prepare_rows()
    mm = K.coords_floormin(spec)
    lin, nn, img = K.warp(spec, mm, src_lin=a, src_nn=l, src_img=b)
    lin2, nn2 = K.warp(spec, mm, src_lin=a, src_nn=l)
    img2, _ = K.warp(spec, mm, src_lin=b)
    assert torch.equal(lin, lin2) and torch.equal(nn, nn2) and torch.equal(img, img2)
    direct = _dual_direct(K, spec, mm, a, b, l, None)
    assert torch.equal(direct[0], lin2) and torch.equal(direct[1], nn2) and torch.equal(direct[2], img2)


def test_dual_warp_refusals_launch_nothing(K):
    """src_img without out_img, out_img without src_img, or a mismatched size: FSG_E_BADARG, outputs untouched."""
    from fetalsyngen_amd import _lib

    shape = (8, 8, 40)
    spec = _random_spec(K, shape, False)
    spec.prepare_rows()  # the lean kernel's domain: per-row coarse values precomputed
    mm = K.coords_floormin(spec)
    a, b = torch.rand(shape, device=DEV), torch.rand(shape, device=DEV)
    out_lin, out_img = torch.full(shape, -7.0, device=DEV), torch.full(shape, -7.0, device=DEV)
    epi = K._epilogue(None, None, None, shape)
    lib, n = _lib.load(), a.numel()

    def call(src_img, dst_img, nvox):
        return lib.fsg_warp_dual_f32(C.byref(spec.c), K._p(mm), K._p(a), K._p(out_lin), K._p(src_img), K._p(dst_img), nvox, None, None,
                                     _lib.LABEL_F32, _lib.LABEL_F32, C.byref(epi), K._stream(mm))

    assert call(b, None, n) == _lib.E_BADARG
    assert call(None, out_img, n) == _lib.E_BADARG
    assert call(b, out_img, n - 1) == _lib.E_BADARG
    assert call(b, b, n) == _lib.E_BADARG
    assert lib.fsg_warp_dual_f32(C.byref(spec.c), K._p(mm), K._p(a), K._p(out_lin), K._p(out_lin), K._p(out_img), n, None, None,
                                 _lib.LABEL_F32, _lib.LABEL_F32, C.byref(epi), K._stream(mm)) == _lib.E_BADARG  # out_lin over src_img
    torch.cuda.synchronize()
    assert bool((out_lin == -7).all()) and bool((out_img == -7).all())
    assert call(b, out_img, n) == 0
    torch.cuda.synchronize()
    assert not bool((out_img == -7).any())
    with pytest.raises(ValueError):
        K.warp(spec, mm, src_lin=a, src_img=torch.rand((8, 8, 41), device=DEV))


def _check(got, ref, what):
    out, seg, img = got[0], got[1], got[2]
    assert np.array_equal(seg.cpu().numpy().astype(np.uint8), ref["seg"].numpy().astype(np.uint8)), what
    assert np.array_equal(img.cpu().numpy(), ref["image"].numpy()), what
    err = float((out.cpu() - ref["scaled"]).abs().max())
    print(f"{what}: max |out - oracle| = {err:.3e}")
    np.testing.assert_allclose(out.cpu().numpy(), ref["scaled"].numpy(), rtol=RTOL, atol=ATOL01, err_msg=what)


def test_keyed_prior_samples_equal_the_oracle(K, subjects):
    """gen.sample(image, seg, seeds=None, key=k) in keyed mode against the oracle's stages on the exported draws: three
    consecutive keys, each naming the next one (look-ahead)."""
    from fetalsyngen_amd import sharding

    seg, _seeds, img = subjects[0]
    gen = make_generator(SHAPE, DEV, rng="keyed", **KW)
    seg_d, img_d = _dev(seg), _dev(img)
    keys = [sharding.sample_key(5, i) for i in range(3)]
    kc = gen.keyed_context(SHAPE)
    for i, k in enumerate(keys):
        got = gen._pipeline(img_d, seg_d, None, {}, scale01=True, key=k, next_key=keys[i + 1] if i + 1 < 3 else None)
        assert got[3]["key"] == k and got[3]["selected_seeds"] == {} and got[3]["seed_intensities"] == {}
        if i < 2:
            assert kc._carried, "the next sample's draw job did not ride along"
        _d, ex = export_draws(kc, K, k)
        _check(got, oracle_with_image(K, SHAPE, k, seg, None, img, ex, KW), f"key {i}")
    # the launches of such a sample: the head without a GMM launch, ONE warp launch (the dual-source kernel, not the two-launch form)
    gen.stage_traces = []
    traced = gen._pipeline(img_d, seg_d, None, {}, scale01=True, key=keys[0])
    stages = [name for name, _us in gen.stage_traces[0].elapsed_us()]
    gen.stage_traces[0].close()
    gen.stage_traces = None
    assert stages.count("warp") == 1 and "head" in stages and "gmm" not in stages, stages
    assert torch.equal(traced[2], gen._pipeline(img_d, seg_d, None, {}, scale01=True, key=keys[0])[2])
    # the public call returns the same triple
    out, seg_o, img_o, _p = gen.sample(img_d, seg_d, None, key=keys[1])
    assert img_o is not None and out.shape == seg_o.shape == img_o.shape


def test_keyed_load_image_with_seeds(K, subjects):
    """With a bank the image must not disturb the synthetic channel: out and labels bitwise those of the same key without an
    image; the warped image equals the oracle's."""
    from fetalsyngen_amd import sharding
    from fetalsyngen_amd.data.datasets import SeedBank

    seg, seeds, img = subjects[1]
    gen = make_generator(SHAPE, DEV, rng="keyed", **KW)
    seg_d, img_d, bank = _dev(seg), _dev(img), SeedBank(seeds, DEV)
    k = sharding.sample_key(6, 0)
    plain = gen._pipeline(None, seg_d, bank, {}, scale01=True, key=k)
    got = gen._pipeline(img_d, seg_d, bank, {}, scale01=True, key=k)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and plain[2] is None
    _d, ex = export_draws(gen.keyed_context(SHAPE), K, k)
    _check(got, oracle_with_image(K, SHAPE, k, seg, seeds, img, ex, KW), "load_image with seeds")


def test_image_samples_depend_on_the_key_only(K, subjects):
    from fetalsyngen_amd import sharding
    from fetalsyngen_amd.data.datasets import SeedBank

    seg, seeds, img = subjects[0]
    seg_d, img_d = _dev(seg), _dev(img)
    k1, k2 = sharding.sample_key(9, 1), sharding.sample_key(9, 2)
    gen = make_generator(SHAPE, DEV, rng="keyed", **KW)
    a = gen._pipeline(img_d, seg_d, None, {}, scale01=True, key=k1)
    gen._pipeline(None, seg_d, SeedBank(seeds, DEV), {}, scale01=True, key=123)  # an unrelated call in between
    b = gen._pipeline(img_d, seg_d, None, {}, scale01=True, key=k2, next_key=k1)  # ... and k1 announced by another sample
    c = gen._pipeline(img_d, seg_d, None, {}, scale01=True, key=k1)
    fresh = make_generator(SHAPE, DEV, rng="keyed", **KW)
    d = fresh._pipeline(_dev(img), _dev(seg), None, {}, scale01=True, key=k1)
    for other in (c, d):
        assert all(torch.equal(x, y) for x, y in zip(a[:3], other[:3]))
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[2], b[2])
    s = fresh._pipeline(None, _dev(seg), SeedBank(seeds, DEV), {}, scale01=True, key=k1)
    pa, ps = a[3]["deform_params"], s[3]["deform_params"]
    assert pa["flip"] == ps["flip"] and all(np.array_equal(pa["affine"][q], ps["affine"][q]) for q in pa["affine"])
    assert pa["non_rigid"]["size_F_small"] == ps["non_rigid"]["size_F_small"] and pa["non_rigid"]["nonlin_std"] == ps["non_rigid"]["nonlin_std"]


def test_gates(K, subjects):
    """Deformation probability 0: image and labels come back untouched and out follows the no-warp branch.  Deformation
    probability 1 with resampling and noise probability 0: the full-resolution tail."""
    from fetalsyngen_amd import sharding

    seg, _seeds, img = subjects[2]
    seg_d, img_d = _dev(seg), _dev(img)
    k = sharding.sample_key(11, 0)
    gen = make_generator(SHAPE, DEV, rng="keyed", **KW)
    gen.spatial_deform.prob = 0.0
    got = gen._pipeline(img_d, seg_d, None, {}, scale01=True, key=k)
    assert torch.equal(got[1], seg_d) and torch.equal(got[2], img_d)
    _d, ex = export_draws(gen.keyed_context(SHAPE), K, k)
    assert ex["deform"] is None
    _check(got, oracle_with_image(K, SHAPE, k, seg, None, img, ex, KW), "no deformation")
    gen2 = make_generator(SHAPE, DEV, rng="keyed", **KW)
    gen2.resampled.prob = gen2.noise.prob = 0.0
    got = gen2._pipeline(img_d, seg_d, None, {}, scale01=True, key=k)
    _d, ex = export_draws(gen2.keyed_context(SHAPE), K, k)
    assert ex["deform"] is not None and ex["resample"] is None and ex["noise_std"] is None
    _check(got, oracle_with_image(K, SHAPE, k, seg, None, img, ex, KW), "no resampling, no noise")


@pytest.mark.parametrize("streams", [1, 2])
def test_generator_batch_equals_per_sample_calls(K, subjects, streams):
    """sample_batch with keys: images only, and a mix of image and seed subjects, bitwise equal to per-sample keyed calls."""
    from fetalsyngen_amd import sharding
    from fetalsyngen_amd.data.datasets import SeedBank

    gen = make_generator(SHAPE, DEV, rng="keyed", **KW)
    dev = [(_dev(s), SeedBank(b, DEV), _dev(i)) for s, b, i in subjects]
    keys = [sharding.sample_key(21, i) for i in range(5)]
    only = [(dev[w][2], dev[w][0], None) for w in (0, 1, 2, 1, 0)]
    mix = [(dev[0][2], dev[0][0], None), (None, dev[1][0], dev[1][1]), (dev[2][2], dev[2][0], dev[2][1]), (None, dev[0][0], dev[0][1]),
           (dev[1][2], dev[1][0], None)]
    for items in (only, mix):
        out, seg, imgs, params = gen.sample_batch(items, scale01=True, streams=streams, keys=keys)
        torch.cuda.synchronize()
        for b, ((im, sg, bank), k) in enumerate(zip(items, keys)):
            one = gen._pipeline(im, sg, bank, {}, scale01=True, key=k)
            assert torch.equal(out[b], one[0]) and torch.equal(seg[b], one[1]), b
            assert (imgs[b] is None) == (im is None) and (im is None or torch.equal(imgs[b], one[2])), b
            assert params[b]["key"] == k


def _per_sample_reference(shape, order, base_seed, with_seeds, volumes=None):
    """What the dataset's batch must hold, made without the dataset: per subject a keyed `_pipeline` call of a fresh generator
    on volumes uploaded here (those tests/util_bids.py::write_tree wrote, or `volumes[i] = (image, segmentation)`), under the key
    `__getitem__` announces, and the [0,1] scaling `FetalSynthDataset.sample` applies to the image.
    Returns [(out, uint8 labels, scaled warped image)] in `order`."""
    from fetalsyngen_amd import kernels as K
    from fetalsyngen_amd import sharding
    from fetalsyngen_amd.data.datasets import SeedBank
    from fetalsyngen_amd.phantom import make_seed_volumes

    gen = make_generator(shape, DEV, rng="keyed", **KW)
    res = []
    for i in order:
        seg, seeds = make_seed_volumes(shape, i)
        if volumes is None:
            img_d, seg_d = _dev((seg * 30).astype(np.float32)), _dev(seg.astype(np.float32))
        else:
            img_d, seg_d = volumes[i]
        gen.register_label_twin(seg_d, seg_d.to(torch.uint8))
        key = sharding.sample_key(base_seed, i)  # epoch 0
        out, lab, img, params = gen._pipeline(img_d, seg_d, SeedBank(seeds, DEV) if with_seeds else None, {}, scale01=True,
                                              labels_u8=True, key=key)
        assert params["key"] == key and lab.dtype == torch.uint8
        res.append((out, lab, K.scale(img.contiguous(), K.reduce_minmax(img.contiguous()), mode=1)))
    return res


def test_dataset_batch_with_regridded_subjects(tmp_path):
    """`regrid=` subjects in keyed mode with images: the regridded image and its prior are cached with the labels and the batch
    equals the per-sample calls on the regridded volumes, the images included."""
    from fetalsyngen_amd.data.datasets import FetalSynthDataset
    from tests.util_bids import write_tree

    shape = SHAPE
    bids, _seeds_root = write_tree(tmp_path, shape, ["sub-00", "sub-01"])
    gen = make_generator(shape, DEV, rng="keyed", **KW)
    ds = FetalSynthDataset(str(bids), gen, None, None, load_image=True, image_as_intensity=True, return_device=True, base_seed=3,
                           regrid=(0.55, shape))
    vols = {i: ds._regridded(i) for i in (0, 1)}
    from fetalsyngen_amd.phantom import make_seed_volumes

    assert not torch.equal(vols[0][1], _dev(make_seed_volumes(shape, 0)[0].astype(np.float32)))  # really regridded
    want = _per_sample_reference(shape, [1, 0], 3, with_seeds=False, volumes=vols)
    batch, gps = ds.sample_batch([1, 0], streams=2)
    ent = ds._labels.peek(0)
    assert len(ent) == 5 and ent[4] is not None and torch.equal(ent[3], vols[0][0])
    for b, i in enumerate([1, 0]):
        one = ds[i]
        assert torch.equal(batch["image"][b], one["image"]) and torch.equal(batch["label"][b], one["label"]), i
        assert "key" in gps[b]
        out_w, lab_w, real_w = want[b]
        assert torch.equal(batch["image"][b, 0], out_w) and torch.equal(batch["label"][b, 0], lab_w), i
        assert torch.equal(batch["real_image"][b, 0], real_w), i


@pytest.mark.parametrize("as_intensity", [True, False])
def test_dataset_batch_equals_getitem(tmp_path, as_intensity):
    """FetalSynthDataset.sample_batch with load_image (and image_as_intensity) on a four-subject BIDS tree: what it refused
    with a ValueError before; bitwise the four __getitem__ calls; and the cache budget evicts subjects, priors included."""
    from fetalsyngen_amd.data.datasets import FetalSynthDataset
    from tests.util_bids import write_tree

    shape = (64, 56, 72)
    subs = [f"sub-{i:02d}" for i in range(4)]
    bids, seeds_root = write_tree(tmp_path, shape, subs)
    gen = make_generator(shape, DEV, rng="keyed", **KW)
    ds = FetalSynthDataset(str(bids), gen, None if as_intensity else str(seeds_root), None, load_image=True,
                           image_as_intensity=as_intensity, return_device=True, base_seed=3)
    order = [2, 0, 3, 1]
    want = _per_sample_reference(shape, order, 3, with_seeds=not as_intensity)
    for streams in (1, 2):
        batch, gps = ds.sample_batch(order, streams=streams)
        assert batch["image"].shape == batch["real_image"].shape == (4, 1, *shape)
        for b, i in enumerate(order):
            one = ds[i]
            assert torch.equal(batch["image"][b], one["image"]) and torch.equal(batch["label"][b], one["label"]), (streams, i)
            assert gps[b]["key"] == ds.generation_params["key"]
            out_w, lab_w, real_w = want[b]
            assert torch.equal(batch["image"][b, 0], out_w) and torch.equal(batch["label"][b, 0], lab_w), (streams, i)
            assert torch.equal(batch["real_image"][b, 0], real_w), (streams, i)
    # the host-copy branch: float32 images and int64 labels on the CPU, the same values
    host = FetalSynthDataset(str(bids), gen, None if as_intensity else str(seeds_root), None, load_image=True,
                             image_as_intensity=as_intensity, return_device=False, base_seed=3)
    batch, _gps = host.sample_batch(order, streams=2)
    assert not batch["real_image"].is_cuda and batch["label"].dtype == torch.int64
    for b in range(4):
        out_w, lab_w, real_w = want[b]
        assert torch.equal(batch["image"][b, 0], out_w.cpu()) and torch.equal(batch["label"][b, 0], lab_w.cpu().long()), b
        assert torch.equal(batch["real_image"][b, 0], real_w.cpu()), b
    ent = ds._labels.peek(0)
    assert len(ent) == 5 and (ent[4] is not None) == as_intensity
    # a budget of two subjects: the cache evicts (with their images and priors) instead of exceeding it
    per_subject = ds._labels.bytes // len(ds._labels)
    small = FetalSynthDataset(str(bids), gen, None if as_intensity else str(seeds_root), None, load_image=True,
                              image_as_intensity=as_intensity, return_device=True, base_seed=3, cache_bytes=2 * per_subject)
    for i in range(4):
        small[i]
    assert small._labels.bytes <= 2 * per_subject and len(small._labels) == 2 and small._labels.evictions == 2
    n = int(np.prod(shape))
    assert per_subject >= n * (4 + 1 + 4) + (n * 4 if as_intensity else 0)  # labels, twin, image (+ prior)


def test_fallbacks_still_answer(K):
    """A shape the fused path declines (FSG_E_ALIGN: its blur needs a z extent that is a multiple of 4), a CPU image and a
    non-contiguous image all return the sample of the existing path -- a "device"-mode sample seeded from the key -- instead of
    raising."""
    from fetalsyngen_amd import sharding
    from fetalsyngen_amd.phantom import make_seed_volumes

    k = sharding.sample_key(31, 0)
    shape = (24, 20, 28)
    seg, _seeds = make_seed_volumes(shape, 0)
    img = phantom_image(shape)
    gen = make_generator(shape, DEV, rng="keyed", **KW)
    seg_d = _dev(seg)
    cpu = gen._pipeline(torch.from_numpy(img), seg_d, None, {}, scale01=True, key=k)
    wide = _dev(np.concatenate([img, img], axis=2))[:, :, ::2]
    assert not wide.is_contiguous()
    nc = gen._pipeline(wide, seg_d, None, {}, scale01=True, key=k)
    for got in (cpu, nc):
        assert got[2] is not None and tuple(got[0].shape) == shape and bool(torch.isfinite(got[0]).all())
        assert "key" not in got[3]  # the stage-by-stage path, seeded from the key
    # declined by the fused kernels: blur taps need a z extent that is a multiple of 4
    shape2 = (24, 20, 30)
    seg2, _ = make_seed_volumes(shape2, 0)
    img2 = phantom_image(shape2)
    gen2 = make_generator(shape2, DEV, rng="keyed", **KW)
    got = gen2._pipeline(_dev(img2), _dev(seg2), None, {}, scale01=True, key=k)
    assert got[2] is not None and tuple(got[0].shape) == shape2 and bool(torch.isfinite(got[0]).all())
    assert float(got[0].min()) >= 0.0 and float(got[0].max()) <= 1.0
    ref_gen = make_generator(shape2, DEV, rng="device", **KW)
    np.random.seed(k & 0xFFFFFFFF)
    torch.default_generator.manual_seed(k >> 1)
    ref = ref_gen._pipeline(_dev(img2), _dev(seg2), None, {}, scale01=True)
    assert all(torch.equal(x, y) for x, y in zip(got[:3], ref[:3]))
