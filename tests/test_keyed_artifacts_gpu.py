"""Keyed samples with the SR-artifact stages configured (GPU, 48^3 phantom subjects, stage parameters of
`generator.defaults.default_artifacts`).

The hot-path part of such a sample is the fused keyed call of the same key; every configured stage runs inside
`rng.keyed_scope(key, its stream)`, so the sample is a function of its key, the caller's global generators are left alone,
and a stage's draws do not depend on what another stage drew.

SimulateMotion's adjoint accumulates with fp32 atomics, so two runs of the same sample differ by summation-order noise.
MOTION_ATOL is 4x the largest difference measured WITHOUT the keyed path: the stage called directly in rng="device" mode, three
runs on the same input under identically seeded global generators, ten keyed 48^3 inputs (images divided by their maximum,
as the stage receives them): largest |difference| 2.384e-07 = 2^-22, so 9.537e-07 = 2^-20 is allowed on such an image.
"""
import numpy as np
import pytest
import torch

from tests import util_pick64 as P
from tests.util_cases import default_artifacts, make_generator

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(nonlin_scale=(0.08, 0.2), bf_scale=(0.05, 0.2))
S48 = (48, 48, 48)
MOTION_ATOL = 4 * 2.384186e-07
STAGES = ("blur_cortex", "struct_noise", "simulate_motion", "boundaries")


def _key(i, base=41):
    from fetalsyngen_amd import sharding

    return sharding.sample_key(base, i)


@pytest.fixture(scope="module")
def subject():
    """(SeedBank, device float32 label map, its uint8 twin) of one phantom subject."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (and libfsg_hip.so); there is no fallback to skip to")
    from fetalsyngen_amd.data.datasets import SeedBank
    from fetalsyngen_amd.phantom import make_seed_volumes

    seg, seeds = make_seed_volumes(S48, 1)
    seg_d = torch.from_numpy(seg).to(DEV)
    return SeedBank(seeds, DEV), seg_d, seg_d.to(torch.uint8)


def generator(subject, gates=None, merge_type="perlin", stages=True):
    """A keyed generator; `gates`: stage name -> on / off (default: all on); stages=False: no artifact stages at all."""
    arts = None
    if stages:
        arts = default_artifacts(prob=1.0, merge_type=merge_type)
        on = {name: True for name in STAGES}
        on.update(gates or {})
        for name in STAGES[:3]:
            arts[name].prob = 1.0 if on[name] else 0.0
        b = arts["boundaries"]
        b.prob_no_mask, b.prob_halo, b.prob_fuzzy = (0.0, 1.0, 1.0) if on["boundaries"] else (1.0, 0.5, 0.5)
    gen = make_generator(S48, DEV, rng="keyed", prob=1.0, artifacts=arts, **KW)
    gen.register_label_twin(subject[1], subject[2])
    return gen


ALL_OFF = {name: False for name in STAGES}
NO_MOTION = {"simulate_motion": False}


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a, b)
    if isinstance(a, (np.ndarray, list, tuple)):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


def _without_artifacts(params):
    return {k: v for k, v in params.items() if k != "artifacts"}


def np_state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale01", [False, True])
@pytest.mark.parametrize("labels_u8", [False, True])
def test_gates_off_is_the_sample_without_stages(subject, scale01, labels_u8):
    bank, seg_d, _twin = subject
    plain, art = generator(subject, stages=False), generator(subject, ALL_OFF)
    for i in range(2):
        k = _key(i)
        a = plain._pipeline(None, seg_d, bank, {}, scale01=scale01, labels_u8=labels_u8, key=k)
        b = art._pipeline(None, seg_d, bank, {}, scale01=scale01, labels_u8=labels_u8, key=k)
        assert b[1].dtype == (torch.uint8 if labels_u8 else torch.float32)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert _same(_without_artifacts(a[3]), _without_artifacts(b[3])) and b[3]["key"] == k
        assert b[3]["artifacts"] == {"blur_cortex": {"nblur": None}, "struct_noise": {}, "simulate_motion": {},
                                     "boundaries": {"no_mask_on": True, "halo_on": None, "fuzzy_on": None}}


# ---- 2 ---------------------------------------------------------------------------------------------------------------
def test_global_generators_are_left_alone(subject):
    bank, seg_d, _twin = subject
    gen = generator(subject)
    np.random.seed(123)
    torch.manual_seed(456)
    np.random.rand(3), torch.rand(3)
    n0, t0 = np.random.get_state(), torch.get_rng_state()
    out = gen.sample(None, seg_d, bank, key=_key(2))
    assert all(out[3]["artifacts"][name] for name in STAGES) and out[3]["artifacts"]["blur_cortex"]["nblur"] is not None
    assert np_state_equal(n0, np.random.get_state()) and torch.equal(t0, torch.get_rng_state())

    class Boom(RuntimeError):
        pass

    def raising(output, seg, device, genparams={}, **kwargs):
        np.random.rand(7), torch.rand(7)
        raise Boom("stage failed")

    gen.artifacts["struct_noise"] = raising
    with pytest.raises(Boom):
        gen.sample(None, seg_d, bank, key=_key(2))
    assert np_state_equal(n0, np.random.get_state()) and torch.equal(t0, torch.get_rng_state())
    from fetalsyngen_amd import rng as R

    assert not R.in_keyed_scope()


# ---- 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merge_type", ["perlin", "gaussian"])
def test_same_key_same_sample_volumetric_stages(subject, monkeypatch, merge_type):
    from fetalsyngen_amd.generator.artifacts import utils as U

    bank, seg_d, _twin = subject
    gen = generator(subject, NO_MOTION, merge_type=merge_type)
    k = _key(3)
    monkeypatch.setattr(U.time, "time", lambda: 1700000000.0)
    np.random.seed(1)
    a = gen._pipeline(None, seg_d, bank, {}, scale01=True, key=k)
    monkeypatch.setattr(U.time, "time", lambda: 1800000123.0)
    np.random.seed(2)
    torch.manual_seed(2)
    b = gen._pipeline(None, seg_d, bank, {}, scale01=True, key=k)
    assert a[3]["artifacts"]["struct_noise"] and a[3]["artifacts"]["boundaries"]["fuzzy_on"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and _same(a[3], b[3])
    c = gen._pipeline(None, seg_d, bank, {}, scale01=True, key=_key(4))
    assert not torch.equal(a[0], c[0])


# ---- 4 ---------------------------------------------------------------------------------------------------------------
def test_same_key_with_motion_within_order_noise(subject):
    bank, seg_d, _twin = subject
    gen = generator(subject, {"blur_cortex": False, "struct_noise": False, "boundaries": False})
    k = _key(5)
    a = gen._pipeline(None, seg_d, bank, {}, scale01=False, key=k)
    np.random.seed(9)
    torch.manual_seed(9)
    b = gen._pipeline(None, seg_d, bank, {}, scale01=False, key=k)
    meta = a[3]["artifacts"]["simulate_motion"]
    assert meta and meta["nstacks"] >= 2 and {"resolution_slice", "slice_thickness", "gap"} <= meta.keys()
    assert _same(a[3], b[3]) and torch.equal(a[1], b[1])
    d = float((a[0] - b[0]).abs().max())
    print(f"motion, same key twice: max |diff| {d:.3e} (allowed {MOTION_ATOL:.3e}), image max {float(a[0].max()):.4f}")
    assert float(a[0].max()) <= 1.5  # the image is on the scale the bound was measured on
    assert d <= MOTION_ATOL


# ---- 5 ---------------------------------------------------------------------------------------------------------------
def test_stage_draws_do_not_depend_on_another_stage(subject):
    bank, seg_d, _twin = subject
    with_blur = generator(subject, NO_MOTION, merge_type="gaussian")
    without = generator(subject, {"simulate_motion": False, "blur_cortex": False}, merge_type="gaussian")
    k = _key(6)
    a = with_blur.sample(None, seg_d, bank, key=k)[3]["artifacts"]
    b = without.sample(None, seg_d, bank, key=k)[3]["artifacts"]
    assert a["blur_cortex"]["nblur"] is not None and b["blur_cortex"]["nblur"] is None
    assert a["struct_noise"] and _same(a["struct_noise"], b["struct_noise"]) and _same(a["boundaries"], b["boundaries"])


# ---- 6 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale01", [False, True])
def test_composition_by_hand(subject, scale01):
    from fetalsyngen_amd import kernels as K
    from fetalsyngen_amd import rng as R

    bank, seg_d, _twin = subject
    plain, art = generator(subject, stages=False), generator(subject, NO_MOTION)
    k = _key(7)
    got = art._pipeline(None, seg_d, bank, {}, scale01=scale01, key=k)
    img, lab, _i, params = plain._pipeline(None, seg_d, bank, {}, scale01=False, key=k)  # the image / max, as the stages get it
    meta = {}
    for name in STAGES:
        with R.keyed_scope(k, R.STAGE_STREAMS[name]):
            img, meta[name] = art.artifacts[name](img, lab, DEV, {}, resolution=art.resolution)
    if scale01:
        img = img.contiguous()
        img = K.scale(img, K.reduce_minmax(img), mode=1)
    assert torch.equal(got[0], img) and torch.equal(got[1], lab)
    assert _same(got[3]["artifacts"], meta) and _same(_without_artifacts(got[3]), _without_artifacts(params))


# ---- 7 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("streams", [1, 2])
def test_batch_equals_single_samples(subject, streams):
    """(SimulateMotion gated off: its order noise would not allow bit equality.)"""
    bank, seg_d, _twin = subject
    gen = generator(subject, NO_MOTION)
    keys = [_key(i, base=43) for i in range(3)]
    items = [(None, seg_d, bank)] * 3
    images, labels, _imgs, params = gen.sample_batch(items, scale01=True, streams=streams, keys=keys)
    torch.cuda.synchronize()
    assert tuple(images.shape) == (3, *S48)
    for b, k in enumerate(keys):
        one = gen._pipeline(None, seg_d, bank, {}, scale01=True, key=k)
        assert torch.equal(images[b], one[0]) and torch.equal(labels[b], one[1]) and _same(params[b], one[3])
        assert params[b]["artifacts"]["struct_noise"]


# ---- 8 ---------------------------------------------------------------------------------------------------------------
def test_replay_and_artifact_params(subject):
    bank, seg_d, _twin = subject
    gen = generator(subject, NO_MOTION)
    k = _key(8)
    a = gen.sample(None, seg_d, bank, key=k)
    b = gen.sample(None, seg_d, bank, genparams={"key": k})
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and _same(a[3], b[3])
    d = gen.sample(None, seg_d, bank, genparams={"key": k, "artifact_params": {"nblur": 7}})
    assert d[3]["artifacts"]["blur_cortex"] == {"nblur": 7} and a[3]["artifacts"]["blur_cortex"]["nblur"] != 7
    assert _same(d[3]["artifacts"]["struct_noise"], a[3]["artifacts"]["struct_noise"])
    assert _same(d[3]["artifacts"]["boundaries"], a[3]["artifacts"]["boundaries"])
    assert not torch.equal(a[0], d[0])


# ---- 9 ---------------------------------------------------------------------------------------------------------------
def test_blur_cortex_centres_are_the_contract_on_the_weight_volume(subject, monkeypatch):
    from fetalsyngen_amd import rng as R
    from fetalsyngen_amd.generator.augmentation import artifacts as A

    bank, seg_d, _twin = subject
    plain = generator(subject, stages=False)
    k = _key(9)
    img, lab, _i, _p = plain._pipeline(None, seg_d, bank, {}, scale01=False, key=k)
    stage = default_artifacts(prob=1.0)["blur_cortex"]
    calls, real = [], A.K.mog3d

    def recording(shape, centers, sigmas, device):
        calls.append(np.array(centers, dtype=np.float32))
        return real(shape, centers, sigmas, device)

    def forbidden(*_a, **_k):
        raise AssertionError("host pass over the cortex weights inside a keyed scope")

    monkeypatch.setattr(A.K, "mog3d", recording)
    monkeypatch.setattr(stage, "_cortex_weights", forbidden)
    monkeypatch.setattr(R, "multinomial_distinct", forbidden)
    with R.keyed_scope(k, R.STAGE_STREAMS["blur_cortex"]):
        _out, meta = stage(img, lab, DEV, {}, resolution=plain.resolution)
    monkeypatch.setattr(A.K, "mog3d", real)
    nblur = meta["nblur"]
    assert len(calls) == 2 and calls[1].shape == (nblur, 3)  # the blob field, then the blobs on the chosen centres
    with R.keyed_scope(k, R.STAGE_STREAMS["blur_cortex"]):
        u = torch.rand(2 * nblur + 8, dtype=torch.float64).numpy()  # the scope's first torch draw
    weight = stage._blob_field(S48, DEV).cpu().numpy()
    want = P.pick(lab.cpu().numpy(), "==", float(stage.cortex_label), nblur, u, weight)
    assert want[0] // 2 > nblur and want[1] == nblur  # one round of uniforms sufficed
    assert np.array_equal(calls[1], np.stack(np.unravel_index(want[2:], S48), -1).astype(np.float32))
