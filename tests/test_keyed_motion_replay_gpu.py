"""Keyed samples WITH SimulateMotion replay bit for bit (GPU, 48^3 phantom subject, stage parameters of
`generator.defaults.default_artifacts`, the helper pattern of test_keyed_artifacts_gpu.py).

Inside a keyed scope the reconstruction's scatter accumulates in 64-bit fixed point (fsg_slice_acq_adjoint_det_f32), so the
one stage whose fp32 atomics made a key's sample differ from run to run is a function of its key like the others: the same
key gives the same bits twice, under another LDS tuning, in a batch, on two streams and as a replay.  A stage forced to the
fp32-atomic path stays within the order noise that path always had (MOTION_ATOL of test_keyed_artifacts_gpu.py: 2^-20 on an
image divided by its maximum)."""
import numpy as np
import pytest
import torch

from tests.util_cases import default_artifacts, make_generator

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(nonlin_scale=(0.08, 0.2), bf_scale=(0.05, 0.2))
S48 = (48, 48, 48)
MOTION_ATOL = 4 * 2.384186e-07
STAGES = ("blur_cortex", "struct_noise", "simulate_motion", "boundaries")
MOTION_ONLY = {"blur_cortex": False, "struct_noise": False, "boundaries": False}


def _key(i, base=47):
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


def generator(subject, gates=None, deterministic=None):
    """A keyed generator with all four stages configured; `gates`: stage name -> on / off (default: all on);
    `deterministic`: the switch of its SimulateMotion stage."""
    arts = default_artifacts(prob=1.0, merge_type="perlin")
    on = {name: True for name in STAGES}
    on.update(gates or {})
    for name in STAGES[:3]:
        arts[name].prob = 1.0 if on[name] else 0.0
    b = arts["boundaries"]
    b.prob_no_mask, b.prob_halo, b.prob_fuzzy = (0.0, 1.0, 1.0) if on["boundaries"] else (1.0, 0.5, 0.5)
    arts["simulate_motion"].deterministic = deterministic
    gen = make_generator(S48, DEV, rng="keyed", prob=1.0, artifacts=arts, **KW)
    gen.register_label_twin(subject[1], subject[2])
    return gen


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a, b)
    if isinstance(a, (np.ndarray, list, tuple)):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


def _equal_samples(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and _same(a[3], b[3])


@pytest.mark.parametrize("gates", [MOTION_ONLY, None], ids=["motion_alone", "all_four_stages"])
@pytest.mark.parametrize("scale01", [False, True])
def test_same_key_twice_same_bits(subject, monkeypatch, gates, scale01):
    from fetalsyngen_amd.generator.artifacts import utils as U

    bank, seg_d, _twin = subject
    gen = generator(subject, gates)
    k = _key(1)
    monkeypatch.setattr(U.time, "time", lambda: 1700000000.0)
    np.random.seed(1)
    torch.manual_seed(1)
    a = gen._pipeline(None, seg_d, bank, {}, scale01=scale01, key=k)
    monkeypatch.setattr(U.time, "time", lambda: 1800000123.0)
    np.random.seed(9)
    torch.manual_seed(9)
    b = gen._pipeline(None, seg_d, bank, {}, scale01=scale01, key=k)
    meta = a[3]["artifacts"]["simulate_motion"]
    assert meta and meta["nstacks"] >= 2
    assert _equal_samples(a, b), f"max |diff| {float((a[0] - b[0]).abs().max()):.3e}"
    assert not torch.equal(a[0], gen._pipeline(None, seg_d, bank, {}, scale01=scale01, key=_key(2))[0])


def test_same_bits_under_another_tuning(subject):
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    bank, seg_d, _twin = subject
    gen = generator(subject, MOTION_ONLY)
    k = _key(3)
    a = gen._pipeline(None, seg_d, bank, {}, scale01=False, key=k)
    got = {}
    for tuning in ((512, 1, 0), (8192, 6, 1000)):
        assert lib.fsg_slice_acq_set_tuning(*tuning) == 0
        try:
            got[tuning] = gen._pipeline(None, seg_d, bank, {}, scale01=False, key=k)
        finally:
            lib.fsg_slice_acq_set_tuning(3072, 0, 20)
    prev = lib.fsg_set_tuning(_lib.TUNE.SA_DIRECT)
    try:
        got["direct"] = gen._pipeline(None, seg_d, bank, {}, scale01=False, key=k)
    finally:
        lib.fsg_set_tuning(prev)
    for name, b in got.items():
        assert _equal_samples(a, b), name


@pytest.mark.parametrize("streams", [1, 2])
def test_batch_with_motion_equals_single_samples(subject, streams):
    bank, seg_d, _twin = subject
    gen = generator(subject)
    keys = [_key(i, base=53) for i in range(3)]
    items = [(None, seg_d, bank)] * 3
    images, labels, _imgs, params = gen.sample_batch(items, scale01=True, streams=streams, keys=keys)
    torch.cuda.synchronize()
    assert tuple(images.shape) == (3, *S48)
    for b, k in enumerate(keys):
        one = gen._pipeline(None, seg_d, bank, {}, scale01=True, key=k)
        assert params[b]["artifacts"]["simulate_motion"]
        assert torch.equal(images[b], one[0]) and torch.equal(labels[b], one[1]) and _same(params[b], one[3])


def test_replay_with_motion(subject):
    bank, seg_d, _twin = subject
    gen = generator(subject)
    k = _key(4)
    a = gen.sample(None, seg_d, bank, key=k)
    np.random.seed(5)
    torch.manual_seed(5)
    b = gen.sample(None, seg_d, bank, genparams={"key": k})
    assert a[3]["artifacts"]["simulate_motion"] and _equal_samples(a, b)


def test_forced_float_stage_stays_within_its_order_noise(subject):
    bank, seg_d, _twin = subject
    k = _key(5)
    det = generator(subject, MOTION_ONLY)._pipeline(None, seg_d, bank, {}, scale01=False, key=k)
    also = generator(subject, MOTION_ONLY, deterministic=True)._pipeline(None, seg_d, bank, {}, scale01=False, key=k)
    flt = generator(subject, MOTION_ONLY, deterministic=False)._pipeline(None, seg_d, bank, {}, scale01=False, key=k)
    assert _equal_samples(det, also)
    assert _same(det[3], flt[3]) and torch.equal(det[1], flt[1])
    d = float((det[0] - flt[0]).abs().max())
    print(f"motion, deterministic against forced float: max |diff| {d:.3e} (allowed {MOTION_ATOL:.3e}), "
          f"image max {float(det[0].max()):.4f}")
    assert float(det[0].max()) <= 1.5  # the image is on the scale the bound was measured on
    assert d <= MOTION_ATOL
