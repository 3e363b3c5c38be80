"""What the generator remembers about a caller's tensors: the uint8 twin of a label volume, the intensity prior of a real
image, the operand checks of the fused path.  A tensor is recognised as an OBJECT (its `id()`, a weak reference that must
still resolve to it, its in-place `_version`), nothing keeps it alive, and the bytes held are budgeted.

The generator-level tests drive CPU tensors through the generator's own methods (no GPU is initialised) and state what
these caches did when each of them carried its own copy of the policy; the tests at the end are about the one class that
holds it now, `fetalsyngen_amd.identity.IdentityCache`.
"""
import gc
import types
import weakref

import pytest
import torch

from tests.util_cases import make_generator

SHAPE = (8, 8, 8)  # 512 voxels: a 512 B twin, a 2048 B prior


@pytest.fixture
def gen():
    return make_generator(SHAPE, "cuda:0", rng="device")


def _labels(fill=None):
    if fill is not None:
        return torch.full(SHAPE, float(fill))
    return (torch.arange(512).reshape(SHAPE) % 7).float()


def _stats(gen, name):
    """(entries, bytes) of the generator's cache `name`; an attribute that is not there holds nothing.  (A dict with these
    two keys is the layout the facts below were first pinned against.)"""
    cache = gen.__dict__.get(name)
    if cache is None:
        return 0, 0
    if isinstance(cache, dict):
        return len(cache["by_id"]), cache["bytes"]
    return len(cache), cache.bytes


def _count_priors(gen):
    """Replace the two-kernel prior by a CPU function that counts its calls."""
    calls = []

    def prior(image):
        calls.append(id(image))
        return (image * 2).contiguous()

    gen._intensity_prior = prior
    return calls


# ---- label twins -----------------------------------------------------------------------------------------------------------
def test_twin_is_made_on_the_second_sighting_and_kept(gen):
    seg = _labels()
    assert gen._label_twin(seg) is None
    assert _stats(gen, "_twins") == (1, 0)
    twin = gen._label_twin(seg)
    assert twin.dtype == torch.uint8 and twin.shape == seg.shape and torch.equal(twin.float(), seg)
    assert gen._label_twin(seg) is twin and gen._label_twin(seg) is twin
    assert _stats(gen, "_twins") == (1, 512)


@pytest.mark.parametrize("bad", [0.5, -1.0, 256.0])
def test_no_twin_for_a_volume_that_is_not_integers_in_0_255(gen, bad):
    seg = _labels()
    seg[3, 4, 5] = bad
    for _ in range(4):
        assert gen._label_twin(seg) is None
    assert _stats(gen, "_twins") == (1, 0)


def test_in_place_write_puts_a_twin_back_to_first_sighting(gen):
    seg = _labels()
    gen._label_twin(seg)
    assert gen._label_twin(seg) is not None
    seg.add_(0)  # same values, new `_version`
    assert gen._label_twin(seg) is None
    assert _stats(gen, "_twins") == (1, 0)
    twin = gen._label_twin(seg)
    assert twin is not None and torch.equal(twin.float(), seg)
    assert _stats(gen, "_twins") == (1, 512)


def test_twin_budget_evicts_the_oldest_twin_with_its_whole_entry(gen):
    gen.label_twin_budget_bytes = 600
    a, b = _labels(1), _labels(2)
    for seg in (a, a, b):
        gen._label_twin(seg)
    assert _stats(gen, "_twins") == (2, 512)
    assert gen._label_twin(b) is not None
    assert _stats(gen, "_twins") == (1, 512)  # a's entry is gone, not only its twin
    assert gen._label_twin(a) is None         # ... so a is at its first sighting again
    assert _stats(gen, "_twins") == (2, 512)
    twin_a = gen._label_twin(a)
    assert twin_a is not None and torch.equal(twin_a.float(), a)
    assert _stats(gen, "_twins") == (1, 512)  # and its twin evicted b's
    assert gen._label_twin(b) is None
    assert gen._label_twin(a) is twin_a


def test_twin_entry_goes_when_the_volume_dies(gen):
    seg, other = _labels(), _labels(3)
    for s in (seg, seg, other):
        gen._label_twin(s)
    assert _stats(gen, "_twins") == (2, 512)
    del seg, s
    gc.collect()
    assert _stats(gen, "_twins") == (1, 0)
    del other
    gc.collect()
    assert _stats(gen, "_twins") == (0, 0)


def test_register_label_twin_validates(gen):
    seg = _labels()
    with pytest.raises(ValueError):
        gen.register_label_twin(seg, seg.clone())  # float32
    with pytest.raises(ValueError):
        gen.register_label_twin(seg, torch.zeros((8, 8, 4), dtype=torch.uint8))
    with pytest.raises(ValueError):
        gen.register_label_twin(seg, None)
    assert _stats(gen, "_twins") == (0, 0)


def test_registered_twin_is_served_at_once_counted_and_evictable(gen):
    gen.label_twin_budget_bytes = 600
    a, b = _labels(1), _labels(2)
    twin = torch.full(SHAPE, 9, dtype=torch.uint8)  # not a's values: the registered twin is taken unchecked
    gen.register_label_twin(a, twin)
    assert gen._label_twin(a) is twin
    assert _stats(gen, "_twins") == (1, 512)
    again = twin.clone()
    gen.register_label_twin(a, again)  # the first one's bytes are released
    assert gen._label_twin(a) is again
    assert _stats(gen, "_twins") == (1, 512)
    gen._label_twin(b)
    assert gen._label_twin(b) is not None  # b's twin takes the room of the registered one
    assert _stats(gen, "_twins") == (1, 512)
    assert gen._label_twin(a) is None


# ---- image priors ----------------------------------------------------------------------------------------------------------
def test_prior_is_computed_once_per_tensor_object(gen):
    calls = _count_priors(gen)
    img = _labels()
    prior = gen._image_prior(img)
    assert torch.equal(prior, img * 2)
    assert gen._image_prior(img) is prior and gen._image_prior(img) is prior
    assert len(calls) == 1 and _stats(gen, "_priors") == (1, 2048)
    same_values = img.clone()  # another object: another prior
    assert gen._image_prior(same_values) is not prior
    assert len(calls) == 2 and _stats(gen, "_priors") == (2, 4096)


def test_prior_is_recomputed_after_an_in_place_write(gen):
    calls = _count_priors(gen)
    img = _labels()
    gen._image_prior(img)
    img.mul_(3)
    prior = gen._image_prior(img)
    assert torch.equal(prior, img * 2) and len(calls) == 2
    assert gen._image_prior(img) is prior and len(calls) == 2
    assert _stats(gen, "_priors") == (1, 2048)


def test_prior_that_does_not_fit_is_computed_per_call_and_not_stored(gen):
    calls = _count_priors(gen)
    gen.label_twin_budget_bytes = 2000
    img = _labels()
    for n in (1, 2, 3):
        assert torch.equal(gen._image_prior(img), img * 2)
        assert len(calls) == n and _stats(gen, "_priors") == (0, 0)


def test_oldest_computed_prior_is_evicted_first(gen):
    calls = _count_priors(gen)
    gen.label_twin_budget_bytes = 4100  # two priors
    a, b, c = _labels(1), _labels(2), _labels(3)
    for img in (a, b, c):  # c takes a's room
        gen._image_prior(img)
    assert len(calls) == 3 and _stats(gen, "_priors") == (2, 4096)
    gen._image_prior(c), gen._image_prior(b)
    assert len(calls) == 3
    gen._image_prior(a)  # takes b's room, the older of (b, c)
    assert len(calls) == 4 and _stats(gen, "_priors") == (2, 4096)
    gen._image_prior(c), gen._image_prior(a)
    assert len(calls) == 4
    gen._image_prior(b)
    assert len(calls) == 5


def test_registered_prior_is_served_uncounted_and_never_evicted(gen):
    calls = _count_priors(gen)
    gen.label_twin_budget_bytes = 2100  # one computed prior
    a, b, c = _labels(1), _labels(2), _labels(3)
    mine = torch.full(SHAPE, 7.0)
    gen.register_image_prior(a, mine)
    assert gen._image_prior(a) is mine and not calls
    assert _stats(gen, "_priors") == (1, 0)
    gen._image_prior(b), gen._image_prior(c)  # c takes b's room, the registered prior stays
    assert len(calls) == 2 and _stats(gen, "_priors") == (2, 2048)
    assert gen._image_prior(a) is mine and len(calls) == 2
    gen._image_prior(b)
    assert len(calls) == 3 and gen._image_prior(a) is mine


def test_register_image_prior_validates(gen):
    img = _labels()
    with pytest.raises(ValueError):
        gen.register_image_prior(img, torch.zeros((8, 8, 16))[:, :, ::2])  # right shape, not contiguous
    with pytest.raises(ValueError):
        gen.register_image_prior(img, torch.zeros(SHAPE, dtype=torch.float64))
    with pytest.raises(ValueError):
        gen.register_image_prior(img, torch.zeros((8, 8, 4)))
    assert _stats(gen, "_priors") == (0, 0)


# ---- all of them -----------------------------------------------------------------------------------------------------------
class _OnDevice(torch.Tensor):
    """A CPU tensor that says it is a device tensor: what `_native_operands` asks of a segmentation it remembers."""

    is_cuda = property(lambda self: True)


def _operands(seg, parts):
    return types.SimpleNamespace(shape=SHAPE, segmentation=seg, label_parts=parts, gm_off=(0, 0, 4))


def test_operands_are_checked_once_per_tensor_object_and_shape(gen):
    gen.device = "cpu"  # the checks run as they are, on tensors that live here
    seg = _labels().as_subclass(_OnDevice)
    parts = [torch.zeros(SHAPE, dtype=torch.uint8) for _ in range(3)]
    checks = gen._flat_buffers()["validated"]
    c = _operands(seg, parts)
    gen._native_operands(c)
    assert c.seg is seg and len(checks) == 4
    gen._native_operands(_operands(seg, parts[:2]))  # another combination of known tensors: nothing new
    assert len(checks) == 4
    bad = _operands(seg, [torch.zeros((8, 8, 4), dtype=torch.uint8)])
    with pytest.raises(ValueError):
        gen._native_operands(bad)
    assert len(checks) == 4
    host = _operands(_labels().double(), parts)  # converted: the copy is checked per call and never remembered
    gen._native_operands(host)
    assert len(checks) == 4


def test_invalidate_label_twins_empties_every_cache(gen):
    _count_priors(gen)
    gen.device = "cpu"
    seg = _labels().as_subclass(_OnDevice)
    gen._label_twin(seg), gen._label_twin(seg), gen._image_prior(seg)
    parts = [torch.zeros(SHAPE, dtype=torch.uint8)]
    gen._native_operands(_operands(seg, parts))
    assert _stats(gen, "_twins") == (1, 512) and _stats(gen, "_priors") == (1, 2048)
    assert len(gen._flat_buffers()["validated"]) == 2
    gen.invalidate_label_twins()
    assert _stats(gen, "_twins") == (0, 0) and _stats(gen, "_priors") == (0, 0)
    assert len(gen._flat_buffers()["validated"]) == 0
    assert gen._label_twin(seg) is None  # first sighting again


def test_caches_do_not_keep_the_generator_alive():
    gen = make_generator(SHAPE, "cuda:0", rng="device")
    _count_priors(gen)
    seg, img = _labels(), _labels(2)
    gen._label_twin(seg), gen._label_twin(seg), gen._image_prior(img)
    gen.register_label_twin(img, torch.zeros(SHAPE, dtype=torch.uint8))
    gen.register_image_prior(seg, torch.zeros(SHAPE))
    alive = weakref.ref(gen)
    del gen
    gc.collect()
    assert alive() is None
    del seg, img  # their death callbacks find no cache: nothing to do, nothing raised
    gc.collect()


# ---- the class -------------------------------------------------------------------------------------------------------------
def _cache(**kw):
    from fetalsyngen_amd.identity import IdentityCache

    return IdentityCache(**kw)


def test_identity_cache_entry_cap_clears_everything():
    cache = _cache(cap=2)
    objs = [torch.zeros(1) for _ in range(4)]
    for o in objs[:3]:
        cache.put(o, "v", nbytes=10)
    assert len(cache) == 3 and cache.bytes == 30  # the cap is looked at before an insert, like the 4096 of the generator
    cache.put(objs[0], "w", nbytes=20)  # a known object is replaced, whatever the size of the cache
    assert len(cache) == 3 and cache.bytes == 40 and cache.get(objs[0]) == "w"
    cache.put(objs[3], "v", nbytes=10)
    assert len(cache) == 1 and cache.bytes == 10
    assert cache.get(objs[3]) == "v" and cache.get(objs[0]) is None


def test_identity_cache_stale_id_is_a_miss():
    cache = _cache()
    a = torch.zeros(1)
    cache.put(a, "a")
    key = id(a)
    del a
    later = []
    for _ in range(64):  # the allocator usually hands the address out again at once
        later.append(torch.zeros(1))
        if id(later[-1]) == key:
            break
    assert len(cache) == 0 and all(cache.get(t) is None for t in later)
    # and an entry that outlived its object's id (which the death callback otherwise prevents) does not hit either
    b, c = torch.zeros(1), torch.zeros(1)
    cache.put(b, "b")
    cache._entries[id(c)] = cache._entries.pop(id(b))
    assert cache.get(c) is None and len(cache) == 0


def test_identity_cache_version_is_required_when_given():
    cache = _cache()
    t = torch.zeros(4)
    cache.put(t, "v", nbytes=16, stamp=t._version)
    assert cache.get(t, t._version) == "v"
    t.add_(1)
    assert cache.get(t, t._version) is None
    assert len(cache) == 0 and cache.bytes == 0  # a stale entry is dropped where it is found


def test_identity_cache_pair_key_misses_when_either_object_is_replaced():
    cache = _cache()

    class Bank:
        pass

    bank, seg = Bank(), torch.zeros(4)
    cache.put((bank, seg), "subject", stamp=seg._version)
    assert cache.get((bank, seg), seg._version) == "subject"
    assert cache.get((Bank(), seg), seg._version) is None
    assert cache.get((bank, seg), seg._version) == "subject"
    assert cache.get((bank, torch.zeros(4)), 0) is None
    assert cache.get((bank, seg), seg._version) == "subject"
    cache.put((None, seg), "seedless", stamp=seg._version)  # None stands for "no bank"
    assert cache.get((None, seg), seg._version) == "seedless" and len(cache) == 2
    del bank
    gc.collect()
    assert len(cache) == 1  # the pair went with its bank
    del seg
    gc.collect()
    assert len(cache) == 0


def test_identity_cache_room_is_made_oldest_first_among_entries_with_bytes():
    cache = _cache()
    pinned, a, b, c = (torch.zeros(1) for _ in range(4))
    cache.put(pinned, "pinned")  # no bytes: never a victim
    cache.put(a, "a", nbytes=40)
    cache.put(b, "b", nbytes=40)
    assert cache.make_room(40, budget=100) and cache.bytes == 40
    assert cache.get(a) is None and cache.get(b) == "b" and cache.get(pinned) == "pinned"
    cache.put(c, "c", nbytes=40)
    assert cache.make_room(40, budget=70) and cache.bytes == 0 and cache.get(pinned) == "pinned"
    cache.drop(pinned)
    assert cache.get(pinned) is None
