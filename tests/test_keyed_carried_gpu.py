"""Keyed look-ahead (GPU): the parameter block a sample fills for the next key belongs to ONE keyed context on one stream --
a sample of another shape in between neither uses nor disturbs it, and a context evicted from the generator takes its
carried block with it.  Every sample is, bit for bit, the (shape, key) sample of a fresh generator without look-ahead."""
import pytest
import torch

from tests.util_cases import make_generator

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(prob=1.0, nonlin_scale=(0.08, 0.2), bf_scale=(0.05, 0.2))  # prob 1: the deformation gate is open, the draw job rides
S32, S48 = (32, 32, 32), (48, 48, 48)


def _subject(shape):
    from fetalsyngen_amd.data.datasets import SeedBank
    from fetalsyngen_amd.phantom import make_seed_volumes

    seg, seeds = make_seed_volumes(shape, 1)
    return torch.from_numpy(seg).to(DEV), SeedBank(seeds, DEV)


def _keys(n, base=57):
    from fetalsyngen_amd import sharding

    return [sharding.sample_key(base, i) for i in range(n)]


def _generator():
    return make_generator(S48, DEV, rng="keyed", **KW)


def _sample(gen, subject, key, next_key=None):
    out, seg, _img, params = gen._pipeline(None, subject[0], subject[1], {}, scale01=True, key=key, next_key=next_key)
    assert params["key"] == key
    return out, seg


def _traced(gen):
    """The `draw_carried` fields of the samples traced since the last call (keyed samples only have one)."""
    got = [bool(tr.meta["draw_carried"]) for tr in gen.stage_traces]
    for tr in gen.stage_traces:
        tr.close()
    del gen.stage_traces[:]
    return got


def _equal(got, ref):
    return torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_a_carried_block_belongs_to_one_context():
    a, b = _subject(S32), _subject(S48)
    k0, k1 = _keys(2)
    fresh = _generator()
    ref = {(s, k): _sample(fresh, subj, k) for s, subj in (("a", a), ("b", b)) for k in (k0, k1)}
    gen = _generator()
    gen.stage_traces = []
    first = _sample(gen, a, k0, next_key=k1)
    assert gen.keyed_context(S32)._carried and not gen.keyed_context(S48)._carried, "the next sample's draw job rode along"
    other = _sample(gen, b, k1)    # the same key on the same stream, but another context: that block is not its own
    second = _sample(gen, a, k1)   # the context the block was filled for
    assert _traced(gen) == [False, False, True]
    assert _equal(first, ref["a", k0]) and _equal(other, ref["b", k1]) and _equal(second, ref["a", k1])
    assert not gen.keyed_context(S32)._carried and not gen.keyed_context(S48)._carried


def test_an_evicted_context_drops_its_carried_block():
    shapes = [S32, (32, 32, 40), (32, 40, 32), (40, 32, 32), (40, 40, 32)]  # the generator keeps four contexts
    subjects = [_subject(s) for s in shapes]
    k0, k1 = _keys(2, base=58)
    ref = _sample(_generator(), subjects[0], k1)
    gen = _generator()
    _sample(gen, subjects[0], k0, next_key=k1)
    kc = gen.keyed_context(S32)
    assert kc._carried
    for subj in subjects[1:]:
        _sample(gen, subj, k0)
    assert S32 not in gen._keyed and len(gen._keyed) == 4 and not kc._carried
    gen.stage_traces = []
    got = _sample(gen, subjects[0], k1)
    assert _traced(gen) == [False]
    assert _equal(got, ref)
