"""Keyed path: the conditional floor(min) launch is skipped where the host proves it a no-op, and the next sample's draw job
rides in the head launch.

The host verdict (fsg_keyed.hip: floormin_settled) bounds the sampling position of the eight corner voxels from above; where
every axis has a corner below 1 the faces job of the head leaves all three keys below key(1.0) and the full pass behind it
would return at once.  Checked here: skipping changes no bit of the image, the labels or the keys; a true verdict is never
wrong; a sample that needs the pass still gets it; the look-ahead carries as before; a draw job too large to be carried is
launched on its own.  Shapes: the last index n - 1 is no multiple of FACE_STEP = 4 on any axis, so the faces job's "last
index always included" rule is what brings the far corners in; the last axis is a multiple of 4 voxels long because the
fused blur + resample kernels take nothing else (36 x 30 x 42 leaves the keyed path altogether).
"""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.util_cases import make_generator

DEV = "cuda:0"
KW = dict(nonlin_scale=(0.08, 0.2), bf_scale=(0.05, 0.2))
S36, S64 = (36, 30, 44), (64, 56, 72)
KEY_ONE = 0x3F800000  # fsg_f2key(1.0f)
NKEYS = 64
# no rotation, no shear, scale < 1: the grid shrinks inside the volume, every corner keeps a coordinate >= 1 on every axis
SHRINK = {"deform_params": {"affine": {"rotations": np.zeros(3), "shears": np.zeros(3), "scalings": np.full(3, 0.9)}}}
SHRINK_RIGID = {"deform_params": {"affine": SHRINK["deform_params"]["affine"], "non_rigid": {"nonlin_std": 0.0}}}


def _keys(n, base=91):
    from fetalsyngen_amd import sharding

    return [sharding.sample_key(base, i) for i in range(n)]


def _subject(shape, variant=1):
    from fetalsyngen_amd.data.datasets import SeedBank
    from fetalsyngen_amd.phantom import make_seed_volumes

    seg, seeds = make_seed_volumes(shape, variant)
    return seg, seeds, SeedBank(seeds, DEV), torch.from_numpy(seg).to(DEV)


def _settled_fn():
    from fetalsyngen_amd import _lib

    f = _lib.load().fsg_internal_keyed_floormin_settled
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]
    return f


def _verdict(gen, shape, key, gp=None):
    """The host verdict of (key, genparams) as fsg_keyed_sample_run reaches it."""
    from fetalsyngen_amd import keyed

    kc = gen.keyed_context(shape)
    ov = keyed.overrides_of(gen._validated_genparams(gp), kc.cfg, DEV) if gp else None
    got = _settled_fn()(kc.handle, C.c_uint64(key), C.byref(ov.c) if ov is not None else None)
    assert got in (0, 1), got
    return bool(got)


def _sample(gen, subj, key, gp=None, next_key=None):
    """(image, labels, the three floor(min) keys read back from the sample's parameter block)."""
    out, seg, _img, params = gen._pipeline(None, subj[3], subj[2], gp or {}, scale01=True, key=key, next_key=next_key)
    assert params["key"] == key
    mus = params["seed_intensities"]["mus"]  # a view of the parameter block, whose first bytes are the keys (off_mm8 = 0)
    mm3 = torch.empty(0, dtype=torch.int32, device=mus.device).set_(mus.untyped_storage(), 0, (3,))
    return out, seg, mm3.cpu().tolist()


def _launched(gen):
    """Per sample traced since the last call: whether the floor(min) launch went out."""
    from fetalsyngen_amd import _lib

    got = []
    for tr in gen.stage_traces:
        n = int(tr.ids[tr.CAP])
        got.append(int(_lib.ST.FLOORMIN) in [int(v) for v in tr.ids[:n]])
        tr.close()
    del gen.stage_traces[:]
    return got


class _Tuning:
    def __init__(self, flag):
        from fetalsyngen_amd import _lib

        self.lib, self.flag = _lib.load(), int(flag)

    def __enter__(self):
        self.prev = self.lib.fsg_set_tuning(0)
        self.lib.fsg_set_tuning(self.prev | self.flag)

    def __exit__(self, *exc):
        self.lib.fsg_set_tuning(self.prev)


@pytest.fixture(scope="module")
def both_ways():
    """NKEYS consecutive keys plus two that shrink the grid, each run with the skip and with FSG_TUNE_NO_FLOORMIN_SKIP:
    [(key, genparams, verdict, (sample, launched) with the skip, (sample, launched) without)]."""
    from fetalsyngen_amd import _lib

    gen = make_generator(S36, DEV, rng="keyed", **KW)
    subj = _subject(S36)
    cases = [(k, None) for k in _keys(NKEYS)] + [(k, SHRINK) for k in _keys(2, base=92)]
    gen.stage_traces = []
    rows = []
    for key, gp in cases:
        a = _sample(gen, subj, key, gp)
        with _Tuning(_lib.TUNE.NO_FLOORMIN_SKIP):
            b = _sample(gen, subj, key, gp)
        la, lb = _launched(gen)
        rows.append((key, gp, _verdict(gen, S36, key, gp), (a, la), (b, lb)))
    gen.stage_traces = None
    return rows


@pytest.mark.gpu
def test_skipping_the_launch_changes_no_bit(both_ways):
    verdicts = [v for _k, _gp, v, _a, _b in both_ways]
    print(f"settled: {sum(verdicts)} of {len(verdicts)} samples at {S36}")
    assert any(verdicts) and not all(verdicts), "the keys must hold both verdicts"
    assert not any(v for _k, gp, v, _a, _b in both_ways if gp is not None), "a grid shrunk inside the volume is never settled"
    for key, gp, verdict, (a, launched_a), (b, launched_b) in both_ways:
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), f"key {key}: image or labels"
        assert a[2] == b[2], f"key {key}: floor(min) keys {a[2]} / {b[2]}"
        assert launched_a == (not verdict), f"key {key}: verdict {verdict}, launch {launched_a}"
        assert launched_b, f"key {key}: FSG_TUNE_NO_FLOORMIN_SKIP always launches"


@pytest.mark.gpu
def test_a_true_verdict_is_never_wrong(both_ways):
    """Hard condition: wherever the host said "settled", the three keys the sample left behind are below key(1.0) -- with the
    launch (the exact full pass would have had nothing to add) and without."""
    seen = 0
    for key, _gp, verdict, (a, _la), (b, _lb) in both_ways:
        if verdict:
            seen += 1
            for keys in (a[2], b[2]):
                assert all(k < KEY_ONE for k in keys), f"key {key}: settled, but the keys are {keys}"
    assert seen > 0


@pytest.mark.gpu
def test_the_full_pass_still_runs_where_it_is_needed():
    """Identity rotation, scale 0.9, no displacement: the minimum coordinate is 0.1 * centre = 1.75 / 1.45 / 2.15 on the three
    axes of 36 x 30 x 44, so no face voxel settles anything.  The verdict is false, the launch goes out, the keys have the
    exact floors and the sample is the oracle's (the bar of tests/test_keyed_overrides_gpu.py)."""
    from fetalsyngen_amd import kernels as K
    from tests.util_keyed_overrides import oracle_sample

    gen = make_generator(S36, DEV, rng="keyed", **KW)
    subj = _subject(S36)
    key = _keys(1, base=93)[0]
    assert not _verdict(gen, S36, key, SHRINK_RIGID)
    gen.stage_traces = []
    out, seg, keys = _sample(gen, subj, key, SHRINK_RIGID)
    assert _launched(gen) == [True]
    floors = [int(np.floor(np.array(k, dtype=np.int32).view(np.float32))) for k in keys]
    assert floors == [1, 1, 2], (keys, floors)
    _d, _ex, r = oracle_sample(gen.keyed_context(S36), K, S36, key, subj[0], subj[1], dict(prob=1.0, **KW),
                               SHRINK_RIGID)
    assert np.array_equal(seg.cpu().numpy().astype(np.uint8), r["seg"].numpy().astype(np.uint8)), "labels"
    np.testing.assert_allclose(out.cpu().numpy(), r["scaled"].numpy(), rtol=0, atol=2e-5)


@pytest.mark.gpu
def test_look_ahead_chain_with_the_draw_job_in_the_head():
    """Six consecutive keys with the next one named against the same keys without: bit-equal, with a wrong announcement at
    sample 1 and a sample whose deformation gate is off (no head launch, so nothing carries) in between.  `rode` -- seen as
    the carried block -- is reported as before: 1 exactly when a next key was named and the sample had its fused head."""
    from fetalsyngen_amd import sharding

    kw = dict(prob=0.5, **KW)
    gen = make_generator(S64, DEV, rng="keyed", **kw)
    kc = gen.keyed_context(S64)
    base = next(b for b in range(200)
                if [bool(kc.draws(sharding.sample_key(b, i)).deform_active) for i in range(6)] in
                ([True, True, True, False, True, True], [True, True, False, True, True, True]))
    keys = [sharding.sample_key(base, i) for i in range(6)]
    active = [bool(kc.draws(k).deform_active) for k in keys]
    subj = _subject(S64)
    ref_gen = make_generator(S64, DEV, rng="keyed", **kw)
    ref = [_sample(ref_gen, subj, k) for k in keys]
    gen.stage_traces = []
    carried = []
    for i, k in enumerate(keys):
        nxt = keys[i + 1] if i + 1 < len(keys) else None
        if i == 1:
            nxt ^= 1  # the wrong announcement: the block it fills is dropped by the next call
        got = _sample(gen, subj, k, next_key=nxt)
        assert torch.equal(got[0], ref[i][0]) and torch.equal(got[1], ref[i][1]) and got[2] == ref[i][2], f"sample {i}"
        carried.append(bool(kc._carried))
    assert carried == active[:-1] + [False], (carried, active)
    used = [bool(tr.meta["draw_carried"]) for tr in gen.stage_traces]
    assert used == [False] + [carried[i - 1] and i != 2 for i in range(1, 6)], used
    _launched(gen)


@pytest.mark.gpu
def test_a_draw_job_too_large_to_carry_is_launched_on_its_own():
    """A coarse grid range up to twice the volume: some keys' draw jobs have more workgroups than the head launch carries
    (4096).  Naming such a key as the next one used to fail the sample; now it is simply not carried (rode = 0) and both
    samples are those of a run without look-ahead."""
    kw = dict(nonlin_scale=(0.05, 2.0), bf_scale=(0.05, 0.2))
    gen = make_generator(S64, DEV, rng="keyed", **kw)
    kc = gen.keyed_context(S64)

    def blocks(d):  # fill_draw's grid (fsg_keyed.hip)
        nb, nf = int(np.prod(list(d.bias_dims))), int(np.prod(list(d.field_dims))) * 3
        return 1 + ((nb + 3) // 4 + (nf + 3) // 4 + 255) // 256

    draws = [(k, kc.draws(k)) for k in _keys(300, base=94)]
    small = next(k for k, d in draws if d.field_dims[1] * d.field_dims[2] * 3 <= 2048 and blocks(d) <= 4096)  # a fused head
    large = next(k for k, d in draws if blocks(d) > 4096)
    subj = _subject(S64)
    ref_gen = make_generator(S64, DEV, rng="keyed", **kw)
    ref = [_sample(ref_gen, subj, k) for k in (small, large)]
    first = _sample(gen, subj, small, next_key=large)
    assert not kc._carried, "rode = 0: the job was not carried"
    second = _sample(gen, subj, large)
    for got, want in ((first, ref[0]), (second, ref[1])):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def _host_config(shape, nonlin=(0.03, 0.06), bf=(0.004, 0.02), nonlin_std_max=4.0):
    """bench.py's build_generator (= tests/util_cases.make_generator's defaults) as a fsg_keyed_config: every gate on."""
    from fetalsyngen_amd import _lib

    labels = [0] + list(range(10, 50))
    classes = [0] + [10] * 10 + [20] * 10 + [30] * 10 + list(range(40, 50))
    c = _lib.KeyedConfig()
    c.shape[:] = list(shape)
    c.size[:] = list(shape)
    c.resolution[:] = [0.5, 0.5, 0.5]
    c.min_subclusters, c.max_subclusters, c.meta_labels = 1, 6, 4
    c.nlabels, c.n_seed_labels, c.tie_classes = max(labels) + 1, len(labels), 1
    for j, (a, b) in enumerate(zip(labels, classes)):
        c.seed_labels[j], c.generation_classes[j] = a, b
    c.deform_prob, c.flip_prb, c.max_rotation, c.max_shear, c.max_scaling = 1.0, 0.5, 20, 0.02, 0.1
    c.nonlinear, c.nonlin_scale_min, c.nonlin_scale_max, c.nonlin_std_max = 1, nonlin[0], nonlin[1], nonlin_std_max
    c.gamma_prob, c.gamma_std = 1.0, 0.1
    c.bias_prob, c.bf_scale_min, c.bf_scale_max, c.bf_std_min, c.bf_std_max = 1.0, bf[0], bf[1], 0.01, 0.3
    c.resample_prob, c.min_resolution, c.max_resolution = 1.0, 0.5, 1.5
    c.noise_prob, c.noise_std_min, c.noise_std_max = 1.0, 5, 15
    return c


@pytest.mark.parametrize("shape,std_max", [(S36, 4.0), (S36, 40.0), (S64, 4.0)])
def test_a_true_verdict_against_the_corner_positions_on_the_host(shape, std_max):
    """CPU only, many keys: the eight corner voxels' positions restated in numpy float64 from what the device reads -- the
    float32 coarse grid of the key (oracle/fsg_keyed_draws.py: device_normals, stream 3) through the registered tap tables
    (tables.axis_table) -- against the verdict, which knows neither.  Settled means: every axis has a corner below 1 by more
    than the 0.25 voxel margin.  std_max 40: displacements of the size of the volume, where the corners' nodes decide."""
    from fetalsyngen_amd import _lib, tables
    from oracle import fsg_keyed_draws as R

    lib = _lib.load()
    cfg = _host_config(shape, nonlin=KW["nonlin_scale"], bf=KW["bf_scale"], nonlin_std_max=std_max)
    h = C.c_void_p()
    _lib.check(lib.fsg_keyed_create(C.byref(cfg), C.byref(h)), "fsg_keyed_create")
    settled = _settled_fn()
    n = np.array(shape)
    centre = np.array([np.float32((s - 1) / 2.0) for s in shape], dtype=np.float64)
    seen = {True: 0, False: 0}
    try:
        for key in _keys(400, base=95):
            verdict = bool(settled(h, C.c_uint64(key), None))
            seen[verdict] += 1
            if not verdict:
                continue
            d = _lib.KeyedDraws()
            _lib.check(lib.fsg_keyed_draw(h, C.c_uint64(key), C.byref(d)), "fsg_keyed_draw")
            f = list(d.field_dims)
            field = (np.float32(d.nonlin_std) * R.device_normals(key, 3, f[0] * f[1] * f[2] * 3)).reshape(*f, 3).astype(np.float64)
            tabs = [tables.axis_table(_lib.KT.FIELD, f[a], shape[a]) for a in range(3)]
            A, c2 = np.array(d.A, dtype=np.float32).reshape(3, 3).astype(np.float64), np.array(d.c2).astype(np.float32).astype(np.float64)
            lowest = np.full(3, np.inf)
            for corner in range(8):
                idx = [(n[a] - 1) if (corner >> a) & 1 else 0 for a in range(3)]
                disp = field
                for a in range(3):  # x, then y, then z: the leading axis is the one interpolated
                    t = tabs[a][idx[a]]
                    disp = float(t["w_lo"]) * disp[int(t["lo"])] + float(t["w_hi"]) * disp[int(t["hi"])]
                pos = np.clip(A @ (np.array(idx) - centre + disp) + c2, 0, n - 1)
                lowest = np.minimum(lowest, pos)
            assert (lowest < 0.75).all(), f"key {key}: settled, but the corners' minima are {lowest}"
    finally:
        lib.fsg_keyed_destroy(h)
    print(f"{shape}, std_max {std_max}: settled {seen[True]} of 400")
    assert seen[True] > 0 and seen[False] > 0


def test_share_of_samples_that_go_without_the_launch():
    """CPU only: the verdict over 20 000 keys of the bench configuration at 256^3 (bench.py: build_generator, keys
    sample_key(1234, i)).  The share is a measurement -- printed and kept in profiles/r12_a_skip_rate.txt --, not a threshold:
    the assert is only that the skip happens at all."""
    from fetalsyngen_amd import _lib, sharding

    lib = _lib.load()
    c = _host_config((256, 256, 256))
    h = C.c_void_p()
    _lib.check(lib.fsg_keyed_create(C.byref(c), C.byref(h)), "fsg_keyed_create")
    settled = _settled_fn()
    n = 20000
    try:
        got = [settled(h, C.c_uint64(sharding.sample_key(1234, i)), None) for i in range(n)]
    finally:
        lib.fsg_keyed_destroy(h)
    assert set(got) <= {0, 1}
    text = (f"# host verdict \"floor(min) is settled\" (fsg_keyed.hip: floormin_settled) over the keys sample_key(1234, 0..{n - 1})\n"
            f"# of the bench configuration at 256^3; written by tests/test_floormin_skip.py\n"
            f"settled {sum(got)} of {n} = {100.0 * sum(got) / n:.2f} %\n")
    print(text)
    try:
        (Path(__file__).resolve().parent.parent / "profiles" / "r12_a_skip_rate.txt").write_text(text)
    except OSError:  # a read-only checkout: the figure is printed above
        pass
    assert sum(got) > 0
