"""Real-image samples, the parts that need no GPU: the header's new fields and indices, keyed draws in prior mode, the
dataset's argument checks."""
import ctypes as C

import pytest

from fetalsyngen_amd import _lib


def test_header_has_the_real_image_fields_and_indices():
    assert [n for n, _t in _lib.SampleImage._fields_] == ["image_in", "image_out", "prior_in"]
    assert all(t is C.c_void_p for _n, t in _lib.SampleImage._fields_)
    assert not {"image_in", "image_out", "prior_in"} & {n for n, _t in _lib.SamplePlan._fields_}  # the plan keeps its layout
    ki = _lib.KEYED_I
    assert (ki.IMAGE_IN, ki.IMAGE_OUT, ki.PRIOR_IN) == (ki.NEXT_BLOCK + 1, ki.NEXT_BLOCK + 2, ki.NEXT_BLOCK + 3)
    assert ki.COUNT == ki.PRIOR_IN + 1
    assert _lib.PLAN_I.COUNT == _lib.PLAN_I.TRACE_CAP + 1 and not hasattr(_lib.PLAN_I, "IMAGE_IN")
    res, args = _lib.PROTOTYPES["fsg_sample_run_image"]
    assert res is C.c_int and args == [C.POINTER(_lib.SamplePlan), C.POINTER(_lib.SampleImage), C.c_void_p]
    assert _lib.ABI_VERSION >= 4
    res, args = _lib.PROTOTYPES["fsg_warp_dual_f32"]
    assert res is C.c_int and len(args) == 13 and args[0] is C.POINTER(_lib.Deform) and args[11] is C.POINTER(_lib.Epilogue)
    assert args[6] is C.c_size_t


def test_library_reports_the_new_layout():
    lib = _lib.load()
    assert lib.fsg_abi_version() == _lib.ABI_VERSION
    assert lib.fsg_sample_plan_layout(_lib.SIZEOF.SAMPLE_IMAGE) == C.sizeof(_lib.SampleImage) == 3 * C.sizeof(C.c_void_p)
    assert lib.fsg_sample_run_image(None, None, None) == _lib.E_BADARG  # no plan: refused before any HIP call


def _config(min_sub, max_sub, meta):
    c = _lib.KeyedConfig()
    c.shape[:] = [64, 56, 72]
    c.size[:] = [64, 56, 72]
    c.resolution[:] = [0.5, 0.5, 0.5]
    c.min_subclusters, c.max_subclusters, c.meta_labels = min_sub, max_sub, meta
    c.nlabels, c.n_seed_labels, c.tie_classes = 50, 0, 0
    c.deform_prob, c.flip_prb, c.max_rotation, c.max_shear, c.max_scaling = 0.9, 0.5, 20, 0.02, 0.1
    c.nonlinear, c.nonlin_scale_min, c.nonlin_scale_max, c.nonlin_std_max = 1, 0.08, 0.2, 4
    c.gamma_prob, c.gamma_std = 0.7, 0.1
    c.bias_prob, c.bf_scale_min, c.bf_scale_max, c.bf_std_min, c.bf_std_max = 0.7, 0.05, 0.2, 0.01, 0.3
    c.resample_prob, c.min_resolution, c.max_resolution = 0.7, 0.5, 1.5
    c.noise_prob, c.noise_std_min, c.noise_std_max = 0.7, 5, 15
    return c


def test_non_gmm_draws_do_not_depend_on_the_gmm_draws():
    """Prior mode leaves the GMM draws unused.  Every draw has a fixed counter, so a key's deformation, gamma, bias,
    resampling and noise draws are those of seed mode whatever the seed configuration is: two contexts that differ in every
    GMM-side setting agree on all non-GMM fields of fsg_keyed_draws."""
    lib = _lib.load()
    gmm_side = {"subclusters", "ntab", "off_mm8", "off_slots", "off_mus", "off_sigmas", "off_bias", "off_field", "block_bytes", "rode"}
    hs = []
    for cfg in (_config(1, 6, 4), _config(2, 3, 1)):
        h = C.c_void_p()
        _lib.check(lib.fsg_keyed_create(C.byref(cfg), C.byref(h)), "create")
        hs.append(h)
    try:
        seen_gates = set()
        for key in range(1, 60):
            ds = []
            for h in hs:
                d = _lib.KeyedDraws()
                _lib.check(lib.fsg_keyed_draw(h, C.c_uint64(key * 0x9E3779B97F4A7C15 & (2**64 - 1)), C.byref(d)), "draw")
                ds.append(d)
            for name, _t in _lib.KeyedDraws._fields_:
                if name in gmm_side:
                    continue
                a, b = getattr(ds[0], name), getattr(ds[1], name)
                a, b = (list(a), list(b)) if hasattr(a, "__len__") else (a, b)
                assert a == b, (key, name)
            seen_gates.add((ds[0].deform_active, ds[0].gamma_active, ds[0].bias_active, ds[0].resample_active, ds[0].noise_active))
        assert len(seen_gates) > 4  # the keys exercise open and closed gates
    finally:
        for h in hs:
            lib.fsg_keyed_destroy(h)


class _Gen:
    device = "cuda:0"

    def _is_keyed(self):
        return True


def test_dataset_argument_checks(tmp_path):
    from fetalsyngen_amd.data.datasets import FetalSynthDataset
    from tests.util_bids import write_tree

    bids, seeds_root = write_tree(tmp_path, (8, 8, 8), ["sub-00"])
    with pytest.raises(ValueError, match="exclude each other"):
        FetalSynthDataset(str(bids), _Gen(), str(seeds_root), None, seeds_from_images=3)
    ds = FetalSynthDataset(str(bids), _Gen(), None, None, load_image=False, image_as_intensity=True)
    with pytest.raises(ValueError, match="an image must be loaded"):
        ds.sample_batch([0])
    ds = FetalSynthDataset(str(bids), _Gen(), None, None, load_image=False)
    with pytest.raises(ValueError, match="seeds, an image"):
        ds.sample_batch([0])
    ds = FetalSynthDataset(str(bids), _Gen(), str(seeds_root), None, load_image=True, cache_on_device=False)
    with pytest.raises(ValueError, match="cache_on_device=True"):
        ds.sample_batch([0])
    assert not ds._keyed_images() and ds._has_seeds()
    assert FetalSynthDataset(str(bids), _Gen(), str(seeds_root), None, load_image=True)._keyed_images()
