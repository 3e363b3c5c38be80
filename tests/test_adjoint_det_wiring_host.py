"""CPU: who asks for the deterministic adjoint.  The reconstruction does inside `rng.keyed_scope` (a keyed sample is a
function of its key) and does not outside it; the explicit switch on PSFReconstructor / SimulateMotion wins over both;
`slice_acquisition_adjoint(deterministic=None)` resolves the same way for a direct caller.  The kernels are replaced by
recorders: nothing here touches a device."""
from dataclasses import fields

import pytest
import torch

from fetalsyngen_amd import rng as R
from fetalsyngen_amd.generator.artifacts import simulate_reco as SR
from fetalsyngen_amd.generator.artifacts.svort import RigidTransform
from fetalsyngen_amd.generator.artifacts.svort import slice_acq as SA
from fetalsyngen_amd.generator.artifacts.utils import ReconMergeParams, ReconParams

KEY = 0x5EED5EED5EED5EED
VS = (6, 6, 6)


def _recon(deterministic=None, **kw):
    args = dict(prob_misreg_slice=0.0, slices_misreg_ratio=0.0, prob_misreg_stack=0.0, txy=0.0, prob_merge=0.0,
                merge_params=ReconMergeParams(merge_type="gaussian", gauss_ngaussians_min=1, gauss_ngaussians_max=3),
                prob_smooth=0.0, prob_rm_slices=0.0, rm_slices_min=0.0, rm_slices_max=0.0)
    args.update(kw)
    return SR.PSFReconstructor(**args) if deterministic is None else SR.PSFReconstructor(**args, deterministic=deterministic)


def _data(n=4):
    trf = RigidTransform(torch.zeros(n, 6), trans_first=True)
    return {"psf_rec": torch.ones(2, 2, 2), "slice_shape": (5, 5), "resolution_slice": 1.0, "resolution_recon": 1.0,
            "slice_thickness": 3.0, "volume_shape": VS, "stacks": torch.zeros(n, 1, 5, 5), "transforms_angle": trf,
            "transforms_gt_angle": trf, "positions": torch.stack([torch.arange(n), torch.zeros(n)], 1),
            "seg_gt": torch.ones(1, 1, *VS), "volume_gt": torch.zeros(1, 1, *VS)}


@pytest.fixture
def seen(monkeypatch):
    calls = []

    def adjoint(transforms, psf, slices, slices_mask, vol_mask, vol_shape, res_slice, interp_psf, equalize, semantics=None,
                slice_ids=None, deterministic="absent"):
        calls.append(deterministic)
        return torch.zeros(1, 1, *vol_shape)

    monkeypatch.setattr(SR, "slice_acquisition_adjoint", adjoint)
    monkeypatch.setattr(SR.K, "_upload", lambda host, device: host)
    return calls


def test_recon_psf_is_deterministic_inside_a_keyed_scope_only(seen):
    _recon().recon_psf(_data(), want_weight=False)
    with R.keyed_scope(KEY, R.STAGE_STREAMS["simulate_motion"]):
        _recon().recon_psf(_data(), want_weight=False)
    _recon().recon_psf(_data(), want_weight=False)
    assert seen == [False, True, False]


@pytest.mark.parametrize("forced", [True, False])
def test_the_explicit_switch_wins_over_both(seen, forced):
    _recon(deterministic=forced).recon_psf(_data(), want_weight=False)
    with R.keyed_scope(KEY, 18):
        _recon(deterministic=forced).recon_psf(_data(), want_weight=False)
    assert seen == [forced, forced]


def test_simulate_motion_hands_its_switch_to_the_reconstructor(monkeypatch):
    from fetalsyngen_amd.generator.augmentation import artifacts as A

    built = []

    class Recon:
        def __init__(self, **kw):
            built.append(kw)

        def recon_psf(self, data, want_weight=True):
            return torch.zeros(1, 1, *VS), None

        def get_seeds(self):
            return {}

    class Scan:
        def __init__(self, **kw):
            pass

        def scan(self, d):
            return {"resolution_recon": 1.0, "resolution_slice": 1.0, "slice_thickness": 1.0, "gap": 1.0,
                    "positions_host": torch.zeros(3, 2)}

    monkeypatch.setattr(A, "PSFReconstructor", Recon)
    monkeypatch.setattr(A, "Scanner", Scan)
    monkeypatch.setattr(A, "_need_gpu", lambda *a: None)
    monkeypatch.setattr(A.K, "threshold", lambda x, v: (x > v).float())
    recon_params = ReconParams(prob_misreg_slice=0.0, slices_misreg_ratio=0.0, prob_misreg_stack=0.0, txy=0.0, prob_smooth=0.0,
                               prob_rm_slices=0.0, rm_slices_min=0.0, rm_slices_max=0.0, prob_merge=0.0,
                               merge_params=ReconMergeParams(merge_type="gaussian"))
    scanner_params = A.ScannerParams(**{f.name: None for f in fields(A.ScannerParams)})
    vol = torch.zeros(VS)
    for kw, want in (({}, None), ({"deterministic": True}, True), ({"deterministic": False}, False)):
        stage = A.SimulateMotion(1.0, scanner_params, recon_params, **kw)
        assert stage.deterministic is want
        stage(vol, vol, "cpu", resolution=(1.0, 1.0, 1.0))
        assert built[-1]["deterministic"] is want
        assert set(built[-1]) - {"deterministic"} == {f.name for f in fields(ReconParams)}


def test_slice_acquisition_adjoint_resolves_none_from_the_scope(monkeypatch):
    calls = []

    def k_adjoint(transforms, psf, slices, sm, vm, vol_shape, res_slice, **kw):
        calls.append((kw["deterministic"], kw["semantics"]))
        return torch.zeros(vol_shape)

    monkeypatch.setattr(SA.K, "slice_acq_adjoint", k_adjoint)
    args = (torch.zeros(2, 3, 4), torch.ones(2, 2, 2), torch.zeros(2, 1, 5, 5), None, None, VS, 1.0, True, True)
    SA.slice_acquisition_adjoint(*args)
    SA.slice_acquisition_adjoint(*args, deterministic=True)
    with R.keyed_scope(KEY, 18):
        SA.slice_acquisition_adjoint(*args)
        SA.slice_acquisition_adjoint(*args, deterministic=False)
        SA.slice_acquisition_adjoint(*args, semantics="torch")  # no deterministic variant of the fallback's arithmetic
    assert calls == [(False, "cuda"), (True, "cuda"), (True, "cuda"), (False, "cuda"), (False, "torch")]
