"""GPU: the slice-acquisition forward (fsg_slice_acq_forward_f32) and the float adjoint (fsg_slice_acq_adjoint_f32), every route of
each, against float64 restatements that share no code with the kernels: tests/util_sa_forward64.forward and
tests/util_sa_adjoint_backward64.adjoint64.  The cases, the routes they are there for and the host census that proves a case
reaches its route are in tests/util_sa_forward_cases.py; DESIGN.md section 26 has the table.

Tolerance (none is derived from what a kernel gives): per case, mode and output 4 * E_cpu * max|float64|, E_cpu the difference of
the fp32-operation restatement to the float64 one, measured on the CPU and written down in util_sa_forward_cases (the CPU test
test_sa_forward64_reference.py asserts that the constants cover the measurements).  For the LINEAR fast and plate kernels the fp32
restatement states their lerp formula; for the adjoint it is util_sa_forward64.adjoint32, one float32 addition per contribution
as the kernels' atomics do (the form that carries the scatter sums in float64 does not state these sums: on the MI355X the LINEAR
adjoint reached up to 18.8 times its bound on multi_chunk, the NEAREST_PSF direct scatter up to 3.2).  The factor 4 is the project's own
(sections 18 to 22): the kernel's own summation order -- four tap phases, atomics, the LDS pre-sum.  On the exact-geometry cases the
weights are exact in both precisions: E_cpu = 0 there and the GPU has to give the float64 weight bit for bit.  Exact-zero
assertions are exact.  Each comparison prints the ratio error / bound before it asserts.
"""
import numpy as np
import pytest
import torch

from tests import util_sa_forward_cases as CS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEFAULT_TUNING = (3072, 0, 20)


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (and libfsg_hip.so); there is no fallback to skip to")
    from fetalsyngen_amd import kernels

    return kernels


@pytest.fixture(scope="module")
def L():
    from fetalsyngen_amd import _lib

    return _lib


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(x):
    return x.detach().cpu().numpy().astype(np.float64)


_REF = {}


def ref(kind, name, mode):
    """The float64 restatement of a case and mode, computed once and shared (read only)."""
    key = (kind, name, mode)
    if key not in _REF:
        _REF[key] = CS.forward_ref(name, mode) if kind == "fwd" else CS.adjoint_ref(name, mode)
    return _REF[key]


def within(label, got, want, e_cpu, per_slice=False):
    """max |got - want| <= 4 * e_cpu * max |want|; prints the ratio reached (0 / 0 counts as 0) and returns it"""
    bound = 4.0 * e_cpu * float(np.abs(want).max())
    err = np.abs(got - want)
    worst = float(err.max())
    ratio = 0.0 if worst == 0 else (worst / bound if bound > 0 else float("inf"))
    print(f"{label}: error {worst:.3e}, bound {bound:.3e}, ratio {ratio:.3f}")
    if per_slice:  # a permuted slice mapping cannot average out: every slice is named
        for i in range(err.shape[0]):
            assert float(err[i].max()) <= bound, (label, "slice", i, float(err[i].max()), bound)
    assert worst <= bound, (label, worst, bound)
    return ratio


class tuning:
    """fsg_set_tuning flags and fsg_slice_acq_set_tuning knobs for a block, both restored whatever happens"""

    def __init__(self, L, flags=0, knobs=None):
        self.lib, self.flags, self.knobs = L.load(), int(flags), knobs

    def __enter__(self):
        self.prev = self.lib.fsg_set_tuning(self.flags)
        try:
            if self.knobs is not None:
                assert self.lib.fsg_slice_acq_set_tuning(*self.knobs) == 0
        except BaseException:
            self.lib.fsg_set_tuning(self.prev)
            raise

    def __exit__(self, *exc):
        try:
            self.lib.fsg_slice_acq_set_tuning(*DEFAULT_TUNING)
        finally:
            self.lib.fsg_set_tuning(self.prev)


# ---- forward ---------------------------------------------------------------------------------------------------------------
def _fwd_runs(L, name, mode):
    """(label, tuning flags, E_cpu key) of the launches of a mode"""
    if mode == "lin_lerp":
        key = "lin_weights" if CS.census(CS.case(name))["route"] == "generic" else "lin_lerp"  # the generic kernel's own order
        return [("auto", 0, key), ("direct", L.TUNE.SA_FWD_DIRECT, key), ("plate", L.TUNE.SA_FWD_PLATE, key)]
    if mode == "lin_weights":
        return [("precise", L.TUNE.PRECISE_MATH, "lin_weights")]
    return [("auto", 0, mode)]


@pytest.mark.parametrize("name", CS.FORWARD_CASES)
def test_forward_against_float64(K, L, name):
    worst = 0.0
    for mode in CS.fwd_modes(name):
        interp_psf, with_vm, _ = CS.FWD_MODES[mode]
        c = CS.case(name, interp_psf)
        r = ref("fwd", name, mode)
        if c["kind"] == "lin_general":
            assert r["bounds_dist"].min() > 1e-3  # precondition: the bounds test cannot flip between fp32 and float64
        sm = np.ones(r["slices"].shape, bool) if c["sm"] is None else c["sm"]
        args = (dev(c["tr"]), dev(c["vol"]), dev(c["vm"]) if with_vm else None, dev(c["sm"]), dev(c["psf"]), c["ss"], c["res"])
        for label, flags, ekey in _fwd_runs(L, name, mode):
            with tuning(L, flags):
                s, w = K.slice_acq_forward(*args, need_weight=True, interp_psf=interp_psf)
                s1 = K.slice_acq_forward(*args, need_weight=False, interp_psf=interp_psf)
            assert torch.equal(s, s1), (name, mode, label, "need_weight=False changes the slices")
            s, w = host(s), host(w)
            e_s, e_w = CS.E_CPU_FWD[CS.row(name), ekey]
            per = name in CS.PER_SLICE
            worst = max(worst, within(f"{name} {mode} {label} slices", s, r["slices"], e_s, per),
                        within(f"{name} {mode} {label} weight", w, r["weight"], e_w, per))
            assert np.all(s[~sm] == 0) and np.all(w[~sm] == 0), (name, mode, label, "outside slices_mask")
            dead = r["weight"] == 0
            assert np.all(s[dead] == 0) and np.all(w[dead] == 0), (name, mode, label, "float64 weight 0")
    print(f"{name}: worst ratio {worst:.3f}")


# ---- float adjoint -----------------------------------------------------------------------------------------------------------
def _adj_runs(L, mode):
    """(label, tuning flags, knobs) of the launches of a mode"""
    if not CS.ADJ_MODES[mode][0]:
        return [("default", 0, None)]
    return [("default", 0, None), ("direct", L.TUNE.SA_DIRECT, None), ("fallback_heavy", 0, (256, 1, 0)), ("lds_heavy", 0, (4096, 3, 20))]


@pytest.mark.parametrize("name", CS.ADJOINT_CASES)
def test_float_adjoint_against_float64(K, L, name):
    worst = 0.0
    for mode, (interp_psf, with_vm) in CS.ADJ_MODES.items():
        c = CS.case(name, interp_psf)
        r = ref("adj", name, mode)
        sm = np.ones(c["g"].shape, bool) if c["sm"] is None else c["sm"]
        if c["kind"] != "exact":  # (exact geometry: the pixel weight is the same number in fp32 and float64, the cut cannot flip)
            live = sm & (r["pixel_weight"] > 0)
            assert np.all(np.abs(r["pixel_weight"][live] - 0.5) > 1e-3)
        untouched = r["vol_weight"] == 0
        empty = interp_psf and c["psf"].shape[0] == 1  # a one-plane PSF accepts no PSF coordinate in NEAREST_PSF
        assert untouched.any() and bool(untouched.all()) == empty
        tr, psf, g, dsm, vm = dev(c["tr"]), dev(c["psf"]), dev(c["g"]), dev(c["sm"]), dev(c["vm"]) if with_vm else None
        e_vol, e_w, e_eq = CS.E_CPU_ADJ[CS.row(name), mode]
        for label, flags, knobs in _adj_runs(L, mode):
            for equalize in (False, True):
                with tuning(L, flags, knobs):
                    v, vw = K.slice_acq_adjoint(tr, psf, g, dsm, vm, c["vs"], c["res"], interp_psf=interp_psf, equalize=equalize,
                                                return_weight=True)
                v, vw = host(v), host(vw)
                tag = f"{name} {mode} {label} eq{int(equalize)}"
                worst = max(worst, within(tag + " vol", v, r["vol_eq"] if equalize else r["vol"], e_eq if equalize else e_vol),
                            within(tag + " vol_weight", vw, r["vol_weight"], e_w))
                assert np.all(v[untouched] == 0) and np.all(vw[untouched] == 0), (tag, "voxels the reference leaves untouched")
        # slice_ids as a permutation: transform z reads slices[ids[z]] and slices_mask[ids[z]]
        n = c["g"].shape[0]
        ids = np.random.default_rng(n).permutation(n)
        gp, smp = np.empty_like(c["g"]), np.empty_like(sm)
        gp[ids], smp[ids] = c["g"], sm
        v, vw = K.slice_acq_adjoint(tr, psf, dev(gp), dev(smp), vm, c["vs"], c["res"], interp_psf=interp_psf, return_weight=True,
                                    slice_ids=torch.from_numpy(ids))
        worst = max(worst, within(f"{name} {mode} slice_ids vol", host(v), r["vol"], e_vol),
                    within(f"{name} {mode} slice_ids vol_weight", host(vw), r["vol_weight"], e_w))
    print(f"{name}: worst ratio {worst:.3f}")
