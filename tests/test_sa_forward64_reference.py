"""CPU: what tests/test_sa_forward_edges_gpu.py rests on.

  * the restatement tests/util_sa_forward64.forward in float32 is the oracle's slice_acq_forward_cuda (measured here: the same
    BITS in slices and weight, LINEAR and NEAREST_PSF, with and without masks, at the golden shape and on two of the cases), and
    in float64 it reproduces the hand-derived closed forms of tests/test_sr_known_answers.py;
  * every case reaches the route it is there for (the host census of util_sa_forward_cases);
  * the E_cpu constants cover what this CPU measures;
  * every mutant of the restatement moves some output of every route class by more than the bound the GPU test uses for that case.
"""
import numpy as np
import pytest

from oracle import fsg_oracle_sr as S
from tests import test_sr_known_answers as KA
from tests import util_sa_backward_cases as BC
from tests import util_sa_forward64 as FW
from tests import util_sa_forward_cases as CS
from tests.util_sa_adjoint_backward64 import adjoint64

F32, F64 = np.float32, np.float64

_REF = {}


def ref(kind, name, mode):
    key = (kind, name, mode)
    if key not in _REF:
        _REF[key] = CS.forward_ref(name, mode) if kind == "fwd" else CS.adjoint_ref(name, mode)
    return _REF[key]


# ---- the restatement is the operator ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp_psf", [False, True], ids=["linear", "nearest_psf"])
@pytest.mark.parametrize("masks", [False, True], ids=["nomask", "masks"])
def test_float32_restatement_has_the_bits_of_the_oracle(golden, interp_psf, masks):
    g = golden("slice_acq")
    stacks = [(g["transforms"], g["vol"], g["vol_mask"], g["slices_mask"], g[f"psf_{pk}"], (14, 18), 1.3) for pk in ("aniso", "iso")]
    for name in ("psf335", "sparse"):
        c = CS.case(name)
        stacks.append((c["tr"], c["vol"], c["vm"], c["sm"], c["psf"], c["ss"], c["res"]))
    for tr, vol, vm, sm, psf, ss, res in stacks:
        vm, sm = (vm, sm) if masks else (None, None)
        es, ew = S.slice_acq_forward_cuda(tr, vol, vm, sm, psf, ss, res, True, interp_psf)
        r = FW.forward(tr, vol, vm, psf, sm, ss, res, interp_psf, F32)
        assert r["slices"].dtype == F32 and np.any(es != 0)
        assert np.array_equal(r["slices"], es) and np.array_equal(r["weight"], ew)
        if not interp_psf and not masks:  # LINEAR is continuous: float64 is close (NEAREST_PSF may flip a decision at these general poses)
            r64 = FW.forward(tr, vol, vm, psf, sm, ss, res, interp_psf, F64)
            assert np.abs(r64["slices"] - es).max() <= 2e-5 * np.abs(es).max()


@pytest.mark.parametrize("tx", [0.0, 0.5])
def test_float64_restatement_reproduces_the_known_answers(tx):
    vol, psf, _ = KA._case()
    for interp_psf, expected in ((False, KA._expected_forward_linear), (True, KA._expected_forward_nn)):
        r = FW.forward(KA._transform(tx), vol, None, psf, None, KA.SS, 1.0, interp_psf)
        es, ew = expected(vol.astype(F64), psf.astype(F64), tx)  # (in float64 throughout)
        np.testing.assert_allclose(r["slices"][0], es, rtol=1e-13)
        np.testing.assert_allclose(r["weight"][0], ew, rtol=1e-13)
        assert np.all(r["k"] == (8 if interp_psf else 27 * 8))
    r = FW.forward(KA._transform(tz=5.5), vol, None, psf, None, KA.SS, 1.0, False)
    assert not r["slices"].any() and not r["weight"].any() and not r["k"].any()


def test_lerp_form_and_vol_mask():
    c = CS.case("psf335")
    a, b = CS.forward_ref("psf335", "lin_weights"), FW.forward(c["tr"], c["vol"], None, c["psf"], c["sm"], c["ss"], c["res"], False, F64, "lerp")
    assert np.abs(a["slices"] - b["slices"]).max() < 1e-13 and np.array_equal(a["weight"], b["weight"]) and np.array_equal(a["k"], b["k"])
    # a masked corner leaves value and weight: with the mask the weight is the sum over the unmasked corners only
    m = CS.forward_ref("psf335", "lin_vm")
    live = a["weight"] > 0
    assert np.all(m["weight"] <= a["weight"]) and np.any(m["weight"][live] < a["weight"][live]) and np.all(m["k"] <= a["k"])
    # the all-ones mask is no mask
    o = FW.forward(c["tr"], c["vol"], np.ones(c["vs"], bool), c["psf"], c["sm"], c["ss"], c["res"], True)
    assert np.array_equal(o["slices"], CS.forward_ref("psf335", "nn")["slices"])
    with pytest.raises(ValueError):
        FW.forward(c["tr"], c["vol"], c["vm"], c["psf"], c["sm"], c["ss"], c["res"], False, F32, "lerp")


def test_equalized_is_the_equalisation_of_adjoint64():
    c = CS.case("psf335")
    want = adjoint64(c["tr"], c["psf"], c["g"], c["sm"], c["vm"], c["vs"], c["res"], False, True)
    got = CS.adjoint_ref("psf335", "lin_vm")
    assert np.array_equal(got["vol_eq"], want["vol"]) and np.array_equal(got["vol_weight"], want["vol_weight"])


@pytest.mark.parametrize("mode", list(CS.ADJ_MODES))
def test_adjoint32_is_adjoint64_in_float32_with_float32_sums(mode):
    """the same pixel weights and the same untouched voxels as adjoint64(ft=float32); the volumes differ by the rounding of the
    float32 additions alone: at most k * 2^-24 * (sum of magnitudes) for k contributions, here bounded by the whole stack's count"""
    interp_psf, with_vm = CS.ADJ_MODES[mode]
    c = CS.case("psf335")
    a = CS.adjoint_ref("psf335", mode, F32)
    b = adjoint64(c["tr"], c["psf"], c["g"], c["sm"], c["vm"] if with_vm else None, c["vs"], c["res"], interp_psf, False, F32)
    assert a["vol"].dtype == F32 and np.array_equal(a["pixel_weight"], b["pixel_weight"])
    assert np.array_equal(a["vol_weight"] == 0, b["vol_weight"] == 0) and np.any(a["vol_weight"] != b["vol_weight"])
    k = 8 * c["psf"].size * c["g"].shape[1] * c["g"].shape[2]  # no voxel receives more contributions from a slice
    assert np.abs(a["vol_weight"].astype(F64) - b["vol_weight"]).max() <= k * 2.0 ** -24 * np.abs(b["vol_weight"]).max()


# ---- every case reaches its route ---------------------------------------------------------------------------------------------
def test_census():
    cen = {name: CS.census(CS.case(name)) for name in CS.EXACT_NAMES}
    for name in ("psf335", "psf223", "psf133", "psf223_big", "sparse"):  # one chunk, both selections in one launch pair
        assert cen[name]["route"] == "two_launches" and cen[name]["slices_direct"] > 0 and cen[name]["slices_plate"] > 0, name
        assert cen[name]["chunks_min"] == cen[name]["chunks_max"] == 1 and cen[name]["direct_planes"] == 0, name
    assert cen["psf223_big"]["tiles"] == 6
    assert cen["delta"]["route"] == "single_tap"
    for name in ("multi_chunk", "tall"):
        assert cen[name]["slices_direct"] > 0 and cen[name]["slices_plate"] > 0 and cen[name]["chunks_max"] >= 2, name
        assert cen[name]["tiles_multi_plane"] > 0 and cen[name]["direct_planes"] == 0, name
    assert cen["tall"]["chunks_min"] == 1
    assert cen["wide"]["route"] == "two_launches" and cen["wide"]["slices_plate"] > 0 and 24 <= cen["wide"]["direct_planes"]
    assert cen["plate_limit"]["route"] == "two_launches" and cen["plate_limit"]["slices_plate"] > 0 and cen["plate_limit"]["chunks_max"] >= 2
    assert cen["direct_only"]["route"] == "direct_only" and cen["generic_big"]["route"] == "generic"
    assert cen["sparse"]["rounds"] == 2 and cen["sparse"]["empty_planes"] == 1 and 0 < cen["sparse"]["taps"] < 0.8 * 105
    assert cen["sparse_zero"]["taps"] == 0 and cen["sparse_zero"]["slices_direct"] > 0 and cen["sparse_zero"]["slices_plate"] > 0
    groups = {n: cen["counts_n%d_13x11" % n]["groups"] for n in CS.COUNTS_N}
    assert groups == {1: 1, 8: 1, 9: 2, 17: 3}
    for n in (8, 9, 17):  # slices beyond the first XCD round in both launches
        for ss in CS.COUNTS_SS:
            c = cen["counts_n%d_%dx%d" % (n, *ss)]
            assert c["slices_direct"] >= 4 and c["slices_plate"] >= 4, (n, ss)
    assert cen["counts_n17_37x29"]["tiles"] == 6
    for ss in CS.SHAPES_SS:
        c = cen["shapes_%dx%d" % ss]
        assert c["slices_direct"] == 1 and c["slices_plate"] == 1 and c["chunks_max"] == 1, ss
    assert {CS.adjoint_tile(name) for name in CS.ADJOINT_CASES} == {8, 16}  # the default tuning covers both adjoint tiles


def test_preconditions_of_the_cases():
    # some slices of an exact stack reach past a face, some pixels are live
    for name in CS.EXACT_NAMES:
        if name in ("sparse_zero", "shapes_faces") or name.startswith(("shapes_1x", "counts_n1_")):
            continue
        r = ref("fwd", name, "lin_weights")
        full = 8 * int((CS.case(name)["psf"] != 0).sum())
        sm = np.ones(r["k"].shape, bool) if CS.case(name)["sm"] is None else CS.case(name)["sm"]
        assert np.any(r["k"][sm] < full) and np.any(r["weight"] > 0), name
    # beyond every face, and without a tap: exact zeros, also in weight
    for name in ("shapes_faces", "sparse_zero"):
        for mode in CS.fwd_modes(name):
            r = ref("fwd", name, mode)
            assert not r["slices"].any() and not r["weight"].any(), (name, mode)
    # the LINEAR interior stacks: no tap coordinate near a face, so the bounds test cannot flip
    for name in CS.LIN_GENERAL:
        assert ref("fwd", name, "lin_weights")["bounds_dist"].min() > 1e-3, name
    # the GENERAL cases under their margin mask: a real stack, no decision near its point, no pixel weight near the 0.5 cut
    for name in CS.GEN_NAMES:
        for interp_psf in (False, True):
            c = CS.case(name, interp_psf)
            assert c["sm"].sum() > 200, (name, interp_psf)
            assert min(BC.reference(c, interp_psf)["dist"].values()) > 1e-3, (name, interp_psf)
            pw = ref("adj", name, "nn" if interp_psf else "lin")["pixel_weight"]
            live = c["sm"] & (pw > 0)
            assert live.sum() > 200 and np.all(np.abs(pw[live] - 0.5) > 1e-3), (name, interp_psf)


# ---- the constants ---------------------------------------------------------------------------------------------------------------
def test_e_cpu_tables_are_complete():
    assert set(CS.E_CPU_FWD) == {(CS.row(n), m) for n in CS.FORWARD_CASES for m in CS.fwd_modes(n)}
    assert set(CS.E_CPU_ADJ) == {(CS.row(n), m) for n in CS.ADJOINT_CASES for m in CS.ADJ_MODES}


@pytest.mark.parametrize("name", CS.FORWARD_CASES)
def test_forward_constants_cover_the_measurement(name):
    for mode in CS.fwd_modes(name):
        got = CS.measure_fwd(name, mode, ref("fwd", name, mode))
        print(name, mode, "measured %.3e %.3e" % got, "constants %.2e %.2e" % CS.E_CPU_FWD[CS.row(name), mode])
        assert all(g <= c < 1e-4 for g, c in zip(got, CS.E_CPU_FWD[CS.row(name), mode])), (name, mode, got)
        if CS.case(name)["kind"] == "exact":
            assert got[1] == 0  # the weights of an exact-geometry case are exact in fp32


@pytest.mark.parametrize("name", CS.ADJOINT_CASES)
def test_adjoint_constants_cover_the_measurement(name):
    for mode in CS.ADJ_MODES:
        got = CS.measure_adj(name, mode, ref("adj", name, mode))
        print(name, mode, "measured %.3e %.3e %.3e" % got, "constants %.2e %.2e %.2e" % CS.E_CPU_ADJ[CS.row(name), mode])
        assert all(g <= c < 1e-4 for g, c in zip(got, CS.E_CPU_ADJ[CS.row(name), mode])), (name, mode, got)


@pytest.mark.parametrize("name", [n for n in CS.ADJOINT_CASES if n != "delta"])
def test_adjoint_without_its_last_tap_exceeds_the_gpu_bound(name):
    """the adjoint of the PSF with its last non-zero tap zeroed moves vol or vol_weight by more than the bound of every mode"""
    for mode, (interp_psf, with_vm) in CS.ADJ_MODES.items():
        c, r = CS.case(name, interp_psf), ref("adj", name, mode)
        if not r["vol_weight"].any():
            continue  # (a one-plane PSF in NEAREST_PSF: all zeros with any tap list)
        psf = c["psf"].copy()
        psf.reshape(-1)[np.flatnonzero(psf)[-1]] = 0
        m = adjoint64(c["tr"], psf, c["g"], c["sm"], c["vm"] if with_vm else None, c["vs"], c["res"], interp_psf, False)
        e_vol, e_w, _ = CS.E_CPU_ADJ[CS.row(name), mode]
        dv, dw = np.abs(m["vol"] - r["vol"]).max(), np.abs(m["vol_weight"] - r["vol_weight"]).max()
        print(f"{name} {mode}: vol moved {dv:.3e} (bound {4 * e_vol * np.abs(r['vol']).max():.3e}), vol_weight {dw:.3e}")
        assert dv > 4 * e_vol * np.abs(r["vol"]).max() and dw > 4 * e_w * np.abs(r["vol_weight"]).max(), (name, mode)


# ---- the bounds catch a wrong operator ---------------------------------------------------------------------------------------------
def _interior(name):
    """every tap of every pixel inside slices_mask is accepted: nothing fails the bounds test"""
    c, r = CS.case(name), ref("fwd", name, "lin_weights")
    return bool(np.all(r["k"] == 8 * int((c["psf"] != 0).sum())))


# (a stack without a sample has nothing a mutant could move: sparse_zero has no tap; shapes_faces is caught by weight_all_taps only)
MUTANT_CASES = tuple(n for n in CS.EXACT_NAMES + tuple(CS.LIN_GENERAL) if n not in ("sparse_zero", "shapes_faces"))
MUTANT_MODES = {"psf335": ("lin_vm", "nn", "nn_vm"), "sparse": ("nn",), "multi_chunk": ("nn",)}  # beside the LINEAR unmasked route


@pytest.mark.parametrize("name", MUTANT_CASES)
def test_every_mutant_exceeds_the_gpu_bound(name):
    modes = [("lin_weights", ("lin_lerp", "lin_weights"))] + [(m, (m,)) for m in MUTANT_MODES.get(name, ())]
    for mode, ekeys in modes:
        r = ref("fwd", name, mode)
        bound_s = 4 * max(CS.E_CPU_FWD[CS.row(name), k][0] for k in ekeys) * np.abs(r["slices"]).max()  # the widest the GPU test uses
        bound_w = 4 * max(CS.E_CPU_FWD[CS.row(name), k][1] for k in ekeys) * np.abs(r["weight"]).max()
        for mutant in FW.MUTANTS:
            if mutant == "weight_all_taps" and name == "lin_psf335":
                assert _interior(name)  # an interior stack by construction: no tap fails the bounds test
                continue
            m = CS.forward_ref(name, mode, mutant=mutant)
            ds, dw = np.abs(m["slices"] - r["slices"]).max(), np.abs(m["weight"] - r["weight"]).max()
            print(f"{name} {mode} {mutant}: slices moved {ds:.3e} (bound {bound_s:.3e}), weight {dw:.3e} (bound {bound_w:.3e})")
            assert ds > bound_s or dw > bound_w, (name, mode, mutant)
    if name == "psf335":  # the zero-output stacks: the one mutant that can show there does
        m = CS.forward_ref("shapes_faces", "lin_weights", mutant="weight_all_taps")
        assert np.any(m["weight"] != 0)
