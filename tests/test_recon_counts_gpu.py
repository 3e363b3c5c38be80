"""GPU: the reconstruction units (fsg_robust.hip, fsg_imatch.hip, fsg_svr.hip, fsg_svr_group.hip) at slice counts past a wave
and a workgroup, and the streaming passes at the slice sizes where they change path.  Inputs, field lists
and the one derived bound are in tests/util_recon_counts.py.

Every assertion is one of
  bit-equality to a restatement     the scalar passes given the device's own rows (rb_update_kernel, im_scale_kernel), svr_update,
                                    svr_compose, svr_group_reduce: + - * /, sqrt and fmax in double (products and sums in fp32
                                    for compose), in slice-index order, built without contraction.
  bit-equality to a smaller run     a slice's row in a tiled batch of 257 or 300 against the 5-slice run; a slice of 257 alone;
                                    shifted pointers against aligned ones; the front ends against the kernel sequence.
  4 * E_cpu                         the streaming passes at the new sizes and the bias path at n = 257, E_cpu measured on the CPU
                                    (util_robust64.E_CPU, util_imatch64.E_CPU, E_CPU_SIZES, E_CPU_N257).
  WS_BOUND                          ws[t] on the quotient branch, 20 * 2^-53, derived in util_recon_counts from the documented
                                    accuracy of exp in double on both sides (1 ulp each); not fitted to the kernel.
"""
import numpy as np
import pytest
import torch

from tests import util_imatch64 as IM
from tests import util_recon_counts as RC
from tests import util_robust64 as RB
from tests import util_svr64 as SV
from tests import util_svr_group64 as GU
from tests.test_imatch_gpu import run_match
from tests.test_robust_gpu import run_em
from tests.test_svr_gpu import _same_state
from tests.test_svr_group_gpu import operands

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (and libfsg_hip.so); there is no fallback to skip to")
    from fetalsyngen_amd import kernels

    return kernels


@pytest.fixture(scope="module")
def svort(K):
    from fetalsyngen_amd.generator.artifacts import svort

    return svort


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(x):
    return x.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def shifted(t):  # the same values one element further: no pointer is 16-byte aligned, the mask not 4-byte
    if t is None:
        return None
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


# ---- 1. the scalar passes, bit-equal given the device's own inputs -----------------------------------------------------------
def robust_slots(K, c, n_em=RC.N_EM):
    """the launch sequence slot by slot; after every update the restatement gets the device's rows, ws[t-1], frozen[t-1] and
    consts, and the slot's figures are compared bit for bit, ws[t] by ws_check -> (frozen per slot, slices on the quotient
    branch, largest ws difference)"""
    y, s, mask, sw = dev(c["y"]), dev(c["s"]), dev(c["mask"]), dev(c["sw"])
    n, h, w = c["y"].shape
    st = K.robust_state(n, n_em, DEV, (h, w))
    S = RB.new_state(n, n_em)
    quotient, worst = 0, 0.0
    for t in range(n_em + 1):
        K.robust_estep(st, t, y, s, mask, sw)
        K.robust_update(st, t)
        got = {k: host(getattr(st, k)).copy() for k in ("rows", "u", "consts", "sigma", "c", "mu1", "mu2", "frozen", "ws")}
        if t > 0:
            S["ws"][t - 1], S["frozen"][t - 1], S["consts"] = got["ws"][t - 1], got["frozen"][t - 1], got["consts"]
        RB.update(S, t, got["rows"])
        diff = RC.differing(RC.robust_fields(got, t, tuple(host(st.scal))), RC.robust_fields(S, t))
        assert diff == [], (t, diff)
        q, d = RC.ws_check(got["ws"][t], S, t)
        quotient, worst = quotient + q, max(worst, d)
    return host(st.frozen).tolist(), quotient, worst


@pytest.mark.parametrize("n", RC.COUNTS)
def test_robust_update_is_bit_equal_given_the_devices_rows(K, n):
    """u, consts, sigma, c, mu1, mu2, frozen and the two floats bit-equal in every slot; ws[t] exactly 1 / 0 / 0 on the two
    early-out branches and on the slices that are not ok, and within WS_BOUND = 20 * 2^-53 on the quotient branch.  The bound:
    both sides call exp in double on bit-equal arguments, each documented to 1 ulp, so the exponentials differ by 4 u relative
    (u = 2^-53); every later operation is the same correctly rounded one on both sides and adds 2 u: / sqrt -> 6 u, * mix ->
    8 u, g1 + g2 -> 10 u, g1 / den -> 20 u, and w <= 1."""
    c = RC.robust_case(n)
    want = RC.robust_em(c)
    RB.assert_margin(want)  # a condition on the inputs, checked first
    assert not want["frozen"].any() and (want["ws"][-1] == 0).sum() > len(RC.not_ok_slices(n))
    frozen, quotient, worst = robust_slots(K, c)
    print(f"n = {n}: {quotient} slice weights on the quotient branch, largest difference {worst:.3e}, bound {RC.WS_BOUND:.3e}")
    assert frozen == [0] * (RC.N_EM + 1) and quotient > 0


def test_robust_freezes_on_a_slice_of_the_last_ragged_trip(K):
    frozen, _, _ = robust_slots(K, RC.robust_freeze_case())
    assert frozen == [1] * (RC.N_EM + 1)
    frozen, _, _ = robust_slots(K, RC.robust_case(300))  # and slice 270 alone makes the difference
    assert frozen == [0] * (RC.N_EM + 1)


def imatch_scalar_pass(K, c):
    d = {k: dev(c[k]) for k in ("y", "s", "mask", "sw", "pw", "b0")}
    n, h, w = c["y"].shape
    st = K.imatch_state(n, DEV, (h, w))
    K.imatch_sums(st, d["y"], d["s"], d["mask"], d["sw"], 0.5, d["pw"], d["b0"])
    K.imatch_scale(st)
    got = {k: host(v).copy() for k, v in st.info().items()}
    want = IM.scale(got["rows"])
    diff = RC.differing(RC.imatch_fields(got), RC.imatch_fields(want))
    assert diff == [], diff
    assert not got["mean"].any()
    return got


@pytest.mark.parametrize("n", RC.COUNTS)
def test_imatch_scale_is_bit_equal_given_the_devices_rows(K, n):
    c = RC.imatch_case(n)
    IM.assert_margin(RC.imatch_run(c))
    got = imatch_scalar_pass(K, c)
    dead = RC.not_ok_slices(n)
    assert int(got["frozen"][0]) == 0 and got["consts"][3] == n - len(dead)
    assert not got["ok"][dead].any() and got["scale"][dead].tolist() == [1.0] * len(dead) and got["ok"].sum() == n - len(dead)


def test_imatch_freezes_on_a_scale_that_leaves_fp32_in_the_last_ragged_trip(K):
    got = imatch_scalar_pass(K, RC.imatch_bad_case())
    assert int(got["frozen"][0]) == 1 and not got["ok"].any() and got["consts"].tolist() == [0, 0, 0, 0]
    assert 0 < got["raw"][RC.LATE] < 1e-46 and np.array_equal(got["scale"], np.ones(300, F32))
    assert int(imatch_scalar_pass(K, RC.imatch_case(300))["frozen"][0]) == 0


# ---- 2. the rows at large n: a slice's row is a function of the slice --------------------------------------------------------
@pytest.fixture(scope="module")
def rows5(K):
    """the rows of the two 5-slice cases at slot 0, computed once"""
    c = RB.synthetic_case("n5_37x29_mw")
    st = K.robust_state(5, 1, DEV, (37, 29))
    K.robust_estep(st, 0, dev(c["y"]), dev(c["s"]), dev(c["mask"]), dev(c["sw"]))
    K.robust_update(st, 0)
    m = IM.case("n5_37x29")
    sm = K.imatch_state(5, DEV, (37, 29))
    K.imatch_sums(sm, dev(m["y"]), dev(m["s"]), dev(m["mask"]), dev(m["sw"]), 0.5, dev(m["pw"]), dev(m["b0"]))
    K.imatch_scale(sm)
    return host(st.rows).copy(), host(sm.rows).copy()


@pytest.mark.parametrize("n", (257, 300))
def test_rows_of_a_tiled_batch_are_the_rows_of_the_five_slices(K, rows5, n):
    idx = np.arange(n) % 5
    c = RC.tiled(RB.synthetic_case("n5_37x29_mw"), n)
    st = K.robust_state(n, 1, DEV, (37, 29))
    K.robust_estep(st, 0, dev(c["y"]), dev(c["s"]), dev(c["mask"]), dev(c["sw"]))
    K.robust_update(st, 0)
    assert np.array_equal(bits(host(st.rows)), bits(rows5[0][idx]))
    m = RC.tiled(IM.case("n5_37x29"), n)
    sm = K.imatch_state(n, DEV, (37, 29))
    K.imatch_sums(sm, dev(m["y"]), dev(m["s"]), dev(m["mask"]), dev(m["sw"]), 0.5, dev(m["pw"]), dev(m["b0"]))
    K.imatch_scale(sm)
    assert np.array_equal(bits(host(sm.rows)), bits(rows5[1][idx]))
    assert rows5[0][:, 1].min() > 0 and rows5[1][:, 1].min() > 0 and len({r.tobytes() for r in rows5[0]}) == 5


def test_svr_normal_of_a_tiled_batch_is_the_stats_of_the_five_slices(K):
    c = SV.general_case("psf223_vm")
    m = c["tr"].shape[0]
    idx = np.arange(257) % m

    def normal(sel):
        return host(K.svr_normal(dev(c["tr"][sel]), dev(c["jac"][sel]), dev(c["vol"]), dev(c["psf"]), dev(c["y"][sel]),
                                 dev(c["sm"][sel]), dev(c["sw"][sel]), c["res"], c["min_weight"]))

    small = normal(np.arange(m))
    assert np.array_equal(bits(normal(idx)), bits(small[idx])) and np.abs(small[:, :21]).max() > 0 and small[:, 29].min() > 0


# ---- 3. slice sizes of the streaming passes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(RC.SIZES), ids=lambda s: "%dx%d" % s)
def test_robust_streaming_passes_at_the_sizes_where_they_change_path(K, shape):
    c = RC.robust_size_case(shape)
    args = [dev(c[k]) for k in ("y", "s", "mask", "sw")]
    got = run_em(K, *args, n_em=RC.SIZE_N_EM)
    other = run_em(K, *(shifted(a) for a in args), n_em=RC.SIZE_N_EM)
    for k in ("sigma", "c", "mu1", "mu2", "ws", "u", "slice", "both", "consts"):
        assert np.array_equal(bits(got[k]), bits(other[k])), k
    for ra, rb in zip(got["rows_hist"], other["rows_hist"]):
        assert np.array_equal(bits(ra), bits(rb))
    if shape[0] * shape[1] < 4:  # fewer than min_pixels pixels: no slice is ok, by rule
        assert not got["ws"].any() and not got["slice"].any() and not got["both"].any() and got["frozen"].tolist() == [1, 1]
        for k in ("sigma", "c", "mu1", "mu2", "ws", "u", "consts", "slice", "both"):
            assert np.isfinite(got[k]).all(), k
        assert all(np.isfinite(r).all() and (r[:, 0] == shape[0] * shape[1]).all() for r in got["rows_hist"])
        return
    want = RC.robust_em(c, n_em=RC.SIZE_N_EM)
    RB.assert_margin(want)
    assert np.array_equal(got["frozen"], want["frozen"]) and not want["frozen"].any()
    for t in range(RC.SIZE_N_EM + 1):
        assert np.array_equal(got["rows_hist"][t][:, 0], want["rows_hist"][t][:, 0])  # the pixel counts
        assert np.array_equal(got["rows_hist"][t][:, 4:], want["rows_hist"][t][:, 4:])  # min y, max y
    assert np.array_equal(got["consts"], want["consts"])
    err = RB.compare(got, want)
    for g in RB.GROUPS:
        print(f"{shape} {g}: GPU {err[g]:.3e}, E_cpu {RC.rb_e_cpu(g):.3e}")
    for g in RB.GROUPS:
        assert err[g] <= 4 * RC.rb_e_cpu(g), (g, err[g])
    assert np.array_equal(got["slice"] != 0, want["slice"] != 0)
    assert np.abs(got["slice"] - want["slice"]).max() <= 4 * RC.rb_e_cpu("ws")


@pytest.mark.parametrize("shape", list(RC.SIZES), ids=lambda s: "%dx%d" % s)
def test_imatch_streaming_passes_at_the_sizes_where_they_change_path(K, shape):
    c = RC.imatch_size_case(shape)
    d = {k: dev(c[k]) for k in ("y", "s", "mask", "sw", "pw", "b0")}
    got = run_match(K, **d)
    other = run_match(K, **{k: shifted(v) for k, v in d.items()})
    for k in ("rows", "raw", "scale", "mean", "consts", "bias", "corrected"):
        assert np.array_equal(bits(got[k]), bits(other[k])), k
    want = RC.imatch_run(c)
    IM.assert_margin(want)
    assert got["frozen"] == want["frozen"] == (1 if shape[0] * shape[1] < 4 else 0) and np.array_equal(got["ok"], want["ok"])
    assert np.array_equal(got["rows"][:, 0], want["rows"][:, 0])  # the pixel counts
    assert np.array_equal(got["rows"][:, 3:], want["rows"][:, 3:])  # min y, max y
    assert got["consts"][0] == want["consts"][0] and got["consts"][3] == want["consts"][3]
    err = IM.compare(got, want)
    for g in IM.GROUPS:
        print(f"{shape} {g}: GPU {err[g]:.3e}, E_cpu {RC.im_e_cpu(g):.3e}")
    for g in IM.GROUPS:
        assert err[g] <= 4 * RC.im_e_cpu(g), (g, err[g])
    for k in ("scale", "raw", "mean", "consts", "rows", "corrected"):
        assert np.isfinite(got[k]).all(), k


# ---- 4. svr_update, svr_compose, svr_group_reduce, im_means --------------------------------------------------------------------
@pytest.mark.parametrize("n", (257, 300))
def test_svr_update_is_bit_equal_past_a_workgroup(K, n):
    seq, theta0 = RC.hand_sequences(n)
    slots = seq.shape[1]
    st, ref = K.svr_state(n, slots - 1, DEV), SV.new_state(n, slots - 1)
    st.buf.fill_(-1)  # the block needs no initialisation
    th_d, th_r = dev(theta0), theta0.copy()
    for k in range(slots):
        K.svr_update(st, k, dev(seq[:, k]), th_d)
        th_r = SV.update(ref, k, seq[:, k], th_r)
        assert np.array_equal(host(th_d).view(np.uint32), th_r.view(np.uint32)), k
        for name in RC.STATE_FIELDS:  # after every slot: the per-slice fields, and the histories up to this slot
            a, b = host(getattr(st, name)), ref[name]
            rows = slice(0, k + 1) if name in ("cost", "lambda_hist", "accepted", "frozen") else slice(None)
            assert a.dtype == b.dtype and np.array_equal(a[rows], b[rows], equal_nan=a.dtype.kind == "f"), (name, k)
    _same_state(st, ref)
    assert ref["frozen"][0].tolist() == ([0, 0, 0, 1, 0, 1, 1] * 43)[:n] and ref["accepted"][:, 256:].sum() > 0


@pytest.mark.parametrize("n,G", ((42, 3), (43, 3), (44, 3), (300, 3), (300, 300)))
def test_compose_is_bit_equal_across_the_workgroup_boundary(K, n, G):
    base, group, phi = RC.compose_inputs(n, G)
    gm, gj = operands(K, phi)
    tr, jac = K.svr_compose(gm, gj, dev(base), dev(group))
    want_tr, want_jac = GU.compose(host(gm), host(gj), base, group, F32)
    assert np.array_equal(bits(host(tr)), bits(want_tr)) and np.array_equal(bits(host(jac)), bits(want_jac))
    fixed = ~((group >= 0) & (group < G))
    assert np.array_equal(bits(host(tr)[fixed]), bits(base[fixed])) and not host(jac)[fixed].any()
    if G == 3:
        assert fixed[:42].any() and (~fixed[:42]).any() and (n < 60 or (fixed[43:].any() and (~fixed[43:]).any()))
    if n > 42:
        assert not fixed[42] and np.abs(host(jac)[42][:, 4:]).max() > 0.1  # the columns of the second workgroup
    live = np.flatnonzero(~fixed)
    assert np.abs(want_jac[live]).reshape(len(live), -1).max(1).min() > 1e-2


@pytest.mark.parametrize("G", (8, 9, 300))
def test_group_reduce_is_bit_equal_across_the_workgroup_boundary(K, G):
    stats, members, offsets = RC.reduce_inputs(300, G)
    got = K.svr_group_reduce(dev(stats), dev(members), dev(offsets), out=torch.full((G, 32), -77.25, dtype=torch.float64, device=DEV))
    want = GU.group_reduce(np.concatenate((stats, np.zeros((1, 32)))), np.where((members < 0) | (members >= 300), 300, members), offsets)
    assert np.array_equal(bits(host(got)), bits(want))
    assert not host(got)[1].any() and np.abs(host(got)[G - 1]).min() > 0


@pytest.fixture(scope="module")
def means_case():
    return RC.imatch_means_case()


def test_bias_path_and_means_at_257_slices(K, means_case):
    c = means_case
    want = RC.imatch_run(c, sigma=RC.MEANS_SIGMA)
    IM.assert_margin(want)
    d = {k: dev(c[k]) for k in ("y", "s", "mask", "sw", "pw", "b0")}
    got = run_match(K, sigma=RC.MEANS_SIGMA, **d)
    assert got["frozen"] == want["frozen"] == 0 and np.array_equal(got["ok"], want["ok"]) and got["ok"][256] and not got["ok"][7]
    assert np.array_equal(got["rows"][:, 0], want["rows"][:, 0]) and np.array_equal(got["rows"][:, 3:], want["rows"][:, 3:])
    err = IM.compare(got, want)
    for g in IM.GROUPS:
        print(f"n = 257 {g}: GPU {err[g]:.3e}, E_cpu {RC.im_e_cpu(g, IM.E_CPU_N257):.3e}")
    for g in IM.GROUPS:
        assert err[g] <= 4 * RC.im_e_cpu(g, IM.E_CPU_N257), (g, err[g])
    # a slice alone, under the batch's floor and its own scale of the batch: the same b1 and the same mean
    for k in (0, 255, 256):
        one = K.imatch_state(1, DEV, (RC.H, RC.W))
        a = {name: (None if v is None else v[k:k + 1].clone()) for name, v in d.items()}
        K.imatch_sums(one, a["y"], a["s"], a["mask"], a["sw"], 0.5, a["pw"], a["b0"])
        K.imatch_scale(one)
        one.consts.copy_(got["state"].consts)
        one.scale.copy_(got["state"].scale[k:k + 1])
        b1 = K.imatch_bias(one, a["y"], a["s"], RC.MEANS_SIGMA, a["mask"], a["sw"], 0.5, a["pw"], a["b0"])
        assert np.array_equal(bits(host(b1)[0]), bits(got["b1"][k])), k
        assert np.array_equal(bits(host(one.mean)), bits(got["mean"][k:k + 1])), k
    assert np.abs(got["mean"][[0, 255, 256]]).min() > 0


# ---- 5. the front ends -----------------------------------------------------------------------------------------------------------
def test_robust_weights_front_end_at_257_slices(K, svort):
    c = RC.robust_case(257)
    y, s, mask = dev(c["y"]), dev(c["s"]), dev(c["mask"])
    ref = run_em(K, y, s, mask, None, n_em=RC.N_EM)
    for level in ("slice", "both"):
        out, info = svort.robust_weights(y[:, None], s[:, None], slices_mask=mask[:, None], n_em=RC.N_EM, level=level, return_info=True)
        assert tuple(out.shape) == (257, RC.H, RC.W)
        assert np.array_equal(bits(host(out)), bits(ref[level]))
        for k in info:
            assert np.array_equal(bits(host(info[k])), bits(ref[k])), k
    assert tuple(ref["ws"].shape) == (RC.N_EM + 1, 257) and ref["ws"][-1, 256] == 0 and 0 < ref["ws"][-1].sum() < 257


def test_intensity_match_front_end_at_257_slices(K, svort, means_case):
    c = means_case
    d = {k: dev(c[k]) for k in ("y", "s", "mask", "sw", "pw", "b0")}
    ref = run_match(K, sigma=RC.MEANS_SIGMA, **d)
    corrected, scale, bias, info = svort.intensity_match(d["y"][:, None], d["s"][:, None], weights=d["pw"][:, None],
                                                         slices_mask=d["mask"][:, None], bias_sigma=RC.MEANS_SIGMA, return_info=True)
    for k, v in (("corrected", corrected), ("scale", scale), ("bias", bias)):
        assert np.array_equal(bits(host(v)), bits(ref[k])), k
    for k in ("raw", "rows", "mean", "consts", "scale"):
        assert np.array_equal(bits(host(info[k])), bits(ref[k])), k
    assert np.array_equal(host(info["ok"]) != 0, ref["ok"]) and int(host(info["frozen"])[0]) == ref["frozen"] == 0
