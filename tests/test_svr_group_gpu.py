"""GPU: grouped slice-to-volume registration and stack alignment (fsg_svr_compose_f32, fsg_svr_group_reduce_f64,
svort.svr(groups=), svort.SVR(groups=), svort.align_stacks; the rule is in include/fsg_hip.h and DESIGN.md section 29) against
the restatement tests/util_svr_group64.py.

Tolerances (none is derived from what the kernels give):
  compose, reduce    bit-equal to the restatement in the device's operation order: products and sums, one rounding each.
  exact geometry     at phi = 0 the transforms are the base bit for bit, so a group's sums are held to the float64 ones within
                     the sum of its members' bounds (K + 16) * 2^-24 * S of util_svr64.bounds (tests/test_svr_gpu.py).
  svr(groups=)       four times the pose errors the fp32-operation restatement in device order reaches on the CPU
                     (util_svr_group64.A32_POSES through poses, A32 on the matrices of SVR): section 23's margin.
  under noise        the grouped translation error is below the per-slice one (float64: at most 0.31 of it).
  align_stacks       four times the restatement's final translation error (B32) and a quarter of the starting error.
"""
import numpy as np
import pytest
import torch

from tests import util_sa_backward_cases as BC
from tests import util_svr64 as U
from tests import util_svr_group64 as GU
from tests import util_transform_convert64 as TC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
F32, F64 = np.float32, np.float64
PHI = np.array([[0.21, -0.13, 0.08, 0.6, -0.4, 0.3], [-0.05, 0.3, 0.11, -1.2, 0.7, 0.25]], F32)


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


def bits(x):
    return host(x).view(np.uint32 if x.dtype == torch.float32 else np.uint64)


def operands(K, phi):
    """[Q | d] and its Jacobian on the device, as the front-end makes them"""
    phi = dev(np.asarray(phi, F32))
    G = phi.shape[0]
    onehot = torch.eye(12, device=DEV).repeat(G, 1).view(12 * G, 3, 4)
    return K.axisangle2mat(phi), K.axisangle2mat_backward(onehot, phi.repeat_interleave(12, 0).contiguous()).view(G, 12, 6)


# ---- bit equality ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", (PHI, np.zeros((2, 6), F32)), ids=("general", "zero"))
def test_compose_is_bit_equal_to_the_restatement(K, phi):
    base = TC.axisangle2mat(U.capability_case()["true"], F64).astype(F32)
    group = np.array([0, 1, -1, 7, 1], np.int32)  # one fixed slice, one id out of range
    gm, gj = operands(K, phi)
    tr, jac = K.svr_compose(gm, gj, dev(base), dev(group))
    want_tr, want_jac = GU.compose(host(gm), host(gj), base, group, F32)
    assert np.array_equal(bits(tr), want_tr.view(np.uint32)) and np.array_equal(bits(jac), want_jac.view(np.uint32))
    for s in (2, 3):
        assert np.array_equal(bits(tr)[s], base[s].view(np.uint32)) and not host(jac)[s].any()
    assert np.abs(host(jac)[0]).max() > 0.1
    if not phi.any():
        assert np.array_equal(bits(tr), base.view(np.uint32))  # round 0 evaluates the poses as given
    # the float64 convention, within the fp32 cost of a handful of products
    assert np.abs(host(tr) - GU.moved64(phi, base, group)).max() < 1e-5


def test_group_reduce_is_bit_equal_to_the_literal_loop(K):
    rng = np.random.default_rng(4)
    n = 9
    stats = rng.standard_normal((n, 32)) * 10.0 ** rng.integers(-8, 8, (n, 32))
    members = np.array([4, 0, 2, 8, 5, 1, 7, 4], np.int32)  # slice 4 twice, slices 3 and 6 in no group
    offsets = np.array([0, 4, 4, 7, 8], np.int32)  # group 1 is empty
    got = K.svr_group_reduce(dev(stats), dev(members), dev(offsets), out=torch.full((4, 32), -77.25, dtype=torch.float64, device=DEV))
    want = GU.group_reduce(stats, members, offsets)
    assert np.array_equal(bits(got), want.view(np.uint64))
    assert not host(got)[1].any() and not np.signbit(host(got)[1]).any()
    alone = K.svr_group_reduce(dev(stats), dev(members[4:7]), dev(np.array([0, 3], np.int32)))
    assert np.array_equal(bits(alone)[0], bits(got)[2])  # a pure function of the members' rows
    # indices that are not slices add nothing
    odd = K.svr_group_reduce(dev(stats), dev(np.array([4, -1, 0, n, 2, 8], np.int32)), dev(np.array([0, 6], np.int32)))
    assert np.array_equal(bits(odd)[0], bits(got)[0])


def test_an_empty_group_freezes_at_slot_0(K):
    stats = np.zeros((3, 32))
    stats[:, [0, 6, 11, 15, 18, 20]] = 1.0  # H = the identity
    stats[:, 27:30] = (0.5, 4.0, 4.0)
    gstats = K.svr_group_reduce(dev(stats), dev(np.array([0, 1, 2], np.int32)), dev(np.array([0, 3, 3], np.int32)))
    st = K.svr_state(2, 2, DEV)
    phi = torch.zeros(2, 6, device=DEV)
    K.svr_update(st, 0, gstats, phi)
    assert host(st.frozen)[0].tolist() == [0, 1] and not host(phi)[1].any()


# ---- exact geometry: the shapes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sw", (True, False), ids=("weights", "noweights"))
@pytest.mark.parametrize("masks", (False, True), ids=("nomask", "mask"))
@pytest.mark.parametrize("name", ("psf223", "psf223_big"))  # 13 x 11 and 37 x 29 (3 x 2 ragged tiles)
def test_group_sums_at_zero_increment_against_float64(K, name, masks, sw):
    b = BC.exact_case(name, masks)
    rng = np.random.default_rng(len(name) + 7 * masks)
    wgt = (rng.integers(2, 7, b["g"].shape) / 4.0).astype(F32) if sw else None
    min_weight = 0.5 * float(b["psf"].astype(F64).sum())
    _, group, members, offsets = GU.relabel([3, 8, 3, -1, 8])
    gm, gj = operands(K, np.zeros((2, 6), F32))
    tr, jac = K.svr_compose(gm, gj, dev(b["tr"]), dev(group))
    assert np.array_equal(bits(tr), b["tr"].view(np.uint32))
    stats = K.svr_normal(tr, jac, dev(b["vol"]), dev(b["psf"]), dev(b["g"]), dev(b["sm"]), dev(wgt), b["res"], min_weight)
    got = host(K.svr_group_reduce(stats, dev(members), dev(offsets)))
    p = U.pixels(b["tr"], host(jac), b["vol"], b["psf"], b["g"], b["sm"], wgt, b["res"], min_weight, F64)
    s64 = U.stats64(p["terms"])
    kk, ss = U.bounds(p)
    per = (kk + 16) * EPS * ss
    want = GU.group_reduce(s64, members, offsets)
    bound = GU.group_reduce(per, members, offsets) + 4 * 2.0 ** -53 * np.abs(want)
    err = np.abs(got - want)
    print("worst error / bound %.4f, pixels per group %s" % ((err / np.maximum(bound, 1e-300)).max(), want[:, 29]))
    assert np.all(err <= bound) and np.array_equal(got[:, 29], want[:, 29]) and np.all(got[:, 30:] == 0)
    assert want[:, 29].min() > 0 and np.abs(want[:, :21]).max() > 0


# ---- svr(groups=) ---------------------------------------------------------------------------------------------------------------
def grouped(K, svort, c, groups=None, idx=None, poses=None, **kw):
    sel = slice(None) if idx is None else idx
    start = K.mat2axisangle(dev(c["start32"][sel])) if poses is None else dev(poses)
    g = c["groups"] if groups is None else groups
    return svort.svr(start, dev(c["y"][sel]), dev(c["vol"]), dev(c["psf"]), c["res"], n_iter=GU.N_ITER_A, groups=g,
                     return_info=True, **kw)


def errors(poses, c, idx=slice(None)):
    return GU.pose_errors(TC.axisangle2mat(host(poses)[idx], F64), c["true"][idx])


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_grouped_solve_recovers_one_motion(K, svort, seed):
    c = GU.group_case(seed)
    out, info = grouped(K, svort, c)
    rot, trans = errors(out, c)
    want = GU.A32_POSES[seed]
    print("poses: errors %.3e %.3e (restatement %.3e %.3e), accepted %s" % (rot, trans, *want, host(info["accepted"]).sum(0)))
    assert tuple(out.shape) == (BC.N, 6) and tuple(info["cost"].shape) == (GU.N_ITER_A + 1, 1) and info["group_ids"] == [0]
    assert rot <= 4 * want[0] and trans <= 4 * want[1]
    mats = svort.SVR(n_iter=GU.N_ITER_A, groups=c["groups"])(dev(c["start32"]), dev(c["y"]), dev(c["vol"]), dev(c["psf"]), c["res"])
    rot, trans = GU.pose_errors(host(mats), c["true"])
    print("matrices: errors %.3e %.3e (restatement %.3e %.3e)" % (rot, trans, *GU.A32[seed]))
    assert rot <= 4 * GU.A32[seed][0] and trans <= 4 * GU.A32[seed][1]


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_grouped_solve_beats_per_slice_under_noise(K, svort, seed):
    c = GU.group_case(seed, 0.03)
    out, _ = grouped(K, svort, c)
    single = svort.svr(K.mat2axisangle(dev(c["start32"])), dev(c["y"]), dev(c["vol"]), dev(c["psf"]), c["res"], n_iter=GU.N_ITER_A)
    g, s = errors(out, c), errors(single, c)
    print("grouped %.3g / %.3g, per slice %.3g / %.3g, ratio %.3f (float64 at most %.2f)" % (*g, *s, g[1] / s[1], GU.A_RATIO64))
    assert g[1] < s[1]


def test_two_groups_alone_relabelled_and_fixed(K, svort):
    c = GU.group_case(1, two_groups=True)  # slices {0,2,4} and {1,3}, one motion each
    out, info = grouped(K, svort, c)
    rot, trans = errors(out, c)
    print("two groups: errors %.3e %.3e (restatement %.3e %.3e)" % (rot, trans, *GU.A32_POSES_TWO))
    assert rot <= 4 * GU.A32_POSES_TWO[0] and trans <= 4 * GU.A32_POSES_TWO[1]
    assert tuple(info["group_poses"].shape) == (2, 6) and tuple(info["cost"].shape) == (GU.N_ITER_A + 1, 2)
    # a group solved alone equals its rows in the batch, bit for bit
    for g, idx in ((0, [0, 2, 4]), (1, [1, 3])):
        alone, ia = grouped(K, svort, c, groups=[0] * len(idx), idx=idx)
        assert np.array_equal(bits(alone), bits(out)[idx])
        assert np.array_equal(bits(ia["group_poses"])[0], bits(info["group_poses"])[g])
        assert np.array_equal(bits(ia["cost"])[:, 0], bits(info["cost"])[:, g])
    # relabelled ids: the same poses, the groups' rows in the order of the ids
    other, io = grouped(K, svort, c, groups=[9, 4, 9, 4, 9])
    assert io["group_ids"] == [4, 9] and np.array_equal(bits(other), bits(out))
    assert np.array_equal(bits(io["group_poses"]), bits(info["group_poses"])[::-1])
    assert np.array_equal(bits(io["cost"]), bits(info["cost"])[:, ::-1])
    # fixed slices keep their pose bits, and the group beside them its result
    start = K.mat2axisangle(dev(c["start32"]))
    part, ip = grouped(K, svort, c, groups=[0, -1, 0, -1, 0])
    assert np.array_equal(bits(part)[[1, 3]], bits(start)[[1, 3]]) and np.array_equal(bits(part)[[0, 2, 4]], bits(out)[[0, 2, 4]])
    mats = svort.SVR(n_iter=GU.N_ITER_A, groups=[0, -1, 0, -1, 0])(dev(c["start32"]), dev(c["y"]), dev(c["vol"]), dev(c["psf"]), c["res"])
    assert np.array_equal(bits(mats)[[1, 3]], c["start32"][[1, 3]].view(np.uint32))
    assert GU.pose_errors(host(mats)[[0, 2, 4]], c["true"][[0, 2, 4]])[1] < 1e-4


def test_a_group_wholly_outside_the_volume_freezes_at_slot_0(K, svort):
    c = GU.group_case(1, two_groups=True)
    poses = host(K.mat2axisangle(dev(c["start32"])))
    poses[[1, 3], 5] = 60.0
    out, info = grouped(K, svort, c, poses=poses)
    assert np.array_equal(bits(out)[[1, 3]], poses[[1, 3]].view(np.uint32))
    assert host(info["frozen"])[:, 1].min() == 1 and host(info["accepted"])[:, 1].max() == 0 and not host(info["group_poses"])[1].any()
    assert host(info["accepted"])[:, 0].sum() >= 3 and errors(out, c, [0, 2, 4])[1] < 1e-4
    for kw in (dict(slices_mask=torch.zeros(c["y"].shape, dtype=torch.bool, device=DEV)), dict(slices_weight=torch.zeros(c["y"].shape, device=DEV))):
        out, info = grouped(K, svort, c, **kw)
        assert np.array_equal(bits(out), bits(K.mat2axisangle(dev(c["start32"])))) and host(info["frozen"]).min() == 1


@pytest.mark.parametrize("extras", (False, True), ids=("plain", "mask_weights"))
def test_replay_on_ragged_tiles(K, svort, extras):
    """37 x 29 slices (3 x 2 ragged tiles), with and without a mask and weights: the same bits twice and on a side stream"""
    b = BC.exact_case("psf223_big", True)
    rng = np.random.default_rng(11)
    poses = np.zeros((BC.N, 6), F32)
    poses[:, :3] = rng.uniform(-0.05, 0.05, (BC.N, 3))
    poses[:, 3:] = rng.uniform(-3, 3, (BC.N, 3))
    kw = dict(slices_mask=dev(b["sm"]), slices_weight=dev(rng.uniform(0.5, 1.5, b["g"].shape).astype(F32))) if extras else {}

    def run():
        return svort.svr(dev(poses), dev(b["g"]), dev(b["vol"]), dev(b["psf"]), b["res"], n_iter=3, groups=[2, 0, 2, -1, 0],
                         return_info=True, **kw)

    a, ia = run()
    b2, _ = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s, isd = run()
    side.synchronize()
    assert np.array_equal(bits(a), bits(b2)) and np.array_equal(bits(a), bits(s))
    assert np.array_equal(bits(ia["cost"]), bits(isd["cost"])) and np.isfinite(host(ia["cost"])).all()
    assert np.array_equal(bits(a)[3], poses[3].view(np.uint32)) and np.all(host(ia["cost"])[-1] <= host(ia["cost"])[0])
    assert host(ia["accepted"]).sum() >= 1


def test_requires_grad_raises(K, svort):
    c = GU.group_case(1)
    start = K.mat2axisangle(dev(c["start32"]))
    with pytest.raises(NotImplementedError, match="poses"):
        svort.svr(start.requires_grad_(True), dev(c["y"]), dev(c["vol"]), dev(c["psf"]), c["res"], n_iter=1, groups=c["groups"])
    with pytest.raises(NotImplementedError, match="vol"):
        svort.svr(start.detach(), dev(c["y"]), dev(c["vol"]).requires_grad_(True), dev(c["psf"]), c["res"], n_iter=1, groups=c["groups"])
    with pytest.raises(TypeError, match="synchronise"):
        svort.svr(start.detach(), dev(c["y"]), dev(c["vol"]), dev(c["psf"]), c["res"], n_iter=1, groups=dev(np.zeros(BC.N, np.int64)))
    with pytest.raises(NotImplementedError, match="slices"):
        svort.align_stacks(dev(c["start32"]), dev(c["y"]).requires_grad_(True), [0, 0, 1, 1, 1], dev(c["psf"]), BC.VS, c["res"])


# ---- align_stacks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (1, 2))
def test_align_stacks_on_three_orthogonal_stacks(svort, seed):
    c = GU.align_case(seed)

    def run():
        return svort.align_stacks(dev(c["start32"]), dev(c["y"]), c["stack"], dev(c["psf"]), BC.VS, c["res"],
                                  srr=dict(lam=GU.LAM_B, n_iter=GU.CG_ITER_B, deterministic=True), svr=dict(n_iter=GU.LM_ITER_B),
                                  return_info=True)

    out, info = run()
    start, end = GU.pose_errors(c["start"], c["true"]), GU.pose_errors(host(out), c["true"])
    print("start %.3g / %.3g -> %.3g / %.3g (restatement translation %.4f)" % (*start, *end, GU.B32[seed]))
    assert tuple(out.shape) == (3 * GU.N_STACK, 3, 4) and len(info["rounds"]) == GU.N_ROUNDS_B and info["template"] == 0
    assert end[1] <= 4 * GU.B32[seed] and end[1] < GU.B_START_FRACTION * start[1]
    assert np.array_equal(bits(out)[:GU.N_STACK], c["start32"][:GU.N_STACK].view(np.uint32))  # the template never moves
    again, _ = run()
    assert np.array_equal(bits(out), bits(again))
