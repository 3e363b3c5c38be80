"""CPU restatement of the grouped registration `svort.svr(groups=)` and of `svort.align_stacks` (the rule
of the two kernels is in include/fsg_hip.h, fsg_svr_compose_f32 / fsg_svr_group_reduce_f64).  Test infrastructure, numpy only;
`ft` is the type every operation is done in, as in tests/util_svr64.

    compose(...)        a slice's transform and its derivative with respect to the GROUP's 6 parameters, in the kernel's
                        operation order (every three-term sum as ((x0 y0) + (x1 y1)) + (x2 y2), one rounding per operation in
                        ft): float32 is bit-equal to the device, float64 the yardstick.  mutant: "old_R" (R'^T d with R in
                        place of R'), "no_dd" (the R'^T dd term dropped), "RQ" (Q R as R Q).
    group_reduce(...)   the groups' sums as a literal loop.
    relabel(groups)     the front-end's host parsing: ids in increasing order, members in increasing slice index.
    solve(...)          the grouped loop on util_svr64.update: axisangle2mat(phi), its Jacobian, compose, the per-slice normal
                        equations of util_svr64, group_reduce, update on G rows; then compose at theta_cur.
    align_stacks(...)   `svort.align_stacks` on util_srr64 / util_tk1_64: round 0 against the template alone, round r >= 1 stack
                        g against all stacks but g at the round's starting poses.  all_stacks=True: the target holds every
                        stack, the moving one included (the failure DESIGN.md section 23 records).

Error measures (pose_errors): rotation = the largest |R' - R_true| entry; translation = the largest component of
|R' t' - R t|, the slice centre in the volume frame.

Experiment A (`group_case`): util_svr64.capability_case(), five 9 x 9 slices against the true volume, all displaced by ONE
rigid motion of the volume frame, default_rng(seed).uniform(-0.03, 0.03, 3) rad then .uniform(-0.75, 0.75, 3) voxels, Gaussian
noise sigma from default_rng(100 + seed) on the slices, 12 rounds.  Experiment B (`align_case`): util_srr64.capability_case(),
three orthogonal 7-slice stacks of 13 x 11; stack 0 is the template, stacks 1 and 2 are displaced by their own motion, from ONE
default_rng(seed): .uniform(-0.03, 0.03, 3) rad then .uniform(-0.75, 0.75, 3) voxels for stack 1, then the same two draws for
stack 2, all times `scale`; targets 12 CG iterations
from 0 with TK1 lam, registrations 10 rounds.  `python -m tests.util_svr_group64` prints both tables; the figures the tests use
are beside the constants at the end.
"""
import numpy as np

from tests import util_sa_backward_cases as BC
from tests import util_srr64 as SR
from tests import util_svr64 as U
from tests import util_tk1_64 as T1
from tests import util_transform_convert64 as TC

F32, F64 = np.float32, np.float64
SLOTS = U.SLOTS


# ---- the two kernels ----------------------------------------------------------------------------------------------------------
def _dot3(a0, b0, a1, b1, a2, b2, ft):
    return (((a0 * b0).astype(ft) + (a1 * b1).astype(ft)).astype(ft) + (a2 * b2).astype(ft)).astype(ft)


def compose(gmat, gjac, base, group, ft=F64, mutant=None):
    """gmat (G,3,4), gjac (G,12,6), base (n,3,4), group (n) -> transforms (n,3,4), jac (n,12,6) in ft"""
    gmat = np.asarray(gmat).astype(ft).reshape(-1, 3, 4)
    G = gmat.shape[0]
    gjac = np.asarray(gjac).astype(ft).reshape(G, 12, 6)
    base = np.asarray(base).astype(ft).reshape(-1, 3, 4)
    group = np.asarray(group).reshape(-1)
    n = base.shape[0]
    tr, jac = base.copy(), np.zeros((n, 12, 6), ft)
    for s in range(n):
        g = int(group[s])
        if not 0 <= g < G:
            continue  # fixed: the base row as it is, no derivative
        Q, d, B = gmat[g, :, :3], gmat[g, :, 3], base[s]
        R = B[:, :3]

        def mul(A):  # A R (the mutant: R A)
            out = np.zeros((3, 3), ft)
            for r in range(3):
                for c in range(3):
                    if mutant == "RQ":
                        out[r, c] = _dot3(R[r, 0], A[0, c], R[r, 1], A[1, c], R[r, 2], A[2, c], ft)
                    else:
                        out[r, c] = _dot3(A[r, 0], R[0, c], A[r, 1], R[1, c], A[r, 2], R[2, c], ft)
            return out

        R1 = mul(Q)
        Rt = R if mutant == "old_R" else R1  # the rotation whose transpose carries d
        tr[s, :, :3] = R1
        for c in range(3):
            tr[s, c, 3] = (B[c, 3] + _dot3(Rt[0, c], d[0], Rt[1, c], d[1], Rt[2, c], d[2], ft)).astype(ft)
        for a in range(6):
            dQ = gjac[g, :, a].reshape(3, 4)
            dR, dd = mul(dQ[:, :3]), dQ[:, 3]
            for r in range(3):
                for c in range(3):
                    jac[s, 4 * r + c, a] = dR[r, c]
            dRt = np.zeros((3, 3), ft) if mutant == "old_R" else dR
            for c in range(3):
                first = _dot3(dRt[0, c], d[0], dRt[1, c], d[1], dRt[2, c], d[2], ft)
                second = _dot3(Rt[0, c], dd[0], Rt[1, c], dd[1], Rt[2, c], dd[2], ft)
                jac[s, 4 * c + 3, a] = first if mutant == "no_dd" else (first + second).astype(ft)
    return tr, jac


def group_reduce(stats, members, offsets):
    stats = np.asarray(stats, F64)
    G = len(offsets) - 1
    out = np.zeros((G, SLOTS), F64)
    for g in range(G):
        for k in range(SLOTS):
            v = F64(0.0)
            for j in range(int(offsets[g]), int(offsets[g + 1])):
                v = v + stats[int(members[j]), k]
            out[g, k] = v
    return out


def relabel(groups):
    """-> (ids, group, members, offsets) as svort.svr.parse_groups"""
    g = [int(v) for v in groups]
    ids = sorted({v for v in g if v >= 0})
    group = [ids.index(v) if v >= 0 else -1 for v in g]
    members, offsets = [], [0]
    for j in range(len(ids)):
        members += [s for s, v in enumerate(group) if v == j]
        offsets.append(len(members))
    return ids, np.array(group, np.int32), np.array(members, np.int32), np.array(offsets, np.int32)


def group_operands(phi, ft):
    """[Q | d] and its (G,12,6) Jacobian at phi, as the front-end makes them"""
    return TC.axisangle2mat(phi, ft), U.jacobian(phi, ft)


# ---- the grouped solve ------------------------------------------------------------------------------------------------------------
def slice_stats(tr, jac, vol, psf, y, sm, sw, res, min_weight, ft, device_order):
    if ft is F64:
        return U.stats64(U._pixels_raw(tr, jac, vol, psf, y, sm, sw, res, min_weight)["terms"])
    p = U.pixels(tr, jac, vol, psf, y, sm, sw, res, min_weight, F32)
    return U.stats_device(p["terms"]) if device_order else U.stats64(p["terms"])


def solve(base, groups, vol, psf, y, res, n_iter, sm=None, sw=None, min_weight=0.5, ft=F64, device_order=None, mutant=None, **opts):
    """-> (transforms (n,3,4), state of G rows, ids).  ft float64: everything in float64; ft float32: what the device computes."""
    device_order = (ft is F32) if device_order is None else device_order
    tdt = F64 if ft is F64 else F32
    base = np.asarray(base).astype(tdt).reshape(-1, 3, 4)
    ids, group, members, offsets = relabel(groups)
    G = len(ids)
    phi = np.zeros((G, 6), tdt)
    st = U.new_state(G, n_iter, tdt)
    for k in range(n_iter + 1):
        gm, gj = group_operands(phi, ft)
        tr, jac = compose(gm, gj, base, group, ft, mutant)
        stats = slice_stats(tr, jac, vol, psf, y, sm, sw, res, min_weight, ft, device_order)
        phi = U.update(st, k, group_reduce(stats, members, offsets), phi, **opts)
    gm, gj = group_operands(st["theta_cur"], ft)
    return compose(gm, gj, base, group, ft)[0], st, ids


def pose_errors(tr, true):
    """(rotation, translation): the largest |R' - R| entry, the largest component of |R' t' - R t|"""
    a, b = np.asarray(tr, F64).reshape(-1, 3, 4), np.asarray(true, F64).reshape(-1, 3, 4)
    rot = float(np.abs(a[:, :, :3] - b[:, :, :3]).max())
    ca, cb = np.einsum("nij,nj->ni", a[:, :, :3], a[:, :, 3]), np.einsum("nij,nj->ni", b[:, :, :3], b[:, :, 3])
    return rot, float(np.abs(ca - cb).max())


def displace(mats, phi):
    """the float64 matrices under the volume-frame motions phi (one row per matrix, or one row for all)"""
    mats = np.asarray(mats, F64).reshape(-1, 3, 4)
    phi = np.asarray(phi, F64).reshape(-1, 6)
    group = np.arange(mats.shape[0]) if phi.shape[0] == mats.shape[0] else np.zeros(mats.shape[0], int)
    return compose(*group_operands(phi, F64), mats, group, F64)[0]


# ---- experiment A ----------------------------------------------------------------------------------------------------------------
N_ITER_A = 12
_A = {}


def group_case(seed, sigma=0.0, two_groups=False):
    """util_svr64.capability_case() displaced by one motion (two_groups: slices {0,2,4} and {1,3} by one motion each)"""
    key = (seed, sigma, two_groups)
    if key not in _A:
        c = U.capability_case()
        true = TC.axisangle2mat(c["true"], F64)
        rng = np.random.default_rng(seed)
        m = 2 if two_groups else 1
        phi = np.concatenate((rng.uniform(-0.03, 0.03, (m, 3)), rng.uniform(-0.75, 0.75, (m, 3))), 1)
        groups = [0, 1, 0, 1, 0] if two_groups else [0] * BC.N
        start = displace(true, phi[groups])
        y64 = c["y64"] + (sigma * np.random.default_rng(100 + seed).standard_normal(c["y64"].shape) if sigma else 0.0)
        _A[key] = dict(vol=c["vol"], psf=c["psf"], res=c["res"], true=true, start=start, start32=start.astype(F32), y64=y64,
                       y=y64.astype(F32), groups=groups)
    return _A[key]


def run_a(seed, sigma, ft=F64, two_groups=False, groups=None, through_poses=False):
    """the grouped solve of experiment A -> (rot, trans, transforms, state); float64 takes the slices unrounded.
    through_poses: in and out as `svort.svr` takes them, (n,6) poses through mat2axisangle / axisangle2mat in ft."""
    c = group_case(seed, sigma, two_groups)
    base, y = (c["start"], c["y64"]) if ft is F64 else (c["start32"], c["y"])
    if through_poses:
        base = TC.axisangle2mat(TC.mat2axisangle(base, ft), ft)
    tr, st, _ = solve(base, c["groups"] if groups is None else groups, c["vol"], c["psf"], y, c["res"], N_ITER_A, ft=ft)
    if through_poses:
        tr = TC.axisangle2mat(TC.mat2axisangle(tr, ft), F64)
    return (*pose_errors(tr, c["true"]), tr, st)


def run_a_per_slice(seed, sigma, ft=F64):
    """today's per-slice svr from the same start -> (rot, trans)"""
    c = group_case(seed, sigma)
    base, y = (c["start"], c["y64"]) if ft is F64 else (c["start32"], c["y"])
    theta, _ = U.solve(TC.mat2axisangle(base, F64 if ft is F64 else F32), c["vol"], c["psf"], y, c["res"], N_ITER_A, ft=ft,
                       device_order=ft is F32)
    return pose_errors(TC.axisangle2mat(theta, F64), c["true"])


# ---- experiment B ----------------------------------------------------------------------------------------------------------------
N_STACK, LAM_B, CG_ITER_B, LM_ITER_B, N_ROUNDS_B = 7, 0.03, 12, 10, 3
_B = {}


def align_case(seed, scale=1.0):
    key = (seed, scale)
    if key not in _B:
        c = SR.capability_case()
        true = c["tr"].astype(F64)
        stack = np.repeat(np.arange(3), N_STACK)
        rng = np.random.default_rng(seed)
        phi = np.zeros((3, 6))
        for s in (1, 2):  # stack 1's six draws, then stack 2's
            phi[s, :3] = scale * rng.uniform(-0.03, 0.03, 3)
            phi[s, 3:] = scale * rng.uniform(-0.75, 0.75, 3)
        start = displace(true, phi[stack])
        start[stack == 0] = true[stack == 0]
        _B[key] = dict(c, true=true, start=start, start32=start.astype(F32), stack=stack)
    return _B[key]


def reconstruct(tr, y, psf, ss, res, keep, lam, n_iter, ft):
    """srr from 0 of the slices `keep` (n bool), TK1 lam, relu on"""
    n = len(keep)
    sm = np.broadcast_to(np.asarray(keep, bool)[:, None, None], (n, *ss)).copy()
    make = lambda g, delta: T1.RegOperator(tr, psf, BC.VS, ss, res, False, sm=sm, ft=ft, lam=lam, guide=g, delta=delta)  # noqa: E731
    return T1.srr(make, y, n_iter, ft=ft)[0]


def align_stacks(tr0, y, stack, psf, ss, res, template=0, n_rounds=N_ROUNDS_B, lam=LAM_B, cg_iter=CG_ITER_B, lm_iter=LM_ITER_B,
                 ft=F64, all_stacks=False, all_lam=0.0, all_iter=6):
    """-> the transforms after every round, [(n,3,4)] * n_rounds.  all_stacks: every target is the reconstruction of ALL
    stacks at the round's poses (all_iter CG iterations, all_lam), the moving stack included."""
    tdt = F64 if ft is F64 else F32
    tr = np.asarray(tr0).astype(tdt).reshape(-1, 3, 4)
    stack = np.asarray(stack)
    y = np.asarray(y, F32)
    moving = [g for g in sorted(set(stack.tolist())) if g != template]
    every = np.ones(len(stack), bool)
    out = []

    def register(cur, idx, groups, target):
        return solve(cur[idx], groups, target, psf, y[idx], res, lm_iter, ft=ft)[0]

    for r in range(n_rounds):
        nxt = tr.copy()
        trf = tr.astype(F32) if ft is F32 else tr
        if all_stacks:
            target = reconstruct(trf, y, psf, ss, res, every, all_lam, all_iter, ft)
        if r == 0:
            if not all_stacks:
                target = reconstruct(trf, y, psf, ss, res, stack == template, lam, cg_iter, ft)
            idx = np.flatnonzero(stack != template)
            nxt[idx] = register(tr, idx, stack[idx], target)
        else:
            for g in moving:
                if not all_stacks:
                    target = reconstruct(trf, y, psf, ss, res, stack != g, lam, cg_iter, ft)
                idx = np.flatnonzero(stack == g)
                nxt[idx] = register(tr, idx, [0] * len(idx), target)
        tr = nxt
        out.append(tr.copy())
    return out


def run_b(seed, scale=1.0, lam=LAM_B, ft=F64, all_stacks=False, n_rounds=N_ROUNDS_B):
    """-> [(rot, trans)] at the start and after every round"""
    c = align_case(seed, scale)
    trs = align_stacks(c["start"] if ft is F64 else c["start32"], c["y"], c["stack"], c["psf"], c["ss"], c["res"], lam=lam, ft=ft,
                       all_stacks=all_stacks, n_rounds=n_rounds)
    return [pose_errors(c["start"], c["true"])] + [pose_errors(t, c["true"]) for t in trs], trs


# ---- constants, each with the measured value beside it (python -m tests.util_svr_group64 prints them) ------------------------
# compose's jac against central differences of step 1e-6 in float64, at a general phi and at phi = 0
JAC_FD_BOUND = 1e-6  # measured 3.8e-10 at a general phi, 4.3e-10 at 0
# experiment A, sigma = 0, fp32 operations in device order on the fp32 slices: (rotation, translation) per seed.  The float64
# run on the unrounded slices reaches 5e-16 / 4.8e-15 at most.
A32 = {1: (1.51e-7, 1.34e-6),  # measured 1.508e-07, 1.334e-06
       2: (1.32e-7, 1.19e-6),  # measured 1.318e-07, 1.188e-06
       3: (1.15e-7, 7.09e-7)}  # measured 1.146e-07, 7.089e-07
# the same runs as `svort.svr` makes them, in and out through (n,6) poses (run_a(through_poses=True)); TWO: the two-group case
A32_POSES = {1: (5.96e-8, 6.12e-7),  # measured 5.955e-08, 6.113e-07
             2: (1.13e-7, 8.77e-7),  # measured 1.126e-07, 8.764e-07
             3: (9.94e-8, 6.01e-7)}  # measured 9.940e-08, 6.009e-07
A32_POSES_TWO = (9.26e-8, 6.74e-7)  # measured 9.259e-08, 6.734e-07
# experiment A, sigma = 0.03, float64: grouped translation error / per-slice translation error, at most
A_RATIO64 = 0.31  # measured 0.100, 0.308, 0.138 (0.21 / 2.1, 0.42 / 1.4, 0.13 / 0.91); fp32 operations give the same digits
# experiment B, lam = 0.03, fp32 operations: the worst translation error after the last round, per seed
B32 = {1: 0.0464,  # measured 0.046356 (float64 0.046372), start 0.8331
       2: 0.0404}  # measured 0.040307 (float64 0.040307), start 0.7529
B_START_FRACTION = 0.25  # a condition, not a measurement; float64 sits at 0.056 and 0.054 of the start


def table_a(ft=F64):
    rows = []
    for seed in (1, 2, 3):
        c = group_case(seed)
        for sigma in (0.0, 0.03, 0.1):
            g = run_a(seed, sigma, ft)[:2]
            rows.append((seed, sigma, pose_errors(c["start"], c["true"]), g, run_a_per_slice(seed, sigma, ft)))
    return rows


def moved64(phi, base, group):
    """the convention stated directly, with matrix products: R' = Q R, t' = t + R'^T d (float64; no shared code with compose)"""
    gm = TC.axisangle2mat(np.asarray(phi, F64).reshape(-1, 6), F64)
    out = np.asarray(base, F64).reshape(-1, 3, 4).copy()
    for s, g in enumerate(group):
        if 0 <= g < gm.shape[0]:
            R1 = gm[g, :, :3] @ out[s, :, :3]
            out[s, :, 3] = out[s, :, 3] + R1.T @ gm[g, :, 3]
            out[s, :, :3] = R1
    return out


def fd_error(phi, base, group, mutant=None):
    """the difference check -> (max |compose's transforms - moved64|, max |compose's jac - central differences of moved64|),
    step 1e-6, float64"""
    phi = np.asarray(phi, F64).reshape(-1, 6)
    tr, jac = compose(*group_operands(phi, F64), base, group, F64, mutant)
    worst = 0.0
    for g in range(phi.shape[0]):
        for a in range(6):
            hi, lo = phi.copy(), phi.copy()
            hi[g, a] += 1e-6
            lo[g, a] -= 1e-6
            d = (moved64(hi, base, group) - moved64(lo, base, group)) / 2e-6
            for s in np.flatnonzero(np.asarray(group) == g):
                worst = max(worst, float(np.abs(d[s].reshape(12) - jac[s, :, a]).max()))
    return float(np.abs(tr - moved64(phi, base, group)).max()), worst


if __name__ == "__main__":
    import sys

    c = group_case(1)
    phis = np.array([[0.21, -0.13, 0.08, 0.6, -0.4, 0.3]])
    print("jac vs central differences: general", fd_error(phis, c["true"], [0] * 5), "at 0", fd_error(np.zeros((1, 6)), c["true"], [0] * 5))
    print("experiment A, float64: seed sigma start grouped per-slice")
    for row in table_a(F64):
        print("  ", row[0], row[1], "start %.3g / %.3g" % row[2], "grouped %.2g / %.2g" % row[3], "per slice %.2g / %.2g" % row[4])
    print("two groups, float64:", run_a(1, 0.0, F64, two_groups=True)[:2])
    for seed in (1, 2, 3):
        print("A32 seed", seed, run_a(seed, 0.0, F32)[:2], "sigma 0.03 fp32 grouped", run_a(seed, 0.03, F32)[:2], "per slice",
              run_a_per_slice(seed, 0.03, F32))
    print("experiment B, float64: lam seed scale: (rot, trans) at start, rounds 0, 1, 2")
    for lam in (0.03, 0.1):
        for seed, scale in ((1, 1.0), (2, 1.0), (1, 2.0)):
            print("  ", lam, seed, scale, ["%.3g / %.3g" % e for e in run_b(seed, scale, lam)[0]])
    print("all stacks, 6 CG, lam 0:", ["%.3g / %.3g" % e for e in run_b(1, all_stacks=True, n_rounds=4)[0]])
    if "--fp32" in sys.argv:
        for seed in (1, 2):
            print("B32 seed", seed, ["%.3g / %.3g" % e for e in run_b(seed, ft=F32)[0]])
