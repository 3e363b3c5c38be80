"""Restatement of the four pose-conversion kernels (fetalsyngen_amd/csrc/fsg_transform_convert.hip) in
numpy, and the cases the CPU and GPU tests share.

The restatement takes a dtype: float64 is the reference of the tests, float32 follows the kernels' operation order and gives
E_cpu, the cost of the formula in fp32 (tests/test_transform_convert_gpu.py).  Rows are evaluated together; branches are
selected per row.  The comparisons with 1e-6 are made in double, as the kernels make them.  `mutant` names one deliberate
error, to show that the cases tell a right rule from a wrong one:
    "no_sign_restore"   mat2axisangle backward: the signs are not restored after the w < 0 flip
    "swap23"            mat2axisangle backward: the stores of the second and third quaternion branches exchanged
    "no_over_theta"     axisangle2mat backward: the division by theta left out

torch_chain is the float64 (or float32) torch-operation form of T.compose(U).inv().axisangle() that the gradient test of
DeviceRigidTransform is held to: branches are chosen per row by indexing, so no branch sees another's rows.
"""
import numpy as np

EPS = 1e-6
SEED = 20261020
N_MAIN = 257


# ---- the restatement -------------------------------------------------------------------------------------------------------
def _gt_eps(v):
    return v.astype(np.float64) > EPS


def axisangle2mat(ax, dtype=np.float64):
    a = np.asarray(ax).astype(dtype)
    one = dtype(1)
    ux, uy, uz = a[:, 0], a[:, 1], a[:, 2]
    theta2 = ux * ux + uy * uy + uz * uz
    big = _gt_eps(theta2)
    m = np.full((a.shape[0], 12), np.nan, dtype)
    with np.errstate(all="ignore"):
        theta = np.sqrt(theta2)
        x, y, z = ux / theta, uy / theta, uz / theta
        s, c = np.sin(theta), np.cos(theta)
        o = one - c
        rod = {0: c + x * x * o, 1: x * y * o - z * s, 2: y * s + x * z * o,
               4: z * s + x * y * o, 5: c + y * y * o, 6: -x * s + y * z * o,
               8: -y * s + x * z * o, 9: x * s + y * z * o, 10: c + z * z * o}
    ones = np.ones_like(ux)
    first = {0: ones, 1: -uz, 2: uy, 4: uz, 5: ones, 6: -ux, 8: -uy, 9: ux, 10: ones}
    for k in rod:
        m[:, k] = np.where(big, rod[k], first[k])
    m[:, 3], m[:, 7], m[:, 11] = a[:, 3], a[:, 4], a[:, 5]
    return m.reshape(-1, 3, 4)


def axisangle2mat_backward(gmat, ax, dtype=np.float64, mutant=None):
    a = np.asarray(ax).astype(dtype)
    gm = np.asarray(gmat).astype(dtype).reshape(-1, 12)
    one, two = dtype(1), dtype(2)
    ux, uy, uz = a[:, 0], a[:, 1], a[:, 2]
    theta2 = ux * ux + uy * uy + uz * uz
    big = _gt_eps(theta2)
    with np.errstate(all="ignore"):
        theta = np.sqrt(theta2)
        x, y, z = ux / theta, uy / theta, uz / theta
        s, c = np.sin(theta), np.cos(theta)
        o = one - c
        zero = np.zeros_like(ux)
        dx, dy, dz, ds, dc = zero, zero, zero, zero, zero
        g = gm[:, 0]
        dc = dc + (one - x * x) * g
        dx = dx + two * o * x * g
        g = gm[:, 1]
        dc = dc - x * y * g; ds = ds - z * g  # noqa: E702
        dx = dx + y * o * g; dy = dy + x * o * g; dz = dz - s * g  # noqa: E702
        g = gm[:, 2]
        dc = dc - x * z * g; ds = ds + y * g  # noqa: E702
        dx = dx + z * o * g; dy = dy + s * g; dz = dz + x * o * g  # noqa: E702
        g = gm[:, 4]
        dc = dc - x * y * g; ds = ds + z * g  # noqa: E702
        dx = dx + y * o * g; dy = dy + x * o * g; dz = dz + s * g  # noqa: E702
        g = gm[:, 5]
        dc = dc + (one - y * y) * g
        dy = dy + two * o * y * g
        g = gm[:, 6]
        dc = dc - y * z * g; ds = ds - x * g  # noqa: E702
        dx = dx - s * g; dy = dy + z * o * g; dz = dz + y * o * g  # noqa: E702
        g = gm[:, 8]
        dc = dc - x * z * g; ds = ds - y * g  # noqa: E702
        dx = dx + z * o * g; dy = dy - s * g; dz = dz + x * o * g  # noqa: E702
        g = gm[:, 9]
        dc = dc - y * z * g; ds = ds + x * g  # noqa: E702
        dx = dx + s * g; dy = dy + z * o * g; dz = dz + y * o * g  # noqa: E702
        g = gm[:, 10]
        dc = dc + (one - z * z) * g
        dz = dz + two * o * z * g
        div = (lambda v: v) if mutant == "no_over_theta" else (lambda v: v / theta)
        along = c * ds - s * dc
        g0 = along * x + div(dx * (one - x * x) - (dy * y + dz * z) * x)
        g1 = along * y + div(dy * (one - y * y) - (dx * x + dz * z) * y)
        g2 = along * z + div(dz * (one - z * z) - (dx * x + dy * y) * z)
    out = np.empty((a.shape[0], 6), dtype)
    out[:, 0] = np.where(big, g0, gm[:, 9] - gm[:, 6])
    out[:, 1] = np.where(big, g1, gm[:, 2] - gm[:, 8])
    out[:, 2] = np.where(big, g2, gm[:, 4] - gm[:, 1])
    out[:, 3], out[:, 4], out[:, 5] = gm[:, 3], gm[:, 7], gm[:, 11]
    return out


def quaternion(mat, dtype=np.float64):
    """(branch 0..3, w, x, y, z, s) of the reference's four formulas, before the sign flip."""
    m = np.asarray(mat).astype(dtype).reshape(-1, 12)
    one, two, q = dtype(1), dtype(2), dtype(0.25)
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = (m[:, k] for k in (0, 1, 2, 4, 5, 6, 8, 9, 10))
    low22 = r22.astype(np.float64) < EPS
    gt, lt = r00 > r11, r00 < -r11
    branch = np.where(~low22 & ~lt, 0, np.where(low22 & gt, 1, np.where(low22 & ~gt, 2, 3)))
    with np.errstate(all="ignore"):
        s = [two * np.sqrt(r00 + r11 + r22 + one), two * np.sqrt(r00 - r11 - r22 + one),
             two * np.sqrt(r11 - r00 - r22 + one), two * np.sqrt(r22 - r00 - r11 + one)]
        w = [q * s[0], (r21 - r12) / s[1], (r02 - r20) / s[2], (r10 - r01) / s[3]]
        x = [(r21 - r12) / s[0], q * s[1], (r01 + r10) / s[2], (r02 + r20) / s[3]]
        y = [(r02 - r20) / s[0], (r01 + r10) / s[1], q * s[2], (r12 + r21) / s[3]]
        z = [(r10 - r01) / s[0], (r02 + r20) / s[1], (r12 + r21) / s[2], q * s[3]]
    pick = lambda v: np.choose(branch, v)  # noqa: E731
    return branch, pick(w), pick(x), pick(y), pick(z), pick(s)


def mat2axisangle(mat, dtype=np.float64):
    m = np.asarray(mat).astype(dtype).reshape(-1, 12)
    two = dtype(2)
    _, w, x, y, z, _ = quaternion(m, dtype)
    neg = w < 0
    w, x, y, z = (np.where(neg, -v, v) for v in (w, x, y, z))
    tmp = x * x + y * y + z * z
    si = np.sqrt(tmp)
    theta = two * np.arctan2(si, w)
    with np.errstate(all="ignore"):
        fac = np.where(_gt_eps(tmp), theta / si, two / w)
    out = np.empty((m.shape[0], 6), dtype)
    out[:, 0], out[:, 1], out[:, 2] = x * fac, y * fac, z * fac
    out[:, 3], out[:, 4], out[:, 5] = m[:, 3], m[:, 7], m[:, 11]
    return out


# per branch: where the six quotients go (flat index, component, sign) and the signs of the diagonal; `own` is the component
# that is 0.25 * s in that branch
_STORES = (
    dict(off=((9, "x", 1), (6, "x", -1), (2, "y", 1), (8, "y", -1), (4, "z", 1), (1, "z", -1)), own="w", diag=(1, 1, 1)),
    dict(off=((9, "w", 1), (6, "w", -1), (2, "z", 1), (8, "z", 1), (4, "y", 1), (1, "y", 1)), own="x", diag=(1, -1, -1)),
    dict(off=((9, "z", 1), (6, "z", 1), (2, "w", 1), (8, "w", -1), (4, "x", 1), (1, "x", 1)), own="y", diag=(-1, 1, -1)),
    dict(off=((9, "y", 1), (6, "y", 1), (2, "x", 1), (8, "x", 1), (4, "w", 1), (1, "w", -1)), own="z", diag=(-1, -1, 1)),
)
# the order in which each branch sums its three products for the diagonal
_DIAG_SUM = (("x", "y", "z"), ("w", "y", "z"), ("x", "w", "z"), ("x", "y", "w"))


def mat2axisangle_backward(mat, gax, dtype=np.float64, mutant=None):
    m = np.asarray(mat).astype(dtype).reshape(-1, 12)
    ga = np.asarray(gax).astype(dtype)
    two, q = dtype(2), dtype(0.25)
    f64 = np.float64
    branch, w, x, y, z, s = quaternion(m, dtype)
    neg = w < 0
    w, x, y, z = (np.where(neg, -v, v) for v in (w, x, y, z))
    tmp = x * x + y * y + z * z
    si = np.sqrt(tmp)
    theta = two * np.arctan2(si, w)
    g0, g1, g2 = ga[:, 0], ga[:, 1], ga[:, 2]
    d = x * g0 + y * g1 + z * g2
    big = _gt_eps(tmp)
    with np.errstate(all="ignore"):
        t = two / (w * w + si * si)
        dw = d * (-t)
        # tmp > 1e-6: the derivative
        fac_b = theta / si
        t_b = (w * t - fac_b) / si
        big_d = [d * (t_b * (v / si)) for v in (x, y, z)]
        # tmp <= 1e-6: the reference's floored rule, in double
        fac_s = two / w
        sie = si.astype(f64) + EPS
        t_s = ((w * t - fac_s).astype(f64) / sie).astype(dtype)
        small_d = [(d.astype(f64) * (t_s.astype(f64) * (v.astype(f64) / sie))).astype(dtype) for v in (x, y, z)]
    fac = np.where(big, fac_b, fac_s)
    dx, dy, dz = (np.where(big, b, sm) for b, sm in zip(big_d, small_d))
    dx, dy, dz = dx + fac * g0, dy + fac * g1, dz + fac * g2
    if mutant != "no_sign_restore":
        w, x, y, z, dx, dy, dz, dw = (np.where(neg, -v, v) for v in (w, x, y, z, dx, dy, dz, dw))
    val = dict(w=w, x=x, y=y, z=z)
    der = dict(w=dw, x=dx, y=dy, z=dz)
    gm = np.full((m.shape[0], 12), np.nan, dtype)
    for b in range(4):
        rows = branch == b
        st = _STORES[{1: 2, 2: 1}.get(b, b) if mutant == "swap23" else b]
        order = _DIAG_SUM[b]
        for k, comp, sign in st["off"]:
            gm[rows, k] = ((der[comp] if sign > 0 else -der[comp]) / s)[rows]
        a, bb, c = order
        ds = -(val[a] * der[a] + val[bb] * der[bb] + val[c] * der[c]) / s + q * der[_STORES[b]["own"]]
        ds = ds * (two / s)
        for k, sign in zip((0, 5, 10), st["diag"]):
            gm[rows, k] = (ds if sign > 0 else -ds)[rows]
    gm[:, 3], gm[:, 7], gm[:, 11] = ga[:, 3], ga[:, 4], ga[:, 5]
    return gm.reshape(-1, 3, 4)


# ---- cases -------------------------------------------------------------------------------------------------------------------
def main_poses(n=N_MAIN, seed=SEED):
    """n poses: axes uniform on the sphere, angles uniform in [0.05, 3.05] rad, translations uniform in [-20, 20], in fp32."""
    rng = np.random.default_rng(seed)
    axis = rng.standard_normal((n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = rng.uniform(0.05, 3.05, (n, 1))
    return np.concatenate((axis * angle, rng.uniform(-20, 20, (n, 3))), 1).astype(np.float32)


def _small(theta2, direction, t):
    d = np.asarray(direction, np.float64)
    return np.concatenate((d / np.linalg.norm(d) * np.sqrt(theta2), t)).astype(np.float32)


ZERO = np.zeros((1, 6), np.float32)
SMALL = np.stack((_small(1.4e-7, (1, -2, 0.5), (3.0, -7.5, 11.25)), _small(9.0e-7, (-0.3, 0.2, 1), (-19.0, 0.125, 4.0))))
NAN_ANGLE = np.array([[0.3, np.nan, -0.2, 1.0, 2.0, 3.0]], np.float32)
INF_TRANS = np.array([[0.3, 0.1, -0.2, 1.0, np.inf, 3.0]], np.float32)


def matrices(poses):
    """The fp32 matrices of fp32 poses: the float64 restatement, rounded."""
    return axisangle2mat(poses, np.float64).astype(np.float32)


def clear_rows(mat):
    """Rows of fp32 matrices in which every decision of mat2axisangle is clear in float64: the three branch tests by 1e-3,
    w > 0.05 after the flip (the rotation vector jumps where w changes sign), tmp > 1e-3."""
    m = np.asarray(mat, np.float64).reshape(-1, 12)
    _, w, x, y, z, _ = quaternion(m, np.float64)
    tmp = x * x + y * y + z * z
    return ((np.abs(m[:, 10] - EPS) > 1e-3) & (np.abs(m[:, 0] - m[:, 5]) > 1e-3) & (np.abs(m[:, 0] + m[:, 5]) > 1e-3)
            & (np.abs(w) > 0.05) & (tmp > 1e-3))


_CACHE = {}
_CHAIN = {}


def cases():
    """The shared cases, computed once and left unchanged:
    ax, gmat            the main stack and a standard-normal gradient on its matrices
    mat, gax, keep      the fp32 matrices of the main stack, a standard-normal gradient on their axis-angle rows, and the rows
                        clear_rows keeps; branch, flipped: the quaternion branch of every row and whether w < 0 before the flip
    small_ax, small_mat the zero pose and the two small-angle poses, and their matrices (tmp <= 1e-6)"""
    if not _CACHE:
        rng = np.random.default_rng(SEED + 1)
        ax = main_poses()
        mat = matrices(ax)
        branch, w = quaternion(mat, np.float64)[:2]
        small_ax = np.concatenate((ZERO, SMALL))
        _CACHE.update(ax=ax, gmat=rng.standard_normal((N_MAIN, 3, 4)).astype(np.float32), mat=mat,
                      gax=rng.standard_normal((N_MAIN, 6)).astype(np.float32), keep=clear_rows(mat), branch=branch,
                      flipped=w < 0, small_ax=small_ax, small_mat=matrices(small_ax),
                      small_gmat=rng.standard_normal((3, 3, 4)).astype(np.float32),
                      small_gax=rng.standard_normal((3, 6)).astype(np.float32))
        for v in _CACHE.values():
            v.setflags(write=False)
    return _CACHE


def rel_err(a, b):
    """max |a - b| / max |b|"""
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(np.asarray(b, np.float64)).max())


def rot_part(v):
    """The rotation entries of (n,3,4) matrices or of (n,6) axis-angle rows; trans_part: the rest."""
    v = np.asarray(v)
    return v[:, :, :3] if v.ndim == 3 else v[:, :3]


def trans_part(v):
    v = np.asarray(v)
    return v[:, :, 3] if v.ndim == 3 else v[:, 3:]


# What e_cpu() and chain_case() gave when they were measured, rounded up in the third digit: the constants the GPU tests' bounds
# are built from (test_transform_convert64_reference.py re-measures them).  Figures seen on the MI355X: DESIGN.md section 21.
# E_CPU: max |restatement in float32 - restatement in float64| / max |float64| of the rotation part over cases()
# (measured 3.985e-7, 1.997e-7, 9.388e-8, 9.679e-8, 2.169e-7).
E_CPU = {"a2m": 3.99e-7, "a2m_bwd": 2.00e-7, "m2a": 9.39e-8, "m2a_bwd": 9.68e-8, "roundtrip_bwd": 2.17e-7}
# max |float64 rotation part of axisangle2mat's backward| / max |incoming gradient| over the same cases: what "times the size
# of the incoming gradient" multiplies
R_A2M_BWD = 1.1416
# the leaf gradients of chain_case() in float32 torch operations against float64: rotation and translation entries, the
# larger of the two leaves (measured 1.26e-7 / 1.68e-7 and 2.86e-7 / 1.95e-7)
E_CHAIN = {"chain_rot": 1.68e-7, "chain_trans": 2.86e-7}


def e_cpu():
    """E_cpu of the four kernels: the float32 restatement's largest deviation from the float64 one over the cases, relative to
    max |float64| of the rotation part; and R, max |float64 rotation part| over max |incoming gradient|, for the backward rules."""
    c = cases()
    k = c["keep"]
    out = {}
    out["a2m"] = rel_err(rot_part(axisangle2mat(c["ax"], np.float32)), rot_part(axisangle2mat(c["ax"])))
    ref = rot_part(axisangle2mat_backward(c["gmat"], c["ax"]))
    out["a2m_bwd"] = rel_err(rot_part(axisangle2mat_backward(c["gmat"], c["ax"], np.float32)), ref)
    out["a2m_bwd_R"] = float(np.abs(ref).max() / np.abs(c["gmat"]).max())
    out["m2a"] = rel_err(rot_part(mat2axisangle(c["mat"][k], np.float32)), rot_part(mat2axisangle(c["mat"][k])))
    ref = rot_part(mat2axisangle_backward(c["mat"][k], c["gax"][k]))
    out["m2a_bwd"] = rel_err(rot_part(mat2axisangle_backward(c["mat"][k], c["gax"][k], np.float32)), ref)
    # the round trip's gradient: gax through mat2axisangle's rule, then through axisangle2mat's, at the main stack
    chain = lambda dt: rot_part(axisangle2mat_backward(  # noqa: E731
        mat2axisangle_backward(axisangle2mat(c["ax"][k], dt), c["gax"][k], dt), c["ax"][k], dt))
    out["roundtrip_bwd"] = rel_err(chain(np.float32), chain(np.float64))
    return out


# ---- the chain of the DeviceRigidTransform gradient test, in torch operations ------------------------------------------------
def torch_axisangle2mat(ax):
    import torch

    ang, t = ax[:, :3], ax[:, 3:]
    th2 = (ang * ang).sum(1)
    big = th2.double() > EPS
    rot = torch.zeros((ax.shape[0], 3, 3), dtype=ax.dtype)
    a = ang[big]
    th = torch.sqrt(th2[big])
    u = a / th[:, None]
    s, c = torch.sin(th), torch.cos(th)
    o = 1 - c
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    rot[big] = torch.stack((c + x * x * o, x * y * o - z * s, y * s + x * z * o,
                            z * s + x * y * o, c + y * y * o, -x * s + y * z * o,
                            -y * s + x * z * o, x * s + y * z * o, c + z * z * o), 1).reshape(-1, 3, 3)
    b = ang[~big]
    one = torch.ones_like(b[:, 0])
    rot[~big] = torch.stack((one, -b[:, 2], b[:, 1], b[:, 2], one, -b[:, 0], -b[:, 1], b[:, 0], one), 1).reshape(-1, 3, 3)
    return torch.cat((rot, t[:, :, None]), 2)


def torch_mat2axisangle(mat):
    """The derivative torch takes of this is the true one in every branch; the kernels' rule differs from it for tmp <= 1e-6
    only (the reference's quirk), and the chain's rows stay far from that."""
    import torch

    r = lambda i, j: mat[:, i, j]  # noqa: E731
    low22 = r(2, 2).double() < EPS
    gt, lt = r(0, 0) > r(1, 1), r(0, 0) < -r(1, 1)
    sel = (~low22 & ~lt, low22 & gt, low22 & ~gt, ~low22 & lt)
    quat = torch.zeros((mat.shape[0], 4), dtype=mat.dtype)
    for b, rows in enumerate(sel):
        m = mat[rows]
        r00, r01, r02, r10, r11, r12, r20, r21, r22 = (m[:, i, j] for i in range(3) for j in range(3))
        if b == 0:
            s = 2 * torch.sqrt(r00 + r11 + r22 + 1)
            q = (0.25 * s, (r21 - r12) / s, (r02 - r20) / s, (r10 - r01) / s)
        elif b == 1:
            s = 2 * torch.sqrt(r00 - r11 - r22 + 1)
            q = ((r21 - r12) / s, 0.25 * s, (r01 + r10) / s, (r02 + r20) / s)
        elif b == 2:
            s = 2 * torch.sqrt(r11 - r00 - r22 + 1)
            q = ((r02 - r20) / s, (r01 + r10) / s, 0.25 * s, (r12 + r21) / s)
        else:
            s = 2 * torch.sqrt(r22 - r00 - r11 + 1)
            q = ((r10 - r01) / s, (r02 + r20) / s, (r12 + r21) / s, 0.25 * s)
        quat[rows] = torch.stack(q, 1)
    quat = torch.where(quat[:, :1] < 0, -quat, quat)
    w, v = quat[:, 0], quat[:, 1:]
    tmp = (v * v).sum(1)
    big = tmp.double() > EPS
    fac = torch.zeros_like(w)
    si = torch.sqrt(tmp[big])
    fac[big] = 2 * torch.atan2(si, w[big]) / si
    fac[~big] = 2 / w[~big]
    return torch.cat((v * fac[:, None], mat[:, :, 3]), 1)


def torch_chain(ax_t, ax_u):
    """T.compose(U).inv().axisangle() for T, U given as axis-angle rows, translation first: (n,6)."""
    import torch

    a, b = torch_axisangle2mat(ax_t), torch_axisangle2mat(ax_u)
    R1, t1, R2, t2 = a[:, :, :3], a[:, :, 3:], b[:, :, :3], b[:, :, 3:]
    m = torch.cat((R1 @ R2, t2 + R2.transpose(-2, -1) @ t1), -1)
    R, t = m[:, :, :3], m[:, :, 3:]
    return torch_mat2axisangle(torch.cat((R.transpose(-2, -1), -(R @ t)), -1))


def chain_case():
    """Pose pairs (T, U) from the main stack whose chain result is clear of every decision of mat2axisangle, a weight on the
    chain's output, and the leaf gradients of sum(weight * chain) in float64 and in float32 torch operations."""
    import torch

    if not _CHAIN:
        ax = main_poses()
        t, u = ax[:128], ax[128:256]
        with torch.no_grad():
            m = torch_axisangle2mat(torch_chain(torch.from_numpy(t).double(), torch.from_numpy(u).double())).numpy()
        keep = clear_rows(m.astype(np.float32))
        t, u = np.ascontiguousarray(t[keep]), np.ascontiguousarray(u[keep])
        wgt = np.random.default_rng(SEED + 2).standard_normal((len(t), 6)).astype(np.float32)
        grads = {}
        for dt in (torch.float64, torch.float32):
            lt, lu = (torch.from_numpy(v).to(dt).requires_grad_() for v in (t, u))
            (torch_chain(lt, lu) * torch.from_numpy(wgt).to(dt)).sum().backward()
            grads[dt] = (lt.grad.numpy().astype(np.float64), lu.grad.numpy().astype(np.float64))
        _CHAIN.update(t=t, u=u, wgt=wgt, g64=grads[torch.float64], g32=grads[torch.float32])
    return _CHAIN
