"""Inputs of tests/test_sa_backward_gpu.py, built on the host with numpy (so the CPU can examine the same cases).

exact_case      rotations are signed axis permutations, translations multiples of 1/8, res_slice 0.75 or 1.5, PSF values
                multiples of 1/32: every coordinate, every trilinear weight and every per-pixel weight is exactly representable
                in fp32, so fp32 and float64 take the same decisions and differ by product roundings and summation order only.
general_case    general rotations.  slices_mask keeps the pixels whose every decision distance (util_sa_backward64:
                bounds, grid, psf_bounds, psf_grid) exceeds 2e-3 in float64: a stack of 5 x 13 x 11 pixels under a 45-tap PSF has
                about 10^5 tap coordinates, so SOME tap of an unrestricted stack always lies within 1e-3 of a decision point
                whatever the seed; restricted to these pixels no fp32 rounding (1e-5 at most here) can flip a decision.
"""
import numpy as np

from tests.util_sa_backward64 import backward64

VS = (20, 18, 22)  # (D, H, W)
N = 5

# proper and improper signed permutations: rows are the images of the slice axes
PERMS = (
    ((1, 0, 0), (0, 1, 0), (0, 0, 1)),
    ((0, -1, 0), (1, 0, 0), (0, 0, 1)),
    ((0, 0, 1), (0, 1, 0), (-1, 0, 0)),
    ((1, 0, 0), (0, 0, -1), (0, 1, 0)),
    ((0, 1, 0), (0, 0, 1), (1, 0, 0)),
    ((-1, 0, 0), (0, 1, 0), (0, 0, 1)),
)

EXACT = {  # name: (psf shape, res_slice, slice shape)
    "psf335": ((3, 3, 5), 0.75, (13, 11)),
    "psf223": ((2, 2, 3), 1.5, (13, 11)),
    "psf133": ((1, 3, 3), 1.5, (13, 11)),  # one plane: NEAREST_PSF accepts no PSF coordinate (0 <= z < 0) and gives zeros
    "psf223_big": ((2, 2, 3), 0.75, (37, 29)),  # 3 x 2 tiles, neither extent a multiple of 16
    "delta": ((1, 1, 1), 1.5, (13, 11)),
}
GENERAL = {  # name: (psf shape, res_slice, seed, with vol_mask)
    "psf335": ((3, 3, 5), 0.75, 101, False),
    "psf223_vm": ((2, 2, 3), 1.5, 102, True),
}


def _common(rng, n, ss, masks):
    vol = rng.standard_normal(VS).astype(np.float32)
    g = rng.standard_normal((n, *ss)).astype(np.float32)
    g[rng.random(g.shape) < 0.1] = 0  # pixels that contribute nothing
    vm = (rng.random(VS) < 0.8) if masks else None
    sm = (rng.random((n, *ss)) < 0.8) if masks else None
    return vol, g, vm, sm


def exact_case(name, masks, n=N, shift=6):
    pshape, res, ss = EXACT[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 2 * masks)
    tr = np.zeros((n, 3, 4), np.float32)
    for i in range(n):
        tr[i, :, :3] = PERMS[(i + len(name)) % len(PERMS)]
        tr[i, :, 3] = rng.integers(-8 * shift, 8 * shift + 1, 3) / 8.0  # some slices reach past a face
    psf = (rng.integers(1, 33, pshape) / 32.0).astype(np.float32)
    if psf.size > 4:
        psf.reshape(-1)[rng.integers(0, psf.size)] = 0  # a tap the kernels skip
    vol, g, vm, sm = _common(rng, n, ss, masks)
    return dict(tr=tr, vol=vol, vm=vm, psf=psf, g=g, sm=sm, res=res)


def rotation(rng, max_angle):
    ax = rng.uniform(-1, 1, 3)
    ax = ax / np.linalg.norm(ax)
    th = rng.uniform(0.1, max_angle)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def general_case(name, interp_psf, n=N, ss=(13, 11)):
    pshape, res, seed, with_vm = GENERAL[name]
    rng = np.random.default_rng(seed)
    tr = np.zeros((n, 3, 4), np.float32)
    for i in range(n):
        tr[i, :, :3] = rotation(rng, 1.0)
        tr[i, :, 3] = rng.uniform(-4, 4, 3)
    psf = rng.uniform(0.1, 1.0, pshape).astype(np.float32)
    vol, g, vm, _ = _common(rng, n, ss, with_vm)
    margin = backward64(tr, vol, None, psf, np.ones_like(g), None, res, interp_psf)["pixel_margin"]
    sm = margin > 2e-3
    return dict(tr=tr, vol=vol, vm=vm, psf=psf, g=g, sm=sm, res=res)


def reference(case, interp_psf, fn=backward64):
    return fn(case["tr"], case["vol"], case["vm"], case["psf"], case["g"], case["sm"], case["res"], interp_psf)


# The fit of the end-to-end test.  Checked on the CPU in float64 (oracle forward + backward64 behind torch.optim.Adam): with
# these settings the loss falls 8.27 -> 4.6e-5 and the translation error 1.5 -> 0.001 voxel in 30 steps; lr 0.1 or betas (0.8, 0.99)
# still end below 0.03 voxel, so the thresholds of the test (tenfold, 0.25 voxel) leave room for fp32.
FIT_SLICE, FIT_OFFSET, FIT_STEPS, FIT_LR, FIT_BETAS = 2, 1.5, 30, 0.15, (0.6, 0.99)


def fit_case():
    """A smooth phantom, five slices through it, and the true pose of slice FIT_SLICE 1.5 voxels along the slice x axis away
    from where the fit starts.  Axis-angle rows [rotation vector | translation], translation first."""
    zz, yy, xx = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in VS), indexing="ij")
    rng = np.random.default_rng(77)
    vol = np.zeros(VS)
    for _ in range(6):
        c = rng.uniform(0.25, 0.75, 3) * np.array(VS)
        s = rng.uniform(3.0, 4.5)
        vol += rng.uniform(0.5, 1.0) * np.exp(-((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2) / (2 * s * s))
    ax = np.zeros((N, 6), np.float32)
    ax[:, :3] = rng.uniform(-0.08, 0.08, (N, 3))
    ax[:, 5] = (np.arange(N) - (N - 1) / 2) * 3.0
    true = ax.copy()
    true[FIT_SLICE, 3] += FIT_OFFSET
    k = np.array([0.25, 0.5, 0.25])
    psf = (k[:, None] * k[None, :])[None].astype(np.float32)
    return dict(vol=vol.astype(np.float32), start=ax, true=true, psf=psf, res=1.5, ss=(13, 11))

