"""Inputs shared by the CPU tests of the float64 reference (tests/test_artifacts64_reference.py) and the GPU tests of the kernels
(tests/test_artifact_kernels_edges.py), so that what the CPU tests establish about a bound or a census holds for the very
cases the GPU tests run (not a test module)."""
import numpy as np
import torch

F = np.float32


def boundary_random_inputs(n=2 ** 22 + 3, seed=6):
    """The inputs of the GPU test's random `boundary_mask` case (shared, so that the census below is of those inputs)."""
    rs = np.random.RandomState(seed)
    mask = (rs.rand(n) < 0.3).astype(F)
    modif = np.maximum(mask, (rs.rand(n) < 0.6).astype(F))
    return dict(image=(rs.rand(n) * 100 + 1).astype(F), mask=mask, mask_modif=modif, mog=rs.rand(n).astype(F),
                dist=rs.randint(0, 7, n).astype(F), n_dilate=6)


NEAR_TIE_CAP = 1e-4


def mog_cases():
    rs = np.random.RandomState(7)
    cases = {}
    for shape in ((24, 20, 28), (3, 5, 1023), (2, 3, 1024), (2, 3, 1025), (5, 4, 2), (1, 1, 1)):
        D, H, W = shape
        for k in (1, 7, 200):
            c = (rs.rand(k, 3) * [W, H, D] * 1.4 - [0.2 * W, 0.2 * H, 0.2 * D]).astype(F)  # inside and outside the grid
            c[0] = [W - 1, 0, D // 2]                                                    # on a face
            s = np.exp(rs.uniform(np.log(0.5), np.log(200.0), (k, 3))).astype(F)
            cases[f"{shape}-k{k}"] = (shape, c, s)
    # ty + tz straddles the skip threshold 176 on row (z, y) = (0, 0): below it the blob is evaluated, above it is skipped
    for t in (175.9, 176.1):
        cases[f"straddle{t}"] = ((5, 4, 2), np.array([[0.5, np.sqrt(t), 0.0], [1.0, 2.0, 3.0]], F),
                                 np.array([[1.0, 1.0, 1.0], [2.0, 2.0, 2.0]], F))
    # one blob alone, far down its tail but well above the skip: exp(-30.5) and exp(-85) must be there (the bound is relative)
    for t in (61.0, 170.0):
        cases[f"tail{t}"] = ((5, 4, 2), np.array([[0.5, np.sqrt(t), 0.0]], F), np.array([[1.0, 1.0, 1.0]], F))
    # seven blobs on one voxel: the sum clamps at exactly 1
    cases["clamp"] = ((5, 4, 6), np.tile(np.array([[3.0, 2.0, 1.0]], F), (7, 1)), np.full((7, 3), 1.5, F))
    return cases


def perlin_octaves(shape, noct, seed):
    rs = np.random.RandomState(seed)
    octs = []
    for q in range(noct):
        r = (q + 1, 8 - q, 2 * q + 2) if noct > 1 else (1 + seed % 3, 2, 5)
        g = rs.randn(r[0] + 1, r[1] + 1, r[2] + 1, 3)
        g /= np.linalg.norm(g, axis=-1, keepdims=True)
        g[-1], g[:, -1], g[:, :, -1] = g[0], g[:, 0], g[:, :, 0]
        lins = [torch.linspace(0, r[a], shape[a]) for a in range(3)]
        assert all(float(v[-1]) == (r[a] if shape[a] > 1 else 0) for a, v in enumerate(lins))  # the last point is r exactly
        octs.append((torch.from_numpy(g.astype(F)), lins, r, 0.5 ** q))
    return octs
