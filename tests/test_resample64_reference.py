"""CPU: the float64 reference of K6 + K7 + K8 (tests/util_resample64.py) pinned to the golden blur and the oracle; the
down-sampling table precondition (tables.is_down_table); the answers of fsg_blur_resample_supported at the edges of its
domain (host code only, no launch)."""
import numpy as np
import pytest
import torch

from fetalsyngen_amd import _lib
from fetalsyngen_amd import tables as T
from oracle import fsg_oracle as O
from tests.util_resample64 import blur_resample64, error_bound

ATOL, RTOL = 1e-3, 1e-5


def tab(lo, hi, wl, wh):
    return T._pack(np.asarray(lo), np.asarray(hi), np.asarray(wl, np.float32), np.asarray(wh, np.float32))


def test_reference_blur_equals_golden(golden):
    g = golden("blur")
    for si in range(3):
        x = g[f"x_{si}"]
        for ti, st in enumerate(g["stds"]):
            taps = [O.gaussian_taps(float(s)).numpy() if s > 0 else None for s in st]
            y = blur_resample64(x, taps, [None] * 3)
            np.testing.assert_allclose(y, g[f"y_{si}_{ti}"], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("shape,res,spacing,u_std", [
    ((20, 24, 12), (0.5, 0.5, 0.5), 1.4, 0.1),
    ((33, 20, 28), (0.5, 0.6, 0.7), 1.3, 0.7),
    ((40, 36, 28), (0.5, 0.5, 0.5), 0.8, 0.6),
    ((17, 9, 40), (0.5, 0.5, 0.5), 2.26, 1.0),  # radius 8 on every axis
])
def test_reference_equals_oracle_resample_down(shape, res, spacing, u_std):
    rs = np.random.RandomState(11)
    x = (rs.rand(*shape) * 255).astype(np.float32)
    x[: shape[0] // 3] *= 0.1
    sp = np.array([spacing] * 3)
    stds, new, _f, pos = O.resample_plan(shape, np.array(res), sp, u_std)
    taps = [O.gaussian_taps(float(s)).numpy() if s > 0 else None for s in stds]
    tabs = [T.position_table(pos[a], shape[a]) for a in range(3)]
    ref, _ = O.resample_down(torch.from_numpy(x), res, sp, u_std)
    y = blur_resample64(x, taps, tabs)
    assert y.shape == tuple(new)
    np.testing.assert_allclose(y, ref.numpy(), rtol=RTOL, atol=ATOL)
    # noise epilogue: + std z, negatives clamped (oracle add_noise)
    z = np.random.RandomState(3).randn(*new).astype(np.float32)
    yn = blur_resample64(x, taps, tabs, noise_std=60.0, z=z)
    np.testing.assert_allclose(yn, O.add_noise(ref, 60.0, torch.from_numpy(z)).numpy(), rtol=RTOL, atol=ATOL)
    assert (yn == 0).any() and yn.min() == 0.0


def test_reference_is_the_dense_separable_operator():
    """Any taps (asymmetric), any table (outside outputs anywhere, shared and repeated neighbours, hi == lo): the reference
    equals the product of per-axis dense matrices, applied with einsum."""
    rs = np.random.RandomState(2)
    shape = (9, 7, 12)
    x = rs.randn(*shape)
    taps = [rs.rand(5), rs.rand(3), rs.rand(9)]
    tabs = [tab([-1, 0, 0, 4, 8, 2, -1], [0, 1, 1, 5, 8, 3, 0], rs.rand(7), rs.rand(7)),
            tab([6, 5, 3], [6, 6, 4], rs.rand(3), rs.rand(3)),
            tab(np.arange(-1, 11), np.minimum(np.arange(0, 12), 11), rs.rand(12), rs.rand(12))]

    def dense(n, k, t):
        R = len(k) // 2
        B = np.zeros((n, n))
        for i in range(n):
            for j in range(len(k)):
                if 0 <= i + j - R < n:
                    B[i, i + j - R] = k[j]
        L = np.zeros((len(t), n))
        for j, e in enumerate(t):
            if e["lo"] >= 0:
                L[j, e["lo"]] += np.float64(e["w_lo"])
                L[j, e["hi"]] += np.float64(e["w_hi"])
        return L @ B

    M = [dense(shape[a], taps[a], tabs[a]) for a in range(3)]
    want = np.einsum("ai,bj,ck,ijk->abc", M[0], M[1], M[2], x)
    np.testing.assert_allclose(blur_resample64(x, taps, tabs), want, rtol=1e-12, atol=1e-12)
    assert (blur_resample64(x, taps, tabs)[[0, 6]] == 0).all()  # outside outputs are exactly 0
    # the bound is zero exactly where the inputs an output depends on are zero
    x0 = x.copy()
    x0[:] = 0
    assert (error_bound(x0, taps, tabs) == 0).all()


def test_down_table_precondition():
    for n in range(2, 70):
        for m in range(1, n):
            assert T.is_down_table(T._resample_axis_table(m, n)), (m, n)
        # m == n: position 0 is outside (lo = -1), output 0 is 0 and no kernel of the fused pair writes it
        t = T._resample_axis_table(n, n)
        assert t["lo"][0] == -1 and not T.is_down_table(t)
    w = np.full(3, 0.5)
    assert T.is_down_table(tab([0, 2, 3], [1, 3, 3], w, w))
    assert not T.is_down_table(tab([0, 0, 2], [1, 1, 3], w, w))      # two outputs share a lower neighbour
    assert not T.is_down_table(tab([0, 3, 2], [1, 4, 3], w, w))      # lo not monotone
    assert not T.is_down_table(tab([0, 2, -1], [1, 3, 0], w, w))     # outside output at the end
    assert not T.is_down_table(tab([0, 2, 4], [1, 4, 5], w, w))      # hi not a neighbour of lo
    assert not T.is_down_table(tab([], [], [], []))


def _rows_fit(n0, n1, n2, R):
    """(16 ceil(n0 / 16) + R + 1) * n1 * n2 * 4 <= 2^32: the x kernel's 32-bit row offsets do not wrap."""
    return (16 * -(-n0 // 16) + R + 1) * n1 * n2 * 4 <= 1 << 32


def test_fused_predicate_at_its_edges():
    sup = _lib.load().fsg_blur_resample_supported
    ok = lambda n, m, nt=(3, 3, 3): bool(sup(*n, *m, *nt))  # noqa: E731
    assert ok((32, 32, 32), (31, 31, 31))
    for a in range(3):  # m == n on one axis: refused (the unfused path writes output 0)
        m = [31, 31, 31]
        m[a] = 32
        assert not ok((32, 32, 32), m), a
    assert ok((32, 32, 32), (1, 1, 1)) and not ok((32, 32, 32), (33, 31, 31))
    # row length: n2 % 4 == 0, and the y,z launch's LDS (4 waves x 9 rows x (n2 + 2 RP) floats) <= 64000 bytes
    assert ok((8, 8, 4), (7, 7, 3))
    assert not ok((8, 8, 6), (7, 7, 5)) and not ok((8, 8, 514), (7, 7, 257))
    assert ok((8, 8, 436), (7, 7, 218)) and not ok((8, 8, 440), (7, 7, 220))                      # R_yz <= 4: RP = 4
    assert ok((8, 8, 428), (7, 7, 214), (3, 11, 3)) and not ok((8, 8, 432), (7, 7, 216), (3, 3, 11))  # R_yz 5..8: RP = 8
    assert not ok((8, 8, 512), (7, 7, 256)) and not ok((8, 8, 516), (7, 7, 258))
    # radii 1..8 on every axis
    assert ok((40, 40, 40), (20, 20, 20), (17, 17, 17))
    for nt in ((19, 3, 3), (3, 19, 3), (3, 3, 19), (1, 3, 3), (4, 3, 3)):
        assert not ok((40, 40, 40), (20, 20, 20), nt), nt
    # the x kernel's row offsets: exactly at the no-wrap bound, and one row of n2 past it (shapes where that bound, not the
    # 2^29-voxel one, is the binding limit: short axes 0, a last chunk mostly past the end)
    for n0 in (2, 5, 9, 17):
        for R in (2, 8):
            n2 = 432
            n1 = (1 << 32) // ((16 * -(-n0 // 16) + R + 1) * n2 * 4)
            assert _rows_fit(n0, n1, n2, R) and not _rows_fit(n0, n1 + 1, n2, R)
            assert n0 * (n1 + 1) * n2 <= 1 << 29
            nt = (2 * R + 1, 3, 3)
            assert ok((n0, n1, n2), (n0 - 1, n1 - 1, n2 // 2), nt), (n0, n1, R)
            assert not ok((n0, n1 + 1, n2), (n0 - 1, n1, n2 // 2), nt), (n0, n1 + 1, R)
    # the shape that read wrapped rows before the bound (two rows of 429 497 856 bytes: rows -8 and 9 landed in rows 1 and 0)
    assert not ok((2, 248552, 432), (1, 124276, 216), (17, 3, 3))
    assert ok((2, 248552, 432), (1, 124276, 216), (3, 3, 3)) == _rows_fit(2, 248552, 432, 1)
