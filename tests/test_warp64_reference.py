"""CPU: the references of tests/util_warp64.py, on the case table of tests/util_warp_cases.py that the GPU tests
(tests/test_warp_kernels_edges.py) run.

  * positions32 / margins / linear32 / nearest reproduce oracle/fsg_oracle.py bit for bit on the `deform_image` goldens (the
    coordinate golden, the margins, apply_deformation with and without flip);
  * hand-computed known answers for the exact-position group;
  * positions32 lies within position_bound of positions64 on every case;
  * linear32 lies within  sum_a position_bound[a] * slope_a  +  LINEAR_ROUNDINGS * 2^-24 * 1.01 * (the blend of |src|)  of linear64
    at the float64 positions, where slope_a is the largest |difference of two source neighbours along axis a| over the cells the
    path from the float32 to the float64 position crosses (the trilinear blend is continuous and piecewise linear: its partial
    derivative inside a cell is a blend of that cell's four differences along the axis); outputs where the two positions fall on
    different sides of the strict > 0 rule (a jump from 0 to the source value) are exempt, and those lie within the bound of 0;
  * labels of nearest at the two positions agree wherever the float64 position is not within position_bound of a tie or of 0; that
    excluded share is at most 0.5 % per case, and the exact-position group excludes nothing.
"""
import numpy as np
import pytest
import torch

from oracle import fsg_oracle as O
from tests import util_warp64 as W
from tests import util_zoom64 as Z
from tests.util_resample64 import U32
from tests.util_warp_cases import GROUPS, all_cases, cases, grid_tabs, sources, warp_kernel

F = np.float32


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == F and np.array_equal(a.view(np.int32), b.view(np.int32))


def shifted(spec, pos):
    """(positions - floor(min)) in the positions' own precision, and the six margins (always from the float32 keys)."""
    keys = W.minmax32(W.positions32(spec))
    return W.subtract_margins(pos, keys), W.margins(keys)


def test_references_are_the_oracle_on_the_deform_goldens(golden):
    g = golden("deform_image")
    rs = np.random.RandomState(5)
    for i in range(int(g["ncases"])):
        shape, size = tuple(int(v) for v in g[f"shape_{i}"]), tuple(int(v) for v in g[f"size_{i}"])
        field = tabs = None
        if f"Fsmall_{i}" in g.files:
            field = g[f"Fsmall_{i}"]
            tabs = grid_tabs(field.shape, shape)
        c2 = torch.tensor(g[f"c2_{i}"]).to(torch.float32).numpy()
        spec = W.make_spec(shape, g[f"A_{i}"], (np.array(size) - 1) / 2, c2, field, tabs)
        pos, m = shifted(spec, W.positions32(spec))
        assert m == list(g[f"margins_{i}"]), i
        for a in range(3):
            assert bits(pos[a], g[f"coords_{i}"][a]), (i, a)
        img = (rs.randn(*shape) * 80).astype(F)
        lab = (rs.rand(*shape) * 9).astype(F)
        co = [torch.from_numpy(np.ascontiguousarray(p)) for p in pos]
        for flip in (False, True):
            r_img, r_seg = O.apply_deformation(torch.from_numpy(img), torch.from_numpy(lab), co, flip)
            assert bits(W.linear32(img, pos, flip), r_img.numpy()), (i, flip)
            assert bits(W.nearest(lab, pos, flip), r_seg.numpy()), (i, flip)
            if shape[2] >= 2:  # the lean kernel's reading: the same values (the sign of a zero aside)
                assert np.array_equal(W.linear32(img, pos, flip, lean=True), r_img.numpy()), (i, flip)


def test_table_names_the_kernel_the_launcher_chooses():
    from fetalsyngen_amd import _lib

    T = _lib.TUNE
    seen = set()
    for c in all_cases():
        assert warp_kernel(c, 0, T, True, True) == c.kernel, c.name
        assert warp_kernel(c, T.GENERIC_WARP, T, True, True) == "voxel"
        for flags in (0, T.NO_LEAN, T.NO_PATCH, T.GENERIC_WARP):
            for rows in (False, True):
                for wb in (False, True):
                    seen.add(warp_kernel(c, flags, T, rows, wb))
    assert seen == {"lean", "patch", "rows", "voxel"}


def _known(case, src, flip):
    """Identity with an integer shift s, by hand: the position along an axis is clip(index + s, 0, n - 1), the margin is its
    minimum, the output is the (flipped) source voxel at position - margin, and 0 in the image where that index is 0 on any axis
    (outside by the strict > 0 rule).  Returns (image, labels)."""
    n = case.spec.shape
    s = [int(round(float(case.spec.c2[a]) - float(case.spec.cen[a]))) for a in range(3)]
    idx = []
    for a in range(3):
        p = np.clip(np.arange(n[a]) + s[a], 0, n[a] - 1)
        idx.append(p - p.min())
    I, J, K = np.meshgrid(*idx, indexing="ij")
    v = src[::-1] if flip else src
    return np.where((I > 0) & (J > 0) & (K > 0), v[I, J, K], F(0)), v[I, J, K]


def test_known_answers_of_the_exact_positions():
    by_name = {c.name: c for c in cases("exact positions")}
    for c in by_name.values():
        assert c.exact and c.spec.field is None
        p32, p64 = W.positions32(c.spec), W.positions64(c.spec)
        assert all(np.array_equal(a.astype(np.float64), b) for a, b in zip(p32, p64)), c.name  # exact: no rounding anywhere
    for flip in (False, True):
        for name in ("identity (the last plane, row and column alone and at once)", "identity, shift (1, 0, 0)",
                     "identity, shift (0, -2, 0)", "identity, shift (0, 0, 3)", "identity, shift (-1, 2, -30)"):
            c = by_name[name]
            S = sources(c)
            pos, _ = shifted(c.spec, W.positions32(c.spec))
            want_img, want_lab = _known(c, S["img"], flip)
            assert np.array_equal(W.linear32(S["img"], pos, flip), want_img), (name, flip)
            assert np.array_equal(W.linear32(S["img"], pos, flip, lean=True), want_img), (name, flip)
            assert np.array_equal(W.nearest(S["lab8"], pos, flip), _known(c, S["lab8"], flip)[1]), (name, flip)
            assert bits(W.nearest(S["labf"], pos, flip), _known(c, S["labf"], flip)[1]), (name, flip)
            assert want_lab.shape == c.spec.shape
        # half a voxel up on one axis: the mean of two neighbours (the last index is clamped onto the last plane: the plane itself);
        # labels round half to even: index + 0.5 -> the even one of the two
        for a in range(3):
            c = by_name[f"shift 0.5 on axis {a} (ties)"]
            S = sources(c)
            n = c.spec.shape
            pos, m = shifted(c.spec, W.positions32(c.spec))
            assert m[:3] == [0, 0, 0]
            v = S["img"][::-1] if flip else S["img"]
            up = np.take(v, np.minimum(np.arange(n[a]) + 1, n[a] - 1), axis=a)
            want = v * F(0.5) + up * F(0.5)
            last = [slice(None)] * 3
            last[a] = n[a] - 1
            want[tuple(last)] = v[tuple(last)]
            for b in range(3):
                if b != a:
                    zero = [slice(None)] * 3
                    zero[b] = 0
                    want[tuple(zero)] = 0
            assert np.array_equal(W.linear32(S["img"], pos, flip), want), (a, flip)
            k = np.arange(n[a])
            even = np.minimum(np.where(k % 2 == 0, k, k + 1), n[a] - 1)
            lab = S["lab8"][::-1] if flip else S["lab8"]
            assert np.array_equal(W.nearest(S["lab8"], pos, flip), np.take(lab, even, axis=a)), (a, flip)
        # a coordinate that is exactly 0 everywhere: the image is 0, the labels are those of plane 0 of that axis
        for a in range(3):
            c = by_name[f"coordinate {a} exactly 0"]
            S = sources(c)
            pos, _ = shifted(c.spec, W.positions32(c.spec))
            assert not pos[a].any()
            out = W.linear32(S["img"], pos, flip)
            assert not out.any() and not np.signbit(out).any()
            lab = S["lab8"][::-1] if flip else S["lab8"]
            plane0 = np.take(lab, np.zeros(c.spec.shape[a], np.int64), axis=a)
            assert np.array_equal(W.nearest(S["lab8"], pos, flip), plane0)
    # -0.0 orders below +0.0 in the keys
    c = by_name["x is -0.0 at i = 0"]
    p = W.positions32(c.spec)
    assert np.signbit(p[0][0]).all() and not np.signbit(p[0][1:]).any() and not p[0].any()
    assert W.minmax32(p)[0] == -1 and W.minmax32(p)[3] == 0 and int(Z.f2key(F(-0.0))) == -1


def test_outside_and_margin_cases_are_what_their_names_say():
    for c in cases("outside"):
        S = sources(c)
        pos, m = shifted(c.spec, W.positions32(c.spec))
        a = int(c.name[-1])
        # every position is clamped onto one face; the margin then takes it to 0: the image is 0, the labels are plane 0's
        assert not pos[a].any(), c.name
        assert m[a] == (0 if "low" in c.name else c.spec.shape[a] - 1)
        assert not W.linear32(S["img"], pos, False).any()
        index = np.broadcast_to(np.arange(c.spec.shape[a], dtype=F).reshape([-1 if b == a else 1 for b in range(3)]), c.spec.shape)
        assert not W.nearest(index, pos, False).any()  # the labels are read from plane 0 of that axis
    m1, m2, m3 = cases("nonzero margins")
    for c in (m1, m2):
        assert min(W.margins(W.minmax32(W.positions32(c.spec)))[:3]) >= 1, c.name
    p = W.positions32(m3.spec)
    face = np.zeros(m3.spec.shape, bool)
    for a in range(3):
        sl = [slice(None)] * 3
        for e in (0, -1):
            sl[a] = e
            face[tuple(sl)] = True
    for a in range(3):
        assert p[a][face].min() >= 1 and p[a][~face].min() < 1, a
    assert W.margins(W.minmax32(p))[:3] == [0, 0, 0]


@pytest.mark.parametrize("group", GROUPS)
def test_position_bound_holds(group):
    worst = 0.0
    for c in cases(group):
        p32, p64, bound = W.positions32(c.spec), W.positions64(c.spec), W.position_bound(c.spec)
        for a in range(3):
            err = np.abs(p32[a].astype(np.float64) - p64[a])
            assert (err <= bound[a]).all(), (c.name, a, float((err / bound[a]).max()))
            worst = max(worst, float((err[bound[a] > 0] / bound[a][bound[a] > 0]).max(initial=0.0)))
    print(f"WARP64 {group}: largest position error {worst:.3f} of the bound")


def _cell_slopes(src, flip, cells, axis):
    """Largest |difference of two neighbours along `axis`| over the cells given by per-axis lists of candidate base indices."""
    n = src.shape
    v = (src[::-1] if flip else src).astype(np.float64)
    out = 0.0
    for x0 in cells[0]:
        for y0 in cells[1]:
            for z0 in cells[2]:
                base = [x0, y0, z0]
                for d1 in (0, 1):
                    for d2 in (0, 1):
                        lo, hi = [], []
                        others = [b for b in range(3) if b != axis]
                        off = {others[0]: d1, others[1]: d2}
                        for b in range(3):
                            if b == axis:
                                lo.append(base[b])
                                hi.append(np.minimum(base[b] + 1, n[b] - 1))
                            else:
                                t = np.minimum(base[b] + off[b], n[b] - 1)
                                lo.append(t)
                                hi.append(t)
                        out = np.maximum(out, np.abs(v[hi[0], hi[1], hi[2]] - v[lo[0], lo[1], lo[2]]))
    return out


@pytest.mark.parametrize("group", GROUPS)
def test_linear32_and_labels_lie_within_their_bounds(group):
    worst, share = 0.0, 0.0
    for c in cases(group):
        S = sources(c)
        n = c.spec.shape
        q32, _ = shifted(c.spec, W.positions32(c.spec))
        q64, _ = shifted(c.spec, W.positions64(c.spec))
        bound = W.position_bound(c.spec)
        excl = W.near_tie_or_zero(q64, bound, q32)
        if c.exact:
            excl = np.zeros(n, bool)  # nothing is excluded where the positions carry no rounding
        assert excl.mean() <= 0.005, (c.name, float(excl.mean()))
        share = max(share, float(excl.mean()))
        cells = [[np.clip(np.floor(q).astype(np.int64), 0, n[a] - 1) for q in (q32[a], q64[a])] for a in range(3)]
        for flip in (False, True):
            for lab in (S["lab8"], S["labf"]):
                l32, l64 = W.nearest(lab, q32, flip), W.nearest(lab, q64, flip)
                assert np.array_equal(l32[~excl], l64[~excl]), (c.name, flip)
            src = S["img"]
            v32, v64 = W.linear32(src, q32, flip), W.linear64(src, q64, flip)
            tol = LIN_TERMS * W.linear_magnitude(src, q64, flip)
            for a in range(3):
                tol = tol + bound[a] * _cell_slopes(src, flip, cells, a)
            ok32 = np.all([(q32[a] > 0) for a in range(3)], axis=0)
            ok64 = np.all([(q64[a] > 0) for a in range(3)], axis=0)
            jump = ok32 != ok64
            assert not (jump & ~excl).any() or c.exact, c.name  # a jump sits within the bound of 0
            err = np.abs(v32.astype(np.float64) - v64)
            good = (err <= tol) | jump
            assert good.all(), (c.name, flip, int((~good).sum()), float(err[~good].max()))
            with np.errstate(all="ignore"):
                r = np.where(tol > 0, err / tol, 0)[~jump]
            worst = max(worst, float(r.max()) if r.size else 0.0)
            if c.exact:
                assert not jump.any() and (err <= LIN_TERMS * W.linear_magnitude(src, q64, flip)).all()
    print(f"WARP64 {group}: largest linear error {worst:.3f} of the bound, largest excluded share {100 * share:.3f} %")


LIN_TERMS = 1.01 * W.LINEAR_ROUNDINGS * U32


def test_epilogue64_by_hand():
    v = np.array([0.0, 300.0, 75.0], F)
    assert np.array_equal(W.epilogue64(v, gamma=0.5), [0.0, 300.0, 150.0])
    assert np.array_equal(W.epilogue64(v), v.astype(np.float64))
    c = cases("generic")[0]
    b = Z.zoom64(c.bias, c.bias_tabs)
    out = W.epilogue64(np.full(c.spec.shape, 2.0, F), gamma=None, bias=c.bias, bias_tabs=c.bias_tabs)
    assert np.allclose(out, 2.0 * np.exp(b), rtol=1e-15)
    assert np.isnan(W.epilogue64(np.array([-1.0], F), gamma=0.9)).all()
