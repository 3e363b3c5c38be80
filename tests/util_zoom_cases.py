"""The case table of the zoom-family tests, shared by the CPU tests of the references (tests/test_zoom64_reference.py) and the GPU
tests of the kernels (tests/test_zoom_kernels_edges.py), so that what the CPU tests establish about the rounding bound holds for
the very cases the GPU tests run (not a test module).

A case is a source shape, three per-axis tables and, unless it brings its own, two sources: `rand * 255` and one with both signs,
exact zeros and twelve decades of magnitude.  Every shape is the smallest that reaches the edge it is named after; x and y stay
tiny wherever only z matters.  Which kernel of csrc/fsg_zoom.hip each group reaches is listed in DESIGN.md.
"""
import zlib
from collections import namedtuple

import numpy as np

from fetalsyngen_amd import tables as T

F = np.float32
Case = namedtuple("Case", "name shape tabs nch sources")

GROUPS = ("row length", "source row length", "rows", "many rows", "tile height", "ratio", "outside", "hand-made", "values",
          "three channels")


def ztab(n_src, n_dst):
    """tables.zoom_table for n_dst samples of an n_src-long axis (factor n_dst / n_src)."""
    t = T.zoom_table(int(n_src), float(n_dst) / float(n_src), int(n_dst))
    assert len(t) == n_dst, (n_src, n_dst, len(t))
    return t


def ztabs(src, dst):
    return [ztab(s, d) for s, d in zip(src, dst)]


def hand(lo, hi, w_hi=None, seed=0):
    """A hand-made table; weights non-negative (the rounding bound's premise), w_lo + w_hi == 1 up to rounding."""
    lo, hi = np.asarray(lo, dtype=np.int32), np.asarray(hi, dtype=np.int32)
    if w_hi is None:
        w_hi = np.random.RandomState(seed).rand(len(lo)).astype(F)
    w_hi = np.asarray(w_hi, dtype=F)
    return T._pack(lo, hi, F(1) - w_hi, w_hi)


def with_outside(tab, sel):
    """A copy of `tab` with the entries `sel` marked outside (lo = -1, hi = 0: what tables.position_table writes)."""
    t = tab.copy()
    t["lo"][sel] = -1
    t["hi"][sel] = 0
    return t


def check_inside(case):
    """Every index of every table lies inside the source (or is the outside mark): asserted on the host before any launch."""
    assert len(case.shape) == 3 and len(case.tabs) == 3, case.name
    for a, t in enumerate(case.tabs):
        assert t.dtype == T.TAP_DTYPE and len(t) >= 1, (case.name, a)
        lo, hi = t["lo"].astype(np.int64), t["hi"].astype(np.int64)
        ok = lo >= 0
        assert (lo[~ok] == -1).all(), (case.name, a)
        assert (lo[ok] < case.shape[a]).all() and (hi[ok] >= 0).all() and (hi[ok] < case.shape[a]).all(), (case.name, a)
        assert (hi[~ok] >= 0).all() and (hi[~ok] < case.shape[a]).all(), (case.name, a)  # never read, but harmless if it were
        assert np.isfinite(t["w_lo"]).all() and np.isfinite(t["w_hi"]).all(), (case.name, a)
        assert (t["w_lo"] >= 0).all() and (t["w_hi"] >= 0).all(), (case.name, a)


def sources(case):
    """[(label, float32 source)]: the case's own, or `rand * 255` and a twelve-decade one with both signs and exact zeros."""
    if case.sources is not None:
        return case.sources
    shape = tuple(case.shape) + ((3,) if case.nch == 3 else ())
    rs = np.random.RandomState(zlib.crc32(case.name.encode()) & 0x7FFFFFFF)
    u = (rs.rand(*shape) * 255).astype(F)
    w = (10.0 ** rs.uniform(-6, 6, shape) * rs.choice([-1.0, 1.0], shape, p=[0.3, 0.7])).astype(F)
    w[rs.rand(*shape) < 0.2] = 0
    return [("u255", u), ("wide", w)]


def _case(name, shape, tabs, nch=1, srcs=None):
    c = Case(name, tuple(int(v) for v in shape), list(tabs), nch, srcs)
    check_inside(c)
    return c


def _row_length():
    # dz % 4 in 0..3, the 64-lane steps, the cached (dz <= 256) and uncached z taps, the slab / prefetch domain limit
    # 41: the smallest dz at which float(m * dz) * RN(1 / dz) < m, so that the tile kernel's estimate of a quad's row is one too low
    assert int(F(2 * 41) * (F(1) / F(41))) == 1 and all(int(F(m * d) * (F(1) / F(d))) == m for d in range(1, 41) for m in range(1, 65))
    src_z = {1: 3, 2: 3, 3: 5, 4: 3, 5: 7, 41: 13, 63: 21, 64: 128, 65: 33, 255: 100, 256: 128, 257: 64, 300: 128}
    return [_case(f"dz={dz} from sz={sz}", (2, 3, sz), ztabs((2, 3, sz), (3, 5, dz))) for dz, sz in src_z.items()]


def _source_row_length():
    # the prefetch / slab domain (sz <= 256), the row kernel up to ZROWCAP = 1024, the per-voxel kernel beyond
    return [_case(f"sz={sz} dz={dz}", (2, 3, sz), ztabs((2, 3, sz), (3, 4, dz)))
            for sz, dz in ((255, 9), (256, 260), (257, 12), (1024, 300), (1025, 7))]


def _rows():
    # nblk of the row kernels below 8, equal to 8, not a multiple of 8
    out = [_case(f"rows={dx * dy} ({dx}x{dy})", (3, 4, 5), ztabs((3, 4, 5), (dx, dy, 6)))
           for dx, dy in ((1, 1), (1, 3), (7, 1), (2, 4), (3, 3), (9, 7), (8, 8), (5, 13))]
    return out


def _many_rows():
    return [
        # 16512 rows: nblk capped at 2048, 9 rows per block
        _case("rows=16512 (129x128)", (5, 6, 4), ztabs((5, 6, 4), (129, 128, 8))),
        # 529984 rows: 259 rows per block, a wave of the prefetch kernel starts a second chunk of 64 rows
        _case("rows=529984 (728x728)", (9, 9, 3), ztabs((9, 9, 3), (728, 728, 4))),
    ]


def _tile_height():
    # against ty in 1, 5, 16, 64 (the paths): nj < TY in the last tile, TY > dy, tiles_y of 1 and 2 and more; dx = 8: the number of
    # tiles is a multiple of 8 (XCD-contiguous remap on), dx = 7: it is not
    out = []
    for dy in (1, 15, 16, 17, 33, 64, 65):
        for dx, dz in ((7, 6), (8, 8)):
            out.append(_case(f"dy={dy} dx={dx} dz={dz}", (3, 9, 6), ztabs((3, 9, 6), (dx, dy, dz))))
    return out


def _ratio():
    n = (6, 10, 12)
    out = [_case(f"up x{f}", n, T.zoom_tables(n, (f, f, f))[0]) for f in (2, 3, 7.3)]
    out.append(_case("identity", n, T.zoom_tables(n, (1.0, 1.0, 1.0))[0]))
    out.append(_case("down to n/2", n, ztabs(n, (3, 5, 6))))
    out.append(_case("down to 1", n, ztabs(n, (1, 1, 1))))
    R = T._resample_axis_table
    out.append(_case("resample m == n (output 0 outside)", n, [R(6, 6), R(10, 10), R(12, 12)]))
    out.append(_case("resample n/2, 1, n", n, [R(3, 6), R(1, 10), R(12, 12)]))
    out.append(_case("mixed: up 7.3, down to 1, identity", n, [ztab(6, 44), ztab(10, 1), ztab(12, 12)]))
    return out


def _outside():
    n, d = (4, 12, 10), (5, 48, 12)
    base = ztabs(n, d)
    out = []
    for a in range(3):  # every entry outside on one axis: the output is all zero, the window code sees nrows <= 0
        tabs = list(base)
        tabs[a] = T.position_table(np.full(d[a], -1.0), n[a])
        assert (tabs[a]["lo"] < 0).all()
        out.append(_case(f"all outside on axis {a}", n, tabs))
    for a, sel in ((0, slice(2, 3)), (1, slice(20, 27)), (2, slice(5, 7))):  # outside entries in the middle of a tile
        tabs = list(base)
        tabs[a] = with_outside(base[a], sel)
        out.append(_case(f"outside in the middle of axis {a}", n, tabs))
    sel = np.r_[0:16, 32:48]  # at ty = 16 the first and the last of three y tiles are wholly outside
    out.append(_case("first and last y tile outside", n, [base[0], with_outside(base[1], sel), base[2]]))
    out.append(_case("outside on all three axes, scattered", n, [with_outside(base[0], [0, 4]), with_outside(base[1], sel[::3]),
                                                               with_outside(base[2], [0, 3, 11])]))
    return out


def _hand_made():
    n = (4, 20, 10)
    base = ztabs(n, (5, 40, 12))
    out = []
    for a in range(3):  # a flip: lo = hi = n - 1 - j, weights (1, 0)
        tabs = list(base)
        idx = n[a] - 1 - np.arange(n[a])
        tabs[a] = hand(idx, idx, np.zeros(n[a]))
        out.append(_case(f"flip on axis {a}", n, tabs))
    rs = np.random.RandomState(12)
    g = [rs.randint(0, n[a], m) for a, m in enumerate((5, 40, 12))]
    out.append(_case("random gather, hi = lo", n, [hand(g[a], g[a], seed=a) for a in range(3)]))
    # y alternates between row 0 and row sy - 1: the window of a tile of two or more rows is the whole axis.  sy = 20: 20 rows
    # against the launch's estimate of TY * 20 / 40 + 3 (11 at TY = 16: above the cap, the unstaged path; 23 at TY = 40: below)
    alt = np.where(np.arange(40) % 2 == 0, 0, 19)
    out.append(_case("y alternates 0 / sy-1, window above the cap", n, [base[0], hand(alt, alt, seed=3), base[2]]))
    # sy = 3: 3 rows against 16 * 3 / 40 + 3 = 4: below the cap at every tile height
    n3 = (4, 3, 10)
    alt3 = np.where(np.arange(40) % 2 == 0, 0, 2)
    out.append(_case("y alternates 0 / sy-1, window below the cap", n3, [ztab(4, 5), hand(alt3, alt3, seed=4), ztab(10, 12)]))
    # hi < lo (the header defines a tap as w_lo * src[lo] + w_hi * src[hi], nothing more): hi below every lo of its tile
    for a in range(3):
        tabs = list(base)
        m = len(base[a])
        lo = np.clip(3 + (np.arange(m) * (n[a] - 4)) // max(m - 1, 1), 0, n[a] - 1)
        tabs[a] = hand(lo, lo - 3, seed=20 + a)
        assert (tabs[a]["hi"] < tabs[a]["lo"]).all()
        out.append(_case(f"hi < lo on axis {a}", n, tabs))
    out.append(_case("hi < lo on every axis", n, [hand(np.full(5, 3), np.arange(5) % 3, seed=30),
                                                 hand(19 - np.arange(40) // 4, np.arange(40) // 4, seed=31),
                                                 hand(np.full(12, 9), np.arange(12) % 9, seed=32)]))
    return out


def _values():
    n, d = (3, 5, 8), (6, 10, 16)
    up = ztabs(n, d)  # output (0, 0, 0) is source (0, 0, 0) exactly (position clamped to 0, weights (1, 0))
    for t in up:
        assert t["lo"][0] == 0 and t["w_lo"][0] == 1 and t["w_hi"][0] == 0
    ident = T.zoom_tables(n, (1.0, 1.0, 1.0))[0]
    rs = np.random.RandomState(77)
    r = rs.rand(*n).astype(F)

    def peak(mx, scale):
        """Positive data below `mx`, and `mx` itself at (0, 0, 0): the maximum of the zoom is exactly `mx`."""
        x = (r * F(scale)).astype(F)
        x[0, 0, 0] = mx
        assert x.max() == mx and (x.ravel()[1:] < mx).all()
        return x

    ones = np.array(0x3FFFFFFF, dtype=np.int32).view(F)  # 1.9999999: an all-ones significand
    neg0 = (r * 3).astype(F)
    neg0[r < 0.4] = -0.0
    neg0[r > 0.9] = 0.0
    zeros_neg = -(r * 5).astype(F)
    zeros_neg[r < 0.5] = 0.0
    nan1 = (r * 255).astype(F)
    nan1[1, 2, 3] = np.nan
    tiny_min = peak(F(100), 90)
    tiny_min[r < 0.3] = 1e-7
    tiny_min[2, 4, 7] = 3e-8
    assert tiny_min.min() > 0 and F(1) - tiny_min.min() / tiny_min.max() == 1
    out = []
    for tname, tabs in (("up x2", up), ("identity", ident)):
        srcs = [
            ("flat c > 0", np.full(n, 7.25, F)), ("flat c < 0", np.full(n, -3.5, F)),
            ("all negative", (-1 - r * 100).astype(F)),
            ("minimum -0.0", neg0), ("maximum 0 (zeros and negatives)", zeros_neg), ("all zero", np.zeros(n, F)),
            ("all -0.0", np.full(n, -0.0, F)), ("one NaN voxel", nan1),
            ("max with an all-ones significand", peak(ones, 1.5)), ("max 1e-20", peak(F(1e-20), 0.9e-20)),
            ("max 1e20", peak(F(1e20), 0.9e20)), ("min / max below 2^-25 (1 - min / max == 1, min / max != 0)", tiny_min),
        ]
        out.append(_case(f"values, {tname}", n, tabs, srcs=srcs))
    # a flat image behind an all-outside axis: min == max == +0.0
    out.append(_case("values, all outside", n, [up[0], T.position_table(np.full(10, -1.0), 5), up[2]],
                     srcs=[("u255", (r * 255).astype(F)), ("negative", (-1 - r).astype(F))]))
    return out


def _three_channels():
    # zoom_nch_kernel<3>: 64 x 4 blocks over (dz * 3, dy); dz * 3 around 64 and 128, dy around 4
    n = (2, 3, 5)
    return [_case(f"3 channels {dx}x{dy}x{dz}", n, ztabs(n, (dx, dy, dz)), nch=3)
            for dx, dy, dz in ((1, 1, 1), (2, 4, 21), (1, 5, 22), (2, 5, 43), (2, 4, 43), (1, 1, 22), (2, 5, 21), (1, 4, 1))] + [
        _case("3 channels, outside on every axis", n, [with_outside(ztab(2, 2), [0]), with_outside(ztab(3, 5), [2]),
                                                      with_outside(ztab(5, 22), [0, 21])], nch=3),
        _case("3 channels, hi < lo", n, [hand([1, 1], [0, 0], seed=1), hand([2, 1, 2, 2, 1], [0, 0, 1, 0, 0], seed=2),
                                         hand(np.full(43, 4), np.arange(43) % 4, seed=3)], nch=3)]


_BUILDERS = {"row length": _row_length, "source row length": _source_row_length, "rows": _rows, "many rows": _many_rows,
             "tile height": _tile_height, "ratio": _ratio, "outside": _outside, "hand-made": _hand_made, "values": _values,
             "three channels": _three_channels}
_CACHE = {}


def cases(group):
    if group not in _CACHE:
        _CACHE[group] = _BUILDERS[group]()
    return _CACHE[group]


def all_cases():
    return [c for g in GROUPS for c in cases(g)]
