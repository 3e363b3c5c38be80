"""GPU: the six kernels of csrc/fsg_zoom.hip behind their dispatcher (zoom1_kernel, zoom1_rows_kernel, zoom1_rows_pf_kernel,
zoom_tile_kernel, zoom_slab_kernel, zoom_nch_kernel<3>) against the references of tests/util_zoom64.py, at the places where the
dispatcher and the kernels branch.  The case table is tests/util_zoom_cases.py (shared with the CPU tests of the references,
tests/test_zoom64_reference.py); which kernel each group reaches is listed in DESIGN.md.

For every case, each of its sources and every path (the default dispatch and each tuning flag that forces one kernel; the tile
and slab kernels also at four tile shapes, one of which, a cap of 256 floats, forces the launcher's fallback chain):
  (a) zoom3d equals zoom32 bit for bit, lies within util_resample64.error_bound of zoom64, is 0 wherever that bound is 0 and
      +0.0 at every outside output (the sign of a zero elsewhere is pinned by the bit-for-bit comparison: a source of -0.0
      legitimately gives -0.0);
  (b) zoom_minmax gives the keys of minmax32(zoom32): outside outputs count as 0, NaN is ignored;
  (c) the sharded min/max at 2, 3 and 64 slots: min over the slots' minima and max over their maxima equal (b), words 2..15 of
      every slot are untouched, every slot no workgroup maps to keeps its identities (slot = workgroup index % nslots; the
      number of workgroups of each path is restated from the launcher, sharded_workgroups);
  (d) zoom_normalise in modes 0 and 1, fed the keys and fed each set of slots, equals normalise32(zoom32, mn, mx, mode) bit for bit.
A NaN is compared as a NaN (its payload is not part of the contract).  No output is left out of any comparison, and no tolerance
is a literal.  Every output buffer is preceded by poison(): an element a kernel never writes is NaN, not a lucky zero.

The comparisons run on the device (the references are uploaded once per case and source); a failure is then located on the host.

kernel -> test
  zoom1_kernel                  test_paths["source row length"] (sz = 1025) and the "generic" path of every case
  zoom1_rows_kernel             "source row length", "row length" (dz > 256) and the "row, no prefetch" path of every case
  zoom1_rows_pf_kernel          the "row" path; "rows", "many rows" (2048-block cap, second 64-row chunk)
  zoom_tile_kernel              the "tile" paths; "tile height", "hand-made" (fits == false), test_misaligned_output,
                                test_large_noise_rows (dz = 198)
  zoom_slab_kernel              the "slab" paths and the default of zoom3d / normalise / sharded min/max; "values" (UniDiv and its
                                IEEE fallback behind a real min/max pass), test_misaligned_output, test_large_noise_rows
  zoom_nch_kernel<3>            test_paths["three channels"]
  argument checks               test_bad_arguments
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util_zoom64 as Z
from tests.test_blur_resample_edges import check as check_noise
from tests.util_zoom_cases import GROUPS, cases, sources

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
DEFAULT_TILE = (16, 12288)
TILE_SHAPES = (None, (1, 12288), (5, 12288), (16, 256), (64, 16000))  # None: the default; a cap of 256: the fallback chain
NSLOTS = (2, 3, 64)
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (and libfsg_hip.so); there is no fallback to skip to")
    from fetalsyngen_amd import kernels

    return kernels


def poison(*shapes):
    """Hand the next allocations of these shapes blocks full of NaN (the caching allocator reuses a freed block of the
    same size): an output a kernel never writes then fails the comparison instead of passing on a lucky zero."""
    for s in shapes:
        t = torch.full(s, float("nan"), device=DEV)
        del t


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def paths():
    """(name, tuning flags, tile shape): the flag names come from the header (_lib.TUNE)."""
    from fetalsyngen_amd import _lib

    T = _lib.TUNE
    out = [("default", 0, None), ("generic", T.GENERIC_ZOOM, None), ("row", T.ROW_ZOOM, None),
           ("row, no prefetch", T.ROW_ZOOM | T.NO_PREFETCH, None)]
    for name, flag in (("tile", T.TILE_ZOOM), ("slab", T.SLAB_ZOOM)):
        out += [(f"{name} {shape or 'default'}", flag, shape) for shape in TILE_SHAPES]
    return out


@contextlib.contextmanager
def on_path(flags, tile):
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    prev = lib.fsg_set_tuning(flags)
    try:
        assert lib.fsg_zoom_set_tuning(*(tile or DEFAULT_TILE)) == 0
        yield
    finally:
        lib.fsg_set_tuning(prev)
        lib.fsg_zoom_set_tuning(*DEFAULT_TILE)


def same(got, want):
    """Bit for bit, a NaN equal to a NaN; both float32 device tensors."""
    return got.shape == want.shape and bool(((got.view(torch.int32) == want.view(torch.int32))
                                             | (torch.isnan(got) & torch.isnan(want))).all())


def explain(what, got, want):
    g, w = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    if g.shape != w.shape:
        return f"{what}: shape {g.shape}, want {w.shape}"
    bad = ~((g.view(np.int32) == w.view(np.int32)) | (np.isnan(g) & np.isnan(w)))
    at = np.argwhere(bad)
    return (f"{what}: {int(bad.sum())} of {bad.size} outputs differ, first at {at[0].tolist()} (last at {at[-1].tolist()}): "
            f"got {g[bad][0]!r}, want {w[bad][0]!r}")


class Ref:
    """The references of one (case, source), computed once and uploaded once."""

    def __init__(self, case, x):
        self.y32 = Z.zoom32(x, case.tabs)
        y64, bound = Z.zoom64(x, case.tabs), Z.zoom_bound(x, case.tabs)
        self.d32, self.d64, self.dbound = dev(self.y32), dev(y64), dev(bound)
        self.dzero = dev(bound == 0)
        self.doutside = dev(Z.outside_mask(case.tabs, x.ndim) & np.ones(self.y32.shape, bool))
        if case.nch == 1:
            self.kmin, self.kmax = Z.minmax32(self.y32)
            self.dkeys = torch.tensor([self.kmin, self.kmax], dtype=torch.int32, device=DEV)
            mn, mx = Z.key2f(self.kmin), Z.key2f(self.kmax)
            self.dnorm = [dev(Z.normalise32(self.y32, mn, mx, mode)) for mode in (0, 1)]


def check_zoom(out, R, what):
    """(a): bit for bit zoom32; within the rounding bound of zoom64; 0 where the bound is 0; +0.0 outside."""
    assert same(out, R.d32), explain(what, out, R.d32)
    err = (out.double() - R.d64).abs()
    ok = (err <= R.dbound) | (torch.isnan(out) & torch.isnan(R.d64))
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} outputs beyond the rounding bound of the float64 zoom"
    assert bool((out[R.dzero] == 0).all()), f"{what}: not 0 where every input is 0"
    assert bool((out.view(torch.int32)[R.doutside] == 0).all()), f"{what}: an outside output is not +0.0"


def new_slots(nslots):
    from fetalsyngen_amd import _lib

    s = torch.full((nslots, _lib.MM_SLOT_STRIDE), SENTINEL, dtype=torch.int32, device=DEV)
    s[:, 0], s[:, 1] = Z.KEY_MIN_IDENTITY, Z.KEY_MAX_IDENTITY
    return s


def minmax_sharded(K, xd, rt, nslots):
    """fsg_zoom3d_minmax_sharded_f32 on slots whose unused words hold a sentinel (kernels.zoom_minmax_sharded zeroes them)."""
    from fetalsyngen_amd import _lib

    slots = new_slots(nslots)
    sx, sy, sz = xd.shape
    rc = _lib.load().fsg_zoom3d_minmax_sharded_f32(C.c_void_p(xd.data_ptr()), sx, sy, sz, *rt.ptrs, *rt.lengths,
                                                   C.c_void_p(slots.data_ptr()), nslots, K._stream(xd))
    assert rc == 0, rc
    return slots


def sharded_workgroups(shape, new, flags, tile):
    """Workgroups of the sharded min/max pass for a source `shape`, an output `new`, tuning flags and a tile shape.  The header
    says slot = workgroup index % nslots; how many workgroups there are is the launcher's choice, restated here from
    launch1<EPI_MINMAX> (csrc/fsg_zoom.hip, mm_shards > 1) so that EVERY slot without a workgroup can be held to its identities.
    A change of the launch shapes there changes this function with it."""
    from fetalsyngen_amd import _lib

    T = _lib.TUNE
    (_sx, sy, sz), (dx, dy, dz) = shape, new
    ty, cap = tile or DEFAULT_TILE
    rows = dx * dy
    if flags & T.TILE_ZOOM and not flags & (T.GENERIC_ZOOM | T.ROW_ZOOM | T.SLAB_ZOOM):
        TY = min(ty, 64, dy)
        est = (TY * sy // dy + 3) * sz
        if est <= cap and est + 4 * dz <= 16000:
            return dx * ((dy + TY - 1) // TY)
    if not flags & (T.GENERIC_ZOOM | T.ROW_ZOOM | T.TILE_ZOOM):
        for mult in (4, 2, 1):  # the tallest tile whose window fits
            TY = min(mult * ty, 64, dy)
            est = (TY * sy // dy + 3) * sz
            fits = est <= cap and est + 5 * 256 <= 16000
            if fits:
                break
        if fits and sz <= 256 and dz <= 256:
            return dx * ((dy + TY - 1) // TY)
    if sz <= 1024 and not flags & T.GENERIC_ZOOM:
        nblk = min((rows + 7) // 8, 2048)
        return nblk & ~7 if nblk >= 8 else nblk
    return min(rows, 4096)


def occupied(slots):
    """Number of slots that left their identities."""
    return int(((slots[:, 0] != Z.KEY_MIN_IDENTITY) | (slots[:, 1] != Z.KEY_MAX_IDENTITY)).sum())


def run_one(K, case, label, R, pname, flags, tile):
    """(a) .. (d) for one (case, source) on the path that is set."""
    what = f"{case.name} / {label} [{pname}]"
    xd, rt = R.xd, R.rt
    new = rt.lengths
    poison(R.y32.shape)
    check_zoom(K.zoom3d(xd, rt), R, f"{what} zoom3d")
    if case.nch != 1:
        return
    mm = K.zoom_minmax(xd, rt)
    assert torch.equal(mm, R.dkeys), f"{what} zoom_minmax: keys {mm.tolist()}, want {R.dkeys.tolist()}"
    fed = [("keys", mm)]
    nwg = sharded_workgroups(case.shape, new, flags, tile)
    assert 1 <= nwg <= new[0] * new[1]
    for nslots in NSLOTS:
        s = minmax_sharded(K, xd, rt, nslots)
        got = torch.stack([s[:, 0].min(), s[:, 1].max()])
        assert torch.equal(got, R.dkeys), f"{what} sharded min/max, {nslots} slots: {got.tolist()}, want {R.dkeys.tolist()}"
        assert bool((s[:, 2:] == SENTINEL).all()), f"{what} sharded min/max, {nslots} slots: words 2..15 of a slot written"
        assert occupied(s[nwg:]) == 0, (f"{what} sharded min/max, {nslots} slots, {nwg} workgroups: a slot no workgroup maps to "
                                        f"lost its identities")
        fed.append((f"{nslots} slots", s))
    for name, keys in fed:
        for mode in (0, 1):
            poison(new)
            out = K.zoom_normalise(xd, rt, keys, mode)
            assert same(out, R.dnorm[mode]), explain(f"{what} zoom_normalise mode {mode} fed the {name}", out, R.dnorm[mode])


@pytest.mark.parametrize("group", GROUPS)
def test_paths(K, group):
    """(a) .. (d) (module docstring) for every case of the group, each source, on every path."""
    for case in cases(group):
        rt = K.DeviceTables(case.tabs, DEV)
        assert rt.lengths == tuple(len(t) for t in case.tabs)
        for label, x in sources(case):
            assert x.shape[:3] == case.shape  # with util_zoom_cases.check_inside: no tap points outside the source
            R = Ref(case, x)  # once per (case, source): every path is held to the same arrays
            R.xd, R.rt = dev(x), rt
            for pname, flags, tile in (paths() if case.nch == 1 else paths()[:1]):  # zoom_nch_kernel has one path
                with on_path(flags, tile):
                    run_one(K, case, label, R, pname, flags, tile)


def zoom_into(K, lib, fn, xd, rt, dst_ptr, extra=()):
    sx, sy, sz = xd.shape
    if fn == "fsg_zoom3d_f32":
        return lib.fsg_zoom3d_f32(C.c_void_p(xd.data_ptr()), sx, sy, sz, 1, *rt.ptrs, C.c_void_p(dst_ptr), *rt.lengths,
                                  K._stream(xd))
    return lib.fsg_zoom3d_normalise_f32(C.c_void_p(xd.data_ptr()), sx, sy, sz, *rt.ptrs, C.c_void_p(dst_ptr), *rt.lengths,
                                        *extra, K._stream(xd))


def test_misaligned_output(K):
    """dst 4, 8 and 12 bytes into a larger poisoned buffer, rows of dz % 4 == 0 floats: the slab and tile kernels must leave
    their 16-byte stores for single ones, write every output and nothing on either side of the range."""
    from fetalsyngen_amd import _lib
    from tests.util_zoom_cases import Case, check_inside, ztabs

    lib, T = _lib.load(), _lib.TUNE
    PAD = 8
    for shape, new in (((3, 9, 6), (8, 17, 8)), ((2, 3, 128), (3, 5, 64)), ((2, 3, 40), (2, 3, 256))):
        case = Case(f"misaligned {new}", shape, ztabs(shape, new), 1, None)
        check_inside(case)
        rt = K.DeviceTables(case.tabs, DEV)
        n = int(np.prod(new))
        for label, x in sources(case):
            R = Ref(case, x)
            xd = dev(x)
            mm = K.zoom_minmax(xd, rt)
            assert torch.equal(mm, R.dkeys)
            for pname, flags, tile in (("default", 0, None), ("tile", T.TILE_ZOOM, None), ("tile (5, 12288)", T.TILE_ZOOM, (5, 12288)),
                                       ("slab", T.SLAB_ZOOM, None), ("slab (5, 12288)", T.SLAB_ZOOM, (5, 12288)),
                                       ("slab (16, 256)", T.SLAB_ZOOM, (16, 256))):
                with on_path(flags, tile):
                    for off in (1, 2, 3):  # floats: 4, 8, 12 bytes
                        for fn, extra, want in (("fsg_zoom3d_f32", (), R.d32),
                                                ("fsg_zoom3d_normalise_f32", (C.c_void_p(mm.data_ptr()), 0), R.dnorm[0]),
                                                ("fsg_zoom3d_normalise_f32", (C.c_void_p(mm.data_ptr()), 1), R.dnorm[1])):
                            buf = torch.full((PAD + n + PAD,), float("nan"), device=DEV)
                            assert buf.data_ptr() % 16 == 0
                            lo = PAD - 4 + off
                            ptr = buf.data_ptr() + 4 * lo
                            assert ptr % 16 == 4 * off
                            assert zoom_into(K, lib, fn, xd, rt, ptr, extra) == 0
                            what = f"{case.name} / {label} [{pname}] {fn}{extra[1:]} dst + {4 * off} bytes"
                            out = buf[lo:lo + n].view(new)
                            assert same(out, want), explain(what, out, want)
                            assert bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + n:]).all()), (
                                f"{what}: a float beside the output range was written")


def test_large_noise_rows(K):
    """K7 + K8 with a noise pointer at rows of 196, 198, 200 and 256 outputs from at most 256 inputs: from 196 on the noise
    epilogues switch from the tile to the slab kernel, for row lengths that are a multiple of 4 only (198 stays on the tile
    kernel).  Against the float64 reference and its rounding bound, as tests/test_blur_resample_edges.py does."""
    from fetalsyngen_amd import _lib
    from fetalsyngen_amd import tables as T

    TUNE = _lib.TUNE
    shape = (4, 6, 256)
    rs = np.random.RandomState(21)
    x = (rs.rand(*shape) * 255).astype(F)
    x[:1] *= 0.1
    xd = dev(x)
    for dz in (196, 198, 200, 256):
        tabs = [T._resample_axis_table(2, 4), T._resample_axis_table(5, 6), T._resample_axis_table(dz, 256)]
        new = tuple(len(t) for t in tabs)
        assert new == (2, 5, dz) and all((t["hi"] < n).all() and (t["lo"] < n).all() for t, n in zip(tabs, shape))
        rt = K.DeviceTables(tabs, DEV)
        zd = K.randn(new, 7, 3, DEV)
        z = zd.cpu().numpy()
        outside = [a for a in range(3) if tabs[a]["lo"][0] < 0]
        for pname, flags in (("default", 0), ("tile", TUNE.TILE_ZOOM), ("slab", TUNE.SLAB_ZOOM), ("row", TUNE.ROW_ZOOM)):
            with on_path(flags, None):
                for std in (11.0, 300.0):  # 300: a good part of the outputs is clamped to exactly 0
                    poison(new)
                    out = K.resample_noise(xd, rt, noise_std=std, noise=zd)
                    torch.cuda.synchronize()
                    e = check_noise(f"noise rows dz={dz}", pname, out, x, (None,) * 3, tabs, z, std, outside)
                poison(new)
                plain = K.resample_noise(xd, rt)  # noise_mode 0
                torch.cuda.synchronize()
                check_noise(f"rows dz={dz}, no noise", pname, plain, x, (None,) * 3, tabs, None, None, outside)
                assert np.array_equal(plain.cpu().numpy().view(np.int32), Z.zoom32(x, tabs).view(np.int32)), (dz, pname)
        print(f"EDGE noise rows dz={dz}: max error {e[0]:.3e} ({e[1]:.3f} of bound)")


def test_bad_arguments(K):
    """Every FSG_E_BADARG / FSG_E_TOOBIG branch of the six zoom entry points and of fsg_zoom_set_tuning.  These return before any
    launch: the poisoned dst, the keys and the slots stay as they were (looked at before any accepted call follows), and a refused
    fsg_zoom_set_tuning leaves the tile shape as it was.  The unchanged argument list of each entry point is run once first (a
    2 x 2 x 2 identity zoom), so that a refusal is the changed argument's."""
    from fetalsyngen_amd import _lib
    from fetalsyngen_amd import tables as T

    lib, st = _lib.load(), K._stream(None)
    BAD, BIG = _lib.E_BADARG, _lib.E_TOOBIG
    assert BAD != 0 and BIG != 0 and BAD != BIG
    tabs = T.zoom_tables((2, 2, 2), (1.0, 1.0, 1.0))[0]
    rt = K.DeviceTables(tabs, DEV)
    x = torch.arange(1, 25, dtype=torch.float32, device=DEV)       # 2 x 2 x 2 x 3: enough for nch = 3
    noise = torch.zeros(8, device=DEV)
    mm, slots = K.new_minmax(DEV), new_slots(64)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    N = C.c_void_p(0)
    S, D = dict(src=P(x), sx=2, sy=2, sz=2), dict(dx=2, dy=2, dz=2)
    TAB = dict(tx=rt.ptrs[0], ty=rt.ptrs[1], tz=rt.ptrs[2])
    dst = torch.full((24,), float("nan"), device=DEV)
    entry = {  # name -> its arguments in order (without the stream), all valid
        "fsg_zoom3d_f32": dict(**S, nch=1, **TAB, dst=P(dst), **D),
        "fsg_resample_noise_f32": dict(**S, **TAB, dst=P(dst), **D, noise_mode=1, noise=P(noise), seed=1, stream_id=2, noise_std=0.5),
        "fsg_zoom3d_minmax_f32": dict(**S, **TAB, **D, mm=P(mm)),
        "fsg_zoom3d_normalise_f32": dict(**S, **TAB, dst=P(dst), **D, mm=P(mm), mode=1),
        "fsg_zoom3d_minmax_sharded_f32": dict(**S, **TAB, **D, slots=P(slots), nslots=64),
        "fsg_zoom3d_normalise_sharded_f32": dict(**S, **TAB, dst=P(dst), **D, slots=P(slots), nslots=64, mode=1),
    }
    assert set(entry) | {"fsg_zoom_set_tuning"} == {n for n in _lib.PROTOTYPES if "zoom" in n or n == "fsg_resample_noise_f32"}
    for fn, good in entry.items():  # the baseline is accepted (min/max first: the normalise passes read its keys)
        assert getattr(lib, fn)(*good.values(), st) == 0, fn
    torch.cuda.synchronize()
    mm_before, slots_before = mm.clone(), slots.clone()
    dst.fill_(float("nan"))
    ncalls = 0
    for fn, good in entry.items():
        changes = [(k, N) for k in good if isinstance(good[k], C.c_void_p)]           # a null pointer for each pointer argument
        changes += [(k, v) for k in ("sx", "sy", "sz", "dx", "dy", "dz") for v in (0, -1)]  # each dimension 0 and negative
        if "dst" in good:
            changes.append(("dst", good["src"]))                                     # src == dst
        if "nch" in good:
            changes += [("nch", v) for v in (0, 2, 4)]
        if "mode" in good:
            changes += [("mode", v) for v in (-1, 2)]
        if "nslots" in good:
            changes += [("nslots", v) for v in (1, 65)]
        if "noise_mode" in good:
            changes += [("noise_mode", 3), ("noise_mode", -1)]  # (noise_mode 1 without a pointer: the null-pointer change above)
        for k, v in changes:
            a = dict(good)
            a[k] = v
            assert getattr(lib, fn)(*a.values(), st) == BAD, (fn, k, v)
            ncalls += 1
        # too large, by dimensions alone over the small buffers: more than 0x7FFFFFFF / 4 source elements, more than
        # 0x7FFFFFFF destination elements
        for dims in (dict(sx=1024, sy=1024, sz=513), dict(dx=2048, dy=2048, dz=513)):
            a = dict(good)
            a.update(dims)
            assert getattr(lib, fn)(*a.values(), st) == BIG, (fn, dims)
            ncalls += 1
        # sizes just below both limits pass the size check: the null output pointer, which is looked at after it, is what
        # refuses them (no launch)
        a = dict(good)
        a.update(dict(sx=1024, sy=1024, sz=511, dx=2048, dy=2048, dz=511))
        a["dst" if "dst" in a else "mm" if "mm" in a else "slots"] = N
        assert getattr(lib, fn)(*a.values(), st) == BAD, fn
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all()), "a refused call wrote to dst"
    assert torch.equal(mm, mm_before) and torch.equal(slots, slots_before), "a refused call wrote keys"
    assert torch.equal(x, torch.arange(1, 25, dtype=torch.float32, device=DEV))
    # a noise pointer is not needed without noise_mode 1 (Philox, or no noise): accepted (into a dst of their own)
    dst2 = torch.full((8,), float("nan"), device=DEV)
    for mode in (0, 2):
        a = dict(entry["fsg_resample_noise_f32"])
        a.update(noise_mode=mode, noise=N, dst=P(dst2))
        assert lib.fsg_resample_noise_f32(*a.values(), st) == 0, mode
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dst2).any())
    # fsg_zoom_set_tuning: a refused call leaves the setting as it was.  Seen from outside through the number of slots the sharded
    # min/max occupies: (2, 4, 64) -> (1, 64, 8) at (64, 256) finds no tile whose window fits 256 floats and runs the row kernel
    # on 8 workgroups; with y_rows turned into 16 it would be the slab kernel on 4, with the cap turned into 12288 on 1
    from tests.util_zoom_cases import ztabs

    shape, new = (2, 4, 64), (1, 64, 8)
    probe_rt = K.DeviceTables(ztabs(shape, new), DEV)
    probe_x = torch.rand(shape, device=DEV) + 1
    held = (64, 256)
    nwg = sharded_workgroups(shape, new, 0, held)
    assert (nwg, sharded_workgroups(shape, new, 0, (16, 256)), sharded_workgroups(shape, new, 0, (64, 12288))) == (8, 4, 1)
    try:
        assert lib.fsg_zoom_set_tuning(*held) == 0
        assert occupied(minmax_sharded(K, probe_x, probe_rt, 64)) == nwg
        for y_rows, cap in ((0, 12288), (65, 12288), (-1, 12288), (16, 255), (16, 16001), (16, -1)):
            assert lib.fsg_zoom_set_tuning(y_rows, cap) == BAD, (y_rows, cap)
            assert occupied(minmax_sharded(K, probe_x, probe_rt, 64)) == nwg, f"refused ({y_rows}, {cap}) changed the setting"
        for y_rows, cap in ((1, 256), (64, 16000)):  # the ends of the domain are inside it
            assert lib.fsg_zoom_set_tuning(y_rows, cap) == 0, (y_rows, cap)
    finally:
        assert lib.fsg_zoom_set_tuning(*DEFAULT_TILE) == 0
    assert ncalls == 134
