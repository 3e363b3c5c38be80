"""GPU: the fused warp (csrc/fsg_warp_lean.hip, csrc/fsg_deform.hip) and its set-up kernels against the references of
tests/util_warp64.py, at the places where the launchers and the kernels branch.  The case table is tests/util_warp_cases.py (shared
with the CPU tests of the references, tests/test_warp64_reference.py); which kernel each group reaches is listed in DESIGN.md.

Paths: the default dispatch, NO_LEAN, NO_PATCH and GENERIC_WARP, each also with PRECISE_MATH, each with and without the row workspace
of DeformSpec.prepare_rows: 16 per case, every case with and without flip.  util_warp_cases.warp_kernel restates launch_warp: it
names the kernel a path lands on, the table names the default's, and the one thing visible from outside -- whether the lean kernel
accepts (fsg_warp_f32_u8_to_f32 and fsg_warp_dual_f32 return FSG_E_ALIGN exactly when it declines) -- is held to it.

For every case and path:
  (a) coords_minmax gives exactly the six keys of minmax32 (-0.0 below +0.0); coords_floormin (six-face pass, conditional full
      pass) and coords_floormin_rest give keys with the same floors; where fsg_coords_floormin_f32 returns FSG_E_TOOBIG
      (3 * f2 > 512) the fallback gives the same floors;
  (b) coords equals positions32 - margins, bit for bit;
  (c) the row workspace equals rows32 bit for bit, from deform_rows_block_kernel and deform_rows_kernel (SPLIT_HEAD, or a grid
      beyond the block kernel's LDS slabs); the floats between `need` and the stride keep their poison; a stride below `need` is
      FSG_E_BADARG and writes nothing;
  (d) warp without epilogue, label forms f32 -> f32, u8 -> u8 and u8 -> f32, image and label sources also as views that start 4
      bytes and 1 byte into their buffers, image-only and label-only launches: labels equal `nearest` bit for bit; the image equals
      linear32 bit for bit, the sign of every zero included, on the patch, row and per-voxel kernels.  The lean kernel clamps no
      index: at an output with a coordinate exactly on the last plane, row or column it multiplies another (finite) neighbour by
      its zero weight than the reference does, so there -- and only there (asserted on the host) -- the sign of a zero output may
      differ; the lean kernel is held bit for bit, zeros included, to linear32(lean=True), which restates that reading, and in value
      to linear32.  (Its v_med3 clamp may turn a coordinate of -0.0 into +0.0: such an output is outside by the strict > 0 rule
      and is the literal +0.0 either way, and rint gives index 0 for both.)
  (e) warp with gamma, with bias and with both lies within atol 1e-3 + rtol 1e-5 (ATOL / RTOL of tests/test_hip_parity.py, the 0..255
      scale) of epilogue64(linear32); an output whose plain value is 0 stays exactly 0; a NaN (negative image under gamma) is a NaN;
      all PRECISE_MATH paths agree bit for bit (between a lean launch and another kernel's: in value, see (d)).  The largest error-to-tolerance ratios are printed (EDGE warp epilogue ...);
  (f) src_img (fsg_warp_dual_f32) inside the lean domain and on the two-launch fallback outside: out_img equals linear32(src_img),
      out_lin and out_nn are what the launch without src_img gives;
  (g) interp3d in both modes: coordinates exactly 0, exactly n - 1, beyond either end, on ties; a non-zero default_value.
Every mm6 handed to a warp comes from the library's own min/max pass.  Every output allocation is preceded by poison(); no output is
left out of any comparison.

kernel -> test
  warp_lean_kernel              test_paths: the default path of every case whose table entry is "lean" ("z extent" n2 = 2 .. 512:
                                one and two steps per loop trip, both pacings in "exact positions"); HAS_IMG: (f)
  warp_patch_kernel             test_paths: NO_LEAN paths; the default of "z extent" n2 = 513, 520 (z taps from global memory),
                                "coarse grids" f2 = 33, 42, b2 = 33
  warp_rows_kernel              test_paths: NO_PATCH paths (n2 > 256: the uncached loop); the default of "coarse grids" f2 = 43, 170
                                and of f2 = 42 with b2 = 3
  warp_kernel                   test_paths: GENERIC_WARP paths; every path of "z extent" (5,4,1) and of "coarse grids" f2 = 171
  coords_minmax_kernel          (a) on GENERIC_WARP paths and at f2 = 171
  coords_minmax_rows_kernel<false>  (a) on the other paths (with and without the workspace; n2 > 256: uncached)
  coords_minmax_rows_kernel<true>   (a) coords_floormin_rest, and coords_floormin of "nonzero margins" (the full pass must run)
  coords_faces_min_kernel       (a) coords_floormin
  coords_kernel                 (b)
  deform_rows_block_kernel      (c)
  deform_rows_kernel            (c) under SPLIT_HEAD, and "coarse grids" field slab 5*140*3 / bias slab 5*52
  interp_kernel                 test_interp3d
  argument checks               test_bad_arguments
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util_warp64 as W
from tests import util_zoom64 as Z
from tests.util_warp_cases import GROUPS, cases, has_workspace, rows_block_fits, rows_need, sources, warp_kernel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
ATOL, RTOL = 1e-3, 1e-5  # tests/test_hip_parity.py, SURVEY section 8(c)
GAMMA = 0.9
RATIO = {"fast": 0.0, "precise": 0.0}


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (and libfsg_hip.so); there is no fallback to skip to")
    from fetalsyngen_amd import kernels

    return kernels


def poison(*shapes, dtype=torch.float32):
    """Hand the next allocations of these shapes blocks full of NaN (0xFF bytes for uint8): the caching allocator reuses a freed
    block of the same size, so an output a kernel never writes fails the comparison instead of passing on a lucky value."""
    for s in shapes:
        t = torch.full(s, float("nan") if dtype == torch.float32 else 255, dtype=dtype, device=DEV)
        del t


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_view(a):
    """The array on the device as a contiguous view that starts one element (4 bytes, or 1 byte for uint8) into its buffer."""
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a[:0].ravel()).dtype, device=DEV)
    v = buf[1:].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + a.itemsize
    return v


def same(got, want):
    """Bit for bit (the sign of a zero included), a NaN equal to a NaN."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype != torch.float32:
        return bool((got == want).all())
    return bool(((got.view(torch.int32) == want.view(torch.int32)) | (torch.isnan(got) & torch.isnan(want))).all())


def explain(what, got, want):
    g, w = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    if g.shape != w.shape or g.dtype != w.dtype:
        return f"{what}: {g.dtype}{g.shape}, want {w.dtype}{w.shape}"
    if g.dtype == F:
        bad = ~((g.view(np.int32) == w.view(np.int32)) | (np.isnan(g) & np.isnan(w)))
    else:
        bad = g != w
    at = np.argwhere(bad)
    return (f"{what}: {int(bad.sum())} of {bad.size} outputs differ, first at {at[0].tolist()} (last at {at[-1].tolist()}): "
            f"got {g[bad][0]!r}, want {w[bad][0]!r}")


def paths():
    """(name, tuning flags, with the row workspace)."""
    from fetalsyngen_amd import _lib

    T = _lib.TUNE
    out = []
    for name, flag in (("default", 0), ("NO_LEAN", T.NO_LEAN), ("NO_PATCH", T.NO_PATCH), ("GENERIC_WARP", T.GENERIC_WARP)):
        for pname, precise in (("", 0), (" PRECISE_MATH", T.PRECISE_MATH)):
            for rows in (False, True):
                out.append((f"{name}{pname}{', rows' if rows else ''}", flag | precise, rows))
    return out


@contextlib.contextmanager
def tuning(flags):
    from fetalsyngen_amd import _lib

    lib = _lib.load()
    prev = lib.fsg_set_tuning(flags)
    try:
        yield
    finally:
        lib.fsg_set_tuning(prev)


def make_spec(K, case, flip, rows, bias=None, bias_tabs=None):
    s = case.spec
    field = tabs = None
    if s.field is not None:
        field, tabs = dev(s.field), K.DeviceTables(s.tabs, DEV)
    spec = K.DeformSpec(s.shape, s.A, s.cen, s.c2, flip, field, tabs, device=DEV)
    if rows:
        if has_workspace(case):
            poison((s.shape[0] * s.shape[1] * ((rows_need(case) + 3) // 4 * 4),))
        spec.prepare_rows(bias, bias_tabs)
        assert bool(spec.c.rows) == has_workspace(case), case.name
    return spec


class Ref:
    """The references of one case, computed once and uploaded once; every path is held to the same arrays."""

    def __init__(self, K, case):
        self.case, s = case, case.spec
        self.S = S = sources(case)
        p32 = W.positions32(s)
        self.keys = W.minmax32(p32)
        self.m = W.margins(self.keys)
        self.pos = W.subtract_margins(p32, self.keys)
        self.dpos = [dev(p) for p in self.pos]
        self.dkeys = torch.tensor(self.keys, dtype=torch.int32, device=DEV)
        self.src = {k: dev(v) for k, v in S.items()}
        self.src["img_v"], self.src["lab8_v"] = dev_view(S["img"]), dev_view(S["lab8"])
        self.bias = self.bt = None
        if case.bias is not None:
            self.bias, self.bt = dev(case.bias), K.DeviceTables(case.bias_tabs, DEV)
        self.rows = W.rows32(s, case.bias, case.bias_tabs) if rows_need(case) else None
        upper = W.on_upper_limit(s.shape, self.pos)
        self.flip = {}
        for flip in (False, True):
            R = {}
            for name in ("img", "signs", "pos"):
                lin = W.linear32(S[name], self.pos, flip)
                R[name, "clamp"] = dev(lin)
                if s.shape[2] >= 2:
                    lean = W.linear32(S[name], self.pos, flip, lean=True)
                    d = lean.view(np.int32) != lin.view(np.int32)
                    assert np.array_equal(lean, lin) and not (d & ~upper).any(), case.name  # zero signs, on the upper limits only
                    R[name, "lean"] = dev(lean)
                R[name, "host"] = lin
            for name in ("lab8", "labf"):
                R[name] = dev(W.nearest(S[name], self.pos, flip))
            R["lab8f"] = R["lab8"].to(torch.float32)
            self.flip[flip] = R
        self.epi = {}

    def epilogue(self, flip, name, gamma, bias):
        """(float64 reference, tolerance, plain-zero mask) on the device, once per (flip, source, epilogue)."""
        key = (flip, name, gamma, bias)
        if key not in self.epi:
            lin = self.flip[flip][name, "host"]
            ref = W.epilogue64(lin, GAMMA if gamma else None, self.case.bias if bias else None, self.case.bias_tabs if bias else None)
            with np.errstate(all="ignore"):
                tol = ATOL + RTOL * np.abs(ref)
            self.epi[key] = (dev(ref), dev(tol), dev(lin == 0))
        return self.epi[key]


def lean_probe(K, spec, mm, img, lab8):
    """fsg_warp_f32_u8_to_f32 called directly: (return code, image, float32 labels)."""
    from fetalsyngen_amd import _lib

    out_lin, out_nn = (torch.full(spec.shape, float("nan"), device=DEV) for _ in range(2))
    epi = K._epilogue(None, None, None, spec.shape)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = _lib.load().fsg_warp_f32_u8_to_f32(C.byref(spec.c), P(mm), P(img), P(out_lin), P(lab8), P(out_nn), C.byref(epi),
                                            K._stream(mm))
    return rc, out_lin, out_nn


def check_setup(K, R, spec, what, flags):
    """(a) and (b) on the path that is set; returns the library's own six keys."""
    from fetalsyngen_amd import _lib

    case = R.case
    mm6 = K.coords_minmax(spec)
    assert torch.equal(mm6, R.dkeys), f"{what} coords_minmax: keys {mm6.tolist()}, want {R.keys}"
    floors = R.m[:3]
    fm = K.coords_floormin(spec)
    assert [int(np.floor(v)) for v in Z.key2f(fm.cpu().numpy()[:3])] == floors, f"{what} coords_floormin: {fm.tolist()}"
    f2 = case.spec.field.shape[2] if case.spec.field is not None else 0
    mm3 = K.new_minmax(DEV, 3, 0)
    rc = _lib.load().fsg_coords_floormin_f32(C.byref(spec.c), C.c_void_p(mm3.data_ptr()), K._stream(mm3))
    assert rc == (_lib.E_TOOBIG if 3 * f2 > 512 else 0), (what, rc)
    if 3 * f2 <= 512:
        rest = K.coords_floormin_rest(spec, K.new_minmax(DEV, 3, 0))
        assert [int(np.floor(v)) for v in Z.key2f(rest.cpu().numpy()[:3])] == floors, f"{what} coords_floormin_rest: {rest.tolist()}"
    poison(spec.shape, spec.shape, spec.shape)
    for a, got in enumerate(K.coords(spec, mm6)):
        assert same(got, R.dpos[a]), explain(f"{what} coords axis {a}", got, R.dpos[a])
    return mm6


def check_rows(K, R, spec, what):
    """(c) for the workspace prepare_rows left."""
    case = R.case
    if not spec.c.rows:
        return
    need, stride = rows_need(case), int(spec.c.row_stride)
    buf = spec._keep[-1].view(-1, stride)
    want = dev(R.rows.reshape(-1, need))
    assert same(buf[:, :need].contiguous(), want), explain(f"{what} rows", buf[:, :need].contiguous(), want)


def check_rows_direct(K, R):
    """(c) through fsg_deform_rows_f32 itself: both kernels, an odd stride, the poison between `need` and the stride, FSG_E_BADARG."""
    from fetalsyngen_amd import _lib

    case, lib = R.case, _lib.load()
    need = rows_need(case)
    if need == 0:
        return
    spec = make_spec(K, case, False, False)
    epi = K._epilogue(None, R.bias, R.bt, spec.shape)
    nrow = spec.shape[0] * spec.shape[1]
    want = dev(R.rows.reshape(nrow, need))
    for name, flags in (("block" if rows_block_fits(case) else "per entry", 0), ("per entry (SPLIT_HEAD)", _lib.TUNE.SPLIT_HEAD)):
        with tuning(flags):
            stride = need + 5
            buf = torch.full((nrow, stride), float("nan"), device=DEV)
            rc = lib.fsg_deform_rows_f32(C.byref(spec.c), C.byref(epi), C.c_void_p(buf.data_ptr()), stride, K._stream(buf))
            assert rc == 0, (case.name, name, rc)
            got = buf[:, :need].contiguous()
            assert same(got, want), explain(f"{case.name} fsg_deform_rows_f32 [{name}]", got, want)
            assert bool(torch.isnan(buf[:, need:]).all()), f"{case.name} fsg_deform_rows_f32 [{name}]: padding written"
            buf.fill_(float("nan"))
            rc = lib.fsg_deform_rows_f32(C.byref(spec.c), C.byref(epi), C.c_void_p(buf.data_ptr()), need - 1, K._stream(buf))
            assert rc == _lib.E_BADARG and bool(torch.isnan(buf).all()), (case.name, name, rc)


def check_warp(K, R, spec, mm6, flip, what, flags, rows):
    """(d) on the path that is set."""
    from fetalsyngen_amd import _lib

    T, case, X, src = _lib.TUNE, R.case, R.flip[flip], R.src
    kern = warp_kernel(case, flags, T, rows, False)
    mode = "lean" if kern == "lean" else "clamp"
    shape = spec.shape

    def image(got, name, label):
        want = X[name, mode]
        assert same(got, want), explain(f"{what} {label} image on {kern}", got, want)
        assert bool((got == X[name, "clamp"]).all()), f"{what} {label}: image differs in value from linear32 on {kern}"

    poison(shape, shape)
    out, lab = K.warp(spec, mm6, src_lin=src["img"], src_nn=src["labf"])
    image(out, "img", "f32 -> f32")
    assert same(lab, X["labf"]), explain(f"{what} f32 -> f32 labels on {kern}", lab, X["labf"])
    poison(shape)
    poison(shape, dtype=torch.uint8)
    out, lab = K.warp(spec, mm6, src_lin=src["img_v"], src_nn=src["lab8_v"])
    image(out, "img", "u8 -> u8 (views)")
    assert same(lab, X["lab8"]), explain(f"{what} u8 -> u8 labels on {kern}", lab, X["lab8"])
    rc, out, lab = lean_probe(K, spec, mm6, src["img"], src["lab8_v"])
    assert rc == (0 if kern == "lean" else _lib.E_ALIGN), f"{what}: the lean kernel {'declined' if rc else 'accepted'}, table: {kern}"
    if rc:  # the caller's fallback (kernels.warp): the float32 copy of the labels through fsg_warp_f32
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(lab).all()), f"{what}: a declined launch wrote"
        poison(shape, shape)
        out, lab = K.warp(spec, mm6, src_lin=src["img"], src_nn=src["lab8_v"], nn_out=torch.float32)
    image(out, "img", "u8 -> f32")
    assert same(lab, X["lab8f"]), explain(f"{what} u8 -> f32 labels on {kern}", lab, X["lab8f"])
    poison(shape)
    out, none = K.warp(spec, mm6, src_lin=src["signs"])
    assert none is None
    image(out, "signs", "image only")
    poison(shape, dtype=torch.uint8)
    none, lab = K.warp(spec, mm6, src_nn=src["lab8"])
    assert none is None and same(lab, X["lab8"]), explain(f"{what} labels only on {kern}", lab, X["lab8"])


def check_epilogue(K, R, spec, mm6, flip, what, flags, rows, precise_seen):
    """(e) on the path that is set."""
    from fetalsyngen_amd import _lib

    precise = bool(flags & _lib.TUNE.PRECISE_MATH)
    combos = [("pos", True, False), ("img", True, False)]
    if R.bias is not None:
        combos += [("pos", False, True), ("pos", True, True), ("img", False, True)]
    for name, g, b in combos:
        ref, tol, zero = R.epilogue(flip, name, g, b)
        poison(spec.shape)
        out, _ = K.warp(spec, mm6, src_lin=R.src[name], gamma=GAMMA if g else None, bias=R.bias if b else None,
                        bias_tabs=R.bt if b else None)
        label = f"{what} {name} gamma={g} bias={b}"
        nan = torch.isnan(ref)
        assert bool((torch.isnan(out) == nan).all()), f"{label}: NaN where the reference has none, or the reverse"
        ratio = torch.where(nan, torch.zeros_like(ref), (out.double() - ref).abs() / tol)
        worst = float(ratio.max())
        assert worst <= 1.0, f"{label}: error {worst:.3f} of the tolerance"
        assert bool((out[zero] == 0).all()), f"{label}: an output whose plain value is 0 is not 0"
        RATIO["precise" if precise else "fast"] = max(RATIO["precise" if precise else "fast"], worst)
        if precise:
            # bit for bit among the lean launches and among the others; between the two the sign of a zero may differ, (d)
            lean = warp_kernel(R.case, flags, _lib.TUNE, rows, b) == "lean"
            first = precise_seen.setdefault((flip, name, g, b, lean), (out, label))
            assert same(out, first[0]), explain(f"{label} against [{first[1]}]", out, first[0])
            other = precise_seen.get((flip, name, g, b, not lean))
            if other is not None:
                assert bool(((out == other[0]) | (torch.isnan(out) & torch.isnan(other[0]))).all()), f"{label} against [{other[1]}]"


def check_dual(K, R, spec, mm6, flip, what, flags, rows):
    """(f) on the path that is set."""
    from fetalsyngen_amd import _lib

    case, X, src = R.case, R.flip[flip], R.src
    b = R.bias is not None
    kern = warp_kernel(case, flags, _lib.TUNE, rows, b)
    epi = dict(gamma=GAMMA, bias=R.bias, bias_tabs=R.bt)
    poison(spec.shape, spec.shape)
    poison(spec.shape, dtype=torch.uint8)
    want_lin, want_nn = K.warp(spec, mm6, src_lin=src["pos"], src_nn=src["lab8"], **epi)
    poison(spec.shape, spec.shape)
    poison(spec.shape, dtype=torch.uint8)
    out, lab, img = K.warp(spec, mm6, src_lin=src["pos"], src_nn=src["lab8"], src_img=src["img"], **epi)
    # outside the lean domain out_img is a launch of its own, without the bias: that one may be the lean kernel's
    kimg = kern if kern == "lean" else warp_kernel(case, flags, _lib.TUNE, rows, False)
    want = X["img", "lean" if kimg == "lean" else "clamp"]
    assert same(img, want), explain(f"{what} out_img on {kimg}", img, want)
    assert bool((img == X["img", "clamp"]).all())
    assert same(out, want_lin), explain(f"{what} out_lin beside src_img", out, want_lin)
    assert same(lab, want_nn) and same(lab, X["lab8"]), explain(f"{what} out_nn beside src_img", lab, X["lab8"])
    if not rows:  # the entry point itself declines exactly when the lean kernel does
        return
    d = K._epilogue(GAMMA, R.bias, R.bt, spec.shape)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    o1, o2 = torch.empty_like(out), torch.empty_like(img)
    rc = _lib.load().fsg_warp_dual_f32(C.byref(spec.c), P(mm6), P(src["pos"]), P(o1), P(src["img"]), P(o2), img.numel(), None, None,
                                      _lib.LABEL_F32, _lib.LABEL_F32, C.byref(d), K._stream(mm6))
    assert rc == (0 if kern == "lean" else _lib.E_ALIGN), f"{what} fsg_warp_dual_f32: rc {rc}, table: {kern}"
    if rc == 0:
        assert same(o2, want) and same(o1, want_lin), f"{what} fsg_warp_dual_f32 without labels"


@pytest.mark.parametrize("group", GROUPS)
def test_paths(K, group):
    """(a) .. (f) (module docstring) for every case of the group on every path, with and without flip."""
    from fetalsyngen_amd import _lib

    T = _lib.TUNE
    for case in cases(group):
        R = Ref(K, case)
        check_rows_direct(K, R)
        precise_seen = {}
        assert warp_kernel(case, 0, T, True, True) == case.kernel
        for pname, flags, rows in paths():
            with tuning(flags):
                for flip in (False, True):
                    what = f"{case.name}{' flipped' if flip else ''} [{pname}]"
                    spec = make_spec(K, case, flip, rows, R.bias, R.bt)
                    if flip:  # the positions do not depend on the flip: (a) .. (c) once per path
                        mm6 = K.coords_minmax(spec)
                        assert torch.equal(mm6, R.dkeys), what
                    else:
                        mm6 = check_setup(K, R, spec, what, flags)
                        check_rows(K, R, spec, what)
                    check_warp(K, R, spec, mm6, flip, what, flags, rows)
                    check_epilogue(K, R, spec, mm6, flip, what, flags, rows, precise_seen)
                    if not flags & (T.NO_PATCH | T.GENERIC_WARP):
                        check_dual(K, R, spec, mm6, flip, what, flags, rows)
        torch.cuda.synchronize()
    print(f"EDGE warp epilogue [{group}]: largest error {RATIO['fast']:.4f} of the tolerance on the fast paths, "
          f"{RATIO['precise']:.4f} on the PRECISE_MATH paths (running maxima over the groups so far)")


def test_interp3d(K):
    """(g): interp_kernel in both modes against linear32 / nearest at hand-placed coordinates: exactly 0 (outside by the strict > 0
    rule: the default value), exactly n - 1 (inside), beyond either end, on ties (half to even), generic ones; default_value 7.5."""
    shape = (5, 4, 7)
    rs = np.random.RandomState(4)
    src = (rs.randn(*shape) * 50).astype(F)
    src[rs.rand(*shape) < 0.2] = -0.0
    per_axis = [np.array([0.0, -0.0, n - 1, -1.5, n - 0.5, n + 3, 0.5, 1.5, 2.5, n - 1.5, 1.25, 2.0, 1e-30, n - 1 - 1e-4], F) for n in shape]
    g = np.meshgrid(*per_axis, indexing="ij")
    co = [np.ascontiguousarray(a.ravel()) for a in g]
    sd, cd = dev(src), [dev(a) for a in co]
    DEFAULT = 7.5
    ok = np.all([(c > 0) & (c <= n - 1) for c, n in zip(co, shape)], axis=0)
    lin = W.linear32(src, [np.clip(c, 0, n - 1) for c, n in zip(co, shape)], False)
    want = np.where(ok, lin, F(DEFAULT))
    assert ok.any() and (~ok).any()
    poison((len(co[0]),))
    got = K.interp3d(sd, *cd, "linear", default_value=DEFAULT)
    assert same(got, dev(want)), explain("interp3d linear", got, dev(want))
    poison((len(co[0]),))
    got0 = K.interp3d(sd, *cd, "linear")
    assert same(got0, dev(np.where(ok, lin, F(0)))), explain("interp3d linear, default 0", got0, dev(np.where(ok, lin, F(0))))
    poison((len(co[0]),))
    got = K.interp3d(sd, *cd, "nearest", default_value=DEFAULT)  # nearest clamps the index: no default
    wantn = dev(W.nearest(src, co, False))
    assert same(got, wantn), explain("interp3d nearest", got, wantn)
    # a grid-stride loop: more points than 8192 blocks of 256 threads cover at once
    n = 8192 * 256 + 77
    big = [rs.rand(n).astype(F) * (s + 1) - 0.5 for s in shape]
    okb = np.all([(c > 0) & (c <= s - 1) for c, s in zip(big, shape)], axis=0)
    wantb = np.where(okb, W.linear32(src, [np.clip(c, 0, s - 1) for c, s in zip(big, shape)], False), F(DEFAULT))
    poison((n,))
    gotb = K.interp3d(sd, *[dev(c) for c in big], "linear", default_value=DEFAULT)
    assert same(gotb, dev(wantb)), explain("interp3d linear, grid-stride", gotb, dev(wantb))


def test_bad_arguments(K):
    """The return codes of launch_warp (fsg_warp_f32, fsg_warp_f32_u8), fsg_warp_f32_u8_to_f32, fsg_warp_dual_f32,
    fsg_deform_rows_f32 and fsg_interp3d_f32 that are reached before any launch: the poisoned outputs stay as they were.  Each
    entry point's unchanged argument list is accepted first, so that a refusal is the changed argument's.  One call is no
    refusal: fsg_warp_f32_u8_to_f32 with src_lin == out_lin launches (the other entry points refuse it), on scratch buffers."""
    from fetalsyngen_amd import _lib
    from tests.util_warp_cases import cases as table

    lib, st = _lib.load(), K._stream(None)
    BAD, BIG, ALIGN = _lib.E_BADARG, _lib.E_TOOBIG, _lib.E_ALIGN
    assert len({0, BAD, BIG, ALIGN}) == 4
    case = table("x, y extent")[3]  # (7, 3, 33), a field and a bias
    R = Ref(K, case)
    spec = make_spec(K, case, False, True, R.bias, R.bt)
    mm6 = K.coords_minmax(spec)
    shape = spec.shape
    n = int(np.prod(shape))
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    N = C.c_void_p(0)
    nan = lambda dt=torch.float32: torch.full(shape, float("nan") if dt == torch.float32 else 255, dtype=dt, device=DEV)  # noqa: E731
    o_lin, o_nn, o_nn8, o_img = nan(), nan(), nan(torch.uint8), nan()
    outs = (o_lin, o_nn, o_nn8, o_img)
    epi = K._epilogue(GAMMA, R.bias, R.bt, shape)
    bad_epi = K._epilogue(GAMMA, R.bias, R.bt, shape)
    bad_epi.bz = None
    neg_epi = K._epilogue(GAMMA, R.bias, R.bt, shape)
    neg_epi.bias_dims[2] = 0
    src = R.src
    D, E = C.byref(spec.c), C.byref(epi)
    warp = {
        "fsg_warp_f32": dict(d=D, mm=P(mm6), src_lin=P(src["img"]), out_lin=P(o_lin), src_nn=P(src["labf"]), out_nn=P(o_nn), epi=E),
        "fsg_warp_f32_u8": dict(d=D, mm=P(mm6), src_lin=P(src["img"]), out_lin=P(o_lin), src_nn=P(src["lab8"]), out_nn=P(o_nn8), epi=E),
        "fsg_warp_f32_u8_to_f32": dict(d=D, mm=P(mm6), src_lin=P(src["img"]), out_lin=P(o_lin), src_nn=P(src["lab8"]), out_nn=P(o_nn),
                                       epi=E),
    }
    dual = dict(d=D, mm=P(mm6), src_lin=P(src["pos"]), out_lin=P(o_lin), src_img=P(src["img"]), out_img=P(o_img), img_voxels=n,
                src_nn=P(src["lab8"]), out_nn=P(o_nn8), din=_lib.LABEL_U8, dout=_lib.LABEL_U8, epi=E)
    for fn, good in list(warp.items()) + [("fsg_warp_dual_f32", dual)]:
        assert getattr(lib, fn)(*good.values(), st) == 0, fn
    torch.cuda.synchronize()
    for t in outs:
        t.fill_(float("nan") if t.dtype == torch.float32 else 255)

    def shaped(**kw):
        """A copy of the deformation with fields changed."""
        d = _lib.Deform.from_buffer_copy(spec.c)
        for k, v in kw.items():
            if isinstance(v, (list, tuple)):
                getattr(d, k)[:] = v
            else:
                setattr(d, k, v)
        return d

    keep = []  # the changed structures stay alive until the calls have returned
    ncalls = 0

    def refused(fn, good, code, **change):
        nonlocal ncalls
        a = dict(good)
        a.update(change)
        assert getattr(lib, fn)(*a.values(), st) == code, (fn, list(change), code)
        ncalls += 1

    def deform_changes():
        out = [(BAD, dict(shape=[0, 3, 33])), (BAD, dict(shape=[7, -1, 33])), (BAD, dict(shape=[7, 3, 0])),
               (BIG, dict(shape=[2048, 2048, 513])), (BAD, dict(field=None)), (BAD, dict(tz=None)),
               (BAD, dict(row_stride=3 * case.spec.field.shape[2] - 1)), (None, dict(row_stride=rows_need(case) - 1))]
        res = []
        for code, kw in out:
            d = shaped(**kw)
            keep.append(d)
            res.append((code, C.byref(d)))
        return res  # None: a workspace that lacks the bias values: FSG_E_BADARG, or FSG_E_ALIGN where only the lean kernel looks

    for fn, good in warp.items():
        refused(fn, good, BAD, d=None)
        refused(fn, good, BAD, mm=N)
        refused(fn, good, BAD, src_lin=N)            # an output without its source
        refused(fn, good, BAD, out_lin=N)            # a source without its output
        refused(fn, good, BAD, src_nn=N)
        refused(fn, good, BAD, out_nn=N)
        refused(fn, good, BAD, src_lin=N, out_lin=N, src_nn=N, out_nn=N)  # nothing to do
        refused(fn, good, BAD, epi=C.byref(bad_epi))  # a bias grid without its tables
        refused(fn, good, BAD, epi=C.byref(neg_epi))  # a bias grid of extent 0
        for code, d in deform_changes():
            refused(fn, good, (ALIGN if fn == "fsg_warp_f32_u8_to_f32" else BAD) if code is None else code, d=d)
    for fn in ("fsg_warp_f32", "fsg_warp_f32_u8"):
        refused(fn, warp[fn], BAD, out_lin=warp[fn]["src_lin"])  # in place
    # ... which fsg_warp_f32_u8_to_f32 alone does not check (nor row_stride against the bias values, above): it launches.  Pinned so
    # that the three entry points' shared operand checks keep the difference; on a scratch copy, whose contents are then anyone's.
    scratch, scratch_nn = src["img"].clone(), torch.empty_like(o_nn)
    in_place = dict(warp["fsg_warp_f32_u8_to_f32"], src_lin=P(scratch), out_lin=P(scratch), out_nn=P(scratch_nn))
    assert lib.fsg_warp_f32_u8_to_f32(*in_place.values(), st) == 0
    # the u8 -> f32 entry is served by the lean kernel alone: FSG_E_ALIGN, nothing launched, under every flag that leaves it
    for flag in (_lib.TUNE.NO_LEAN, _lib.TUNE.NO_PATCH, _lib.TUNE.GENERIC_WARP):
        with tuning(flag):
            refused("fsg_warp_f32_u8_to_f32", warp["fsg_warp_f32_u8_to_f32"], ALIGN)
            refused("fsg_warp_dual_f32", dual, ALIGN)
    refused("fsg_warp_dual_f32", dual, BAD, d=None)
    refused("fsg_warp_dual_f32", dual, BAD, mm=N)
    refused("fsg_warp_dual_f32", dual, BAD, src_lin=N)
    refused("fsg_warp_dual_f32", dual, BAD, out_lin=N)
    # no trilinear source at all: the entry point's own check (the pair checks above answer for half a pair; without src_img the
    # lean launcher's "src_img needs src_lin" cannot answer in its place), then nothing to do at all
    refused("fsg_warp_dual_f32", dual, BAD, src_lin=N, out_lin=N, src_img=N, out_img=N)
    refused("fsg_warp_dual_f32", dual, BAD, src_lin=N, out_lin=N, src_img=N, out_img=N, src_nn=N, out_nn=N)
    refused("fsg_warp_dual_f32", dual, BAD, out_lin=dual["src_lin"])
    refused("fsg_warp_dual_f32", dual, BAD, src_img=N)
    refused("fsg_warp_dual_f32", dual, BAD, out_img=N)
    refused("fsg_warp_dual_f32", dual, BAD, img_voxels=n - 1)
    refused("fsg_warp_dual_f32", dual, BAD, out_img=dual["src_img"])
    refused("fsg_warp_dual_f32", dual, BAD, out_img=dual["src_lin"])
    refused("fsg_warp_dual_f32", dual, BAD, out_img=dual["out_lin"])
    refused("fsg_warp_dual_f32", dual, BAD, out_lin=dual["src_img"])
    refused("fsg_warp_dual_f32", dual, BAD, src_nn=N)
    refused("fsg_warp_dual_f32", dual, BAD, out_nn=N)
    refused("fsg_warp_dual_f32", dual, BAD, din=7)
    refused("fsg_warp_dual_f32", dual, BAD, dout=7)
    refused("fsg_warp_dual_f32", dual, BAD, din=_lib.LABEL_F32, dout=_lib.LABEL_U8)  # float32 labels stay float32
    refused("fsg_warp_dual_f32", dual, BAD, epi=C.byref(bad_epi))
    for code, d in deform_changes():
        refused("fsg_warp_dual_f32", dual, BAD if code is None else code, d=d)
    # fsg_deform_rows_f32
    need = rows_need(case)
    rows = torch.full((shape[0] * shape[1] * need,), float("nan"), device=DEV)
    plain = make_spec(K, case, False, False)
    rgood = dict(d=C.byref(plain.c), epi=E, rows=P(rows), stride=need)
    assert lib.fsg_deform_rows_f32(*rgood.values(), st) == 0
    torch.cuda.synchronize()
    rows.fill_(float("nan"))
    refused("fsg_deform_rows_f32", rgood, BAD, d=None)
    refused("fsg_deform_rows_f32", rgood, BAD, rows=N)
    refused("fsg_deform_rows_f32", rgood, BAD, stride=need - 1)
    refused("fsg_deform_rows_f32", rgood, BAD, stride=0)
    refused("fsg_deform_rows_f32", rgood, BAD, epi=C.byref(bad_epi))
    big = shaped(shape=[65536, 1, 2], rows=None, row_stride=0)
    refused("fsg_deform_rows_f32", rgood, BIG, d=C.byref(big))
    nofield = make_spec(K, table("generic")[1], False, False)  # no field, no bias: nothing to compute, accepted, nothing written
    assert lib.fsg_deform_rows_f32(C.byref(nofield.c), None, P(rows), 0, st) == 0
    # fsg_interp3d_f32
    pts = torch.zeros(4, device=DEV)
    dst = torch.full((4,), float("nan"), device=DEV)
    igood = dict(src=P(src["img"]), sx=shape[0], sy=shape[1], sz=shape[2], ii=P(pts), jj=P(pts), kk=P(pts), npts=4, mode=0,
                 defval=1.0, dst=P(dst))
    assert lib.fsg_interp3d_f32(*igood.values(), st) == 0
    torch.cuda.synchronize()
    dst.fill_(float("nan"))
    for k in ("src", "ii", "jj", "kk", "dst"):
        refused("fsg_interp3d_f32", igood, BAD, **{k: N})
    for k in ("sx", "sy", "sz"):
        for v in (0, -1):
            refused("fsg_interp3d_f32", igood, BAD, **{k: v})
    for v in (-1, 2):
        refused("fsg_interp3d_f32", igood, BAD, mode=v)
    refused("fsg_interp3d_f32", igood, BIG, sx=2048, sy=2048, sz=513)
    assert lib.fsg_interp3d_f32(*dict(igood, npts=0).values(), st) == 0  # no points: accepted, nothing launched
    torch.cuda.synchronize()
    for t in outs + (rows, dst):
        assert bool((torch.isnan(t) if t.dtype == torch.float32 else t == 255).all()), "a refused call wrote to an output"
    assert ncalls == 3 * 17 + 2 + 6 + 20 + 8 + 6 + 14
