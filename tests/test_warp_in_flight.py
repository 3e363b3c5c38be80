"""GPU: the lean fused warp (csrc/fsg_warp_lean.hip) with the next step's gathers in flight across the blend, at the shapes
where its loop -- two steps per trip, the last one or two steps of a row as straight-line code after it -- and its workgroup
shape (8 x 4 rows, 32 voxels of each per step) can go wrong.

References, both computed by kernels this loop is no part of:
  * without epilogue: the materialised path -- coords_kernel writes the three coordinate volumes, interp_kernel samples the
    (flipped) sources at them -- bit for bit in value, for the image (trilinear) and the labels (nearest).  (Where a coordinate
    lies exactly on the last plane, row or column the lean kernel multiplies another finite neighbour by its zero weight than
    interp_kernel does, so the SIGN of a zero may differ there: tests/test_warp_kernels_edges.py (d).  Values are compared.)
  * with the gamma / bias epilogue: the patch kernel (fsg_set_tuning NO_LEAN), which tests/test_hip_parity.py holds bit for bit
    to the lean kernel.
Every label form (u8 -> f32, u8 -> u8, f32 -> f32), the image-only and label-only launches and the dual-source form are
compared in every case; fsg_warp_f32_u8_to_f32, which only the lean kernel serves, must accept (return 0), so no case passes
on a fallback.  Every barrier period (fsg_warp_set_variant 5, 6, 7) must reproduce the default.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (and libfsg_hip.so); there is no fallback to skip to")
    from fetalsyngen_amd import kernels

    return kernels


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def affine(rot, scale=(1.05, 0.95, 1.02)):
    from fetalsyngen_amd.utils.generation import make_affine_matrix

    return make_affine_matrix([rot, -rot, rot], [0.01, -0.02, 0.015], list(scale)).astype(F)


def run_case(K, shape, A, *, flip, fdim=None, bdim=None, gamma=None, shift=0.3, amp=2.0, seed=0, paces=False):
    """One deformation on `shape`: every launch form of the lean kernel against the references of the module docstring.
    Returns the six min/max keys as floats."""
    from fetalsyngen_amd import _lib
    from fetalsyngen_amd import tables as T

    lib = _lib.load()
    rs = np.random.RandomState(seed)
    n = int(np.prod(shape))
    img = (rs.rand(*shape) * 255).astype(F)
    img2 = (rs.rand(*shape) * 100).astype(F)
    lab = rs.randint(0, 8, shape).astype(np.uint8)
    c = (np.array(shape) - 1) / 2
    fs = ft = bias = bt = None
    if fdim is not None:
        fs = dev((rs.randn(*fdim, 3) * amp).astype(F))
        ft = K.DeviceTables(T.zoom_tables(fdim, np.array(shape) / np.array(fdim))[0], DEV)
    if bdim is not None:
        bias = dev((rs.randn(*bdim) * 0.3).astype(F))
        bt = K.DeviceTables(T.zoom_tables(bdim, np.array(shape) / np.array(bdim))[0], DEV)
    what = f"shape {shape} flip {flip} field {fdim} bias {bdim} gamma {gamma}"

    def make_spec():
        spec = K.DeformSpec(shape, A, c, c.astype(F) + F(shift), flip, fs, ft, device=DEV)
        spec.prepare_rows(bias, bt)
        return spec

    spec = make_spec()
    mm6 = K.coords_minmax(spec)
    d_img, d_img2, d_lab = dev(img), dev(img2), dev(lab)
    d_labf = d_lab.to(torch.float32)

    # the materialised path
    co = K.coords(spec, mm6)
    fl = (lambda t: torch.flip(t, [0]).contiguous()) if flip else (lambda t: t)
    want_img = K.interp3d(fl(d_img), *co, "linear")
    want_img2 = K.interp3d(fl(d_img2), *co, "linear")
    want_lab = K.interp3d(fl(d_labf), *co, "nearest")

    # u8 -> f32, the form of the benchmarked step, through the entry point that only the lean kernel serves
    out = torch.full(shape, float("nan"), device=DEV)
    labf = torch.full(shape, float("nan"), device=DEV)
    epi0 = K._epilogue(None, None, None, shape)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.fsg_warp_f32_u8_to_f32(C.byref(spec.c), P(mm6), P(d_img), P(out), P(d_lab), P(labf), C.byref(epi0), K._stream(mm6))
    assert rc == 0, f"{what}: the lean kernel declined ({rc})"
    assert torch.equal(out, want_img), f"{what}: u8 -> f32 image"
    assert torch.equal(labf, want_lab), f"{what}: u8 -> f32 labels"
    forms = {
        "u8 -> u8": lambda **e: K.warp(spec, mm6, src_lin=d_img, src_nn=d_lab, **e),
        "f32 -> f32": lambda **e: K.warp(spec, mm6, src_lin=d_img, src_nn=d_labf, **e),
        "u8 -> f32": lambda **e: K.warp(spec, mm6, src_lin=d_img, src_nn=d_lab, nn_out=torch.float32, **e),
        "image only": lambda **e: K.warp(spec, mm6, src_lin=d_img, **e),
        "labels only": lambda **e: K.warp(spec, mm6, src_nn=d_lab),
        "dual": lambda **e: K.warp(spec, mm6, src_lin=d_img, src_nn=d_lab, src_img=d_img2, **e),
    }
    plain = {}
    for name, fn in forms.items():
        got = fn()
        plain[name] = got
        if got[0] is not None:
            assert torch.equal(got[0], want_img), f"{what}: {name} image"
        if got[1] is not None:
            assert torch.equal(got[1].to(torch.float32), want_lab), f"{what}: {name} labels"
        if name == "dual":
            assert torch.equal(got[2], want_img2), f"{what}: second source"

    # the epilogue against the patch kernel
    epis = [e for e in (dict(gamma=gamma) if gamma else None, dict(bias=bias, bias_tabs=bt) if bias is not None else None,
                        dict(gamma=gamma, bias=bias, bias_tabs=bt) if gamma and bias is not None else None) if e]
    for e in epis:
        got = {name: fn(**e) for name, fn in forms.items() if name != "labels only"}
        prev = lib.fsg_set_tuning(_lib.TUNE.NO_LEAN)
        try:
            spec_p = make_spec()
            want, want_l = K.warp(spec_p, mm6, src_lin=d_img, src_nn=d_labf, **e)
        finally:
            lib.fsg_set_tuning(prev)
        assert torch.equal(want_l, want_lab), f"{what}: patch kernel labels"
        for name, g in got.items():
            assert torch.equal(g[0], want), f"{what}: {name} image with {sorted(e)}"
            if g[1] is not None:
                assert torch.equal(g[1].to(torch.float32), want_lab), f"{what}: {name} labels with {sorted(e)}"
            if name == "dual":
                assert torch.equal(g[2], want_img2), f"{what}: second source beside {sorted(e)}"

    if paces:  # the barrier period changes nothing
        e = epis[-1] if epis else {}
        base = forms["u8 -> f32"](**e)
        based = forms["dual"](**e)
        prev = lib.fsg_warp_set_variant(0)
        try:
            for v in (5, 6, 7):
                lib.fsg_warp_set_variant(v)
                got, gotd = forms["u8 -> f32"](**e), forms["dual"](**e)
                assert all(torch.equal(a, b) for a, b in zip(got, base)), f"{what}: variant {v}"
                assert all(torch.equal(a, b) for a, b in zip(gotd, based)), f"{what}: variant {v}, dual"
        finally:
            lib.fsg_warp_set_variant(prev)
    torch.cuda.synchronize()
    assert n == out.numel()
    return [K.key_to_float(k) for k in mm6.cpu().tolist()]


@pytest.mark.parametrize("n2", [2, 31, 32, 33, 64, 65, 96, 97, 128, 130])
def test_steps_per_row(K, n2):
    """1 .. 5 steps of 32 voxels per row: every remainder of the step count modulo 2 and modulo 3, a row that ends inside the
    loop's trip and one that ends in the straight-line tail, a last step with 1, 2 or 31 live lanes, a row shorter than a step."""
    for flip in (False, True):
        run_case(K, (9, 5, n2), affine(0.2), flip=flip, fdim=(3, 2, max(2, n2 // 16)), bdim=(2, 2, 3), gamma=1.13, seed=n2,
                 paces=not flip)


@pytest.mark.parametrize("n0", [1, 7, 8, 9])
def test_workgroup_coverage(K, n0):
    """Rows past the volume in the last tile: 8 planes x 4 rows per workgroup, so n0 = 1, 7, 9 and n1 = 1, 3, 5, 9 leave waves
    and half-waves without a row; n2 = 33 ends every row with a step of one live lane."""
    for n1 in (1, 3, 4, 5, 9):
        run_case(K, (n0, n1, 33), affine(0.15), flip=bool((n0 + n1) & 1), fdim=(2, 2, 3), bdim=(2, 2, 2), gamma=0.9,
                 seed=10 * n0 + n1)


@pytest.mark.parametrize("fz,bz", [(2, None), (32, None), (None, 2), (None, 32), (2, 32), (32, 2), (5, 3)])
def test_sources(K, fz, bz):
    """Field only, bias only and both, with coarse z extents 2 and 32 (the ends of the LDS rows the kernel stages them in),
    flip on and off, gamma on and off."""
    for flip in (False, True):
        for gamma in (None, 1.2):
            run_case(K, (9, 6, 70), affine(0.25), flip=flip, fdim=None if fz is None else (3, 2, fz),
                     bdim=None if bz is None else (2, 3, bz), gamma=gamma, seed=3)


def test_edge_positions(K):
    """Identity affine, no field, no shift: every sample sits exactly on a voxel, the last plane, row and column included (and
    plane, row and column 0 are outside by the strict > 0 rule).  Then a draw (small rotation, a field, a shift of 6 voxels) whose
    smallest position is above 1 on every axis, so that the margins floor(min) are not zero."""
    eye = np.eye(3, dtype=F)
    for shape in ((9, 5, 33), (8, 4, 64), (3, 9, 97)):
        for flip in (False, True):
            keys = run_case(K, shape, eye, flip=flip, gamma=1.1, shift=0.0, paces=True)
            assert keys[:3] == [0.0, 0.0, 0.0] and keys[3:] == [float(s - 1) for s in shape]
    nonzero = 0
    for flip in (False, True):
        keys = run_case(K, (12, 9, 65), affine(0.05), flip=flip, fdim=(3, 3, 4), bdim=(2, 2, 2), gamma=0.8, shift=6.0, amp=0.5,
                        seed=7, paces=True)
        nonzero += sum(int(np.floor(k)) != 0 for k in keys[:3])
    assert nonzero, "the draw was meant to have non-zero margins"
