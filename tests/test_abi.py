"""CPU: the C-ABI library loads and exports every symbol include/fsg_hip.h declares; the binding that fetalsyngen_amd/_lib.py
derives from that header is the compiler's reading of it; argument validation happens before any launch (no GPU needed for
these calls)."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest

from fetalsyngen_amd import _lib

REPO = Path(__file__).resolve().parent.parent


def header_symbols():
    text = (REPO / "include" / "fsg_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fsg_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    syms = header_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/fsg_hip.h but not exported"
    bound = set(_lib.PROTOTYPES)  # header_symbols() is a scan of its own: a prototype the parser drops or invents shows here
    assert set(syms) == bound, f"parsed prototypes and header disagree: {set(syms) ^ bound}"


def test_version_and_error_strings():
    lib = _lib.load()
    assert lib.fsg_abi_version() == _lib.ABI_VERSION
    assert b"bad argument" in lib.fsg_error_string(-1)
    assert lib.fsg_error_string(0) == b"success"


def test_key_roundtrip_orders_floats():
    lib = _lib.load()
    import numpy as np

    vals = np.array([-np.inf, -3.5, -0.0, 0.0, 1e-30, 2.0, 255.0, np.inf], dtype=np.float32)
    bits = vals.view(np.int32)
    keys = np.where(bits >= 0, bits, bits ^ 0x7FFFFFFF)
    assert (np.diff(keys.astype(np.int64)) > 0).all()
    for v, k in zip(vals, keys):
        assert lib.fsg_key_to_float(int(k)) == v


def test_bad_arguments_are_rejected_before_launch():
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    assert lib.fsg_randn_f32(null, 16, 0, 0, null) == _lib.E_BADARG
    assert lib.fsg_gamma_f32(null, 16, 1.0, null, null) == _lib.E_BADARG
    assert lib.fsg_blur_axis_f32(null, null, 4, 4, 4, 0, null, 3, null) == _lib.E_BADARG
    one = ctypes.c_void_p(16)
    two = ctypes.c_void_p(32)
    assert lib.fsg_blur_axis_f32(one, two, 4, 4, 4, 3, one, 3, null) == _lib.E_BADARG  # axis
    assert lib.fsg_blur_axis_f32(one, two, 4, 4, 4, 0, one, 4, null) == _lib.E_BADARG  # even taps
    assert lib.fsg_blur_axis_f32(one, one, 4, 4, 4, 0, one, 3, null) == _lib.E_BADARG  # in place
    assert lib.fsg_zoom3d_f32(one, 0, 4, 4, 1, one, one, one, two, 4, 4, 4, null) == _lib.E_BADARG
    assert lib.fsg_interp3d_f32(one, 4, 4, 4, one, one, one, 8, 2, 0.0, two, null) == _lib.E_BADARG  # mode
    d = _lib.Deform()
    assert lib.fsg_coords_minmax_f32(ctypes.byref(d), one, null) == _lib.E_BADARG  # zero shape
    d.shape[:] = [2048, 2048, 2048]
    assert lib.fsg_coords_minmax_f32(ctypes.byref(d), one, null) == _lib.E_TOOBIG
    with pytest.raises(_lib.FsgError):
        _lib.check(-1, "x")


def test_product_refuses_cpu_tensors():
    import torch

    from fetalsyngen_amd import kernels as K

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.gamma(torch.zeros(2, 2, 2), 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.blur_axis(torch.zeros(4, 4, 4), 0, [0.25, 0.5, 0.25])


def test_sample_plan_mirror_has_the_c_layout():
    """The ctypes mirror of fsg_sample_plan against the compiled struct: total size and the offsets of a field behind the
    large tap array, of the last r01 field, and of the two newest ones (a mirror that drifts would hand every later
    pointer to the wrong slot)."""
    import ctypes as C

    from fetalsyngen_amd import _lib

    lib = _lib.load()
    P = _lib.SamplePlan
    assert lib.fsg_sample_plan_layout(0) == C.sizeof(P)
    assert lib.fsg_sample_plan_layout(1) == P.blur_taps.offset
    assert lib.fsg_sample_plan_layout(2) == P.out.offset
    assert lib.fsg_sample_plan_layout(3) == P.seg_in_u8.offset
    assert lib.fsg_sample_plan_layout(4) == P.ws_seq.offset
    assert lib.fsg_sample_plan_layout(5) == P.code_sel.offset
    assert lib.fsg_sample_plan_layout(6) == C.sizeof(_lib.Tap)
    assert lib.fsg_sample_plan_layout(7) == C.sizeof(_lib.Deform)
    assert lib.fsg_sample_plan_layout(8) == C.sizeof(_lib.Epilogue)
    assert lib.fsg_sample_plan_layout(9) == C.sizeof(_lib.KeyedConfig)
    assert lib.fsg_sample_plan_layout(10) == C.sizeof(_lib.KeyedDraws)
    assert lib.fsg_sample_plan_layout(11) == -1
    assert lib.fsg_sample_plan_layout(99) == -1


def _header_without_comments():
    return re.sub(r"/\*.*?\*/", "", (REPO / "include" / "fsg_hip.h").read_text(), flags=re.S)


def test_parsed_header_is_what_the_compiler_sees(tmp_path):
    """The parser against the compiler: a host program that includes the header prints sizeof of every struct, offsetof and
    sizeof of every field and the value of every constant the parser found; each must equal the ctypes mirror.  The number
    of fields per struct is held against a count of declarators made here, so a member the parser loses is seen as well."""
    from fetalsyngen_amd import _build

    try:
        cc = _build.hipcc()
    except RuntimeError:
        pytest.skip("no compiler")
    lines = ["#include <cstdio>", "#include <cstddef>", f'#include "{REPO / "include" / "fsg_hip.h"}"', "int main() {"]
    want = {}
    for cname, cls in _lib.STRUCTS.items():
        lines.append(f'  printf("sizeof {cname} %zu\\n", sizeof({cname}));')
        want[f"sizeof {cname}"] = ctypes.sizeof(cls)
        for fname, ftype in cls._fields_:
            lines.append(f'  printf("field {cname}.{fname} %zu %zu\\n", offsetof({cname}, {fname}), sizeof((({cname}*)0)->{fname}));')
            want[f"field {cname}.{fname}"] = (getattr(cls, fname).offset, ctypes.sizeof(ftype))
    for name, value in _lib.CONSTANTS.items():
        lines.append(f'  printf("const {name} %lld\\n", (long long)(FSG_{name}));')
        want[f"const {name}"] = value
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-x", "c++", "-std=c++17", str(src), "-o", str(exe)], check=True)
    got = {}
    for row in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        kind, name, *nums = row.split()
        got[f"{kind} {name}"] = int(nums[0]) if len(nums) == 1 else tuple(int(v) for v in nums)
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}

    text = _header_without_comments()
    bodies = dict(re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\w+\s*;", text, flags=re.S))
    assert list(bodies) == list(_lib.STRUCTS)
    for cname, body in bodies.items():  # one declarator per ';' plus one per ',' (no member of the header has a ',' elsewhere)
        assert body.count(";") + body.count(",") == len(_lib.STRUCTS[cname]._fields_), cname
    assert len(_lib.CONSTANTS) == len(set(re.findall(r"\bFSG_[A-Z0-9_]+(?=\s*=|\s+[-(\d])", text)))
    assert len(_lib.CONSTANTS) >= 140 and sum(len(c._fields_) for c in _lib.STRUCTS.values()) >= 149


def test_binding_names():
    """Constants are reachable by header name only, grouped by family; every pointer field is c_void_p; prototypes take
    what the call sites pass (struct pointers by reference, every other pointer as address, array or byref)."""
    assert _lib.PLAN_I.COUNT == len(_lib.SamplePlan._fields_) + 14 == 71  # iv slots: the header's own count
    assert (_lib.E_BADARG, _lib.E_TOOBIG, _lib.E_ALIGN, _lib.E_NOTABLE) == (-1, -2, -3, -4)
    assert _lib.KEYED_I.NEXT_BLOCK == 88 and _lib.KEYED_FLAG.BLOCK_FILLED == 1 and _lib.KEYED_FLAG.NEXT_NAMED == 4
    assert _lib.STAGE_NAMES[:3] == ("begin", "upload", "draw") and len(_lib.STAGE_NAMES) == _lib.ST.COUNT
    for missing in ("NOPE", "count"):
        with pytest.raises(AttributeError):
            getattr(_lib.PLAN_I, missing)
    with pytest.raises(AttributeError):
        _lib.TUNE_NO_SUCH_FLAG
    assert _lib.SamplePlan.deform.size == ctypes.sizeof(_lib.Deform) and _lib.SamplePlan.epi.size == ctypes.sizeof(_lib.Epilogue)
    assert ctypes.sizeof(_lib.SamplePlan().blur_taps) == 3 * 129 * 4 and len(_lib.SamplePlan().blur_taps[2]) == 129
    assert ctypes.sizeof(_lib.SamplePlan().label_parts) == 4 * ctypes.sizeof(ctypes.c_void_p)
    for cls in _lib.STRUCTS.values():
        for fname, ftype in cls._fields_:
            assert not issubclass(ftype, ctypes._Pointer), (cls, fname)
    res, args = _lib.PROTOTYPES["fsg_sample_head_codes_f32"]
    assert res is ctypes.c_int and args[4] is ctypes.c_void_p and args[12] is ctypes.POINTER(_lib.Deform)  # sel[4], d
    assert _lib.PROTOTYPES["fsg_deform_rows_f32"][1][1] is ctypes.POINTER(_lib.Epilogue)  # declared before the struct is defined
    assert _lib.PROTOTYPES["fsg_zoom3d_f32"][1][5] is ctypes.c_void_p  # fsg_tap tables are device addresses
    assert _lib.PROTOTYPES["fsg_error_string"] == (ctypes.c_char_p, [ctypes.c_int])
    assert _lib.PROTOTYPES["fsg_event_create"] == (ctypes.c_void_p, [])
    assert _lib.PROTOTYPES["fsg_em1d_work_bytes"] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int64])
    assert _lib.PROTOTYPES["fsg_key_to_float"] == (ctypes.c_float, [ctypes.c_int32])
    lib = _lib.load()
    taps, ms = (ctypes.c_float * 3)(0.25, 0.5, 0.25), ctypes.c_float()
    null = ctypes.c_void_p(0)
    assert lib.fsg_blur_axis_taps_host_f32(null, null, 4, 4, 4, 0, taps, 3, null) == _lib.E_BADARG  # a ctypes array
    assert lib.fsg_blur_axis_taps_host_f32(None, 0, 4, 4, 4, 0, ctypes.cast(taps, ctypes.POINTER(ctypes.c_float)), 3, None) == _lib.E_BADARG
    assert lib.fsg_event_elapsed_ms(null, null, ctypes.byref(ms)) != 0  # byref of a scalar where the header says float*


@pytest.mark.parametrize("snippet, line, what", [
    ("#define FSG_A 1\ntypedef struct fsg_x {\n  int32_t a;\n  wchar_t b;\n} fsg_x;\n", 4, "unknown type 'wchar_t'"),
    ("#define FSG_A 1\n\ntypedef struct fsg_x {\n  int32_t a;\n", 3, "without an end"),
    ("enum {\n  FSG_A = 1,\n  FSG_B = 1.5\n};\n", 3, "not an integer constant"),
    ("enum { FSG_A = 1, FSG_B };\n", 1, "not FSG_NAME = value"),
    ("#define FSG_A sizeof(int)\n", 1, "not an integer constant"),
    ("int fsg_f(int a);\nint fsg_g(int a,\n          FILE* f);\n", 3, "unknown type 'FILE'"),
    ("union fsg_u { int a; float b; };\n", 1, "not recognised"),
    ("typedef int fsg_int;\n", 1, "not recognised"),
    ("#pragma once\n", 1, "not recognised"),
])
def test_parser_refuses_what_it_does_not_know(snippet, line, what):
    with pytest.raises(_lib.HeaderError, match=f"line {line}: .*{re.escape(what)}"):
        _lib.parse(snippet)


def test_no_restated_header_numbers():
    """Keeps the clean-up done: tuning flags and flat-array slots are spelled by their header names."""
    lit = re.compile(r"fsg_set_tuning\(\s*(?!0\s*\))\d")
    for folder in ("fetalsyngen_amd", "tests", "tools"):
        for path in sorted((REPO / folder).rglob("*.py")):
            assert not lit.search(path.read_text()), f"{path}: fsg_set_tuning with a bare number"
    slot = re.compile(r"\b[if]v\[\d")
    for rel in ("fetalsyngen_amd/generator/model.py", "fetalsyngen_amd/keyed.py", "tools/host_phases.py"):
        hits = [ln for ln in (REPO / rel).read_text().splitlines() if slot.search(ln)]
        assert not hits, f"{rel}: {hits[:3]}"
    # the solvers' iteration cap and row widths are the header's: kernels.py binds its names to them and restates no number
    kernels = (REPO / "fetalsyngen_amd" / "kernels.py").read_text().splitlines()
    bare = re.compile(r"\b\w*(MAX_ITER|MAX_EM|SLOTS|ROW)\s*=\s*\d")
    hits = [ln for ln in kernels if bare.search(ln) or ("4096" in ln and "_DT_CACHE" not in ln)]
    assert not hits, f"fetalsyngen_amd/kernels.py: {hits[:3]}"
    # one overlap test and one finite test for every unit
    csrc = "".join(p.read_text() for p in sorted((REPO / "fetalsyngen_amd" / "csrc").iterdir()))
    for name in ("_overlap(", "_finite("):
        defs = re.findall(r"^[\w \t]*\bbool\s+(\w*" + re.escape(name[:-1]) + r")\(", csrc, flags=re.M)
        assert defs == ["fsg" + name[:-1]], f"{name} is defined as {defs}"


def test_solver_constants_are_the_headers():
    from fetalsyngen_amd import kernels as K

    assert (_lib.SOLVER_MAX_ITER, _lib.SVR_SLOTS, _lib.ROBUST_ROW) == (4096, 32, 6)  # the contracts' figures
    assert K.CG_MAX_ITER == K.SVR_MAX_ITER == K.ROBUST_MAX_EM == _lib.SOLVER_MAX_ITER
    assert K.SVR_SLOTS == _lib.SVR_SLOTS and K.ROBUST_ROW == _lib.ROBUST_ROW


# the layout paragraphs of include/fsg_hip.h, field by field in their order: (attribute, dtype name, shape); s = iterations + 1
def _cg_fields(n, k):
    s, b = k + 1, min(max(-(-n // 1024), 1), 1024)
    return [("rr", "float64", (s,)), ("pq", "float64", (s,)), ("partial_rr", "float64", (b,)), ("partial_pq", "float64", (b,)),
            ("alpha", "float32", (s,)), ("beta", "float32", (s,)), ("frozen", "int32", (s,))]


def _svr_fields(n, k):
    s = k + 1
    return [("stats_cur", "float64", (n, 32)), ("lam", "float64", (n,)), ("m0", "float64", (n,)), ("cost", "float64", (s, n)),
            ("lambda_hist", "float64", (s, n)), ("theta_cur", "float32", (n, 6)), ("frozen_now", "int32", (n,)),
            ("accepted", "int32", (s, n)), ("frozen", "int32", (s, n))]


def _robust_fields(n, t):
    s = t + 1
    return [("consts", "float64", (4,)), ("rows", "float64", (n, 6)), ("u", "float64", (n,)), ("sigma", "float64", (s,)),
            ("c", "float64", (s,)), ("mu1", "float64", (s,)), ("mu2", "float64", (s,)), ("ws", "float64", (s, n)),
            ("scal", "float32", (2,)), ("frozen", "int32", (s,))]


@pytest.mark.parametrize("make,fields,n,k", [("cg_workspace", _cg_fields, 2049, 4), ("svr_state", _svr_fields, 5, 3),
                                             ("robust_state", _robust_fields, 3, 4)])
def test_state_views_tile_the_block_in_the_headers_order(make, fields, n, k):
    """on the host (the classes take device="cpu"): the views follow one another from byte 0 of `buf` with no gap and no
    overlap, and end within the rounding to 8 of the size the library counts"""
    from fetalsyngen_amd import kernels as K

    st = getattr(K, make)(n, k, "cpu")
    off = 0
    for name, dtype, shape in fields(n, k):
        v = getattr(st, name)
        assert (str(v.dtype), tuple(v.shape)) == ("torch." + dtype, shape) and v.is_contiguous(), name
        assert v.data_ptr() - st.buf.data_ptr() == off, name
        off += v.numel() * v.element_size()
    assert -(-off // 8) * 8 == st.nbytes == st.buf.numel() * st.buf.element_size()
