"""ctypes binding of libfsg_hip.so, derived from include/fsg_hip.h when this module is imported.

The header is the one statement of the C ABI: its constants, struct layouts and prototypes are read from it here (`parse`),
so a field, a slot or an entry point added there needs no edit in this file.  The parser covers what that header uses and
refuses, with the line, anything else.

    constants   header name without FSG_: ABI_VERSION, E_ALIGN, MM_SLOT_STRIDE, ...; the families in GROUPS as namespaces:
                PLAN_I.MUS, KEYED_I.NEXT_KEY, TUNE.NO_SEED_CODES, ...  A name the header lacks raises AttributeError.
    structs     fsg_sample_plan -> SamplePlan, ...; every pointer field is c_void_p.
    prototypes  set on the library by load(); a pointer to one of the header's structs is POINTER(that struct), any other
                pointer c_void_p (which takes byref(), ctypes arrays and pointers, integers and None).

There is NO fallback: if the library is missing or does not load, every entry point raises.
"""
from __future__ import annotations

import ast
import ctypes as C
import os
import re
from pathlib import Path
from types import SimpleNamespace

PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("FSG_LIB", PKG / "libfsg_hip.so"))  # FSG_LIB: A/B another build of the same ABI
HEADER_PATH = PKG.parent / "include" / "fsg_hip.h"

GROUPS = ("PLAN_I", "PLAN_F", "KEYED_I", "KEYED_FLAG", "KO", "TUNE", "ST", "KT", "SA", "SIZEOF")
# fsg_tap only ever crosses the boundary as the address of a DEVICE table (tensor.data_ptr()), which POINTER(Tap) would refuse
DEVICE_STRUCTS = ("fsg_tap",)

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
            "char": C.c_char, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong}
# what carries nothing of the ABI: include guard, includes, the extern "C" bracket, forward declarations
_IGNORED = re.compile(r'#\s*(ifndef|ifdef|endif|include)\b.*|#\s*define\s+FSG_HIP_H|extern\s+"C"\s*\{|\}|struct\s+\w+\s*;')


class FsgError(RuntimeError):
    def __init__(self, code: int, where: str, msg: str):
        super().__init__(f"{where}: {msg} (code {code})")
        self.code = code


class HeaderError(RuntimeError):
    def __init__(self, line: int, msg: str):
        super().__init__(f"fsg_hip.h line {line}: {msg}")


def _statements(text):
    """(line, statement) for every preprocessor line and every `;`-terminated statement (braces balanced), comments removed."""
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group().count("\n"), text, flags=re.S)
    bracket = re.compile(r'#[^\n]*|extern\s+"C"\s*\{|\}')
    punct = re.compile(r"[;{}]")
    pos, n = 0, len(text)
    while True:
        while pos < n and text[pos].isspace():
            pos += 1
        if pos == n:
            return
        line = text.count("\n", 0, pos) + 1
        m = bracket.match(text, pos)
        if m:
            end = m.end()
        else:
            depth = 0
            for m in punct.finditer(text, pos):
                if m.group() == ";" and not depth:
                    break
                depth += (m.group() == "{") - (m.group() == "}")
            else:
                raise HeaderError(line, f"statement without an end: {text[pos:pos + 40]!r}")
            end = m.end()
        yield line, text[pos:end]
        pos = end


def _split(text, sep, line):
    """(line, piece) for the pieces of `text` between `sep`; `line` is that of the first character of `text`."""
    pos = 0
    for piece in text.split(sep):
        lead = len(piece) - len(piece.lstrip())
        yield line + text.count("\n", 0, pos + lead), piece.strip()
        pos += len(piece) + len(sep)


def _int(expr, line):
    """Value of an integer literal or a sum / difference / product of them: `3`, `(-1)`, `16 + 70`."""
    def ev(node):
        if isinstance(node, ast.Constant) and type(node.value) is int:
            return node.value
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.USub):
            return -ev(node.operand)
        if isinstance(node, ast.BinOp) and isinstance(node.op, (ast.Add, ast.Sub, ast.Mult)):
            a, b = ev(node.left), ev(node.right)
            return a + b if isinstance(node.op, ast.Add) else a - b if isinstance(node.op, ast.Sub) else a * b
        raise ValueError
    try:
        return ev(ast.parse(expr.strip(), mode="eval").body)
    except (ValueError, SyntaxError):
        raise HeaderError(line, f"not an integer constant: {expr.strip()!r}") from None


def _declarator(text, line, structs, base=None):
    """'const float* const* grads' -> ('float', c_float, 2, 'grads', []); 'float blur_taps[3][129]' -> (.., 0, 'blur_taps', [3, 129]).
    base: the type name when `text` is a later declarator of a member (`uint64_t gmm_seed, gmm_stream`)."""
    m = re.fullmatch(r"([\w\s*]*?)(\w+)\s*((?:\[\d+\])*)", text)
    if not m:
        raise HeaderError(line, f"not a declarator: {text!r}")
    toks = [t for t in m.group(1).replace("*", " * ").split() if t not in ("const", "struct")]
    base = " ".join(t for t in toks if t != "*") or base
    stars = toks.count("*")
    ctype = _SCALARS.get(base) or structs.get(base)
    if ctype is None and not (base == "void" and stars):
        raise HeaderError(line, f"unknown type {base!r} in {text!r}")
    return base, ctype, stars, m.group(2), [int(d) for d in re.findall(r"\d+", m.group(3))]


def _fields(body, line, structs):
    *members, rest = _split(body, ";", line)
    if rest[1]:
        raise HeaderError(rest[0], f"struct member without ';': {rest[1]!r}")
    out = []
    for mline, member in members:
        base = None
        for decl in member.split(","):
            base, ctype, stars, name, dims = _declarator(decl.strip(), mline, structs, base)
            ctype = C.c_void_p if stars else ctype
            for d in reversed(dims):
                ctype = ctype * d
            out.append((name, ctype))
    return out


def _prototype(stmt, line, structs):
    m = re.fullmatch(r"([\w\s*]+?)(\w+)\s*\((.*)\)\s*;", stmt, re.S)
    if not m:
        raise HeaderError(line, f"not recognised: {' '.join(stmt.split())[:60]!r}")
    _, res, stars, name, _ = _declarator(m.group(1) + m.group(2), line, structs)
    if stars:
        res = C.c_char_p if res is C.c_char else C.c_void_p
    args = []
    params = m.group(3)
    for pline, p in [] if params.strip() == "void" else _split(params, ",", line + stmt.count("\n", 0, m.start(3))):
        base, ctype, stars, _, dims = _declarator(p, pline, structs)
        if stars or dims:
            by_struct = stars == 1 and not dims and base in structs and base not in DEVICE_STRUCTS
            ctype = C.POINTER(ctype) if by_struct else C.c_void_p
        args.append(ctype)
    return name, (res, args)


def parse(text):
    """constants {name without FSG_: int}, structs {C name: ctypes.Structure, in header order}, prototypes {name: (restype,
    argtypes)}.  HeaderError for anything that is not a constant, an enum, a struct or a prototype as fsg_hip.h writes them."""
    consts, structs, protos = {}, {}, []
    for line, stmt in _statements(text):
        if _IGNORED.fullmatch(stmt):
            continue
        m = re.fullmatch(r"#\s*define\s+FSG_(\w+)\s+(.*)", stmt)
        if m:
            consts[m.group(1)] = _int(m.group(2), line)
            continue
        m = re.fullmatch(r"enum\s*\{(.*)\}\s*;", stmt, re.S)
        if m:
            for eline, item in _split(m.group(1), ",", line + stmt.count("\n", 0, m.start(1))):
                em = re.fullmatch(r"FSG_(\w+)\s*=(.*)", item, re.S)
                if not em:
                    raise HeaderError(eline, f"not FSG_NAME = value: {item!r}")
                consts[em.group(1)] = _int(em.group(2), eline)
            continue
        m = re.fullmatch(r"typedef\s+struct\s+(fsg_\w+)\s*\{(.*)\}\s*(\w+)\s*;", stmt, re.S)
        if m and m.group(1) == m.group(3):
            fields = _fields(m.group(2), line + stmt.count("\n", 0, m.start(2)), structs)
            name = "".join(w.capitalize() for w in m.group(1).split("_")[1:])  # fsg_sample_plan -> SamplePlan
            structs[m.group(1)] = type(name, (C.Structure,), {"_fields_": fields})
            continue
        if stmt.startswith(("#", "typedef", "enum", "struct")):
            raise HeaderError(line, f"not recognised: {' '.join(stmt.split())[:60]!r}")
        protos.append((line, stmt))  # resolved below: a prototype may name a struct that is defined after it
    return consts, structs, dict(_prototype(stmt, line, structs) for line, stmt in protos)


def _bind(consts):
    """Module-level names and the GROUPS namespaces from the header's constants (longest group prefix wins)."""
    flat, groups = {}, {g: {} for g in GROUPS}
    for name, v in consts.items():
        g = max((g for g in GROUPS if name.startswith(g + "_")), key=len, default=None)
        if g is None:
            flat[name] = v
        else:
            groups[g][name[len(g) + 1:]] = v
    flat.update({g: SimpleNamespace(**members) for g, members in groups.items()})
    return flat


if not HEADER_PATH.exists():
    raise RuntimeError(f"{HEADER_PATH} is missing: the binding of libfsg_hip.so is derived from it")
CONSTANTS, STRUCTS, PROTOTYPES = parse(HEADER_PATH.read_text())
globals().update(_bind(CONSTANTS))
globals().update({cls.__name__: cls for cls in STRUCTS.values()})
STAGE_NAMES = tuple(n.lower() for n, _v in sorted(vars(ST).items(), key=lambda kv: kv[1]) if n != "COUNT")  # noqa: F821

_lib = None


def load():
    """dlopen libfsg_hip.so and declare prototypes.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). fetalsyngen_amd has no CPU or PyTorch fallback."
        )
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    if lib.fsg_abi_version() != ABI_VERSION:  # noqa: F821
        raise RuntimeError(f"libfsg_hip.so ABI version {lib.fsg_abi_version()}, this binding expects {ABI_VERSION}")  # noqa: F821
    # the structs cross the boundary by pointer: a mirror that disagrees on their size would have the library read past its end
    for cname, cls in STRUCTS.items():
        size = lib.fsg_sample_plan_layout(getattr(SIZEOF, cname[4:].upper()))  # noqa: F821
        if size != C.sizeof(cls):
            raise RuntimeError(f"{cname} is {size} bytes in libfsg_hip.so, {C.sizeof(cls)} in the ctypes mirror")
    _lib = lib
    return lib


def check(code: int, where: str):
    if code != 0:
        msg = load().fsg_error_string(code)
        raise FsgError(code, where, msg.decode() if msg else "?")
