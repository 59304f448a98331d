"""ctypes binding of libe4s_hip.so, derived at import from include/e4s_hip.h.

This is the thin host-side shim a maintainer of the reference would add in place of
``torch.utils.cpp_extension.load(...)`` (src/models/stylegan2/op/fused_act.py:8-15,
upfirdn2d.py:7-14): PyTorch supplies device memory (``Tensor.data_ptr()``) and the current HIP
stream; the library gets raw pointers and sizes.  There is NO fallback: if the shared object is
missing, or a tensor is not a contiguous fp32 tensor on a ROCm device, we raise.

The header is the single source of the ABI: its typedef structs become the ``ctypes.Structure`` classes exported here (``e4s_conv_params`` ->
``ConvParams``), its prototypes ``SIGNATURES`` / ``INT64_RETURN``, its integer #defines ``DEFINES``.  A new entry point, struct or field is
declared there, with a bump of ``E4S_ABI_VERSION``; nothing in this file changes.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("E4S_LIB_PATH") or os.path.join(_HERE, "libe4s_hip.so")      # (E4S_LIB_PATH: A/B runs of two builds)
HEADER = os.path.join(os.path.dirname(_HERE), "include", "e4s_hip.h")

c_p = ctypes.c_void_p
c_i = ctypes.c_int
c_l = ctypes.c_int64
c_f = ctypes.c_float
c_d = ctypes.c_double

C_SCALARS = {"int": c_i, "unsigned": ctypes.c_uint, "int64_t": c_l, "uint8_t": ctypes.c_uint8, "float": c_f, "double": c_d}
_POINTEES = {"void", "char", "int32_t"}                # what else may stand behind a `*`
_RETURNS = {"int": c_i, "int64_t": c_l, "const char*": ctypes.c_char_p}
_DECL = r"\w+(?:\s*\[\s*\w+\s*\])*"                    # a declarator: name, name[3], name[3][2], name[A_DEFINE]


def _spell(s):
    """One spelling per C type: single spaces, every `*` attached to its left."""
    return re.sub(r"\s*\*", "*", " ".join(s.split()))


def _ctype(spelling, structs, what):
    """C type -> ctypes type.  Scalars map exactly; every pointer is c_void_p, whatever it points to: device memory, a host struct passed
    with byref and a host ctypes array are all `T*` in the header, and c_void_p takes each of them and None."""
    base = " ".join(re.sub(r"\bconst\b|\*", " ", spelling).split())
    if "*" in spelling and (base in C_SCALARS or base in _POINTEES or base in structs):
        return c_p
    if "*" not in spelling and base in C_SCALARS:
        return C_SCALARS[base]
    raise RuntimeError(f"e4s_hip.h: {what}: " + (f"struct {base} by value" if base in structs else f"unknown type '{spelling}'"))


def parse_header(text):
    """The text of include/e4s_hip.h (plain C99: integer #defines, typedef structs of scalars, pointers and fixed arrays, prototypes) ->
    (defines {name: int}, structs {C name: ctypes.Structure class}, functions {name: (return type, [(parameter type, its ctypes type), ...])}),
    the C types as spelled.  Whatever it cannot read is a RuntimeError naming the declaration, never skipped: an entry point left out here
    would be called with ctypes' defaults, pointers as 32-bit ints."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    ncalls = len(re.findall(r"e4s_\w+\s*\(", text))
    text = re.sub(r"#\s*ifdef\s+__cplusplus.*?#\s*endif", " ", text, flags=re.S)
    defines, structs, functions = {}, {}, {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S[^\n]*)$", text, flags=re.M):
        if not re.fullmatch(r"\d+|0[xX][0-9a-fA-F]+", value.strip()):
            raise RuntimeError(f"e4s_hip.h: #define {name}: '{value.strip()}' is no integer literal")
        defines[name] = int(value, 0)
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)

    def struct(m):
        cname, fields = m.group(2), []
        for stmt in filter(None, (s.strip() for s in m.group(1).split(";"))):
            d = re.fullmatch(rf"(.*?[\s*])({_DECL}(?:\s*,\s*{_DECL})*)", stmt, flags=re.S)
            if not d:
                raise RuntimeError(f"e4s_hip.h: {cname}: cannot split the field declaration '{stmt}'")
            ctype = _ctype(_spell(d.group(1)), structs, f"{cname}: '{stmt}'")
            for decl in d.group(2).split(","):
                name, *dims = re.findall(r"\w+", decl)
                ftype = ctype
                for dim in reversed(dims):
                    if not dim.isdigit() and dim not in defines:
                        raise RuntimeError(f"e4s_hip.h: {cname}: unknown array size in '{stmt}'")
                    ftype = ftype * (defines[dim] if dim in defines else int(dim))
                fields.append((name, ftype))
        cls = "".join(w.capitalize() for w in cname.split("_")[1:])
        structs[cname] = type(cls, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"``{cname}`` of include/e4s_hip.h."})
        return " "

    text = re.sub(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"([\w\s*]*?[\s*])(e4s_\w+)\s*\(([^()]*)\)", stmt)
        if not m:
            raise RuntimeError(f"e4s_hip.h: cannot split the declaration '{' '.join(stmt.split())[:160]}'")
        ret, name, params = _spell(m.group(1)), m.group(2), m.group(3).strip()
        if ret not in _RETURNS:
            raise RuntimeError(f"e4s_hip.h: {name}: unknown return type '{ret}'")
        args = []
        for par in ([] if params in ("", "void") else params.split(",")):
            d = re.fullmatch(r"(.*?[\s*])\w+", par.strip(), flags=re.S)
            if not d:
                raise RuntimeError(f"e4s_hip.h: {name}: cannot split the parameter '{par.strip()}'")
            args.append((_spell(d.group(1)), _ctype(_spell(d.group(1)), structs, f"{name}: parameter '{par.strip()}'")))
        functions[name] = (ret, args)
    if len(functions) != ncalls:
        raise RuntimeError(f"e4s_hip.h: {ncalls} times 'e4s_*(' but {len(functions)} functions parsed")
    return defines, structs, functions


with open(HEADER) as _fh:
    DEFINES, STRUCTS, FUNCTIONS = parse_header(_fh.read())
globals().update({_cls.__name__: _cls for _cls in STRUCTS.values()})       # ConvParams, ConvBwdParams, RetinaGeom, StyleGradJob, RowdotJob, ...
ABI_VERSION = DEFINES["E4S_ABI_VERSION"]
STYLE_GRAD_MAX_JOBS = DEFINES["E4S_STYLE_GRAD_MAX_JOBS"]
# name -> argtypes; all return int except INT64_RETURN (size queries: a count, not an error code) and the two info calls, bound in load()
SIGNATURES = {name: [t for _, t in args] for name, (_, args) in FUNCTIONS.items() if name not in ("e4s_abi_version", "e4s_build_arch")}
INT64_RETURN = {name for name, (ret, _) in FUNCTIONS.items() if ret == "int64_t"}

_lib = None


def load():
    """dlopen libe4s_hip.so (built in-tree by e4s_amd.build / __graft_entry__.build). Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: run `python -m e4s_amd.build` (hipcc, gfx950). "
                           "e4s_amd has no CPU / eager fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    lib.e4s_abi_version.restype = c_i
    lib.e4s_build_arch.restype = ctypes.c_char_p
    if lib.e4s_abi_version() != ABI_VERSION:
        raise RuntimeError("libe4s_hip.so ABI version mismatch: rebuild with `python -m e4s_amd.build --force`")
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = c_l if name in INT64_RETURN else c_i
    _lib = lib
    return lib


def stream():
    return c_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a contiguous fp32/uint8/int32/f64 ROCm tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("e4s_amd kernels need tensors on a ROCm device (no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError("e4s_amd kernels need contiguous tensors")
    return c_p(t.data_ptr())


def fptr(t):
    if t is not None and t.dtype != torch.float32:
        raise RuntimeError(f"expected float32, got {t.dtype}")
    return ptr(t)


def check(code, what):
    if code != 0:
        raise RuntimeError(f"{what} failed: hipError {code}")


def call(name, *args):
    check(getattr(load(), name)(*args), name)
