"""e4s_amd.lib derives its whole ctypes binding from include/e4s_hip.h.  Host-only checks of that derivation against a C compiler: every
struct's layout, every #define, every prototype, the scalar map; that the parser refuses what it cannot read; and the bytes of the one
table Python packs itself (kernels.rowdot_jobs)."""
import ctypes
import os
import re
import struct
import subprocess

import pytest
import torch

from e4s_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
STRUCT_NAMES = {"e4s_conv_params": "ConvParams", "e4s_conv_bwd_params": "ConvBwdParams", "e4s_conv_wgrad_params": "ConvWgradParams",
                "e4s_rrdb_params": "RrdbParams", "e4s_pconv_params": "PconvParams", "e4s_rconv_params": "RconvParams",
                "e4s_retina_geom": "RetinaGeom", "e4s_conv3d_params": "Conv3dParams", "e4s_conv3dx_params": "Conv3dxParams",
                "e4s_pose_params": "PoseParams", "e4s_spade_shared_params": "SpadeSharedParams", "e4s_spade_conv_params": "SpadeConvParams",
                "e4s_style_grad_job": "StyleGradJob", "e4s_rowdot_job": "RowdotJob"}


def _header():
    with open(lib.HEADER) as fh:
        return re.sub(r"/\*.*?\*/|//[^\n]*", " ", fh.read(), flags=re.S)


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """What gcc says: {"D name": value, "S struct": size, "F struct.field": (offset, size), "T scalar spelling": size}, from one C program
    generated from the parsed header."""
    lines = ['printf("D %s %%lld\\n", (long long)%s);' % (d, d) for d in lib.DEFINES]
    lines += ['printf("T %s %%zu\\n", sizeof(%s));' % (t, t) for t in lib.C_SCALARS]
    for cname, cls in lib.STRUCTS.items():
        lines.append('printf("S %s %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['printf("F %s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (cname, f, cname, f, cname, f) for f, _ in cls._fields_]
    tmp = tmp_path_factory.mktemp("abi")
    src, exe = tmp / "layout.c", tmp / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "e4s_hip.h"\nint main(void){\n' + "\n".join(lines) + "\nreturn 0;}\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", INCLUDE, str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        kind, name, *vals = line.split()
        got[kind + " " + name] = int(vals[0]) if len(vals) == 1 else tuple(int(v) for v in vals)
    return got


def test_every_struct_and_define_matches_the_compiler(compiled):
    assert {c: cls.__name__ for c, cls in lib.STRUCTS.items()} == STRUCT_NAMES
    for cname, cls in lib.STRUCTS.items():
        assert getattr(lib, cls.__name__) is cls
        assert compiled["S " + cname] == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert compiled[f"F {cname}.{f}"] == (getattr(cls, f).offset, getattr(cls, f).size), (cname, f)
    assert {k[2:]: v for k, v in compiled.items() if k[0] == "D"} == lib.DEFINES
    assert lib.ABI_VERSION == lib.DEFINES["E4S_ABI_VERSION"] and lib.STYLE_GRAD_MAX_JOBS == lib.DEFINES["E4S_STYLE_GRAD_MAX_JOBS"]
    # pointers in a struct are c_void_p, arrays keep their shape
    assert all(t in (lib.c_p, lib.c_i, lib.c_l, lib.c_f) for _, t in lib.ConvParams._fields_)
    assert lib.RetinaGeom().min_size._length_ == 3 and lib.RetinaGeom().min_size[0]._length_ == 2 and lib.RetinaGeom().lh._length_ == 3


def test_conv_params_fields_are_the_headers_in_order():
    """An independent reading of the field names of e4s_conv_params: none dropped, none reordered."""
    body = re.search(r"typedef struct \{([^}]*)\} e4s_conv_params;", _header()).group(1)
    names = [re.findall(r"\w+\s*$", part)[0].strip() for stmt in body.split(";") if stmt.strip() for part in stmt.split(",")]
    assert names == [f for f, _ in lib.ConvParams._fields_] and len(names) == 43


def test_rowdot_job_record(compiled):
    """The record kernels.rowdot_jobs packs: 3 x int64, 2 x pointer, 3 x int, float = 56 bytes with no tail padding."""
    fields = ["in_off", "in_stride", "out_off", "M", "bias", "G", "O", "K", "scale"]
    assert [f for f, _ in lib.RowdotJob._fields_] == fields
    assert compiled["S e4s_rowdot_job"] == ctypes.sizeof(lib.RowdotJob) == struct.calcsize("qqqQQiiif") == 56
    assert [compiled["F e4s_rowdot_job." + f][0] for f in fields] == [getattr(lib.RowdotJob, f).offset for f in fields] == [0, 8, 16, 24, 32, 40, 44, 48, 52]


def test_style_grad_jobs_fit_the_kernel_arguments(compiled):
    """The jobs travel by value in the kernel arguments: the header's limit of them, which the Python side enforces, stays under 4 KB."""
    size, max_jobs = compiled["S e4s_style_grad_job"], compiled["D E4S_STYLE_GRAD_MAX_JOBS"]
    assert size == ctypes.sizeof(lib.StyleGradJob) and max_jobs == lib.STYLE_GRAD_MAX_JOBS == 32
    assert size * max_jobs + 4 * (max_jobs + 1) + 4 + 32 <= 4096          # jobs + block offsets + count + the other arguments of stage 2


def test_scalar_map_matches_the_compiler(compiled):
    assert set(lib.C_SCALARS) == {"int", "unsigned", "int64_t", "uint8_t", "float", "double"}
    for spelling, ctype in lib.C_SCALARS.items():
        assert compiled["T " + spelling] == ctypes.sizeof(ctype), spelling
    assert ctypes.sizeof(lib.c_p) == ctypes.sizeof(ctypes.c_size_t)


def test_every_prototype_as_parsed_compiles_against_the_header(tmp_path):
    """One function pointer per entry point, typed from the parser's reading of it, initialised with the entry point itself: a dropped,
    merged or misread parameter or return type is an incompatible pointer."""
    decls = ["%s (*chk_%d)(%s) = %s;" % (ret, i, ", ".join(t for t, _ in args) or "void", name)
             for i, (name, (ret, args)) in enumerate(lib.FUNCTIONS.items())]
    src = tmp_path / "protos.c"
    src.write_text('#include "e4s_hip.h"\n' + "\n".join(decls) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Werror=incompatible-pointer-types", "-Werror=int-conversion", "-I", INCLUDE, "-c", str(src),
                           "-o", str(tmp_path / "protos.o")])
    for name, (ret, args) in lib.FUNCTIONS.items():
        if name in lib.SIGNATURES:
            assert lib.SIGNATURES[name] == [c for _, c in args] and (name in lib.INT64_RETURN) == (ret == "int64_t") and ret in ("int", "int64_t")
            assert all(c is lib.c_p for t, c in args if "*" in t) and all(c is lib.C_SCALARS[t] for t, c in args if "*" not in t)
    assert set(lib.FUNCTIONS) - set(lib.SIGNATURES) == {"e4s_abi_version", "e4s_build_arch"}


def test_no_entry_point_is_left_unbound():
    assert len(re.findall(r"e4s_\w+\s*\(", _header())) == len(lib.SIGNATURES) + 2


GOOD = "typedef struct { int n; } e4s_s;\nint e4s_a(const float* x, int64_t n, void* stream);\n%s\nint64_t e4s_z(const e4s_s* s);\n"


@pytest.mark.parametrize("line", ["int e4s_b(size_t n, void* stream);",            # an unknown type
                                  "int e4s_b(e4s_s s, void* stream);",             # a struct by value
                                  "int e4s_b(int (*cb)(int), void* stream);",      # a function pointer
                                  "double* e4s_b(int n);",                         # a return type with no restype
                                  "int e4s_b(int n, void* stream)"])               # an unterminated prototype
def test_parser_refuses_what_it_cannot_read(line):
    _, structs, functions = lib.parse_header(GOOD % "int e4s_b(int n, void* stream);")
    assert list(functions) == ["e4s_a", "e4s_b", "e4s_z"] and list(structs) == ["e4s_s"]
    with pytest.raises(RuntimeError, match="e4s_b"):
        lib.parse_header(GOOD % line)


def test_rowdot_jobs_table_bytes():
    from e4s_amd import kernels as K
    m = [torch.zeros(8, 4), torch.zeros(4, 8), torch.zeros(12, 4)]
    b = [torch.zeros(8), None, torch.zeros(12)]
    jobs = [dict(in_off=0, in_stride=512, out_off=0, M=m[0], bias=b[0], G=2, O=8, K=4, scale=0.5),
            dict(in_off=2 ** 33 + 4, in_stride=1024, out_off=16, M=m[1], bias=b[1], G=3, O=4, K=8, scale=1.0 / 3.0),
            dict(in_off=8, in_stride=-512, out_off=2 ** 40, M=m[2], bias=b[2], G=1, O=12, K=4, scale=-2.0)]
    table, njobs, max_o, max_g = K.rowdot_jobs(jobs, "cpu")
    want = (struct.pack("qqqQQiiif", 0, 512, 0, m[0].data_ptr(), b[0].data_ptr(), 2, 8, 4, 0.5) +
            struct.pack("qqqQQiiif", 2 ** 33 + 4, 1024, 16, m[1].data_ptr(), 0, 3, 4, 8, 1.0 / 3.0) +
            struct.pack("qqqQQiiif", 8, -512, 2 ** 40, m[2].data_ptr(), b[2].data_ptr(), 1, 12, 4, -2.0))
    assert table.dtype == torch.uint8 and table.numpy().tobytes() == want and len(want) == 3 * 56
    assert (njobs, max_o, max_g) == (3, 12, 3)
