"""CPU: include/instag_hip.h is the only statement of the C ABI -- instag_amd/_cabi.py reads the ctypes structs,
prototypes and constants from its text.  The grammar on literal snippets, every struct layout against a C compiler,
and the arities the hand-kept table once got wrong."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from instag_amd import _cabi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = "typedef struct instag_demo_args { int32_t n; const float* x; } instag_demo_args;\n"


def one(text):
    """The single prototype of a snippet."""
    protos = _cabi.parse(text)[1]
    assert len(protos) == 1
    return next(iter(protos.values()))


def fields(body):
    structs = _cabi.parse("typedef struct { %s } instag_demo_job;" % body)[0]
    assert list(structs) == ["instag_demo_job"] and structs["instag_demo_job"].__name__ == "DemoJob"
    return structs["instag_demo_job"]._fields_


# ---- accepted forms ---------------------------------------------------------------------------------------------------
def test_comments_preprocessor_lines_and_the_extern_braces_are_skipped():
    text = """/* top
 * comment */
#ifndef INSTAG_HIP_H
#define INSTAG_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* instag_stream_t; /* hipStream_t */
#define INSTAG_OK 0
#define INSTAG_E_ARG 1     /* invalid argument */
#define INSTAG_MASK 0x20
int instag_demo(const float* x /* [N] */, int64_t* n /* (host) */,
                instag_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif /* INSTAG_HIP_H */
"""
    structs, protos, constants = _cabi.parse(text)
    assert structs == {} and constants == {"INSTAG_OK": 0, "INSTAG_E_ARG": 1, "INSTAG_MASK": 32}
    assert protos == {"instag_demo": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p])}


def test_scalar_parameters_and_return_types():
    res, args = one("size_t instag_demo(int a, int32_t b, uint32_t c, int64_t d, size_t e, float f, double g, "
                    "instag_stream_t s);")
    assert res is C.c_size_t
    assert args == [C.c_int32, C.c_int32, C.c_uint32, C.c_int64, C.c_size_t, C.c_float, C.c_double, C.c_void_p]
    assert one("const char* instag_demo(void);") == (C.c_char_p, [])
    assert one("int64_t instag_demo(void);") == (C.c_int64, [])
    assert one("uint32_t instag_demo(int32_t N);") == (C.c_uint32, [C.c_int32])


def test_pointers_to_scalars_and_void_are_void_pointers_const_ignored():
    _, args = one("int instag_demo(const float* a, float *b, void* c, const void *d, const uint8_t* e, uint64_t* f, "
                  "double* g, const int32_t* h, int64_t* i);")
    assert args == [C.c_void_p] * 9
    # the host arrays of device pointers (instag_frame_code_forward's params, instag_frame_code_backward's grads)
    assert one("int instag_demo(const float* const* params, float* const* grads);")[1] == [C.c_void_p, C.c_void_p]


def test_pointer_to_a_declared_struct():
    structs, protos, _ = _cabi.parse(ARGS + "int instag_demo(const instag_demo_args* a, instag_stream_t s);")
    assert protos["instag_demo"][1][0] is C.POINTER(structs["instag_demo_args"])
    assert structs["instag_demo_args"].__name__ == "DemoArgs"
    assert structs["instag_demo_args"]._fields_ == [("n", C.c_int32), ("x", C.c_void_p)]
    # an untagged struct, and a tag that repeats the name
    assert list(_cabi.parse("typedef struct { int32_t n; } instag_a; typedef struct instag_b { float x; } instag_b;")[0]) \
        == ["instag_a", "instag_b"]


def test_struct_declarators():
    assert fields("int32_t G, F;") == [("G", C.c_int32), ("F", C.c_int32)]
    assert fields("const float *bg, *viewmatrix;") == [("bg", C.c_void_p), ("viewmatrix", C.c_void_p)]
    assert fields("const float* means3D; /* [N,3] */ uint32_t *walk_hints;") == [("means3D", C.c_void_p),
                                                                               ("walk_hints", C.c_void_p)]
    assert fields("float* p, q;") == [("p", C.c_void_p), ("q", C.c_float)]           # the star belongs to the declarator
    (name, t), = fields("const void* w[32];")
    assert name == "w" and t._type_ is C.c_void_p and t._length_ == 32
    assert fields("double sigma, gamma; int64_t off; const uint8_t* store; uint8_t* dst;") == [
        ("sigma", C.c_double), ("gamma", C.c_double), ("off", C.c_int64), ("store", C.c_void_p), ("dst", C.c_void_p)]


def test_class_names_are_mechanical():
    for c_name, py_name in (("instag_raster_args", "RasterArgs"), ("instag_wgrad_job", "WgradJob"),
                            ("instag_face_loss_cfg", "FaceLossCfg"), ("instag_ave_encoder_weights", "AveEncoderWeights")):
        assert _cabi.class_name(c_name) == py_name
    with pytest.raises(ValueError, match="other_args"):
        _cabi.class_name("other_args")


# ---- rejected forms: ValueError that names the declaration ---------------------------------------------------------------
@pytest.mark.parametrize("text, named", [
    ("int instag_demo(long n);", "instag_demo"),                                         # unknown base type
    ("int instag_demo(unsigned int n);", "instag_demo"),
    ("long instag_demo(int32_t n);", "instag_demo"),
    ("int instag_demo(const instag_other_args* a);", "instag_demo"),                     # a struct nobody declared
    (ARGS + "int instag_demo(instag_demo_args** a);", "instag_demo"),                    # pointer to pointer
    ("typedef struct { instag_stream_t* s; } instag_demo_job;", "instag_demo_job"),
    ("int instag_demo(char** names);", "instag_demo"),
    ("int instag_demo(void (*done)(int32_t), int32_t n);", "instag_demo"),               # function pointer
    ("typedef struct { int32_t (*done)(void); } instag_demo_job;", "instag_demo_job"),
    ("typedef struct { int32_t flags : 3; } instag_demo_job;", "instag_demo_job"),       # bit-field
    (ARGS + "int instag_demo(instag_demo_args a);", "instag_demo"),                      # struct by value
    (ARGS + "typedef struct { instag_demo_args a; } instag_demo_job;", "instag_demo_job"),
    (ARGS + "instag_demo_args instag_demo(void);", "instag_demo"),
    ("int instag_demo(const char* fmt, ...);", "instag_demo"),                           # variadic
    ("int instag_demo(int32_t n, ...);", "instag_demo"),
    ("int instag_demo(void* p, char c);", "instag_demo"),
    ("void instag_demo(int32_t n);", "instag_demo"),                                     # (no entry point returns void)
    ("int instag_demo(float x[3]);", "instag_demo"),                                     # array parameter
    ("int instag_demo(int32_t);", "instag_demo"),                                        # unnamed parameter
    ("int instag_demo(int32_t n) { return n; }", "instag_demo"),                         # a definition
    ("int instag_demo(int32_t n); int instag_demo(int32_t n);", "instag_demo"),          # declared twice
    ("int other_demo(int32_t n);", "other_demo"),
    ("typedef struct instag_x { int32_t n; } instag_demo_job;", "instag_demo_job"),      # tag and name differ
    ("typedef struct { struct { int32_t n; } in; } instag_demo_job;", "typedef struct"),  # nested struct
    ("typedef union { int32_t n; float x; } instag_demo_job;", "typedef union"),
    ("enum instag_demo_kind { A, B };", "enum instag_demo_kind"),
    ("typedef int32_t instag_demo_t;", "instag_demo_t"),
    ("extern int32_t instag_demo_count;", "instag_demo_count"),
    ("int instag_demo(int32_t n)", "instag_demo"),                                       # no semicolon
    ("// a line comment\nint instag_demo(int32_t n);", "a line comment"),
    ("#define INSTAG_DEMO 1.5f", "INSTAG_DEMO"),                                         # constants are integers
    ("#define INSTAG_DEMO (1 << 3)", "INSTAG_DEMO"),
    ("#define INSTAG_DEMO(x) x", "INSTAG_DEMO"),
])
def test_anything_else_raises_and_names_the_declaration(text, named):
    with pytest.raises(ValueError, match=named):
        _cabi.parse("typedef void* instag_stream_t;\n" + text)


# ---- the header itself --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def header():
    return _cabi.read()


def test_lib_publishes_what_the_header_declares(header):
    from instag_amd import _lib
    structs, protos, constants = header
    assert len(structs) == 10 and _lib.EXPORTED_SYMBOLS == tuple(protos) and len(protos) == 143
    for name, cls in structs.items():
        assert getattr(_lib, _cabi.class_name(name))._fields_ == cls._fields_
    assert _lib.ABI_VERSION == constants["INSTAG_ABI_VERSION"] and _lib.E_ARG == constants["INSTAG_E_ARG"] == 1
    from instag_amd import losses
    assert [losses.FLAG_HAIR_TO_BG, losses.FLAG_ALPHA, losses.FLAG_HAIR_ATTN, losses.FLAG_LIPS, losses.FLAG_MOUTH,
            losses.FLAG_PLAIN] == [1, 2, 4, 8, 16, 32]
    handle = _lib.lib()
    for name, (res, args) in protos.items():         # (by name: each parse makes its own struct classes)
        fn = getattr(handle, name)
        assert fn.restype is res and [t.__name__ for t in fn.argtypes] == [t.__name__ for t in args], name
    assert _lib.lib() is handle


def test_pinned_prototypes(header):
    structs, protos, _ = header
    assert len(protos["instag_raster_backward"][1]) == 31
    assert len(protos["instag_mlp_backward_glue"][1]) == 22
    assert protos["instag_last_error"][1] == [] and protos["instag_abi_version"][1] == []
    assert protos["instag_frame_store_stride"][0] is C.c_int64
    assert protos["instag_debug_depth_sort_blocks"][0] is C.c_uint32
    assert protos["instag_lpips_forward"][1][0] is C.POINTER(structs["instag_lpips_weights"])
    assert structs["instag_lpips_weights"].__name__ == "LpipsWeights"
    from instag_amd import _lib
    assert _lib.lib().instag_raster_backward.argtypes[0] is C.POINTER(_lib.RasterArgs)
    assert len(_lib.lib().instag_raster_backward.argtypes) == 31


def _host_compiler():
    if shutil.which("cc"):
        return shutil.which("cc")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc())))
    for cand in (os.path.join(rocm, "lib", "llvm", "bin", "clang"), os.path.join(rocm, "bin", "amdclang")):
        if os.path.exists(cand):
            return cand
    raise AssertionError("no host C compiler: neither cc nor the clang beside hipcc")


def test_struct_layouts_match_the_compiler(header, tmp_path):
    """sizeof of every struct, offsetof and size of every field, as a C compiler lays include/instag_hip.h out."""
    structs = header[0]
    lines = ['#include <stdio.h>', '#include "instag_hip.h"', 'int main(void) {']
    want = []
    for name, cls in structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        want.append(f"{name} {C.sizeof(cls)}")
        for field, _ in cls._fields_:
            lines.append(f'  printf("{name}.{field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name}*)0)->{field}));')
            want.append(f"{name}.{field} {getattr(cls, field).offset} {getattr(cls, field).size}")
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([_host_compiler(), "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(want) == 10 + sum(len(c._fields_) for c in structs.values()) and len(want) > 100
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w]
