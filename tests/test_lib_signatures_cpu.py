"""_lib.EXPORTS comes from include/vstab.h: the parser on declarations written here, the real header's names, hand-written answers
for real exports of every scalar kind and pointer rule, and the hand-written Structures against the C compiler's layout."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, U, F, D, Z, LL, ULL, P = C.c_int, C.c_uint, C.c_float, C.c_double, C.c_size_t, C.c_longlong, C.c_ulonglong, C.c_void_p

LITERAL = """
#define VSTAB_API __attribute__((visibility("default")))
typedef struct vstab_ctx vstab_ctx;
typedef struct vstab_tensor { const char *name; const float *data; int32_t ndim; int32_t shape[4]; } vstab_tensor;
VSTAB_API int vstab_three_lines(vstab_ctx *ctx, const float *x,
                                int B, float scale,
                                void *stream);
/* a comment with (parentheses); and a semicolon; VSTAB_API int vstab_not_declared(int a); */
VSTAB_API const char *vstab_text(void);   // VSTAB_API int vstab_not_declared_either(int a);
VSTAB_API void vstab_slots(const uint8_t *const *slots9, float *const *outs, unsigned long long count, unsigned long long *bad,
                           unsigned seed, double thresh);
VSTAB_API size_t vstab_bytes(long long rows, int C);
VSTAB_API long long vstab_pack(const double *scale, size_t cap);
VSTAB_API int vstab_load(vstab_ctx **out, const vstab_tensor *tensors, int count);
"""


def test_parser_on_literal_declarations():
    assert _lib.parse_header(LITERAL) == {
        "vstab_three_lines": (I, [P, P, I, F, P]),
        "vstab_text": (C.c_char_p, []),
        "vstab_slots": (None, [P, P, ULL, P, U, D]),
        "vstab_bytes": (Z, [LL, I]),
        "vstab_pack": (LL, [P, Z]),
        "vstab_load": (I, [P, C.POINTER(_lib.VstabTensor), I]),
    }


@pytest.mark.parametrize("decl,names", [
    ("VSTAB_API int vstab_bad_type(int a, short b);", "vstab_bad_type"),                   # a type outside the dict
    ("VSTAB_API int vstab_bad_ptr(const long *p);", "vstab_bad_ptr"),
    ("VSTAB_API short vstab_bad_ret(int a);", "vstab_bad_ret"),
    ("VSTAB_API int vstab_unnamed(int, float *);", "vstab_unnamed"),
    ("VSTAB_API int vstab_array(int shape[4]);", "vstab_array"),
    ("VSTAB_API int vstab_callback(int a, int (*cb)(int));", "vstab_callback"),            # the pattern cannot split these three
    ("VSTAB_API int vstab_no_semicolon(int a)", "vstab_no_semicolon"),
    ("VSTAB_API int other_prefix(int a);", "other_prefix"),
    ("VSTAB_API int vstab_twice(int a);\nVSTAB_API int vstab_twice(int a);", "vstab_twice"),
])
def test_parser_refuses_what_it_does_not_know(decl, names):
    with pytest.raises(RuntimeError, match=names):
        _lib.parse_header(decl)


def test_missing_header_names_the_path(monkeypatch):
    monkeypatch.setattr(_lib, "HEADER", os.path.join(ROOT, "include", "no_such_header.h"))
    with pytest.raises(RuntimeError, match="no_such_header.h"):
        _lib._read_header()


def test_real_header_names():
    hdr = open(os.path.join(ROOT, "include", "vstab.h")).read()
    assert os.path.samefile(_lib.HEADER, os.path.join(ROOT, "include", "vstab.h"))
    declared = set(re.findall(r"VSTAB_API[^;(]*?\b(vstab_\w+)\s*\(", hdr))         # test_library_exports_every_declared_symbol's pattern
    assert set(_lib.EXPORTS) == declared and len(declared) >= 166


# Written from the header by hand, not by the parser.
REAL = {
    "vstab_conv_dgrad": (I, [P] + [I] * 6 + [P, P] + [I] * 3 + [P] + [I] * 6 + [P, Z, P]),
    "vstab_adam_step": (I, [P, P, P, P, LL, F, F, F, F, P]),
    "vstab_homography_fit": (I, [P, I, I, I, I, U, D, I, I, P, P, P, Z, P]),
    "vstab_selftest_div_const": (I, [F, U, ULL, P, P]),
    "vstab_last_error": (C.c_char_p, [P]),
    "vstab_version": (C.c_char_p, []),
    "vstab_destroy": (None, [P]),
    "vstab_create": (I, [P, I]),
    "vstab_load_weights": (I, [P, C.POINTER(_lib.VstabTensor), I]),
    "vstab_workspace_layout": (I, [I, I, I, I, C.POINTER(_lib.VstabWsEntry), I]),
    "vstab_loss_main_workspace_bytes": (Z, [P, I, I]),                                # callers pass addressof(descriptor array)
    "vstab_deconv4x4_winograd": (I, [P, I, I, I, I, P, P, I, P] + [I] * 6 + [C.POINTER(_lib.PredictUpArgs), P, Z, P]),
    "vstab_host_pack_layer": (LL, [I, I, P, P, P, LL]),
    "vstab_assemble_input": (I, [P, I, I, I, P, P]),                                  # const uint8_t *const *
    "vstab_column_sum_scratch_bytes": (Z, [LL, I]),
}


@pytest.mark.parametrize("name", REAL)
def test_real_exports_literal(name):
    assert _lib.EXPORTS[name] == REAL[name]


STRUCTS = {"vstab_tensor": _lib.VstabTensor, "vstab_ws_entry": _lib.VstabWsEntry, "vstab_loss_level_desc": _lib.LossLevelDesc,
           "vstab_predict_up_args": _lib.PredictUpArgs}


def test_struct_layouts_match_the_c_compiler(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler on the path")
    lines = []
    for cname, cls in STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, *_ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vstab.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    want = {}
    for cname, cls in STRUCTS.items():
        want[cname] = str(C.sizeof(cls))
        want.update({f"{cname}.{f}": str(getattr(cls, f).offset) for f, *_ in cls._fields_})
    assert got == want
    # every member the header declares is mirrored: same number of declarators between the struct's braces
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "vstab.h")).read(), flags=re.S)
    for cname, cls in STRUCTS.items():
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, flags=re.S).group(1)
        assert sum(len(d.split(",")) for d in body.split(";") if d.strip()) == len(cls._fields_), cname
