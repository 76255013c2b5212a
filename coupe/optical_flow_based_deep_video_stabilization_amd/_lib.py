"""ctypes binding of libvstab_hip.so.  include/vstab.h is the one statement of the C ABI: every function's restype and argtypes
are read from its declaration there (`EXPORTS`), so a new entry point is declared in the header and wrapped, nothing else.  No CPU
fallback: if the HIP library cannot be built or loaded every entry point raises."""
from __future__ import annotations

import ctypes as C
import os
import re

from . import build as _build

HEADER = os.path.normpath(os.path.join(_build.HERE, "..", "..", "include", "vstab.h"))     # build.HEADERS hashes it into the build stamp

c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)


class VstabTensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", c_float_p), ("ndim", C.c_int32), ("shape", C.c_int32 * 4)]


class VstabWsEntry(C.Structure):
    _fields_ = [("name", C.c_char * 24), ("offset_bytes", C.c_int64), ("n", C.c_int32), ("h", C.c_int32),
                ("w", C.c_int32), ("c", C.c_int32), ("c_stride", C.c_int32)]


class PredictUpArgs(C.Structure):
    """vstab_predict_up_args (include/vstab.h): vstab_predict_up's arguments without the batch and the stream."""
    _fields_ = [("taps", C.c_void_p), ("ks", C.c_int), ("slab_stride", C.c_longlong), ("h", C.c_int), ("w", C.c_int), ("bias2", C.c_void_p),
                ("prev", C.c_void_p), ("ph", C.c_int), ("pw", C.c_int), ("out", C.c_void_p), ("up_w", c_float_p), ("up_b", c_float_p),
                ("concat", C.c_void_p), ("oh", C.c_int), ("ow", C.c_int), ("Cs", C.c_int), ("c_off", C.c_int)]


class LossLevelDesc(C.Structure):
    """vstab_loss_level_desc (include/vstab.h)."""
    _fields_ = [("pf", C.c_void_p), ("grad", C.c_void_p), ("h", C.c_int), ("w", C.c_int), ("cs_pf", C.c_int), ("cs_grad", C.c_int),
                ("tv_weight", C.c_float)]


# ---- the header's types, `const` dropped and tokens joined by one blank.  A struct that callers fill in as a ctypes Structure or an
# array of them is passed as POINTER(Structure); every other pointer -- data, the opaque vstab_ctx handle and the address it is
# returned through -- is c_void_p, which takes None, an address (data_ptr(), addressof), a ctypes array, a pointer instance and byref(...).
RETURN_TYPES = {"void": None, "int": C.c_int, "size_t": C.c_size_t, "long long": C.c_longlong, "char *": C.c_char_p}
PARAM_TYPES = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
               "long long": C.c_longlong, "unsigned long long": C.c_ulonglong,
               "vstab_tensor *": C.POINTER(VstabTensor), "vstab_ws_entry *": C.POINTER(VstabWsEntry),
               "vstab_predict_up_args *": C.POINTER(PredictUpArgs)}
PARAM_TYPES.update({t: C.c_void_p for t in (
    "void *", "char *", "float *", "double *", "int *", "int32_t *", "uint8_t *", "unsigned char *", "unsigned long long *",
    "void * *", "float * *", "uint8_t * *", "vstab_ctx *", "vstab_ctx * *",
    "vstab_loss_level_desc *")})          # its callers (and the refusal tests) pass addressof(array), an int, which POINTER(...) refuses


def _c_type(text):
    """'const float *const *' -> 'float * *'; None when the text holds anything but identifiers and stars."""
    if not re.fullmatch(r"(?:\s*(?:\w+|\*))*\s*", text):
        return None
    return [t for t in re.findall(r"\w+|\*", text) if t != "const"]


def parse_header(text: str) -> dict:
    """{name: (restype, argtypes)} of every `VSTAB_API <ret> vstab_name(<params>);` in a header's text.  A declaration that does not
    split that way, an unnamed parameter or a type outside RETURN_TYPES / PARAM_TYPES raises RuntimeError: nothing is guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)                       # VSTAB_API's own #define among them
    out = {}
    for chunk in re.split(r"\bVSTAB_API\b", text)[1:]:
        decl = " ".join(chunk.partition(";")[0].split())
        m = re.fullmatch(r"([^()]*?)\b(vstab_\w+) ?\(([^()]*)\)", decl) if ";" in chunk else None
        if m is None:
            raise RuntimeError(f"vstab.h: cannot split the declaration `VSTAB_API {decl[:200]}`")
        ret, name, params = m.groups()
        ret = _c_type(ret)
        if ret is None or " ".join(ret) not in RETURN_TYPES:
            raise RuntimeError(f"vstab.h: {name}: return type `{m.group(1).strip()}` is not in _lib.RETURN_TYPES")
        args = []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            toks = _c_type(p)
            if not toks or " ".join(toks[:-1]) not in PARAM_TYPES or toks[-1] == "*":          # the last token is the parameter's name
                raise RuntimeError(f"vstab.h: {name}: parameter `{p.strip()}` is unnamed or its type is not in _lib.PARAM_TYPES")
            args.append(PARAM_TYPES[" ".join(toks[:-1])])
        if name in out:
            raise RuntimeError(f"vstab.h: {name} is declared twice")
        out[name] = (RETURN_TYPES[" ".join(ret)], args)
    return out


def _read_header():
    try:
        with open(HEADER) as f:
            return f.read()
    except OSError as e:
        raise RuntimeError(f"the C ABI's header {HEADER} cannot be read: {e}") from None


EXPORTS = parse_header(_read_header())          # name: (restype, argtypes)

INTERP = {'bilinear': 0, 'bicubic': 1}          # VSTAB_INTERP_*
INTERP_NAMES = tuple(INTERP)                    # code -> name

_lib = None


def lib():
    """Load (building if needed) libvstab_hip.so.  Raises if that is impossible."""
    global _lib
    if _lib is None:
        path = _build.LIB
        if os.environ.get("VSTAB_LIB"):                 # an explicitly chosen build of the same sources (the sanitizer build of the host side)
            path = os.environ["VSTAB_LIB"]
            if not os.path.exists(path):
                raise RuntimeError(f"VSTAB_LIB={path} does not exist")
        elif os.environ.get("VSTAB_NO_BUILD") != "1":
            path = _build.build()
        elif not os.path.exists(path):
            raise RuntimeError(f"{path} is missing and VSTAB_NO_BUILD=1")
        L = C.CDLL(path)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(L, name)          # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class VstabError(RuntimeError):
    pass


def check(code: int, ctx=None):
    if code == 0:
        return
    msg = lib().vstab_last_error(ctx)
    msg = msg.decode() if msg else "?"
    if code in (-1, -2):          # VSTAB_E_SHAPE / VSTAB_E_ALIGN
        raise ValueError(f"vstab error {code}: {msg}")
    raise VstabError(f"vstab error {code}: {msg}")
