"""ctypes binding of libmdil_ripu.so (include/mdil_ripu.h), the sliding-region acquisition add-on.  Like
the training library it has NO fallback: if the library is missing or an entry point fails, a
RuntimeError is raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_ripu.so")
MIN_CLASSES, MAX_CLASSES = 2, 32              # MDIL_RIPU_MIN_CLASSES / _MAX_CLASSES
MIN_RADIUS, MAX_RADIUS = 1, 32                # MDIL_RIPU_MIN_RADIUS / _MAX_RADIUS
MAX_PICKS = 65536                             # MDIL_RIPU_MAX_PICKS
MAX_IMAGE_PIXELS = 1 << 24                    # MDIL_RIPU_MAX_IMAGE_PIXELS
TLOG_SHIFT = 14                               # MDIL_RIPU_TLOG_SHIFT

_P = C.c_void_p
_I = C.c_int
_L = C.c_longlong

_SIGNATURES = {
    "mdil_ripu_version": (_I, []),
    "mdil_ripu_last_error": (C.c_char_p, []),
    "mdil_ripu_score": (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _L, _L, _P, _P]),
    "mdil_ripu_select": (_I, [_P, _P, _I, _I, _I, _I, _L, _I, _P, _P, _P, _P, _P]),
    "mdil_ripu_apply": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_ripu", "ripu")
