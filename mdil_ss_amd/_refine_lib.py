"""ctypes binding of libmdil_refine.so (include/mdil_refine.h), the refinement add-on.  Like the
training library it has NO fallback: if the library is missing or an entry point fails, a
RuntimeError is raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_refine.so")
MIN_CLASSES, MAX_CLASSES = 2, 32              # MDIL_REFINE_MIN_CLASSES / _MAX_CLASSES
MAX_ITERATIONS = 16                           # MDIL_REFINE_MAX_ITERATIONS (from 0)
MAX_RADIUS = 5                                # MDIL_REFINE_MAX_RADIUS (from 1)
MAX_DILATION = 4                              # MDIL_REFINE_MAX_DILATION (from 1)

_P = C.c_void_p
_I = C.c_int
_L = C.c_longlong
_F = C.c_float

_SIGNATURES = {
    "mdil_refine_version": (_I, []),
    "mdil_refine_last_error": (C.c_char_p, []),
    "mdil_refine_workspace_bytes": (_L, [_I, _I, _I, _I, _I]),
    "mdil_refine_head": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _F, _F, _F, _F, _P, _L, _P, _P, _P, _P,
                              _I, _P, _P, _P, _P]),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_refine", "refinement")
