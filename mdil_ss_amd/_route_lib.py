"""ctypes binding of libmdil_route.so (include/mdil_route.h), the routing add-on.  Like the
training library it has NO fallback: if the library is missing or an entry point fails, a
RuntimeError is raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_route.so")
MIN_CLASSES, MAX_CLASSES = 2, 32              # MDIL_ROUTE_MIN_CLASSES / _MAX_CLASSES
STEM_CHANNELS = 16                            # MDIL_ROUTE_STEM_CHANNELS

_P = C.c_void_p
_I = C.c_int
_L = C.c_longlong

_SIGNATURES = {
    "mdil_route_version": (_I, []),
    "mdil_route_last_error": (C.c_char_p, []),
    "mdil_route_stem_workspace_bytes": (_L, [_I, _I, _I]),
    "mdil_route_stem": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _L, _P]),
    "mdil_route_head_workspace_bytes": (_L, [_I, _I, _I, _I]),
    "mdil_route_head": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _L, _P]),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_route", "routing")
