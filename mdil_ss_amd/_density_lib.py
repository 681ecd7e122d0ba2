"""ctypes binding of libmdil_density.so (include/mdil_density.h), the density add-on.  Like the
training library it has NO fallback: if the library is missing or an entry point fails, a
RuntimeError is raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_density.so")
MIN_CLASSES, MAX_CLASSES = 2, 32              # MDIL_DENSITY_MIN_CLASSES / _MAX_CLASSES
MAX_MEANS = 32                                # MDIL_DENSITY_MAX_MEANS
MAX_CHANNELS = 128                            # MDIL_DENSITY_MAX_CHANNELS
MAX_ROWS = 1 << 24                            # MDIL_DENSITY_MAX_ROWS

_P = C.c_void_p
_I = C.c_int
_L = C.c_longlong

_SIGNATURES = {
    "mdil_density_version": (_I, []),
    "mdil_density_last_error": (C.c_char_p, []),
    "mdil_density_head": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "mdil_density_rows": (_I, [_P, _L, _I, _P, _P, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_density", "density")
