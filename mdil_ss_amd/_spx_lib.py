"""ctypes binding of libmdil_spx.so (include/mdil_spx.h), the superpixel acquisition add-on.  Like
the training library it has NO fallback: if the library is missing or an entry point fails, a
RuntimeError is raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_spx.so")
MIN_CLASSES, MAX_CLASSES = 2, 32              # MDIL_SPX_MIN_CLASSES / _MAX_CLASSES
MIN_STEP, MAX_STEP = 4, 64                    # MDIL_SPX_MIN_STEP / _MAX_STEP
MIN_COMPACTNESS, MAX_COMPACTNESS = 1, 64      # MDIL_SPX_MIN_COMPACTNESS / _MAX_COMPACTNESS
MAX_ITERATIONS = 32                           # MDIL_SPX_MAX_ITERATIONS
MAX_SIDE = 4096                               # MDIL_SPX_MAX_SIDE
MAX_CELLS = 1 << 31                           # MDIL_SPX_MAX_CELLS
FRACTION_BITS = 4                             # MDIL_SPX_FRACTION_BITS
FIELDS = 4                                    # MDIL_SPX_FIELDS

_P = C.c_void_p
_I = C.c_int
_L = C.c_longlong

_SIGNATURES = {
    "mdil_spx_version": (_I, []),
    "mdil_spx_last_error": (C.c_char_p, []),
    "mdil_spx_slic": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "mdil_spx_table": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "mdil_spx_apply": (_I, [_P] * 7 + [_I] * 7 + [_P] * 12),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_spx", "superpixel")
