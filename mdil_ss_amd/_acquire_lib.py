"""ctypes binding of libmdil_acquire.so (include/mdil_acquire.h), the acquisition add-on.  Like the
training library it has NO fallback: if the library is missing or an entry point fails, a
RuntimeError is raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_acquire.so")
MIN_CLASSES, MAX_CLASSES = 2, 32              # MDIL_ACQUIRE_MIN_CLASSES / _MAX_CLASSES
MIN_TILE, MAX_TILE = 2, 256                   # MDIL_ACQUIRE_MIN_TILE / _MAX_TILE
TILE_FIELDS = 4                               # MDIL_ACQUIRE_TILE_FIELDS

_P = C.c_void_p
_I = C.c_int
_F = C.c_float

_SIGNATURES = {
    "mdil_acquire_version": (_I, []),
    "mdil_acquire_last_error": (C.c_char_p, []),
    "mdil_acquire_head": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _P, _I, _P, _P, _P, _P, _P, _P]),
    "mdil_acquire_apply": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_acquire", "acquisition")
