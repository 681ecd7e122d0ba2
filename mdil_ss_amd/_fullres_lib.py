"""ctypes binding of libmdil_fullres.so (include/mdil_fullres.h), the full-resolution add-on.  Like
the training library it has NO fallback: if the library is missing or the entry point fails, a
RuntimeError is raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_fullres.so")
MIN_CLASSES, MAX_CLASSES = 2, 32              # MDIL_FULLRES_MIN_CLASSES / _MAX_CLASSES
MAX_SIZE = 1 << 22                            # MDIL_FULLRES_MAX_SIZE

_P = C.c_void_p
_I = C.c_int

_SIGNATURES = {
    "mdil_fullres_version": (_I, []),
    "mdil_fullres_last_error": (C.c_char_p, []),
    # x w bias | N H W nc Ho Wo | id_map palette target | ignore_index | label colour confusion bad | stream
    "mdil_fullres_head": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_fullres", "full-resolution")
