"""ctypes binding of libmdil_predict.so (include/mdil_predict.h), the inference add-on.  Like the
training library it has NO fallback: if the library is missing or the entry point fails, a
RuntimeError is raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_predict.so")
MIN_CLASSES, MAX_CLASSES = 2, 32              # MDIL_PREDICT_MIN_CLASSES / _MAX_CLASSES

_P = C.c_void_p
_I = C.c_int

_SIGNATURES = {
    "mdil_predict_version": (_I, []),
    "mdil_predict_last_error": (C.c_char_p, []),
    "mdil_predict_head": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_predict", "prediction")
