"""ctypes binding of libmdil_audit.so (include/mdil_audit.h), the label-audit add-on.  Like the
training library it has NO fallback: if the library is missing or an entry point fails, a
RuntimeError is raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_audit.so")
MIN_CLASSES, MAX_CLASSES = 2, 32              # MDIL_AUDIT_MIN_CLASSES / _MAX_CLASSES

_P = C.c_void_p
_I = C.c_int
_L = C.c_longlong

_SIGNATURES = {
    "mdil_audit_version": (_I, []),
    "mdil_audit_last_error": (C.c_char_p, []),
    "mdil_audit_head": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mdil_audit_apply": (_I, [_P, _P, _P, _L, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P]),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_audit", "label-audit")
