"""ctypes binding of libmdil_drift.so (include/mdil_drift.h), the drift add-on.  Like the training
library it has NO fallback: if the library is missing or the entry point fails, a RuntimeError is
raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_drift.so")
MIN_CLASSES, MAX_CLASSES = 2, 32              # MDIL_DRIFT_MIN_CLASSES / _MAX_CLASSES

_P = C.c_void_p
_I = C.c_int
_L = C.c_longlong

_SIGNATURES = {
    "mdil_drift_version": (_I, []),
    "mdil_drift_last_error": (C.c_char_p, []),
    "mdil_drift_workspace_bytes": (_L, [_I, _I, _I, _I]),
    # xa wa ba xb wb bb | N H W nc | target ignore_index | label_a label_b kl_map change |
    # transition confusion_a confusion_b outcome bad_targets | sums workspace workspace_bytes | stream
    "mdil_drift_head": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                             _P, _P, _L, _P]),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_drift", "drift")
