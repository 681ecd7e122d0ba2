"""ctypes binding of libmdil_calib.so (include/mdil_calib.h), the calibration add-on.  Like the
training library it has NO fallback: if the library is missing or the entry point fails, a
RuntimeError is raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_calib.so")
MIN_CLASSES, MAX_CLASSES = 2, 32              # MDIL_CALIB_MIN_CLASSES / _MAX_CLASSES
MAX_TEMPS, MAX_BINS = 16, 32                  # MDIL_CALIB_MAX_TEMPS / _MAX_BINS

_P = C.c_void_p
_I = C.c_int
_L = C.c_longlong

_SIGNATURES = {
    "mdil_calib_version": (_I, []),
    "mdil_calib_last_error": (C.c_char_p, []),
    "mdil_calib_workspace_bytes": (_L, [_I, _I, _I, _I, _I]),
    # x w bias | N H W nc | target ignore_index | temps (HOST) K bins class_temp | label conf_map nll_map |
    # hist class_hist sums nonfinite bad_targets | workspace workspace_bytes | stream
    "mdil_calib_head": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P,
                             _P, _L, _P]),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_calib", "calibration")
