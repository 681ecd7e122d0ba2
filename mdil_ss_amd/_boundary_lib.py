"""ctypes binding of libmdil_boundary.so (include/mdil_boundary.h), the boundary add-on.  Like the
training library it has NO fallback: if the library is missing or the entry point fails, a
RuntimeError is raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_boundary.so")
MIN_CLASSES, MAX_CLASSES = 2, 32              # MDIL_BOUNDARY_MIN_CLASSES / _MAX_CLASSES
MAX_SIZE = 1 << 22                            # MDIL_BOUNDARY_MAX_SIZE
MAX_WIDTHS, MAX_WIDTH = 8, 128                # MDIL_BOUNDARY_MAX_WIDTHS / _MAX_WIDTH

_P = C.c_void_p
_I = C.c_int
_L = C.c_longlong

_SIGNATURES = {
    "mdil_boundary_version": (_I, []),
    "mdil_boundary_last_error": (C.c_char_p, []),
    "mdil_boundary_workspace_bytes": (_L, [_I, _I, _I]),
    # pred target | N H W nc | widths (host) n_widths | ignore_index | workspace bytes | dist_pred dist_target |
    # target_hist pred_hist both_hist confusion bad_targets bad_preds | stream
    "mdil_boundary_count": (_I, [_P, _P, _I, _I, _I, _I, C.POINTER(_I), _I, _I, _P, _L, _P, _P,
                                 _P, _P, _P, _P, _P, _P, _P]),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_boundary", "boundary")
