"""ctypes binding of libmdil_ensemble.so (include/mdil_ensemble.h), the multi-scale / flip ensemble
add-on.  Like the training library it has NO fallback: if the library is missing or the entry point
fails, a RuntimeError is raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_ensemble.so")
MIN_CLASSES, MAX_CLASSES = 2, 32              # MDIL_ENSEMBLE_MIN_CLASSES / _MAX_CLASSES
MAX_SIZE = 1 << 22                            # MDIL_ENSEMBLE_MAX_SIZE
MAX_VIEWS = 8                                 # MDIL_ENSEMBLE_MAX_VIEWS
MODES = {"prob": 0, "logit": 1}               # MDIL_ENSEMBLE_MODE_PROB / _LOGIT

_P = C.c_void_p
_I = C.c_int


class View(C.Structure):
    """mdil_ensemble_view: one entry of the HOST view table."""
    _fields_ = [("x", _P), ("H", _I), ("W", _I), ("mirrored", _I)]


_SIGNATURES = {
    "mdil_ensemble_version": (_I, []),
    "mdil_ensemble_last_error": (C.c_char_p, []),
    # views nviews | w bias | N nc Ho Wo mode | id_map palette target | ignore_index |
    # label colour confidence confusion bad | stream
    "mdil_ensemble_head": (_I, [C.POINTER(View), _I, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P,
                                _P]),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_ensemble", "ensemble")


def view_table(entries):
    """[(device pointer, H, W, mirrored)] -> a ctypes array of View (host memory)."""
    return (View * len(entries))(*[View(p, int(h), int(w), int(bool(m))) for p, h, w, m in entries])
