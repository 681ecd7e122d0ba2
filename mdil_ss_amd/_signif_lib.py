"""ctypes binding of libmdil_signif.so (include/mdil_signif.h), the significance add-on.  Like the
training library it has NO fallback: if the library is missing or an entry point fails, a
RuntimeError is raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_signif.so")
MIN_CLASSES, MAX_CLASSES = 2, 32              # MDIL_SIGNIF_MIN_CLASSES / _MAX_CLASSES
MAX_GROUPS = 2                                # MDIL_SIGNIF_MAX_GROUPS
MAX_SIZE = 1 << 15                            # MDIL_SIGNIF_MAX_SIZE
MAX_IMAGES = 1 << 20                          # MDIL_SIGNIF_MAX_IMAGES
MAX_REPLICATES = 1 << 32                      # MDIL_SIGNIF_MAX_REPLICATES
MAX_ENTRY = 1 << 31                           # entries of a count table the resampler takes: [0, 2^31)
BOOTSTRAP, JACKKNIFE, SWAP = 0, 1, 2          # MDIL_SIGNIF_BOOTSTRAP / _JACKKNIFE / _SWAP

_P = C.c_void_p
_I = C.c_int
_L = C.c_longlong

_SIGNATURES = {
    "mdil_signif_version": (_I, []),
    "mdil_signif_last_error": (C.c_char_p, []),
    # pred target | N H W nc | ignore_index | first_image M G g | counts bad_targets unpredicted | stream
    "mdil_signif_count": (_I, [_P, _P, _I, _I, _I, _I, _I, _L, _L, _I, _I, _P, _P, _P, _P]),
    # counts M G nc | ignore_index mode | first_replicate B seed | sums miou iou empty | stream
    "mdil_signif_resample": (_I, [_P, _L, _I, _I, _I, _I, _L, _L, C.c_ulonglong, _P, _P, _P, _P, _P]),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_signif", "significance")
