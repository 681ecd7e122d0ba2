"""ctypes binding of libmdil_segments.so (include/mdil_segments.h), the segments add-on.  Like the
training library it has NO fallback: if the library is missing or an entry point fails, a
RuntimeError is raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_segments.so")
MIN_CLASSES, MAX_CLASSES = 2, 32              # MDIL_SEGMENTS_MIN_CLASSES / _MAX_CLASSES
MAX_SIZE = 1 << 15                            # MDIL_SEGMENTS_MAX_SIZE
MAX_EDGES, MAX_EDGE = 8, 1 << 30              # MDIL_SEGMENTS_MAX_EDGES / _MAX_EDGE
MAX_COVER_DEN = 1000                          # MDIL_SEGMENTS_MAX_COVER_DEN

_P = C.c_void_p
_I = C.c_int
_L = C.c_longlong

_SIGNATURES = {
    "mdil_segments_version": (_I, []),
    "mdil_segments_last_error": (C.c_char_p, []),
    "mdil_segments_workspace_bytes": (_L, [_I, _I, _I]),
    # map | N H W | connectivity | root area | workspace bytes | stream
    "mdil_segments_label": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _L, _P]),
    # map other root area | N H W nc | map_ignore other_ignore | edges (host) n_edges | cover_num cover_den |
    # workspace bytes | hit void | segments pixels hit_pixels covered missed unjudged bad_labels | stream
    "mdil_segments_count": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I, _I, _I, _P, _L, _P, _P,
                                 _P, _P, _P, _P, _P, _P, _P, _P]),
    # map root area | N H W | min_area keep_id fill | out | removed_segments removed_pixels | stream
    "mdil_segments_filter": (_I, [_P, _P, _P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _P]),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_segments", "segments")
