"""ctypes binding of libmdil_similarity.so (include/mdil_similarity.h), the representation-similarity
add-on: moments of paired feature rows on the device.  Like the training library it has NO
fallback: if the library is missing or an entry point fails, a RuntimeError is raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_similarity.so")
MAX_CX = 128                                  # MDIL_SIM_MAX_CX
MAX_CY = 128                                  # MDIL_SIM_MAX_CY
MAX_CLASSES = 32                              # MDIL_SIM_MAX_CLASSES
MAX_ROWS = 16777216                           # MDIL_SIM_MAX_ROWS
CHAIN = 1024                                  # MDIL_SIM_CHAIN

_P = C.c_void_p
_I = C.c_int
_L = C.c_longlong

_SIGNATURES = {
    "mdil_sim_version": (_I, []),
    "mdil_sim_last_error": (C.c_char_p, []),
    "mdil_sim_state_bytes": (_L, [_I, _I, _I]),
    "mdil_sim_workspace_bytes": (_L, [_L, _I, _I, _I]),
    # x y labels | rows cx cy nc | pivot_x pivot_y | state workspace stream
    "mdil_sim_accumulate": (_I, [_P, _P, _P, _L, _I, _I, _I, _P, _P, _P, _P, _P]),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_sim", "similarity")
