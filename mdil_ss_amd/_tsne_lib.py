"""ctypes binding of libmdil_tsne.so (include/mdil_tsne.h), the latent-space add-on: exact t-SNE on
the device.  Like the training library it has NO fallback: if the library is missing or an entry
point fails, a RuntimeError is raised."""
import ctypes as C
import os

from . import _addon_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdil_tsne.so")
MAX_POINTS = 32768                            # MDIL_TSNE_MAX_POINTS
MAX_DIM = 128                                 # MDIL_TSNE_MAX_DIM

_P = C.c_void_p
_I = C.c_int
_F = C.c_float

_SIGNATURES = {
    "mdil_tsne_version": (_I, []),
    "mdil_tsne_last_error": (C.c_char_p, []),
    "mdil_tsne_workspace_bytes": (C.c_longlong, [_I]),
    # X N d | D | stream
    "mdil_tsne_sqdist": (_I, [_P, _I, _I, _P, _P]),
    # D N perplexity | beta_out P | workspace stream
    "mdil_tsne_affinities": (_I, [_P, _I, C.c_double, _P, _P, _P, _P]),
    # P N | Y update gains | iters first_iter exaggeration_iters exaggeration learning_rate | kl_every kl_log |
    # partials stream
    "mdil_tsne_run": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _F, _F, _I, _P, _P, _P]),
}

EXPORTS = tuple(_SIGNATURES)
load, check = _addon_lib.bind(LIB_PATH, _SIGNATURES, "mdil_tsne", "latent-space")
