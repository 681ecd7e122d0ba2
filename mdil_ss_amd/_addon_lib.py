"""The loader the add-ons' ctypes bindings (_predict_lib, _fullres_lib, _ensemble_lib,
_drift_lib, _calib_lib, _tsne_lib, _similarity_lib, _boundary_lib, _pseudo_lib, _route_lib, _segments_lib, _refine_lib,
_signif_lib, _openset_lib, _audit_lib, _acquire_lib, _ripu_lib, _spx_lib, _density_lib) share.  Like the training library they have NO fallback: if a library is missing or
an entry point fails, a RuntimeError is raised.  (_lib.py, the training library's binding, keeps its
own loader: it belongs to the build id.)"""
import ctypes as C
import os


def bind(lib_path, signatures, prefix, path_name):
    """-> (load, check) for the library at ``lib_path``; ``signatures``: {name: (restype, argtypes)},
    ``prefix``: "mdil_predict" ..., ``path_name``: what the "no fallback" message calls the path."""
    state = []
    file_name = os.path.basename(lib_path)

    def load():
        """Load (once) and return the ctypes handle; raises RuntimeError when the library is absent."""
        if state:
            return state[0]
        if not os.path.exists(lib_path):
            raise RuntimeError(
                f"{file_name} not found at {lib_path}: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
                f"There is no CPU / eager fallback for the {path_name} path.")
        lib = C.CDLL(lib_path)
        for name, (res, args) in signatures.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        state.append(lib)
        return lib

    def check(rc, what):
        if rc != 0:
            msg = getattr(load(), prefix + "_last_error")().decode()
            raise RuntimeError(f"{what} failed (rc={rc}): {msg}")

    return load, check
