"""The device-memory twins of the data-carrying entry points (no GPU needed): declared in include/ddamg_hip.h, exported from the
library with the argument types of their host twins, mirrored in the Python API, and an error -- not a crash -- on a null context."""
import ctypes, os, re
import pytest
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, dp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)

# name: (argument types, declaration in the header, mirror in the Python API)
ENTRY_POINTS = {
    "ddamg_hip_set_gauge_device": ([vp, dp, ctypes.c_int, dp],
                                   "int ddamg_hip_set_gauge_device(ddamg_hip_ctx* ctx, const double* gauge_dev_lex, int anti_pbc, double* plaquette);",
                                   (api.Context, "set_gauge_device")),
    "ddamg_hip_set_gauge2_device": ([vp, dp, dp, ctypes.c_int, dp],
                                    "int ddamg_hip_set_gauge2_device(ddamg_hip_ctx* ctx, const double* hopp_gauge_dev_lex, const double* clover_gauge_dev_lex, int anti_pbc, double* plaquette);",
                                    (api.Context, "set_gauge2_device")),
    "ddamg_hip_vec_upload_device": ([vp, vp, dp],
                                    "int ddamg_hip_vec_upload_device(ddamg_hip_ctx* ctx, ddamg_hip_vec* v, const double* dev_lex);",
                                    (api.Vector, "upload_device")),
    "ddamg_hip_vec_download_device": ([vp, vp, dp],
                                      "int ddamg_hip_vec_download_device(ddamg_hip_ctx* ctx, const ddamg_hip_vec* v, double* dev_lex);",
                                      (api.Vector, "download_device")),
    "ddamg_hip_solve_device": ([vp, dp, dp, ctypes.c_double, ip, ip, dp],
                               "int ddamg_hip_solve_device(ddamg_hip_ctx* ctx, double* x_dev_lex, const double* b_dev_lex, double tol, int* iterations, int* coarse_iterations, double* relres);",
                               (api.Context, "solve_device")),
    "ddamg_hip_preconditioner_device": ([vp, dp, dp],
                                        "int ddamg_hip_preconditioner_device(ddamg_hip_ctx* ctx, double* out_dev_lex, const double* in_dev_lex);",
                                        (api.Context, "preconditioner_device")),
}


def null_arguments(types):
    """a null context, null pointers and zeros"""
    return [None if t in (vp, dp, ip) else t(0) for t in types]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(dd.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return api.load_library()


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_entry_point_is_declared_exported_and_mirrored(lib, name):
    types, declaration, (cls, method) = ENTRY_POINTS[name]
    assert name in dd.declared_symbols()
    header = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "ddamg_hip.h")).read())
    assert declaration in header
    entry = getattr(lib, name)
    assert entry.argtypes == types and entry.restype == ctypes.c_int
    assert callable(getattr(cls, method))
    # a null context is an error with a message, not a crash
    assert entry(*null_arguments(types)) != 0 and lib.ddamg_hip_last_error()


def test_addresses_and_objects_with_data_ptr_are_accepted():
    """the mirror takes an integer address or any object with data_ptr(), and refuses anything else before the library is called"""
    class Holder:
        def data_ptr(self):
            return 4096
    assert ctypes.cast(api._dev(4096, 8, "x"), vp).value == 4096
    assert ctypes.cast(api._dev(Holder(), 8, "x"), vp).value == 4096
    with pytest.raises(api.DDAMGError):
        api._dev([1.0, 2.0], 2, "x")
    # torch is imported only when a tensor is handed in: no import at module level
    assert "import torch" not in "".join(l for l in open(api.__file__) if not l.startswith(" "))
