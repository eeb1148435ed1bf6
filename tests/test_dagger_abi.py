"""D^dagger, gamma5 and the D^dagger / D^dagger D solves at the boundary (no GPU needed): declared in include/ddamg_hip.h, exported
from the library, mirrored in the Python API with the argument types of the declaration, and an error -- not a crash -- on a null
context."""
import ctypes, os, re
import pytest
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, dp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
C_TYPES = {"ddamg_hip_ctx*": vp, "ddamg_hip_vec*": vp, "const ddamg_hip_vec*": vp, "double*": dp, "const double*": dp, "int*": ip,
           "double": ctypes.c_double}

SOLVE = "double tol, int* iterations, int* coarse_iterations, double* relres);"
SQUARED = "double tol, int iterations[2], int coarse_iterations[2], double* relres);"
# name: (declaration in the header, mirror in the Python API)
ENTRY_POINTS = {
    "ddamg_hip_dirac_apply_dagger": "int ddamg_hip_dirac_apply_dagger(ddamg_hip_ctx* ctx, ddamg_hip_vec* out, const ddamg_hip_vec* in);",
    "ddamg_hip_gamma5": "int ddamg_hip_gamma5(ddamg_hip_ctx* ctx, ddamg_hip_vec* out, const ddamg_hip_vec* in);",
    "ddamg_hip_solve_dagger": "int ddamg_hip_solve_dagger(ddamg_hip_ctx* ctx, double* x_lex, const double* b_lex, " + SOLVE,
    "ddamg_hip_solve_dagger_vec": "int ddamg_hip_solve_dagger_vec(ddamg_hip_ctx* ctx, ddamg_hip_vec* x, const ddamg_hip_vec* b, " + SOLVE,
    "ddamg_hip_solve_dagger_device": "int ddamg_hip_solve_dagger_device(ddamg_hip_ctx* ctx, double* x_dev_lex, const double* b_dev_lex, " + SOLVE,
    "ddamg_hip_solve_squared": "int ddamg_hip_solve_squared(ddamg_hip_ctx* ctx, double* x_lex, const double* b_lex, " + SQUARED,
    "ddamg_hip_solve_squared_vec": "int ddamg_hip_solve_squared_vec(ddamg_hip_ctx* ctx, ddamg_hip_vec* x, const ddamg_hip_vec* b, " + SQUARED,
    "ddamg_hip_solve_squared_device": "int ddamg_hip_solve_squared_device(ddamg_hip_ctx* ctx, double* x_dev_lex, const double* b_dev_lex, " + SQUARED,
}


def argument_types(declaration):
    """the ctypes of a declaration's parameters: the last word of each is its name, `name[2]` an int*"""
    out = []
    for par in declaration[declaration.index("(") + 1:declaration.rindex(")")].split(","):
        ctype, name = par.strip().rsplit(" ", 1)
        out.append(ip if name.endswith("[2]") and ctype == "int" else C_TYPES[ctype])
    return out


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(dd.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return api.load_library()


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_entry_point_is_declared_exported_and_mirrored(lib, name):
    declaration = ENTRY_POINTS[name]
    assert name in dd.declared_symbols()
    header = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "ddamg_hip.h")).read())
    assert declaration in header
    # a comment in front of the declaration (or of the group it closes) names what it does
    assert re.search(r"\*/\s*(int ddamg_hip_[a-z0-9_]+\([^;]*;\s*)*" + re.escape(declaration), header)
    entry = getattr(lib, name)                       # AttributeError where the library does not export it
    types = argument_types(declaration)
    assert entry.argtypes == types and entry.restype == ctypes.c_int
    assert callable(getattr(api.Context, name[len("ddamg_hip_"):]))
    # a null context is an error with a message, not a crash
    assert entry(*[None if t in (vp, dp, ip) else t(0) for t in types]) != 0 and lib.ddamg_hip_last_error()


def test_squared_solves_return_both_iteration_pairs():
    """the mirror hands two-element arrays to every solve and reads both counts for the squared forms"""
    class Lib:
        def ddamg_hip_solve_squared_vec(self, h, x, b, tol, it, ci, rr):
            it[0], it[1], ci[0], ci[1] = 3, 4, 5, 6
            return 0

        def ddamg_hip_solve_dagger_vec(self, h, x, b, tol, it, ci, rr):
            it[0], ci[0] = 7, 8
            return 0

    class V:
        _h = None
    ctx = object.__new__(api.Context)
    ctx._lib, ctx._h = Lib(), None
    assert ctx.solve_squared_vec(V, V, 1e-9) == ((3, 4), (5, 6), 0.0)
    assert ctx.solve_dagger_vec(V, V, 1e-9) == (7, 8, 0.0)
