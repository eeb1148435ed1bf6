"""The solves from a starting vector and the store of past solutions at the boundary (no GPU needed): declared in include/ddamg_hip.h
behind a comment, exported from the library, mirrored in the Python API with the argument types of the declaration, and an error -- not
a crash -- on a null context."""
import ctypes, os, re
import pytest
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, dp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
C_TYPES = {"ddamg_hip_ctx*": vp, "ddamg_hip_vec*": vp, "const ddamg_hip_vec*": vp, "ddamg_hip_chrono*": vp, "ddamg_hip_chrono**": ctypes.POINTER(vp),
           "double*": dp, "const double*": dp, "int*": ip, "double": ctypes.c_double, "int": ctypes.c_int}

GUESS = "double tol, int* iterations, int* coarse_iterations, double* relres, double* guess_relres);"
SQUARED = "double tol, int iterations[2], int coarse_iterations[2], double* relres);"
ENTRY_POINTS = {
    "ddamg_hip_solve_guess": "int ddamg_hip_solve_guess(ddamg_hip_ctx* ctx, int system, double* x_lex, const double* b_lex, " + GUESS,
    "ddamg_hip_solve_guess_vec": "int ddamg_hip_solve_guess_vec(ddamg_hip_ctx* ctx, int system, ddamg_hip_vec* x, const ddamg_hip_vec* b, " + GUESS,
    "ddamg_hip_solve_guess_device": "int ddamg_hip_solve_guess_device(ddamg_hip_ctx* ctx, int system, double* x_dev_lex, const double* b_dev_lex, " + GUESS,
    "ddamg_hip_chrono_create": "int ddamg_hip_chrono_create(ddamg_hip_ctx* ctx, int depth, ddamg_hip_chrono** h);",
    "ddamg_hip_chrono_destroy": "int ddamg_hip_chrono_destroy(ddamg_hip_ctx* ctx, ddamg_hip_chrono* h);",
    "ddamg_hip_chrono_reset": "int ddamg_hip_chrono_reset(ddamg_hip_ctx* ctx, ddamg_hip_chrono* h);",
    "ddamg_hip_chrono_count": "int ddamg_hip_chrono_count(ddamg_hip_ctx* ctx, ddamg_hip_chrono* h, int* n);",
    "ddamg_hip_chrono_push_vec": "int ddamg_hip_chrono_push_vec(ddamg_hip_ctx* ctx, ddamg_hip_chrono* h, const ddamg_hip_vec* x);",
    "ddamg_hip_chrono_guess_vec": "int ddamg_hip_chrono_guess_vec(ddamg_hip_ctx* ctx, ddamg_hip_chrono* h, int system, ddamg_hip_vec* x0, "
                                  "const ddamg_hip_vec* b, int* kept, double* predicted_relres);",
    "ddamg_hip_solve_chrono_vec": "int ddamg_hip_solve_chrono_vec(ddamg_hip_ctx* ctx, ddamg_hip_chrono* h, int system, ddamg_hip_vec* x, "
                                  "const ddamg_hip_vec* b, " + GUESS,
    "ddamg_hip_solve_chrono_device": "int ddamg_hip_solve_chrono_device(ddamg_hip_ctx* ctx, ddamg_hip_chrono* h, int system, double* x_dev_lex, "
                                     "const double* b_dev_lex, " + GUESS,
    "ddamg_hip_solve_squared_chrono_vec": "int ddamg_hip_solve_squared_chrono_vec(ddamg_hip_ctx* ctx, ddamg_hip_chrono* hy, ddamg_hip_chrono* hx, "
                                          "ddamg_hip_vec* x, const ddamg_hip_vec* b, " + SQUARED,
    "ddamg_hip_solve_squared_chrono_device": "int ddamg_hip_solve_squared_chrono_device(ddamg_hip_ctx* ctx, ddamg_hip_chrono* hy, ddamg_hip_chrono* hx, "
                                             "double* x_dev_lex, const double* b_dev_lex, " + SQUARED,
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


def test_the_thirteen_entry_points():
    assert len(ENTRY_POINTS) == 13


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
    # a null context is an error with a message, not a crash -- the destruction of no store included
    nulls = [t(0) if t in (ctypes.c_double, ctypes.c_int) else None for t in types]
    assert entry(*nulls) != 0 and b"null" in lib.ddamg_hip_last_error()


def test_the_header_says_what_the_residual_history_of_a_guessed_solve_is_relative_to():
    header = re.sub(r"\s+", " ", re.sub(r"\n \* ", "\n", open(os.path.join(REPO, "include", "ddamg_hip.h")).read()))
    comment = header[header.index("/* A solve that starts from the caller's vector"):header.index("int ddamg_hip_solve_guess(")]
    assert "ddamg_hip_residual_history" in comment and "relative to ||r0||" in comment


def test_the_mirror_passes_the_stores_and_reads_the_counts():
    """Chrono and the Context methods hand the store, the system and the vectors over in the order of the declaration; a store that is
    None becomes a null pointer"""
    seen = {}

    class Lib:
        def ddamg_hip_solve_chrono_vec(self, h, store, system, x, b, tol, it, ci, rr, gr):
            seen["chrono"] = (store, system, x, b, tol)
            it._obj.value, ci._obj.value, rr._obj.value, gr._obj.value = 3, 4, 0.5, 0.25
            return 0

        def ddamg_hip_solve_squared_chrono_vec(self, h, hy, hx, x, b, tol, it, ci, rr):
            seen["squared"] = (hy, hx, x, b)
            it[0], it[1], ci[0], ci[1] = 3, 4, 5, 6
            return 0

    class V:
        def __init__(self, h):
            self._h = h
    ctx = object.__new__(api.Context)
    ctx._lib, ctx._h = Lib(), None
    assert ctx.solve_chrono_vec(V("s"), V("x"), V("b"), 1e-9, system=1) == (3, 4, 0.5, 0.25)
    assert seen["chrono"] == ("s", 1, "x", "b", 1e-9)
    assert ctx.solve_squared_chrono_vec(None, V("hx"), V("x"), V("b"), 1e-9) == ((3, 4), (5, 6), 0.0)
    assert seen["squared"] == (None, "hx", "x", "b")
