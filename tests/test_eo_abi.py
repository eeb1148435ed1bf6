"""The even-odd preconditioned system at the boundary (no GPU needed): half-field upload / download, the Schur complement, its
solves and log det D_ss are declared in include/ddamg_hip.h, exported from the library and mirrored in the Python API with the
argument types of the declaration; a null context is an error, not a crash; the mirror passes its arguments in the order of the
declaration; and the half-field index lex >> 1 is a bijection of the sites of one parity."""
import ctypes, os, re
import numpy as np
import pytest
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, dp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
C_TYPES = {"ddamg_hip_ctx*": vp, "ddamg_hip_vec*": vp, "const ddamg_hip_vec*": vp, "double*": dp, "const double*": dp, "int*": ip,
           "double": ctypes.c_double, "int": ctypes.c_int}

SOLVE = "double tol, int* iterations, int* coarse_iterations, double* relres);"
SQUARED = "double tol, int iterations[2], int coarse_iterations[2], double* relres);"
ENTRY_POINTS = {
    "ddamg_hip_vec_upload_parity_device": "int ddamg_hip_vec_upload_parity_device(ddamg_hip_ctx* ctx, ddamg_hip_vec* v, int parity, const double* half_dev, int zero_other);",
    "ddamg_hip_vec_download_parity_device": "int ddamg_hip_vec_download_parity_device(ddamg_hip_ctx* ctx, const ddamg_hip_vec* v, int parity, double* half_dev);",
    "ddamg_hip_schur_apply": "int ddamg_hip_schur_apply(ddamg_hip_ctx* ctx, ddamg_hip_vec* out, const ddamg_hip_vec* in, int dagger);",
    "ddamg_hip_schur_apply_device": "int ddamg_hip_schur_apply_device(ddamg_hip_ctx* ctx, double* out_e_dev, const double* in_e_dev, int dagger);",
    "ddamg_hip_solve_schur_vec": "int ddamg_hip_solve_schur_vec(ddamg_hip_ctx* ctx, int dagger, int use_guess, ddamg_hip_vec* x, const ddamg_hip_vec* b, " + SOLVE,
    "ddamg_hip_solve_schur_device": "int ddamg_hip_solve_schur_device(ddamg_hip_ctx* ctx, int dagger, int use_guess, double* x_e_dev, double* x_o_dev, "
                                    "const double* b_e_dev, " + SOLVE,
    "ddamg_hip_solve_schur_squared_vec": "int ddamg_hip_solve_schur_squared_vec(ddamg_hip_ctx* ctx, ddamg_hip_vec* x, const ddamg_hip_vec* b, " + SQUARED,
    "ddamg_hip_solve_schur_squared_device": "int ddamg_hip_solve_schur_squared_device(ddamg_hip_ctx* ctx, double* x_e_dev, double* x_o_dev, "
                                            "const double* b_e_dev, " + SQUARED,
    "ddamg_hip_clover_logdet": "int ddamg_hip_clover_logdet(ddamg_hip_ctx* ctx, int parity, double* log_abs_det, int* sign);",
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


def test_the_header_states_the_conventions():
    header = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "ddamg_hip.h")).read())
    for phrase in ("(t+z+y+x) mod 2 of its GLOBAL coordinates", "a local lattice extent is odd", "half index = lexicographic index >> 1",
                   "Dhat = D_ee - D_eo D_oo^-1 D_oe", "Dhat^dagger = gamma5 Dhat gamma5"):
        assert phrase in header, phrase


class Recorder:
    """a library that records every call and fills the outputs of the solves"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            if name.startswith("ddamg_hip_solve_schur"):
                it, ci = args[-3], args[-2]
                it[0], it[1], ci[0], ci[1] = 3, 4, 5, 6
            return 0
        return call


class V:
    def __init__(self, h):
        self._h = h


def test_the_mirror_passes_its_arguments_in_the_order_of_the_declaration():
    ctx = object.__new__(api.Context)
    ctx._lib, ctx._h = Recorder(), "ctx"
    p = api.Params()
    for mu in range(4):
        p.local_lattice[0][mu] = 2
    ctx.params = p
    x, b = V("x"), V("b")
    addr = lambda a: ctypes.cast(a, vp).value if a is not None else None
    ctx.schur_apply(x, b, dagger=True)
    assert ctx._lib.calls.pop() == ("ddamg_hip_schur_apply", ("ctx", "x", "b", 1))
    ctx.schur_apply_device(1000, 2000, dagger=False)
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_schur_apply_device" and (a[0], addr(a[1]), addr(a[2]), a[3]) == ("ctx", 1000, 2000, 0)
    assert ctx.solve_schur_vec(x, b, 1e-9, dagger=True, use_guess=False) == (3, 5, 0.0)
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_solve_schur_vec" and a[:6] == ("ctx", 1, 0, "x", "b", 1e-9) and len(a) == 9
    assert ctx.solve_schur_vec(x, b, 1e-9, dagger=False, use_guess=True) == (3, 5, 0.0)
    assert ctx._lib.calls.pop()[1][1:3] == (0, 1)
    assert ctx.solve_schur_device(1000, None, 3000, 1e-8, dagger=True) == (3, 5, 0.0)
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_solve_schur_device" and (a[0], a[1], a[2], addr(a[3]), a[4], addr(a[5]), a[6]) == ("ctx", 1, 0, 1000, None, 3000, 1e-8)
    assert ctx.solve_schur_squared_vec(x, b, 1e-9) == ((3, 4), (5, 6), 0.0)
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_solve_schur_squared_vec" and a[:4] == ("ctx", "x", "b", 1e-9) and len(a) == 7
    assert ctx.solve_schur_squared_device(1000, 2000, 3000, 1e-9) == ((3, 4), (5, 6), 0.0)
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_solve_schur_squared_device" and (a[0], addr(a[1]), addr(a[2]), addr(a[3]), a[4]) == ("ctx", 1000, 2000, 3000, 1e-9)
    assert ctx.clover_logdet(1) == (0.0, 0)
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_clover_logdet" and a[:2] == ("ctx", 1) and len(a) == 4
    vec = object.__new__(api.Vector)
    vec.ctx, vec._h, vec.V, vec.ndof = ctx, "v", 16, 12
    vec.upload_parity_device(1, 1000, zero_other=False)
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_vec_upload_parity_device" and (a[0], a[1], a[2], addr(a[3]), a[4]) == ("ctx", "v", 1, 1000, 0)
    vec.download_parity_device(0, 2000)
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_vec_download_parity_device" and (a[0], a[1], a[2], addr(a[3])) == ("ctx", "v", 0, 2000)


def test_half_index_is_a_bijection_of_each_parity():
    """4x6x8x10 (T,Z,Y,X; X fastest, every extent even): the sites of one parity, taken in lexicographic order, have the half
    indices 0, 1, 2, ... = lex >> 1, and the two sites 2k, 2k+1 of a pair differ in parity"""
    L = [4, 6, 8, 10]
    V = int(np.prod(L))
    t, z, y, x = np.meshgrid(*[np.arange(n) for n in L], indexing="ij")
    lex = ((t * L[1] + z) * L[2] + y) * L[3] + x
    assert np.array_equal(lex.ravel(), np.arange(V))
    parity = ((t + z + y + x) % 2).ravel()
    for par in (0, 1):
        sites = np.flatnonzero(parity == par)
        assert np.array_equal(sites >> 1, np.arange(V // 2))
    assert np.all(parity[0::2] != parity[1::2])
