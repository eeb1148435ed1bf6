"""The fermion force at the boundary (no GPU needed): ddamg_hip_force_bilinear_vec, _device and ddamg_hip_force_logdet are declared
in include/ddamg_hip.h behind a comment, exported from the library and mirrored in the Python API with the argument types of the
declaration; a null context is an error, not a crash; the mirror passes its arguments in the order of the declaration; and the header
states the definition of the force and the left-multiplied variation."""
import ctypes, os, re
import pytest
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, dp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
C_TYPES = {"ddamg_hip_ctx*": vp, "const ddamg_hip_vec*": vp, "double*": dp, "const double*": dp, "double": ctypes.c_double, "int": ctypes.c_int}
ENTRY_POINTS = {
    "ddamg_hip_force_bilinear_vec": "int ddamg_hip_force_bilinear_vec(ddamg_hip_ctx* ctx, double* force_dev, const ddamg_hip_vec* y, "
                                    "const ddamg_hip_vec* x, double coeff, int accumulate);",
    "ddamg_hip_force_bilinear_device": "int ddamg_hip_force_bilinear_device(ddamg_hip_ctx* ctx, double* force_dev, const double* y_dev, "
                                       "const double* x_dev, double coeff, int accumulate);",
    "ddamg_hip_force_logdet": "int ddamg_hip_force_logdet(ddamg_hip_ctx* ctx, double* force_dev, int parity, double coeff, int accumulate);",
}


def header():
    return re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "ddamg_hip.h")).read())


def argument_types(declaration):
    """the ctypes of a declaration's parameters: the last word of each is its name"""
    return [C_TYPES[par.strip().rsplit(" ", 1)[0]] for par in declaration[declaration.index("(") + 1:declaration.rindex(")")].split(",")]


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
    assert declaration in header()
    # a comment in front of the declaration (or of the group it closes) names what it does
    assert re.search(r"\*/\s*(int ddamg_hip_[a-z0-9_]+\([^;]*;\s*)*" + re.escape(declaration), header())
    entry = getattr(lib, name)                       # AttributeError where the library does not export it
    types = argument_types(declaration)
    assert entry.argtypes == types and entry.restype == ctypes.c_int
    assert callable(getattr(api.Context, name[len("ddamg_hip_"):]))
    # a null context is an error with a message, not a crash
    assert entry(*[None if t in (vp, dp) else t(0) for t in types]) != 0 and b"null" in lib.ddamg_hip_last_error()


def test_the_header_states_the_definition():
    h = header()
    for phrase in ("W_mu(x) -> exp(eps Omega_mu(x)) W_mu(x)", "traceless anti-Hermitian: multiplication from the left",
                   "what D stores, times 2, with the anti-periodic sign in it", "d/d eps S |_{eps=0} = sum_{x,mu} tr( Omega_mu(x) G_mu(x) )",
                   "TA(M) = 1/2 (M - M^dagger) - 1/6 tr(M - M^dagger) 1", "[V][4][9] complex fp64", "S = Re <Y, D X>",
                   "F_mu_nu = (Q_mu_nu - Q_mu_nu^dagger) / 16", "log|det C(x)|", "force_dev (+)= coeff * G",
                   "a context on a process grid: not built yet", "did not come from ONE link field", "free of atomics"):
        assert phrase in h, phrase


class Recorder:
    """a library that records every call"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
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
    x, y = V("x"), V("y")
    addr = lambda a: ctypes.cast(a, vp).value
    assert ctx.force_bilinear_vec(1000, y, x, coeff=-2.0, accumulate=True) == 1000
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_force_bilinear_vec" and (a[0], addr(a[1])) + a[2:] == ("ctx", 1000, "y", "x", -2.0, 1)
    assert ctx.force_bilinear_device(1000, 2000, 3000, 0.5) == 1000
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_force_bilinear_device" and (a[0], addr(a[1]), addr(a[2]), addr(a[3])) + a[4:] == ("ctx", 1000, 2000, 3000, 0.5, 0)
    assert ctx.force_logdet(1000, 1, coeff=-2.0, accumulate=True) == 1000
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_force_logdet" and (a[0], addr(a[1])) + a[2:] == ("ctx", 1000, 1, -2.0, 1)
