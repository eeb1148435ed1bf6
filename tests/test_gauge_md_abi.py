"""The gauge sector at the boundary (no GPU needed): the six entry points are declared in include/ddamg_hip.h behind a comment,
exported from the library and mirrored in the Python API with the argument types of the declaration; a null context is an error, not
a crash; the mirror passes its arguments in the order of the declaration; and the header states the definitions."""
import ctypes, os, re
import pytest
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, dp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
C_TYPES = {"ddamg_hip_ctx*": vp, "double*": dp, "const double*": dp, "double": ctypes.c_double, "int": ctypes.c_int}
ENTRY_POINTS = {
    "ddamg_hip_gauge_loops_device": "int ddamg_hip_gauge_loops_device(ddamg_hip_ctx* ctx, const double* links_dev, double* plaquette_sum, "
                                    "double* rectangle_sum);",
    "ddamg_hip_gauge_force_device": "int ddamg_hip_gauge_force_device(ddamg_hip_ctx* ctx, double* force_dev, const double* links_dev, double beta, "
                                    "double c1, double coeff, int accumulate);",
    "ddamg_hip_links_update_device": "int ddamg_hip_links_update_device(ddamg_hip_ctx* ctx, double* links_dev, const double* mom_dev, double eps);",
    "ddamg_hip_links_reunitarize_device": "int ddamg_hip_links_reunitarize_device(ddamg_hip_ctx* ctx, double* links_dev, double* max_deviation);",
    "ddamg_hip_momentum_update_device": "int ddamg_hip_momentum_update_device(ddamg_hip_ctx* ctx, double* mom_dev, const double* force_dev, double eps);",
    "ddamg_hip_momentum_kinetic_device": "int ddamg_hip_momentum_kinetic_device(ddamg_hip_ctx* ctx, const double* mom_dev, double* kinetic);",
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


def test_the_header_states_the_definitions():
    h = header()
    for phrase in ("Gauge sector", "WITHOUT the anti-periodic sign", "there is no anti_pbc argument",
                   "S_g = beta sum_x [ c0 sum_{mu<nu} (1 - 1/3 Re tr P_mu_nu(x)) + c1 sum_{mu!=nu} (1 - 1/3 Re tr R_mu_nu(x)) ]", "c0 = 1 - 8 c1",
                   "6 plaquettes and 12 rectangles per site", "-1/12 tree-level Symanzik", "-0.331 Iwasaki",
                   "M_mu(x) = -(beta/3) U_mu(x) [ c0 sum(6 plaquette staples) + c1 sum(18 rectangle staples) ]",
                   "two plaquette staples and six rectangle staples", "each above and below", "dU/dt = P U, dP/dt = G", "U <- exp(eps P) U",
                   "H = 1/2 |P|^2 + S", "row 2 = conj(row 0 x row 1)", "P <- P + eps F", "1/2 sum |P_ij|^2", "two calls give the same bits",
                   "a context on a process grid: all six are refused there", "the _grid twins are not built yet"):
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


def test_the_mirror_passes_its_arguments_in_the_order_of_the_declaration():
    ctx = object.__new__(api.Context)
    ctx._lib, ctx._h = Recorder(), "ctx"
    p = api.Params()
    for mu in range(4):
        p.local_lattice[0][mu] = 2
    ctx.params = p
    addr = lambda a: ctypes.cast(a, vp).value
    assert ctx.gauge_loops_device(1000) == (0.0, 0.0)
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_gauge_loops_device" and (a[0], addr(a[1])) == ("ctx", 1000) and a[2] is not None and a[3] is not None
    assert ctx.gauge_loops_device(1000, rectangles=False) == (0.0, None)
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_gauge_loops_device" and a[2] is not None and a[3] is None
    assert ctx.gauge_force_device(1000, 2000, 5.6, -0.331, coeff=-2.0, accumulate=True) == 1000
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_gauge_force_device" and (a[0], addr(a[1]), addr(a[2])) + a[3:] == ("ctx", 1000, 2000, 5.6, -0.331, -2.0, 1)
    assert ctx.gauge_force_device(1000, 2000, 6.0) == 1000
    name, a = ctx._lib.calls.pop()
    assert a[3:] == (6.0, 0.0, 1.0, 0)
    assert ctx.links_update_device(2000, 3000, 0.125) == 2000
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_links_update_device" and (a[0], addr(a[1]), addr(a[2]), a[3]) == ("ctx", 2000, 3000, 0.125)
    assert ctx.links_reunitarize_device(2000) == 0.0
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_links_reunitarize_device" and (a[0], addr(a[1])) == ("ctx", 2000) and a[2] is not None
    assert ctx.momentum_update_device(3000, 1000, -0.25) == 3000
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_momentum_update_device" and (a[0], addr(a[1]), addr(a[2]), a[3]) == ("ctx", 3000, 1000, -0.25)
    assert ctx.momentum_kinetic_device(3000) == 0.0
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_momentum_kinetic_device" and (a[0], addr(a[1])) == ("ctx", 3000) and a[2] is not None
