"""The many-pair and rational force entry points at the boundary (no GPU needed): every new symbol is declared in
include/ddamg_hip.h behind a comment, exported from the library and mirrored in the Python API with the argument types of the
declaration; a null context is an error, not a crash; the mirror passes its arguments in the order of the declaration; the group size
of the header is the one of the kernels and of the Python API; and the header says what the calls compute, refuse and send."""
import ctypes, os, re
import pytest
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
from test_force_abi import Recorder, V, header, lib, vp, dp, REPO  # noqa: F401  (lib: the fixture)

C_TYPES = {"ddamg_hip_ctx*": vp, "double*": dp, "const double*": dp, "double": ctypes.c_double, "int": ctypes.c_int,
           "const ddamg_hip_vec* const*": ctypes.POINTER(vp), "const double* const*": ctypes.POINTER(dp)}
TAIL = {"vec": "const ddamg_hip_vec* const* y, const ddamg_hip_vec* const* x, const double* weights, double coeff, int accumulate);",
        "device": "const double* const* y_dev, const double* const* x_dev, const double* weights, double coeff, int accumulate);",
        "rational": "const double* rho, const double* const* x_e_dev, const double* const* x_o_dev, double coeff, int accumulate);"}
ENTRY_POINTS = {}
for sfx in ("", "_grid"):
    for form in ("vec", "device"):
        name = f"ddamg_hip_force_bilinear_multi_{form}{sfx}"
        ENTRY_POINTS[name] = f"int {name}(ddamg_hip_ctx* ctx, double* force_dev, int npairs, " + TAIL[form]
    name = f"ddamg_hip_force_rational_device{sfx}"
    ENTRY_POINTS[name] = f"int {name}(ddamg_hip_ctx* ctx, double* force_dev, int nshift, " + TAIL["rational"]


def argument_types(declaration):
    """the ctypes of a declaration's parameters: the last word of each is its name"""
    return [C_TYPES[par.strip().rsplit(" ", 1)[0]] for par in declaration[declaration.index("(") + 1:declaration.rindex(")")].split(",")]


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_entry_point_is_declared_exported_and_mirrored(lib, name):
    declaration = ENTRY_POINTS[name]
    assert name in dd.declared_symbols()
    assert declaration in header()
    # a comment in front of the declaration (or of the group it closes, behind the enum of that group) names what it does
    assert re.search(r"\*/\s*(enum \{[^}]*\};\s*)?(int ddamg_hip_[a-z0-9_]+\([^;]*;\s*)*" + re.escape(declaration), header())
    entry = getattr(lib, name)                       # AttributeError where the library does not export it
    types = argument_types(declaration)
    assert entry.argtypes == types and entry.restype == ctypes.c_int
    assert callable(getattr(api.Context, name[len("ddamg_hip_"):]))
    if name.endswith("_grid"):                       # the twin without _grid takes the same arguments
        assert getattr(lib, name[:-len("_grid")]).argtypes == types
    # a null context is an error with a message, not a crash
    assert entry(*[None if t not in (ctypes.c_int, ctypes.c_double) else t(0) for t in types]) != 0 and b"null" in lib.ddamg_hip_last_error()


def test_the_group_size_is_one_number():
    h = header()
    m = re.search(r"enum \{ DDAMG_HIP_MAX_FORCE_PAIRS = (\d+), DDAMG_HIP_FORCE_GROUP = (\d+) \};", h)
    assert m, "the enum of the many-pair force is not in the header"
    assert (int(m.group(1)), int(m.group(2))) == (api.MAX_FORCE_PAIRS, api.FORCE_GROUP) == (32, api.FORCE_GROUP)
    kernels = open(os.path.join(REPO, "ddalphaamg_amd", "csrc", "force.h")).read()
    assert re.search(r"#define DDAMG_FORCE_GROUP (\d+)", kernels).group(1) == m.group(2)
    assert "static_assert(DDAMG_HIP_FORCE_GROUP == force::GROUP" in open(os.path.join(REPO, "ddalphaamg_amd", "csrc", "capi.cpp")).read()
    assert 1 <= api.FORCE_GROUP <= 8


def test_the_header_states_what_the_calls_compute_refuse_and_send():
    h = header()
    for phrase in ("force_dev (+)= coeff * sum_s weights[s] * G(Y_s, X_s)", "in groups of DDAMG_HIP_FORCE_GROUP per launch", "ascending order",
                   "two calls give the same bits", "outside 1 .. DDAMG_HIP_MAX_FORCE_PAIRS", "a weight that is not finite", "overlaps force_dev",
                   "Inputs may repeat", "2 DDAMG_HIP_FORCE_GROUP full vectors", "ceil(npairs / DDAMG_HIP_FORCE_GROUP)", "384 bytes per face site and pair",
                   "sends 5 npairs", "refused before the first message", "they are the plain calls, bit for bit",
                   "X_s = (x_s, -D_oo^-1 D_oe x_s)", "Y_s = (Dhat x_s, -gamma5 D_oo^-1 D_oe gamma5 Dhat x_s)", "x_o_dev NULL, or entries NULL",
                   "without a lexicographic round trip"):
        assert phrase in h, phrase


def test_the_mirror_passes_its_arguments_in_the_order_of_the_declaration():
    ctx = object.__new__(api.Context)
    ctx._lib, ctx._h = Recorder(), "ctx"
    p = api.Params()
    for mu in range(4):
        p.local_lattice[0][mu] = 2
    ctx.params = p
    addr = lambda a: ctypes.cast(a, vp).value
    x0, x1, y0, y1 = V(11), V(12), V(21), V(22)
    for sfx in ("", "_grid"):
        assert getattr(ctx, "force_bilinear_multi_vec" + sfx)(1000, [y0, y1], [x0, x1], [0.3, -1.1], coeff=-2.0, accumulate=True) == 1000
        name, a = ctx._lib.calls.pop()
        assert name == "ddamg_hip_force_bilinear_multi_vec" + sfx and (a[0], addr(a[1]), a[2]) == ("ctx", 1000, 2)
        assert (list(a[3]), list(a[4]), list(a[5])) + a[6:] == ([21, 22], [11, 12], [0.3, -1.1], -2.0, 1)
        assert getattr(ctx, "force_bilinear_multi_device" + sfx)(1000, [2000, 2100], [3000, 3100], [0.3, -1.1], 0.5) == 1000
        name, a = ctx._lib.calls.pop()
        assert name == "ddamg_hip_force_bilinear_multi_device" + sfx and (a[0], addr(a[1]), a[2]) == ("ctx", 1000, 2)
        assert ([addr(q) for q in a[3]], [addr(q) for q in a[4]], list(a[5])) + a[6:] == ([2000, 2100], [3000, 3100], [0.3, -1.1], 0.5, 0)
        assert getattr(ctx, "force_rational_device" + sfx)(1000, [0.3, 1.1], [4000, 4100], [5000, None], coeff=-2.0, accumulate=True) == 1000
        name, a = ctx._lib.calls.pop()
        assert name == "ddamg_hip_force_rational_device" + sfx and (a[0], addr(a[1]), a[2], list(a[3])) == ("ctx", 1000, 2, [0.3, 1.1])
        assert ([addr(q) for q in a[4]], [addr(q) for q in a[5]]) + a[6:] == ([4000, 4100], [5000, None], -2.0, 1)
        getattr(ctx, "force_rational_device" + sfx)(1000, [0.3], [4000])
        assert ctx._lib.calls.pop()[1][5] is None                       # no odd parts: a null array
    with pytest.raises(api.DDAMGError):
        ctx.force_bilinear_multi_vec(1000, [y0], [x0, x1], [1.0, 1.0])
    with pytest.raises(api.DDAMGError):
        ctx.force_rational_device(1000, [1.0, 2.0], [4000])
