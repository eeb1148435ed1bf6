"""The collective force entry points at the boundary (no GPU needed): ddamg_hip_force_bilinear_vec_grid, _device_grid and
ddamg_hip_force_logdet_grid are declared in include/ddamg_hip.h behind a comment, exported from the library and mirrored in the Python
API with the argument types of the declaration; a null context is an error, not a crash; the mirror passes its arguments in the order
of the declaration; and the header says what travels and that a refusal comes before the first message."""
import ctypes
import pytest
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
from test_force_abi import Recorder, V, argument_types, header, lib, vp, dp  # noqa: F401  (lib: the fixture)

ENTRY_POINTS = {
    "ddamg_hip_force_bilinear_vec_grid": "int ddamg_hip_force_bilinear_vec_grid(ddamg_hip_ctx* ctx, double* force_dev, const ddamg_hip_vec* y, "
                                         "const ddamg_hip_vec* x, double coeff, int accumulate);",
    "ddamg_hip_force_bilinear_device_grid": "int ddamg_hip_force_bilinear_device_grid(ddamg_hip_ctx* ctx, double* force_dev, const double* y_dev, "
                                            "const double* x_dev, double coeff, int accumulate);",
    "ddamg_hip_force_logdet_grid": "int ddamg_hip_force_logdet_grid(ddamg_hip_ctx* ctx, double* force_dev, int parity, double coeff, int accumulate);",
}


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_entry_point_is_declared_exported_and_mirrored(lib, name):
    declaration = ENTRY_POINTS[name]
    assert name in dd.declared_symbols()
    assert declaration in header()
    entry = getattr(lib, name)                       # AttributeError where the library does not export it
    types = argument_types(declaration)
    assert entry.argtypes == types and entry.restype == ctypes.c_int
    assert callable(getattr(api.Context, name[len("ddamg_hip_"):]))
    # the twin without _grid takes the same arguments
    assert getattr(lib, name[:-len("_grid")]).argtypes == types
    # a null context is an error with a message, not a crash
    assert entry(*[None if t in (vp, dp) else t(0) for t in types]) != 0 and b"null" in lib.ddamg_hip_last_error()


def test_the_header_states_what_is_collective():
    h = header()
    for phrase in ("COLLECTIVE: every process of the grid calls them", "576 bytes per slab site", "432 bytes per slab site", "384 bytes per face site",
                   "is refused before the first message", "before any shell is sent", "process returns the same error", "they are the calls above, bit for bit"):
        assert phrase in h, phrase


def test_the_mirror_passes_its_arguments_in_the_order_of_the_declaration():
    ctx = object.__new__(api.Context)
    ctx._lib, ctx._h = Recorder(), "ctx"
    p = api.Params()
    for mu in range(4):
        p.local_lattice[0][mu] = 2
    ctx.params = p
    x, y = V("x"), V("y")
    addr = lambda a: ctypes.cast(a, vp).value
    assert ctx.force_bilinear_vec_grid(1000, y, x, coeff=-2.0, accumulate=True) == 1000
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_force_bilinear_vec_grid" and (a[0], addr(a[1])) + a[2:] == ("ctx", 1000, "y", "x", -2.0, 1)
    assert ctx.force_bilinear_device_grid(1000, 2000, 3000, 0.5) == 1000
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_force_bilinear_device_grid" and (a[0], addr(a[1]), addr(a[2]), addr(a[3])) + a[4:] == ("ctx", 1000, 2000, 3000, 0.5, 0)
    assert ctx.force_logdet_grid(1000, 1, coeff=-2.0, accumulate=True) == 1000
    name, a = ctx._lib.calls.pop()
    assert name == "ddamg_hip_force_logdet_grid" and (a[0], addr(a[1])) + a[2:] == ("ctx", 1000, 1, -2.0, 1)
