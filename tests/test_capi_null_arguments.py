"""Every entry point of include/ddamg_hip.h that takes a context, called with a null context, null pointers and zeros (no GPU
needed): an error with a message, not a crash.  The list comes from the header, so a new entry point is covered the day it is
declared.  ddamg_hip_comm_stats takes a context too but returns a string, not a status: it answers "{}" and is not listed."""
import ctypes, os, re
import pytest
import ddalphaamg_amd as dd
from ddalphaamg_amd import api

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ddamg_hip.h")

# the only entry points that answer 0 to nulls, and why
RETURN_ZERO = {
    "ddamg_hip_destroy": "destroying no context is no error, as free(NULL)",
    "ddamg_hip_vec_destroy": "destroying no vector is no error, as free(NULL): the context is not looked at",
}


def context_taking_entry_points():
    """names of the functions declared as  int ddamg_hip_*(ddamg_hip_ctx* ...  in the header, comments removed as in declared_symbols()"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\bint\s+(ddamg_hip_[a-z0-9_]+)\s*\(\s*ddamg_hip_ctx\s*\*", txt)))


NAMES = context_taking_entry_points()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(dd.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return api.load_library()


def null_arguments(types):
    """a null for every pointer and callback, zero for every number"""
    numbers = (ctypes.c_int, ctypes.c_longlong, ctypes.c_double, ctypes.c_float, ctypes.c_size_t)
    return [t(0) if issubclass(t, numbers) else t() if issubclass(t, ctypes._CFuncPtr) else None for t in types]


def test_the_header_lists_the_context_taking_entry_points():
    assert len(NAMES) >= 64, NAMES
    assert set(NAMES) <= set(dd.declared_symbols()) and set(RETURN_ZERO) <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_null_context_and_null_pointers_are_an_error_not_a_crash(lib, name):
    entry = getattr(lib, name)
    assert entry.argtypes, f"{name}: api.load_library() sets no argument types"
    status = entry(*null_arguments(entry.argtypes))
    if name in RETURN_ZERO:
        assert status == 0, RETURN_ZERO[name]
    else:
        assert status != 0 and b"null" in lib.ddamg_hip_last_error()


def test_a_vector_without_a_context_is_not_destroyed(lib):
    """ddamg_hip_vec_destroy(NULL, v) is an error: the address is only compared with null before the context is required"""
    assert lib.ddamg_hip_vec_destroy(None, ctypes.c_void_p(4096)) != 0 and b"null context" in lib.ddamg_hip_last_error()
