"""CPU tests of the 16-bit transfer storage's plumbing: DDAMG_TRANSFER_HALF in knobs.h (a host program that includes nothing
but that header, as tests/test_knobs.py builds it) and ddamg_hip_set_transfer_storage in the header, the library and the ctypes
mirror.  No GPU."""
import ctypes, os, shutil, subprocess
import pytest
import ddalphaamg_amd as dd
from ddalphaamg_amd import api

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "ddalphaamg_amd", "csrc")

PROBE = r"""
#include "knobs.h"
#include <cstdio>
int main() { printf("%d\n", (int)ddamg::Knobs::from_env().transfer_half); }
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("transfer_half")
    src = d / "probe.cpp"; exe = d / "probe"
    src.write_text(PROBE)
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [cxx] if cxx else [hipcc, "-x", "c++"]
    subprocess.run(cmd + ["-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    return lambda env: int(subprocess.run([str(exe)], env=env, check=True, capture_output=True, text=True).stdout)


def test_transfer_half_is_on_for_a_non_zero_integer_only(probe):
    assert probe({}) == 0
    assert probe({"DDAMG_TRANSFER_HALF": "1"}) == 1
    assert probe({"DDAMG_TRANSFER_HALF": "7"}) == 1
    assert probe({"DDAMG_TRANSFER_HALF": "0"}) == 0
    assert probe({"DDAMG_TRANSFER_HALF": ""}) == 0
    assert probe({"DDAMG_COARSE_HALF": "1"}) == 0


def test_entry_point_is_declared_exported_and_mirrored():
    assert "ddamg_hip_set_transfer_storage" in dd.declared_symbols()
    if not os.path.exists(dd.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    lib = api.load_library()
    assert lib.ddamg_hip_set_transfer_storage.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert hasattr(api.Context, "set_transfer_storage")
    # a null context is an error with a message, not a crash
    assert lib.ddamg_hip_set_transfer_storage(None, 16) != 0 and lib.ddamg_hip_last_error()
