"""CPU tests of the 16-bit intermediate storage's plumbing: DDAMG_INTERMEDIATE_HALF in knobs.h and the refusals of
ddamg_hip_set_intermediate_storage (intermediate_refusal.h) through a host program that includes nothing but those two headers,
as tests/test_knobs.py builds it; the entry point in the header, the library and the ctypes mirror.  No GPU."""
import ctypes, os, shutil, subprocess
import pytest
import ddalphaamg_amd as dd
from ddalphaamg_amd import api

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "ddalphaamg_amd", "csrc")

PROBE = r"""
#include "knobs.h"
#include "intermediate_refusal.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
  if (argc == 1) { printf("%d\n", (int)ddamg::Knobs::from_env().intermediate_half); return 0; }
  const char* why = ddamg::intermediate_half_refusal(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]) != 0);
  printf("%s\n", why ? why : "");
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("intermediate_half")
    src = d / "probe.cpp"; exe = d / "probe"
    src.write_text(PROBE)
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [cxx] if cxx else [hipcc, "-x", "c++"]
    subprocess.run(cmd + ["-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    return lambda env, *args: subprocess.run([str(exe)] + [str(a) for a in args], env=env, check=True, capture_output=True, text=True).stdout.strip()


def test_intermediate_half_is_on_for_a_non_zero_integer_only(probe):
    assert probe({}) == "0"
    assert probe({"DDAMG_INTERMEDIATE_HALF": "1"}) == "1"
    assert probe({"DDAMG_INTERMEDIATE_HALF": "7"}) == "1"
    assert probe({"DDAMG_INTERMEDIATE_HALF": "0"}) == "0"
    assert probe({"DDAMG_INTERMEDIATE_HALF": ""}) == "0"
    assert probe({"DDAMG_COARSE_HALF": "1"}) == "0"


def test_refusals(probe):
    """(num_levels, method, mixed_precision, an intermediate level decomposed over processes)"""
    for levels in (3, 4):
        for method in (1, 2, 3):
            for mp in (1, 2):
                assert probe({}, levels, method, mp, 0) == ""
    assert "three levels" in probe({}, 2, 2, 1, 0)
    assert "three levels" in probe({}, 1, 2, 1, 0)
    for method in (0, 4, 5):
        assert "method 1 to 3" in probe({}, 3, method, 1, 0)
    assert "mixed_precision" in probe({}, 3, 2, 0, 0)
    assert "one process" in probe({}, 3, 2, 1, 1)
    assert "one process" in probe({}, 4, 1, 2, 1)


def test_entry_point_is_declared_exported_and_mirrored():
    assert "ddamg_hip_set_intermediate_storage" in dd.declared_symbols()
    if not os.path.exists(dd.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    lib = api.load_library()
    assert lib.ddamg_hip_set_intermediate_storage.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert hasattr(api.Context, "set_intermediate_storage")
    # a null context is an error with a message, not a crash
    assert lib.ddamg_hip_set_intermediate_storage(None, 16) != 0 and lib.ddamg_hip_last_error()
    # the entry point consults the function that test_refusals checks
    src = open(os.path.join(CSRC, "capi.cpp")).read()
    body = src[src.index("int ddamg_hip_set_intermediate_storage("):]
    assert "intermediate_half_refusal(c)" in body[:body.index("DDAMG_API_END")]
    assert "ddamg::intermediate_half_refusal(c->par.num_levels, c->par.method, c->par.mixed_precision, decomposed)" in src
