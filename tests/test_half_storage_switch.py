"""CPU tests of the plumbing of the three 16-bit storage switches (coarse, transfer, intermediate): DDAMG_*_HALF in knobs.h and
the refusals of ddamg_hip_set_*_storage (storage_refusal.h) through one host program that includes nothing but those two headers,
as tests/test_knobs.py builds it; the entry points in the header, the library and the ctypes mirror.  No GPU."""
import ctypes, os, shutil, subprocess
import pytest
import ddalphaamg_amd as dd
from ddalphaamg_amd import api

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "ddalphaamg_amd", "csrc")
KINDS = ("coarse", "transfer", "intermediate")
ENV = {k: f"DDAMG_{k.upper()}_HALF" for k in KINDS}

# probe KIND: the knob as the environment sets it;  probe KIND integers...: the refusal for these parameters (empty: none)
PROBE = r"""
#include "knobs.h"
#include "storage_refusal.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
int main(int argc, char** argv) {
  const ddamg::Knobs k = ddamg::Knobs::from_env();
  const char kind = argv[1][0];
  if (argc == 2) { printf("%d\n", (int)(kind == 'c' ? k.coarse_half : kind == 't' ? k.transfer_half : k.intermediate_half)); return 0; }
  int a[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 2; i < argc && i < 8; i++) a[i - 2] = atoi(argv[i]);
  const char* why = kind == 'c' ? ddamg::coarse_half_refusal(a[0], a[1], a[2], a[3], a[4] != 0, a[5] != 0)
                  : kind == 't' ? ddamg::transfer_half_refusal(a[0], a[1], a[2])
                                : ddamg::intermediate_half_refusal(a[0], a[1], a[2], a[3] != 0);
  printf("%s\n", why ? why : "");
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("half_storage")
    src = d / "probe.cpp"; exe = d / "probe"
    src.write_text(PROBE)
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [cxx] if cxx else [hipcc, "-x", "c++"]
    subprocess.run(cmd + ["-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    return lambda env, *args: subprocess.run([str(exe)] + [str(a) for a in args], env=env, check=True, capture_output=True, text=True).stdout.strip()


@pytest.mark.parametrize("kind", KINDS)
def test_knob_is_on_for_a_non_zero_integer_only(probe, kind):
    assert probe({}, kind) == "0"
    assert probe({ENV[kind]: "1"}, kind) == "1"
    assert probe({ENV[kind]: "7"}, kind) == "1"
    assert probe({ENV[kind]: "0"}, kind) == "0"
    assert probe({ENV[kind]: ""}, kind) == "0"
    for other in [ENV[k] for k in KINDS if k != kind] + ["DDAMG_PIPELINED_ARNOLDI"]:
        assert probe({other: "1"}, kind) == "0"


def test_coarse_refusals(probe):
    """(num_levels, method, mixed_precision, odd_even, the coarsest level decomposed over processes, gather_coarsest)"""
    for levels in (2, 3, 4):
        for method in (1, 2, 3, 4):
            for mp in (1, 2):
                for decomposed, gathered in ((0, 0), (0, 1), (1, 1)):
                    assert probe({}, "coarse", levels, method, mp, 1, decomposed, gathered) == ""
    assert "odd_even = 1" in probe({}, "coarse", 2, 2, 1, 0, 0, 0)
    assert "one process" in probe({}, "coarse", 2, 2, 1, 1, 1, 0)
    assert "one process" in probe({}, "coarse", 3, 1, 2, 1, 1, 0)
    assert "mixed_precision" in probe({}, "coarse", 2, 2, 0, 1, 0, 0)
    assert "two levels" in probe({}, "coarse", 1, 2, 1, 1, 0, 0)
    for method in (-1, 0, 5):
        assert "method 1 to 4" in probe({}, "coarse", 2, method, 1, 1, 0, 0)
    # the first reason that applies is the one given: hierarchy, precision, odd-even, processes
    assert "two levels" in probe({}, "coarse", 1, 2, 0, 0, 1, 0)
    assert "mixed_precision" in probe({}, "coarse", 2, 2, 0, 0, 1, 0)
    assert "odd_even = 1" in probe({}, "coarse", 2, 2, 1, 0, 1, 0)


def test_transfer_refusals(probe):
    """(num_levels, method, mixed_precision)"""
    for levels in (2, 3, 4):
        for method in (1, 2, 3, 4):
            for mp in (1, 2):
                assert probe({}, "transfer", levels, method, mp) == ""
    assert "mixed_precision" in probe({}, "transfer", 2, 2, 0)
    assert "two levels" in probe({}, "transfer", 1, 2, 1)
    for method in (-1, 0, 5):
        assert "method 1 to 4" in probe({}, "transfer", 2, method, 1)
    assert "two levels" in probe({}, "transfer", 1, 2, 0)


def test_intermediate_refusals(probe):
    """(num_levels, method, mixed_precision, an intermediate level decomposed over processes)"""
    for levels in (3, 4):
        for method in (1, 2, 3):
            for mp in (1, 2):
                assert probe({}, "intermediate", levels, method, mp, 0) == ""
    assert "three levels" in probe({}, "intermediate", 2, 2, 1, 0)
    assert "three levels" in probe({}, "intermediate", 1, 2, 1, 0)
    for method in (0, 4, 5):
        assert "method 1 to 3" in probe({}, "intermediate", 3, method, 1, 0)
    assert "mixed_precision" in probe({}, "intermediate", 3, 2, 0, 0)
    assert "one process" in probe({}, "intermediate", 3, 2, 1, 1)
    assert "one process" in probe({}, "intermediate", 4, 1, 2, 1)


# what capi.cpp's storage_refusal hands to the function of storage_refusal.h that the tables above check
CONSULTS = {
    "coarse": "coarse_half_refusal(p.num_levels, p.method, p.mixed_precision, p.odd_even, c->levels.back()->geom.distributed(), p.gather_coarsest != 0)",
    "transfer": "transfer_half_refusal(p.num_levels, p.method, p.mixed_precision)",
    "intermediate": "intermediate_half_refusal(p.num_levels, p.method, p.mixed_precision, decomposed)",
}


@pytest.mark.parametrize("kind", KINDS)
def test_entry_point_is_declared_exported_and_mirrored(kind):
    name = f"ddamg_hip_set_{kind}_storage"
    assert name in dd.declared_symbols()
    if not os.path.exists(dd.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    lib = api.load_library()
    entry = getattr(lib, name)
    assert entry.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert hasattr(api.Context, f"set_{kind}_storage")
    # a null context is an error with a message, not a crash
    assert entry(None, 16) != 0 and lib.ddamg_hip_last_error()
    # the entry point consults the function that the refusal tables check: it is one call of set_storage with its kind, set_storage
    # asks storage_refusal before it changes anything, and storage_refusal calls the header's function for that kind
    src = open(os.path.join(CSRC, "capi.cpp")).read()
    assert f'int {name}(ddamg_hip_ctx* c, int bits) {{ return set_storage(c, {kind.capitalize()}, bits, "{kind}"); }}' in src
    helper = src[src.index("static const char* storage_refusal("):src.index("static int set_storage(")]
    assert f"if (kind == {kind.capitalize()}) return {CONSULTS[kind]};" in helper or f"  return {CONSULTS[kind]};" in helper
    body = src[src.index("static int set_storage("):]
    body = body[:body.index("DDAMG_API_END")]
    assert "storage_refusal(c, kind)" in body and body.index("storage_refusal(c, kind)") < body.index("set_storage(kind, bits)")
