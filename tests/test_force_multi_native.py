"""The kernel bodies of the many-pair fermion force on the CPU (no GPU needed): tests/native/force_multi_check.cpp runs
site_planes_multi and site_hop_multi of csrc/force.h thread by thread, as force_planes_multi_kernel and force_hop_multi_kernel of
force.hip run them, and compares with the weighted sum of what site_force_tensor writes pair by pair on the undivided lattice: 4^4 and
4x4x6x6 with 1, G, G + 1 and 2 G + 1 pairs (the write form, the add form and a last partial group), with and without a clover term,
and the GRID form with the faces of a whole group in one message on emulated 2x1x1x1 and 2x2x1x1 grids.  Bar: 1e-13 of the norm.
Built by the host compiler under -fsanitize=address,undefined, linked statically, and run as a child process, as
test_clover_force_native.py does.  Measured: 2.4e-16 to 3.0e-16."""
import os, shutil, subprocess
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_many_pair_bodies_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = next((c for c in ("c++", "g++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler with static sanitizer runtimes (c++ / g++)")
    csrc = os.path.join(REPO, "ddalphaamg_amd", "csrc")
    exe = tmp_path / "force_multi_check"
    build = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", csrc, "-o", str(exe),
                            os.path.join(REPO, "tests", "native", "force_multi_check.cpp")], capture_output=True, text=True)
    if build.returncode != 0 and ("libasan" in build.stderr or "libubsan" in build.stderr):
        pytest.skip("the host compiler has no static sanitizer runtimes: " + build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(run.stdout[-8000:])
    assert run.returncode == 0 and "FORCE_MULTI_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    # two lattices x two csw x four pair counts undivided; two grids x two csw x three cases
    assert run.stdout.count(": ok") == 2 * 2 * 4 + 2 * 2 * 3
