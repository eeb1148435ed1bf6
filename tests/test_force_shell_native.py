"""The kernel bodies of the force on a process grid, on the CPU (no GPU needed): tests/native/force_shell_check.cpp runs the tensor
slab pack / unpack of csrc/force.h and the extended stage_offsets / stage_links / stage_tensor / site_clover_derivative thread by thread
on emulated process grids (2x1x1x1, 1x1x1x2, 2x2x1x1, 2x2x2x2 and the process as its own neighbour; local lattices with tile tails and
with an extent of 2).  Every real of A that is staged for a site, the corners included, must be the one the periodic global lattice
holds there, and the derivative of every site must have the bits the same bodies give on the undivided lattice.  Built by the host
compiler under -fsanitize=address,undefined and run directly, as link_shell_check.cpp is (test_link_shell_native.py)."""
import os, shutil, subprocess
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = 15


def test_force_shell_bodies_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = next((c for c in ("c++", "g++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler with static sanitizer runtimes (c++ / g++)")
    csrc = os.path.join(REPO, "ddalphaamg_amd", "csrc")
    exe = tmp_path / "force_shell_check"
    build = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", csrc, "-o", str(exe),
                            os.path.join(REPO, "tests", "native", "force_shell_check.cpp")], capture_output=True, text=True)
    if build.returncode != 0 and ("libasan" in build.stderr or "libubsan" in build.stderr):
        pytest.skip("the host compiler has no static sanitizer runtimes: " + build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(run.stdout[-6000:])
    assert run.returncode == 0 and "FORCE_SHELL_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    assert run.stdout.count(": ok") == CASES       # every case of the table ran
