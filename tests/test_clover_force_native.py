"""The kernel bodies of the fermion force on the CPU (no GPU needed): tests/native/clover_force_check.cpp runs site_force_tensor,
site_inverse_tensor, stage_tensor, site_clover_derivative and site_assemble of csrc/force.h thread by thread, as the kernels of
force.hip run them, on 4^4 (the tile is larger than the lattice), 4x6x8x10 (four extents, tile tails) and 4x4x12x12 (two tiles in a
direction) and compares every link's force with a brute-force loop over all leaves of the global lattice.  Built by the host
compiler under -fsanitize=address,undefined, linked statically, and run as a child process, as test_link_shell_native.py does."""
import os, shutil, subprocess
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_force_bodies_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = next((c for c in ("c++", "g++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler with static sanitizer runtimes (c++ / g++)")
    csrc = os.path.join(REPO, "ddalphaamg_amd", "csrc")
    exe = tmp_path / "clover_force_check"
    build = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", csrc, "-o", str(exe),
                            os.path.join(REPO, "tests", "native", "clover_force_check.cpp")], capture_output=True, text=True)
    if build.returncode != 0 and ("libasan" in build.stderr or "libubsan" in build.stderr):
        pytest.skip("the host compiler has no static sanitizer runtimes: " + build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(run.stdout[-6000:])
    assert run.returncode == 0 and "CLOVER_FORCE_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    # three lattices, each with the bilinear force with and without a clover term and the determinant force of both parities
    assert run.stdout.count(": ok") == 3 * 4
