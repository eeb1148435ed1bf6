"""The kernel bodies that take links in device memory on a process grid, on the CPU (no GPU needed): tests/native/link_shell_check.cpp
runs extend, pack, unpack and the extended stage_offsets / stage_links / site_field_strength of csrc/field_strength.h thread by thread
on emulated process grids and compares every factor a leaf reads with a brute-force periodic global lattice.  Built by the host
compiler under -fsanitize=address,undefined, as the LIME host code is (test_lime_formats.py)."""
import os, shutil, subprocess
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_link_shell_bodies_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = next((c for c in ("c++", "g++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler with static sanitizer runtimes (c++ / g++)")
    csrc = os.path.join(REPO, "ddalphaamg_amd", "csrc")
    exe = tmp_path / "link_shell_check"
    build = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", csrc, "-o", str(exe),
                            os.path.join(REPO, "tests", "native", "link_shell_check.cpp")], capture_output=True, text=True)
    if build.returncode != 0 and ("libasan" in build.stderr or "libubsan" in build.stderr):
        pytest.skip("the host compiler has no static sanitizer runtimes: " + build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(run.stdout[-6000:])
    assert run.returncode == 0 and "LINK_SHELL_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    # every case of the table ran, with and without the anti-periodic sign
    assert run.stdout.count(": ok") == 2 * 16
