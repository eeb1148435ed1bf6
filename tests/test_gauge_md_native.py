"""The kernel bodies of the gauge sector on the CPU (no GPU needed): tests/native/gauge_md_check.cpp runs stage_offsets, stage_links,
site_gauge_force and site_gauge_loops of csrc/gauge_md.h at both depths of the staged neighbourhood, force::site_assemble behind them,
and link_update, link_reunitarize, momentum_update and kinetic_part thread by thread, as the kernels of gauge_md.hip run them, on 4^4
(the tile is larger than the lattice and the two-deep neighbourhood wraps onto itself), 4x6x8x10 (four extents, tile tails) and
4x4x12x12 (two tiles in a direction) and compares every link's force with a brute-force loop over all plaquettes and rectangles of
the global lattice.  Built by the host compiler under -fsanitize=address,undefined, linked statically, and run as a child process,
as test_clover_force_native.py does."""
import os, shutil, subprocess
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gauge_md_bodies_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = next((c for c in ("c++", "g++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler with static sanitizer runtimes (c++ / g++)")
    csrc = os.path.join(REPO, "ddalphaamg_amd", "csrc")
    exe = tmp_path / "gauge_md_check"
    build = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", csrc, "-o", str(exe),
                            os.path.join(REPO, "tests", "native", "gauge_md_check.cpp")], capture_output=True, text=True)
    if build.returncode != 0 and ("libasan" in build.stderr or "libubsan" in build.stderr):
        pytest.skip("the host compiler has no static sanitizer runtimes: " + build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(run.stdout[-6000:])
    assert run.returncode == 0 and "GAUGE_MD_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    # three lattices, each with the loops and the force of three actions (c1 = 0 at both depths); then links, reunitarisation, momenta
    assert run.stdout.count(": ok") == 3 * 5 + 3
