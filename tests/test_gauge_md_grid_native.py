"""The gauge sector on a process grid, on the CPU (no GPU needed): tests/native/gauge_md_grid_check.cpp emulates process grids on the
host.  Every emulated process cuts its part out of a periodic global field, builds the lattice extended by the neighbours' links at
depth 1 and at depth 2 with fs::extend_links and fs::slab_copy in the exchange order of ExtendedLinks::fill (the messages are memcpys
between the processes' buffers), and runs the extended forms of stage_offsets, stage_links, site_gauge_force and site_gauge_loops of
csrc/gauge_md.h thread by thread, force::site_assemble behind them.  Every link's force is compared with the brute-force loop over all
plaquettes and rectangles of the GLOBAL lattice and the summed loops with the global sums, at the bar of gauge_md_check.cpp (1e-13 of
the largest entry, 1e-13 V for the sums); the bytes of every message are compared with the formula of docs/design/06_multi_gpu.md,
and the whole extended array with the global lattice.

Grids on 4x4x8x12: 2,1,1,1 (local T = 2: the depth-2 shell is the whole neighbour), 1,1,2,2 (corners of the (Y, X) plane from the
diagonal process; wrapped and shell directions side by side) and 2,2,2,2; and 4x6x8x10 with every direction split and the process its
own neighbour (tile tails; the extended extents 10 and 14 open a second tile).  Actions c1 = 0 (depth 1), -1/12 and -0.331 (depth 2).
Built by the host compiler under -fsanitize=address,undefined, linked statically, and run as a child process, as
test_gauge_md_native.py does."""
import os, shutil, subprocess
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gauge_md_grid_bodies_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = next((c for c in ("c++", "g++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler with static sanitizer runtimes (c++ / g++)")
    csrc = os.path.join(REPO, "ddalphaamg_amd", "csrc")
    exe = tmp_path / "gauge_md_grid_check"
    build = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", csrc, "-o", str(exe),
                            os.path.join(REPO, "tests", "native", "gauge_md_grid_check.cpp")], capture_output=True, text=True)
    if build.returncode != 0 and ("libasan" in build.stderr or "libubsan" in build.stderr):
        pytest.skip("the host compiler has no static sanitizer runtimes: " + build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(run.stdout[-8000:])
    assert run.returncode == 0 and "GAUGE_MD_GRID_OK" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    # four grids, each: the shell at two depths, then the force and the loops of three actions
    assert run.stdout.count(": ok") == 4 * (2 + 2 * 3)
