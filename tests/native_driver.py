"""Starts a host program of tests/native/ -- blas_driver (one operation of blas.h / krylov.h per process) or transfer_driver
(operations of transfer.h / coarse_mg.h on one transfer object per process) -- and reads what it wrote.

A case is a directory: case.txt with "key value" lines and raw little-endian arrays <name>.bin; the driver answers with
out_<name>.bin.  Every invocation is a child process with a time limit.  A driver that died of a signal, aborted, or ran into
its time limit may have left the GPU in a bad state: from then on every later driver test of the session fails at once and
the driver is not started again.
"""
import os
import subprocess
import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "tests", "native")

_dead = None   # why the driver is not started any more


class DriverError(AssertionError):
    pass


class Result:
    def __init__(self, path, returncode, stderr):
        self.path, self.returncode, self.stderr = path, returncode, stderr

    def read(self, name, dtype):
        return np.fromfile(os.path.join(self.path, "out_" + name + ".bin"), dtype=dtype)


def run(path, scalars, arrays, timeout=60, expect_error=None, driver="blas_driver"):
    """Write the case into `path` (a fresh directory of the test), run the program `driver` once, return a Result.

    scalars: {key: value} for case.txt; arrays: {name: ndarray}, written as they are (dtype included).
    expect_error: a text the driver must refuse the case with (exit status 2, text on stderr); otherwise status 0 is required.
    """
    global _dead
    if _dead is not None:
        raise DriverError("the native driver is not started again in this session: " + _dead)
    program = os.path.join(NATIVE, driver)
    if not os.path.isfile(program):
        raise DriverError(f"tests/native/{driver} is not built (make -C ddalphaamg_amd/csrc)")
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "case.txt"), "w") as f:
        for k, v in scalars.items():
            f.write(f"{k} {v!r}\n" if isinstance(v, float) else f"{k} {v}\n")
    for name, a in arrays.items():
        np.ascontiguousarray(a).tofile(os.path.join(path, name + ".bin"))
    try:
        p = subprocess.run([program, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True)
    except subprocess.TimeoutExpired:
        _dead = f"a case ran into its time limit of {timeout} s ({scalars.get('op')})"
        raise DriverError(_dead)
    if p.returncode < 0 or p.returncode in (134, 139):
        _dead = f"the driver ended with status {p.returncode} ({scalars.get('op')}): {p.stderr[-500:]}"
        raise DriverError(_dead)
    if expect_error is not None:
        assert p.returncode == 2 and expect_error in p.stderr, f"expected a refusal with '{expect_error}', got status {p.returncode}: {p.stderr[-500:]}"
    elif p.returncode != 0:
        raise DriverError(f"the driver ended with status {p.returncode}: {p.stderr[-1000:]}")
    return Result(str(path), p.returncode, p.stderr)
