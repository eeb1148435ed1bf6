#!/usr/bin/env python3
"""tools/device_interface_bench.py -- the gauge field and the vectors taken from host memory against the same taken from device
memory, ONE process, ONE seeded field, ONE context per hierarchy.  Run it under a time limit:

  timeout -k 10 600 python tools/device_interface_bench.py --lattice 32 [--levels 2] [--reps 7] [--out FILE.json]

  set_gauge          seconds per ddamg_hip_set_gauge (host clock around the call, which ends in a synchronise): links up,
                     D and clover term down, both up again twice
  set_gauge_device   seconds per ddamg_hip_set_gauge_device on the same links in device memory
  field_strength     milliseconds per launch of field_strength_kernel alone, of the three device-path kernels together, and of the
                     host path's clover_kernel alone, on the same links between the context's timer events
                     (ddamg_hip_clover_kernel_time); GB/s of the field-strength kernel are the links read once and F written
                     (576 + 432 bytes per site) over its time
  solve              seconds per ddamg_hip_solve and per ddamg_hip_solve_device (rhs = ones, tol 1e-10) after one setup
  --grid T Z Y X     a process grid with entries 1 and -1 (-1: the process is its own neighbour in that direction, over RCCL;
                     -1 -1 -1 -1 is the full self-exchange): set_gauge against set_gauge_device_grid on the SAME context and
                     field, in alternation, then milliseconds per launch of field_strength_kernel on the extended lattice
                     (ddamg_hip_clover_kernel_time, which = 3); no solve leg
Every figure is the median over --reps calls after --warmup untimed ones, the two forms in alternation.  Device arrays come from
the HIP runtime the library is linked to."""
import argparse, ctypes, json, os, statistics, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tools"))


def hip_runtime():
    path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
    lib = ctypes.CDLL(path)
    lib.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.hipFree.argtypes = [ctypes.c_void_p]
    return lib


def to_device(hip, a):
    p = ctypes.c_void_p()
    if hip.hipMalloc(ctypes.byref(p), a.nbytes) != 0 or hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) != 0:
        raise SystemExit("hipMalloc / hipMemcpy failed")
    return p.value


def alternate(calls, warmup, reps):
    """median seconds of every call in `calls` (name -> function), taken in alternation"""
    t = {k: [] for k in calls}
    for r in range(warmup + reps):
        for k, fn in calls.items():
            t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
            if r >= warmup:
                t[k].append(dt)
    return {k: statistics.median(v) for k, v in t.items()}, {k: (min(v), max(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=32)
    ap.add_argument("--levels", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--grid", type=int, nargs=4, metavar=("T", "Z", "Y", "X"), help="process-grid entries, 1 or -1")
    ap.add_argument("--out")
    a = ap.parse_args()
    import synth
    import ddalphaamg_amd as dd
    from ddalphaamg_amd import api
    n = a.lattice; L = [n] * 4; V = n ** 4
    import bench   # the hierarchy, gauge generator and right-hand side of bench.py's solve legs
    p = bench.amg_params(api, L, a.levels, 0)
    if n >= 64:
        p.restart, p.max_restart = 10, 100
    U = synth.synth_gauge(L, bench.GAUGE_EPS, bench.GAUGE_SEED)
    if a.grid:
        if any(e not in (1, -1) for e in a.grid) or all(e == 1 for e in a.grid):
            raise SystemExit("--grid takes entries 1 and -1, at least one of them -1 (one process)")
        for mu in range(4):
            p.process_grid[mu] = a.grid[mu]
    ctx = dd.Context(p)
    hip = hip_runtime()
    dU = to_device(hip, U)
    res = {"lattice": L, "levels": a.levels}
    plaq = {}
    if a.grid:
        ctx.comm_init_rccl(api.rccl_unique_id())
        res["grid"] = a.grid
        med, spread = alternate({"set_gauge": lambda: plaq.__setitem__("host", ctx.set_gauge(U, anti_pbc=True)),
                                 "set_gauge_device_grid": lambda: plaq.__setitem__("device", ctx.set_gauge_device_grid(dU, anti_pbc=True))}, a.warmup, a.reps)
        res["set_gauge_s"] = med["set_gauge"]; res["set_gauge_device_grid_s"] = med["set_gauge_device_grid"]
        res["set_gauge_spread_s"] = spread
        res["plaquette"] = plaq
        for name in ("field_strength_extended_kernel_ms", "field_strength_extended_kernel_ms_again"):
            res[name], _ = ctx.clover_kernel_time(dU, 3, a.kernel_reps)
        res["comm"] = ctx.comm_stats().get("device_sendrecv")
        a.no_solve = True
    else:
        med, spread = alternate({"set_gauge": lambda: plaq.__setitem__("host", ctx.set_gauge(U, anti_pbc=True)),
                                 "set_gauge_device": lambda: plaq.__setitem__("device", ctx.set_gauge_device(dU, anti_pbc=True))}, a.warmup, a.reps)
        res["set_gauge_s"] = med["set_gauge"]; res["set_gauge_device_s"] = med["set_gauge_device"]
        res["set_gauge_spread_s"] = spread
        res["plaquette"] = plaq
        for which, name in ((0, "field_strength_kernel_ms"), (1, "clover_kernel_ms"), (2, "device_path_kernels_ms"), (0, "field_strength_kernel_ms_again"),
                            (1, "clover_kernel_ms_again")):
            res[name], _ = ctx.clover_kernel_time(dU, which, a.kernel_reps)
        res["field_strength_GBps"] = V * (576 + 432) / (res["field_strength_kernel_ms"] * 1e-3) / 1e9
    if not a.no_solve:
        ctx.set_gauge_device(dU, anti_pbc=True)
        ctx.setup(p.setup_iter[0])
        b = np.zeros((V, 12, 2)); b[..., 0] = 1.0
        x = np.empty_like(b)
        db = to_device(hip, b); dx = to_device(hip, x)
        its = {}
        med, spread = alternate({"solve": lambda: its.__setitem__("host", ctx.solve(b, 1e-10, out=x)[1:]),
                                 "solve_device": lambda: its.__setitem__("device", ctx.solve_device(dx, db, 1e-10))}, a.warmup, a.reps)
        res["solve_s"] = med["solve"]; res["solve_device_s"] = med["solve_device"]
        res["solve_spread_s"] = spread
        res["solve_iterations"] = its
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
