#!/usr/bin/env python3
"""tools/force_bench.py -- the three force entry points per call, ONE process, ONE seeded field, 4^4 blocks, csw = 1: the method of
the "Fermion force" table of docs/design/04_kernels.md.  Run it under a time limit:

  timeout -k 10 300 python tools/force_bench.py [--lattice 32] [--grid 0|1] [--calls 20] [--warmup 3] [--out FILE.json]

--grid 0: ddamg_hip_force_bilinear_vec / _device / _logdet on an undivided context.
--grid 1: the _grid forms on a context whose four process-grid entries are -1, so that the process is its own neighbour over RCCL
          and every shell travels through pack -> send/recv -> unpack; with the bytes sent per call (ddamg_hip_comm_stats).
Per entry point: milliseconds per call by the host clock around the call, which waits for its result; the median of --calls calls
after --warmup untimed ones, and the smallest and the largest.  Kernel times come from a run of this script under
`rocprofv3 --kernel-trace --stats`, a run of its own (--calls 8 is enough there)."""
import argparse, ctypes, json, os, statistics, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=32)
    ap.add_argument("--grid", type=int, default=0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import synth
    import ddalphaamg_amd as dd
    from ddalphaamg_amd import api
    n = a.lattice; L = [n] * 4; V = n ** 4
    p = api.default_params(); p.num_levels = 1
    for mu in range(4):
        p.local_lattice[0][mu] = n; p.block_lattice[0][mu] = 4
        p.process_grid[mu] = -1 if a.grid else 1
    p.m0, p.csw = -0.1, 1.0
    ctx = dd.Context(p)
    if a.grid:
        ctx.comm_init_rccl(api.rccl_unique_id())
    ctx.set_gauge(synth.synth_gauge(L, 0.35, 20260101), anti_pbc=True)
    hip = ctypes.CDLL(next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l))
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]

    def device(nbytes, src=None):
        ptr = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(ptr), nbytes) == 0
        if src is not None:
            assert hip.hipMemcpy(ptr.value, src.ctypes.data, nbytes, 1) == 0
        return ptr.value
    rng = np.random.default_rng(1)
    X = rng.uniform(-0.5, 0.5, (V, 12, 2)); Y = rng.uniform(-0.5, 0.5, (V, 12, 2))
    vx = ctx.vector(0, 64).upload(X); vy = ctx.vector(0, 64).upload(Y)
    dx = device(X.nbytes, X); dy = device(Y.nbytes, Y); out = device(V * 72 * 8)
    if a.grid:
        calls = {"ddamg_hip_force_bilinear_vec_grid": lambda: ctx.force_bilinear_vec_grid(out, vy, vx),
                 "ddamg_hip_force_bilinear_device_grid": lambda: ctx.force_bilinear_device_grid(out, dy, dx),
                 "ddamg_hip_force_logdet_grid": lambda: ctx.force_logdet_grid(out, 1)}
    else:
        calls = {"ddamg_hip_force_bilinear_vec": lambda: ctx.force_bilinear_vec(out, vy, vx),
                 "ddamg_hip_force_bilinear_device": lambda: ctx.force_bilinear_device(out, dy, dx),
                 "ddamg_hip_force_logdet": lambda: ctx.force_logdet(out, 1)}
    res = {"lattice": L, "grid": [-1] * 4 if a.grid else [1] * 4, "calls": a.calls, "warmup": a.warmup, "library": dd.library_path()}
    for name, fn in calls.items():
        ms = []
        for r in range(a.warmup + a.calls):
            if a.grid:
                ctx.comm_stats(reset=True)
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if r >= a.warmup:
                ms.append((t1 - t0) * 1e3)
        res[name] = {"ms": statistics.median(ms), "min": min(ms), "max": max(ms)}
        if a.grid:
            res[name]["device_sendrecv"] = ctx.comm_stats()["device_sendrecv"]
    vx.free(); vy.free()
    ctx.close()
    for ptr in (dx, dy, out):
        hip.hipFree(ptr)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
