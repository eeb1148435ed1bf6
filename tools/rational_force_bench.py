#!/usr/bin/env python3
"""tools/rational_force_bench.py -- the force of many pairs in one pass against the loop of single calls it replaces, ONE process, ONE
seeded field, 4^4 blocks, csw = 1: the method of the "Fermion force" table of docs/design/04_kernels.md (host clock around calls that
wait for their result, the median of --calls calls after --warmup untimed ones).  Run it under a time limit:

  timeout -k 10 300 python tools/rational_force_bench.py [--lattice 32] [--pairs 12] [--grid 0|1] [--calls 20] [--warmup 3] [--out FILE.json]

--grid 0, on an undivided context:
  (a) loop_bilinear_vec      the loop of --pairs ddamg_hip_force_bilinear_vec calls, accumulate = s > 0
  (b) bilinear_multi_vec     ddamg_hip_force_bilinear_multi_vec, and the ratio (a) / (b)
  (c) loop_recipe            per shift: schur_apply_device, schur_odd_part_device, four vec_upload_parity_device, force_bilinear_vec
  (d) rational_device        ddamg_hip_force_rational_device with the odd parts given, and the ratio (c) / (d)
--grid 1, (e): (b) and (d) through their _grid forms on a context whose four process-grid entries are -1, so that the process is its
  own neighbour over RCCL, with the messages and bytes per call (ddamg_hip_comm_stats).
The half fields of (c) and (d) are random numbers: the time does not depend on their values.  Kernel times come from a run of this
script under `rocprofv3 --kernel-trace --stats`, a run of its own (--calls 4 is enough there).  The group size of a build is
DDAMG_FORCE_GROUP of csrc/force.h; a library built with another one is measured through DDAMG_HIP_LIBRARY."""
import argparse, ctypes, json, os, statistics, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=12)
    ap.add_argument("--grid", type=int, default=0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated names of the measurements to run (default: all of the mode)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import synth
    import ddalphaamg_amd as dd
    from ddalphaamg_amd import api
    n = a.lattice; L = [n] * 4; V = n ** 4; N = a.pairs
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
    held = []

    def device(nbytes, src=None):
        ptr = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(ptr), nbytes) == 0
        if src is not None:
            assert hip.hipMemcpy(ptr.value, src.ctypes.data, nbytes, 1) == 0
        held.append(ptr.value)
        return ptr.value
    rng = np.random.default_rng(1)
    vys = [ctx.vector(0, 64).upload(rng.uniform(-0.5, 0.5, (V, 12, 2))) for _ in range(N)]
    vxs = [ctx.vector(0, 64).upload(rng.uniform(-0.5, 0.5, (V, 12, 2))) for _ in range(N)]
    xe = [device(V * 12 * 8, rng.uniform(-0.5, 0.5, (V // 2, 12, 2))) for _ in range(N)]
    xo = [device(V * 12 * 8, rng.uniform(-0.5, 0.5, (V // 2, 12, 2))) for _ in range(N)]
    ye, yo = device(V * 12 * 8), device(V * 12 * 8)
    vx, vy = ctx.vector(0, 64), ctx.vector(0, 64)
    out = device(V * 72 * 8)
    w = [(-1.0) ** s * (0.3 + 0.1 * s) for s in range(N)]

    def loop_bilinear():
        for s in range(N):
            ctx.force_bilinear_vec(out, vys[s], vxs[s], -2.0 * w[s], accumulate=s > 0)

    def loop_recipe():
        for s in range(N):
            ctx.schur_apply_device(ye, xe[s])
            ctx.schur_odd_part_device(yo, ye, dagger=True)
            ctx.vec_upload_parity_device(vx, 0, xe[s]); ctx.vec_upload_parity_device(vx, 1, xo[s], zero_other=False)
            ctx.vec_upload_parity_device(vy, 0, ye); ctx.vec_upload_parity_device(vy, 1, yo, zero_other=False)
            ctx.force_bilinear_vec(out, vy, vx, -2.0 * w[s], accumulate=s > 0)
    if a.grid:
        calls = {"bilinear_multi_vec_grid": lambda: ctx.force_bilinear_multi_vec_grid(out, vys, vxs, w, -2.0),
                 "rational_device_grid": lambda: ctx.force_rational_device_grid(out, w, xe, xo, -2.0)}
    else:
        calls = {"loop_bilinear_vec": loop_bilinear,
                 "bilinear_multi_vec": lambda: ctx.force_bilinear_multi_vec(out, vys, vxs, w, -2.0),
                 "loop_recipe": loop_recipe,
                 "rational_device": lambda: ctx.force_rational_device(out, w, xe, xo, -2.0)}
    if a.only:
        calls = {k: v for k, v in calls.items() if k in a.only.split(",")}
    res = {"lattice": L, "pairs": N, "group": api.FORCE_GROUP, "grid": [-1] * 4 if a.grid else [1] * 4, "calls": a.calls, "warmup": a.warmup,
           "library": dd.library_path()}
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
    if "loop_bilinear_vec" in res and "bilinear_multi_vec" in res:
        res["ratio_a_over_b"] = res["loop_bilinear_vec"]["ms"] / res["bilinear_multi_vec"]["ms"]
    if "loop_recipe" in res and "rational_device" in res:
        res["ratio_c_over_d"] = res["loop_recipe"]["ms"] / res["rational_device"]["ms"]
    for v in vys + vxs + [vx, vy]:
        v.free()
    ctx.close()
    for ptr in held:
        hip.hipFree(ptr)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
