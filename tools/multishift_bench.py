#!/usr/bin/env python3
"""tools/multishift_bench.py -- the multi-shift CG solve on Dhat^dagger Dhat + sigma_s and its update kernel, ONE process, ONE seeded
field, a one-level context.  Run it under a time limit:

  timeout -k 10 600 python tools/multishift_bench.py [--lattice 32] [--shifts 12] [--reps 5] [--out FILE.json]

  solve        iterations per shift, relres, Ritz values and seconds per ddamg_hip_solve_schur_multishift_device (host clock around
               the call, which ends in a synchronise): shifts geometric from 1e-4 to 10, tol 1e-10, rhs = seeded uniform numbers
  update       milliseconds per launch of multishift_update_kernel alone with all shifts active and with 4 active (the base system
               counts as one), between the context's timer events (ddamg_hip_multishift_update_time); bytes/s over the algorithmic
               traffic of (1 + 4 n_active) half fields of 12 V complex fp64 numbers, as a fraction of the 8 TB/s HBM peak the design
               notes normalise by
  axpy_chain   the same updates done with ddamg_hip_vec_axpy on full-length fp64 vectors with zeros on the odd sites, two launches per
               active shift (x_s += a p_s; p_s = r + b p_s), between the same timer events, in the same process: the cost without
               the kernel.  Its traffic is (1 + 5 n_active) FULL fields, twice the sites and one more read per shift
Every figure is the median over --reps measurements after one untimed one."""
import argparse, json, os, statistics, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tools"))
from device_interface_bench import hip_runtime, to_device  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=32)
    ap.add_argument("--block", type=int, default=4)
    ap.add_argument("--shifts", type=int, default=12)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--m0", type=float, default=-0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import synth
    import ddalphaamg_amd as dd
    from ddalphaamg_amd import api
    L = [a.lattice] * 4
    V = a.lattice ** 4
    p = api.default_params(); p.num_levels = 1
    for mu in range(4):
        p.local_lattice[0][mu] = L[mu]; p.block_lattice[0][mu] = a.block
    p.m0, p.csw, p.tol = a.m0, 1.0, a.tol
    ctx = dd.Context(p)
    hip = hip_runtime()
    U = synth.synth_gauge(L, 0.35, 20260101)
    ctx.set_gauge_device(to_device(hip, np.ascontiguousarray(U)), anti_pbc=True)
    del U
    shifts = [float(s) for s in np.geomspace(1e-4, 10.0, a.shifts)]
    half = V // 2 * 24
    rng = np.random.default_rng(7)
    db = to_device(hip, rng.uniform(-0.5, 0.5, half))
    xe = [to_device(hip, np.zeros(half)) for _ in shifts]
    res = {"lattice": L, "m0": a.m0, "shifts": shifts, "tol": a.tol}

    # the solve
    times = []
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        its, rr, ritz = ctx.solve_schur_multishift_device(shifts, xe, None, db)
        if r:
            times.append(time.perf_counter() - t0)
    res["solve"] = {"iterations": its, "relres": rr, "ritz": ritz, "seconds": statistics.median(times), "seconds_min_max": (min(times), max(times))}

    # the update kernel alone, and the same updates by vec_axpy on full-length vectors
    field = V // 2 * 12 * 16                       # bytes of a half field
    vr = ctx.vector(0, 64); vp = [ctx.vector(0, 64) for _ in shifts]; vx = [ctx.vector(0, 64) for _ in shifts]
    zero = np.zeros((V, 12, 2))
    for v in [vr] + vp + vx:
        v.upload(zero)
    res["update"], res["axpy_chain"] = {}, {}
    for nact in (a.shifts, 4):
        ms = [ctx.multishift_update_time(a.shifts, nact - 1, a.kernel_reps) for _ in range(a.reps + 1)][1:]
        t = statistics.median(ms) * 1e-3
        nbytes = (1 + 4 * nact) * field
        res["update"][nact] = {"ms_per_launch": t * 1e3, "ms_min_max": (min(ms), max(ms)), "algorithmic_bytes": nbytes, "bytes_per_s": nbytes / t,
                               "fraction_of_hbm_peak": nbytes / t / HBM_PEAK}
        chain = []
        for r in range(a.reps + 1):
            ctx.timer_begin()
            for _ in range(a.kernel_reps):
                for s in range(nact):
                    ctx.vec_axpy(vx[s], vx[s], vp[s], 0.5)
                    ctx.vec_axpy(vp[s], vr, vp[s], 0.5)
            dt = ctx.timer_end() / a.kernel_reps
            if r:
                chain.append(dt)
        tc = statistics.median(chain) * 1e-3
        res["axpy_chain"][nact] = {"ms_per_update": tc * 1e3, "ms_min_max": (min(chain), max(chain)), "launches": 2 * nact,
                                   "bytes_moved": (1 + 5 * nact) * 2 * field, "fused_over_chain": t / tc}
    for v in [vr] + vp + vx:
        v.free()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
