#!/usr/bin/env python3
"""tools/coarse_half_bench.py -- the coarsest level's couplings in 32- and in 16-bit storage (ddamg_hip_set_coarse_storage) on
the 32^4 two-level hierarchy of the committed profiles (4^4 aggregates, 24 test vectors: coarsest lattice 8^4, n = 48), timed
with ddamg_hip_timer_* in ONE process.  Run it under a time limit:

  timeout -k 10 600 python tools/coarse_half_bench.py [--out FILE.json]

What is timed, each after warm-up launches, as the median over --reps brackets of --inner launches (the kernels
behind a plug of queued launches, so that they run back to back), each storage twice (32, 16,
32, 16) so that drift shows as a difference between the two passes:
  hop       a half hopping term (ddamg_hip_coarse_hop onto the odd sites: the eight couplings of 2048 sites read once).  The
            32-bit figure is coarse_site_kernel's hopping-term instantiation, the kernel the fp32-storage solve runs
  self_mul  the self-coupling product on one parity (ddamg_hip_coarse_self_mul), and its inverse form
  schur     one coarsest odd-even solve per iteration (two half hopping terms and two self_mul, plus the Arnoldi step)
  solve     the 32^4 solve (rhs = ones, tol 1e-10): wall time per solve, outer and coarse iterations
GB/s are the bytes of the couplings a launch reads (vectors and scales are about 1 %) over the time."""
import argparse, json, os, statistics, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tools"))


def median_ms(ctx, fn, warmup, reps, inner, plug=None):
    """plug: launches queued in front of every bracket, so that the host is ahead of the device when the first event is reached
    and the timed launches run back to back (a 10 us kernel is shorter than the host's way to its launch)"""
    for _ in range(warmup):
        fn()
    ctx.sync()
    samples = []
    for _ in range(reps):
        for _ in range(40 if plug else 0):
            plug()
        ctx.timer_begin()
        for _ in range(inner):
            fn()
        samples.append(ctx.timer_end() / inner)
    return statistics.median(samples), min(samples), max(samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.pop("DDAMG_COARSE_HALF", None)
    import synth
    import ddalphaamg_amd as dd
    from ddalphaamg_amd import api
    from bench import amg_params, GAUGE_EPS, GAUGE_SEED
    L = [args.lattice] * 4
    q = amg_params(api, L, 2, 0)
    ctx = dd.Context(q)
    ctx.set_gauge(synth.synth_gauge(L, GAUGE_EPS, GAUGE_SEED, [1, 1, 1, 1], [0, 0, 0, 0]), anti_pbc=True)
    t0 = time.perf_counter(); ctx.setup(q.setup_iter[0]); ctx.sync()
    print(f"setup {time.perf_counter() - t0:.2f} s", flush=True)
    V, Vc, n = ctx.volume(0), ctx.volume(1), ctx.ndof(1)
    nt = (n + 7) // 8
    matrix_bytes = {32: nt * nt * 64 * 8, 16: nt * nt * 64 * 4}
    rng = np.random.default_rng(7)
    vi = ctx.vector(1, 32).upload(rng.standard_normal((Vc, n, 2))); vo = ctx.vector(1, 32)
    bv = ctx.vector(0, 64).upload(np.stack([np.ones((V, 12)), np.zeros((V, 12))], axis=-1)); xv = ctx.vector(0, 64)
    res = {"lattice": L, "coarse_lattice": [args.lattice // 4] * 4, "n": n, "warmup": args.warmup, "reps": args.reps, "inner": args.inner}
    for bits in (32, 16, 32, 16):
        ctx.set_coarse_storage(bits)
        r = {}
        for key, fn, nmat in (("hop", lambda: ctx.coarse_hop(vo, vi, 1, -1.0, False), 8), ("self_mul", lambda: ctx.coarse_self_mul(vo, vi, 0, False), 1),
                              ("self_mul_inverse", lambda: ctx.coarse_self_mul(vo, vi, 1, True), 1)):
            med, lo, hi = median_ms(ctx, fn, args.warmup, args.reps, args.inner, plug=lambda: ctx.coarse_hop(vo, vi, 1, -1.0, False))
            r[key + "_us"] = med * 1e3; r[key + "_us_min_max"] = [lo * 1e3, hi * 1e3]
            r[key + "_GBps"] = nmat * (Vc // 2) * matrix_bytes[bits] / (med * 1e-3) / 1e9
        its = []
        med, lo, hi = median_ms(ctx, lambda: its.append(ctx.coarse_solve(vo, vi)), 3, max(5, args.reps // 3), 1)
        r["coarsest_solve_ms"] = med; r["coarsest_solve_iterations"] = its[-1]; r["schur_us_per_iteration"] = med * 1e3 / max(its[-1], 1)
        ctx.solve_vec(xv, bv, 1e-10)                                    # warm-up
        walls = []
        for _ in range(args.solves):
            ctx.sync(); t0 = time.perf_counter(); it, cit, rr = ctx.solve_vec(xv, bv, 1e-10); walls.append(time.perf_counter() - t0)
        r["solve_ms"] = statistics.median(walls) * 1e3; r["solve_ms_min_max"] = [min(walls) * 1e3, max(walls) * 1e3]
        r["iterations"], r["coarse_iterations"], r["true_relres"] = it, cit, rr
        r["device_bytes"] = api.memory_in_use()[0]
        res.setdefault(f"storage_{bits}", []).append(r)
        print(bits, json.dumps(r), flush=True)
    a, b = res["storage_32"][-1], res["storage_16"][-1]
    res["ratio_16_over_32"] = {k: b[k] / a[k] for k in ("hop_us", "self_mul_us", "self_mul_inverse_us", "schur_us_per_iteration", "coarsest_solve_ms", "solve_ms")}
    print(json.dumps(res["ratio_16_over_32"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    for v in (vi, vo, bv, xv):
        v.free()
    ctx.close()


if __name__ == "__main__":
    main()
