#!/usr/bin/env python3
"""tools/intermediate_half_bench.py -- the intermediate level's couplings in 32- and in 16-bit storage
(ddamg_hip_set_intermediate_storage) on the three-level hierarchy that bench.py --full times as three_level_48 (48^4, 4^4 then
2^4 aggregates, 24 / 28 test vectors: intermediate lattice 12^4, n = 48), ONE context, ONE setup, timed with ddamg_hip_timer_*
in ONE process.  Run it under a time limit:

  timeout -k 10 900 python tools/intermediate_half_bench.py [--lattice 48] [--out FILE.json]

What is timed on intermediate-level vectors, each after warm-up calls, as the median over --reps brackets of --inner calls, each
storage twice (32, 16, 32, 16) so that drift shows as a difference between the two passes:
  apply     the operator (ddamg_hip_coarse_apply: every link read once, five matrices per site, plus the finish pass)
  smoother  one smoother call as the V-cycle makes it (post_smooth_iter[1] cycles from a given start: residual updates and the
            fused block solver)
  kcycle    one K-cycle (ddamg_hip_kcycle: FGMRES on the operator, preconditioned by the level's V-cycle)
  solve     the whole solve (rhs = ones, tol 1e-10): wall time per solve, outer and coarse iterations
The fp32 figures are the kernels of coarse_op.hip.  GB/s of apply are the bytes of the couplings it reads (vectors, scales and
the backward products are about 2 %) over the time; the byte model says the 16-bit apply reads half of them."""
import argparse, json, os, statistics, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tools"))


def median_ms(ctx, fn, warmup, reps, inner):
    for _ in range(warmup):
        fn()
    ctx.sync()
    samples = []
    for _ in range(reps):
        ctx.timer_begin()
        for _ in range(inner):
            fn()
        samples.append(ctx.timer_end() / inner)
    return statistics.median(samples), min(samples), max(samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--solves", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for k in ("DDAMG_INTERMEDIATE_HALF", "DDAMG_COARSE_HALF", "DDAMG_TRANSFER_HALF"):
        os.environ.pop(k, None)
    import synth
    import ddalphaamg_amd as dd
    from ddalphaamg_amd import api
    from bench import amg_params, GAUGE_EPS, GAUGE_SEED
    L = [args.lattice] * 4
    q = amg_params(api, L, 3, 0)
    ctx = dd.Context(q)
    ctx.set_gauge(synth.synth_gauge(L, GAUGE_EPS, GAUGE_SEED, [1, 1, 1, 1], [0, 0, 0, 0]), anti_pbc=True)
    t0 = time.perf_counter(); ctx.setup(q.setup_iter[0]); ctx.sync()
    print(f"setup {time.perf_counter() - t0:.2f} s", flush=True)
    V, V1, n = ctx.volume(0), ctx.volume(1), ctx.ndof(1)
    nt = (n + 7) // 8
    coupling_bytes = {32: V1 * 5 * nt * nt * 64 * 8, 16: V1 * 5 * nt * nt * 64 * 4}
    cycles = int(q.post_smooth_iter[1])
    rng = np.random.default_rng(7)
    vi = ctx.vector(1, 32).upload(rng.standard_normal((V1, n, 2))); vo = ctx.vector(1, 32)
    start = rng.standard_normal((V1, n, 2)); ph = ctx.vector(1, 32).upload(start)
    bv = ctx.vector(0, 64).upload(np.stack([np.ones((V, 12)), np.zeros((V, 12))], axis=-1)); xv = ctx.vector(0, 64)
    res = {"lattice": L, "intermediate_lattice": [args.lattice // 4] * 4, "n": n, "smoother_cycles": cycles, "warmup": args.warmup, "reps": args.reps,
           "inner": args.inner, "coupling_bytes": coupling_bytes}
    for bits in (32, 16, 32, 16):
        ctx.set_intermediate_storage(bits)
        r = {}
        med, lo, hi = median_ms(ctx, lambda: ctx.coarse_apply(vo, vi), args.warmup, args.reps, args.inner)
        r["apply_us"] = med * 1e3; r["apply_us_min_max"] = [lo * 1e3, hi * 1e3]; r["apply_GBps"] = coupling_bytes[bits] / (med * 1e-3) / 1e9
        med, lo, hi = median_ms(ctx, lambda: ctx.smoother(ph, vi, cycles, initial_guess_zero=False), args.warmup, args.reps, args.inner)
        r["smoother_us"] = med * 1e3; r["smoother_us_min_max"] = [lo * 1e3, hi * 1e3]
        ph.upload(start)
        its = []
        med, lo, hi = median_ms(ctx, lambda: its.append(ctx.kcycle(vo, vi)), 2, max(5, args.reps // 3), 1)
        r["kcycle_us"] = med * 1e3; r["kcycle_us_min_max"] = [lo * 1e3, hi * 1e3]; r["kcycle_iterations"] = its[-1]
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
    res["ratio_16_over_32"] = {k: b[k] / a[k] for k in ("apply_us", "smoother_us", "kcycle_us", "solve_ms")}
    print(json.dumps(res["ratio_16_over_32"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    for v in (vi, vo, ph, bv, xv):
        v.free()
    ctx.close()


if __name__ == "__main__":
    main()
