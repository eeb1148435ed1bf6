#!/usr/bin/env python3
"""tools/transfer_half_bench.py -- the fine level's interpolation operator in 32- and in 16-bit storage
(ddamg_hip_set_transfer_storage) on the 32^4 two-level hierarchy of the committed profiles (4^4 aggregates, 24 test vectors),
timed with ddamg_hip_timer_* in ONE process.  Run it under a time limit:

  timeout -k 10 600 python tools/transfer_half_bench.py [--out FILE.json]

What is timed, each after warm-up launches, as the median over --reps brackets of --inner launches back to back, each storage
twice (32, 16, 32, 16) so that drift shows as a difference between the two passes:
  restrict     ddamg_hip_restrict of a fine vector.  The 32-bit figure is restrict_kernel<float, 1>, the kernel the fp32-storage
               solve runs; the 16-bit one restrict_half_kernel
  interpolate  ddamg_hip_interpolate, add = 0 and add = 1 (interpolate_kernel<float> / interpolate_half_kernel)
  solve        the 32^4 solve (rhs = ones, tol 1e-10) through solve_vec: wall time per solve, outer and coarse iterations
Algorithmic bytes per fine site: Nvec * 96 (fp32) or Nvec * 48 (16-bit) of P plus 96 of the fine vector (192 with add = 1: read
and written); coarse vector and scales are below 1 %.  The fraction of the HBM peak is these bytes over the time over 8 TB/s."""
import argparse, json, os, statistics, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tools"))

HBM_PEAK = 8.0e12


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
    ap.add_argument("--lattice", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.pop("DDAMG_TRANSFER_HALF", None); os.environ.pop("DDAMG_COARSE_HALF", None)
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
    nvec = n // 2
    rng = np.random.default_rng(7)
    vf = ctx.vector(0, 32).upload(rng.standard_normal((V, 12, 2))); vc = ctx.vector(1, 32).upload(rng.standard_normal((Vc, n, 2))); vr = ctx.vector(1, 32)
    bv = ctx.vector(0, 64).upload(np.stack([np.ones((V, 12)), np.zeros((V, 12))], axis=-1)); xv = ctx.vector(0, 64)
    res = {"lattice": L, "aggregate_sites": V // Vc, "nvec": nvec, "warmup": args.warmup, "reps": args.reps, "inner": args.inner, "hbm_peak": HBM_PEAK}
    for bits in (32, 16, 32, 16):
        ctx.set_transfer_storage(bits)
        p_bytes = nvec * 24 * (4 if bits == 32 else 2)
        r = {}
        for key, fn, vec_bytes in (("restrict", lambda: ctx.restrict(vr, vf), 96), ("interpolate", lambda: ctx.interpolate(vf, vc, add=False), 96),
                                   ("interpolate_add", lambda: ctx.interpolate(vf, vc, add=True), 192)):
            if key == "interpolate_add":
                vf.upload(np.zeros((V, 12, 2)))          # the sums of many add calls stay finite: c is fixed, the vector grows linearly
            med, lo, hi = median_ms(ctx, fn, args.warmup, args.reps, args.inner)
            nbytes = V * (p_bytes + vec_bytes)
            r[key + "_us"] = med * 1e3; r[key + "_us_min_max"] = [lo * 1e3, hi * 1e3]
            r[key + "_bytes"] = nbytes; r[key + "_fraction_of_hbm_peak"] = nbytes / (med * 1e-3) / HBM_PEAK
        vf.upload(rng.standard_normal((V, 12, 2)))
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
    res["ratio_16_over_32"] = {k: b[k] / a[k] for k in ("restrict_us", "interpolate_us", "interpolate_add_us", "solve_ms")}
    res["byte_model_ratio"] = {k: b[k] / a[k] for k in ("restrict_bytes", "interpolate_bytes", "interpolate_add_bytes")}
    print("measured 16/32:", json.dumps(res["ratio_16_over_32"]), "byte model:", json.dumps(res["byte_model_ratio"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    for v in (vf, vc, vr, bv, xv):
        v.free()
    ctx.close()


if __name__ == "__main__":
    main()
