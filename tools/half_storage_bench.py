#!/usr/bin/env python3
"""tools/half_storage_bench.py -- one of the operators the solve streams in 32- and in 16-bit storage, ONE context, ONE setup,
timed with ddamg_hip_timer_* in ONE process.  Run it under a time limit:

  timeout -k 10 600 python tools/half_storage_bench.py --which coarse [--out FILE.json]
  timeout -k 10 600 python tools/half_storage_bench.py --which transfer [--out FILE.json]
  timeout -k 10 900 python tools/half_storage_bench.py --which intermediate [--lattice 48] [--out FILE.json]

Every figure is taken after warm-up calls, as the median over --reps brackets of --inner calls back to back, each storage twice
(32, 16, 32, 16) so that drift shows as a difference between the two passes.  All three end with
  solve     the whole solve (rhs = ones, tol 1e-10) through solve_vec: wall time per solve, outer and coarse iterations

--which coarse: the coarsest level's couplings (ddamg_hip_set_coarse_storage) on the 32^4 two-level hierarchy of the committed
profiles (4^4 aggregates, 24 test vectors: coarsest lattice 8^4, n = 48).  The kernels run behind a plug of queued launches, so
that they run back to back.
  hop       a half hopping term (ddamg_hip_coarse_hop onto the odd sites: the eight couplings of 2048 sites read once).  The
            32-bit figure is coarse_site_kernel's hopping-term instantiation, the kernel the fp32-storage solve runs
  self_mul  the self-coupling product on one parity (ddamg_hip_coarse_self_mul), and its inverse form
  schur     one coarsest odd-even solve per iteration (two half hopping terms and two self_mul, plus the Arnoldi step)
GB/s are the bytes of the couplings a launch reads (vectors and scales are about 1 %) over the time.

--which transfer: the fine level's interpolation operator (ddamg_hip_set_transfer_storage) on the same hierarchy.
  restrict     ddamg_hip_restrict of a fine vector.  The 32-bit figure is restrict_kernel<float, 1>, the kernel the fp32-storage
               solve runs; the 16-bit one restrict_half_kernel
  interpolate  ddamg_hip_interpolate, add = 0 and add = 1 (interpolate_kernel<float> / interpolate_half_kernel)
Algorithmic bytes per fine site: Nvec * 96 (fp32) or Nvec * 48 (16-bit) of P plus 96 of the fine vector (192 with add = 1: read
and written); coarse vector and scales are below 1 %.  The fraction of the HBM peak is these bytes over the time over 8 TB/s.

--which intermediate: the intermediate level's couplings (ddamg_hip_set_intermediate_storage) on the three-level hierarchy that
bench.py --full times as three_level_48 (48^4, 4^4 then 2^4 aggregates, 24 / 28 test vectors: intermediate lattice 12^4, n = 48),
on intermediate-level vectors.
  apply     the operator (ddamg_hip_coarse_apply: every link read once, five matrices per site, plus the finish pass)
  smoother  one smoother call as the V-cycle makes it (post_smooth_iter[1] cycles from a given start: residual updates and the
            fused block solver)
  kcycle    one K-cycle (ddamg_hip_kcycle: FGMRES on the operator, preconditioned by the level's V-cycle)
The fp32 figures are the kernels of coarse_op.hip.  GB/s of apply are the bytes of the couplings it reads (vectors, scales and
the backward products are about 2 %) over the time; the byte model says the 16-bit apply reads half of them."""
import argparse, json, os, statistics, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tools"))

HBM_PEAK = 8.0e12
#           levels and the defaults of --lattice, --warmup, --reps, --inner, --solves
DEFAULTS = {"coarse": (2, 32, 20, 31, 10, 5), "transfer": (2, 32, 20, 31, 10, 5), "intermediate": (3, 48, 5, 15, 5, 3)}


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


# One function per --which: (the hierarchy's own entries of the JSON head before and after warmup / reps / inner, the vectors it
# made, timed(bits, r) that fills r with the figures of one pass, the keys of the measured ratio, those of the byte model)
def coarse(ctx, q, args, rng):
    Vc, n = ctx.volume(1), ctx.ndof(1)
    nt = (n + 7) // 8
    matrix_bytes = {32: nt * nt * 64 * 8, 16: nt * nt * 64 * 4}
    vi = ctx.vector(1, 32).upload(rng.standard_normal((Vc, n, 2))); vo = ctx.vector(1, 32)

    def timed(bits, r):
        for key, fn, nmat in (("hop", lambda: ctx.coarse_hop(vo, vi, 1, -1.0, False), 8), ("self_mul", lambda: ctx.coarse_self_mul(vo, vi, 0, False), 1),
                              ("self_mul_inverse", lambda: ctx.coarse_self_mul(vo, vi, 1, True), 1)):
            med, lo, hi = median_ms(ctx, fn, args.warmup, args.reps, args.inner, plug=lambda: ctx.coarse_hop(vo, vi, 1, -1.0, False))
            r[key + "_us"] = med * 1e3; r[key + "_us_min_max"] = [lo * 1e3, hi * 1e3]
            r[key + "_GBps"] = nmat * (Vc // 2) * matrix_bytes[bits] / (med * 1e-3) / 1e9
        its = []
        med, lo, hi = median_ms(ctx, lambda: its.append(ctx.coarse_solve(vo, vi)), 3, max(5, args.reps // 3), 1)
        r["coarsest_solve_ms"] = med; r["coarsest_solve_iterations"] = its[-1]; r["schur_us_per_iteration"] = med * 1e3 / max(its[-1], 1)
    return ({"coarse_lattice": [args.lattice // 4] * 4, "n": n}, {}, [vi, vo], timed,
            ("hop_us", "self_mul_us", "self_mul_inverse_us", "schur_us_per_iteration", "coarsest_solve_ms", "solve_ms"), ())


def transfer(ctx, q, args, rng):
    V, Vc, n = ctx.volume(0), ctx.volume(1), ctx.ndof(1)
    nvec = n // 2
    vf = ctx.vector(0, 32).upload(rng.standard_normal((V, 12, 2))); vc = ctx.vector(1, 32).upload(rng.standard_normal((Vc, n, 2))); vr = ctx.vector(1, 32)

    def timed(bits, r):
        p_bytes = nvec * 24 * (4 if bits == 32 else 2)
        for key, fn, vec_bytes in (("restrict", lambda: ctx.restrict(vr, vf), 96), ("interpolate", lambda: ctx.interpolate(vf, vc, add=False), 96),
                                   ("interpolate_add", lambda: ctx.interpolate(vf, vc, add=True), 192)):
            if key == "interpolate_add":
                vf.upload(np.zeros((V, 12, 2)))          # the sums of many add calls stay finite: c is fixed, the vector grows linearly
            med, lo, hi = median_ms(ctx, fn, args.warmup, args.reps, args.inner)
            nbytes = V * (p_bytes + vec_bytes)
            r[key + "_us"] = med * 1e3; r[key + "_us_min_max"] = [lo * 1e3, hi * 1e3]
            r[key + "_bytes"] = nbytes; r[key + "_fraction_of_hbm_peak"] = nbytes / (med * 1e-3) / HBM_PEAK
        vf.upload(rng.standard_normal((V, 12, 2)))
    return ({"aggregate_sites": V // Vc, "nvec": nvec}, {"hbm_peak": HBM_PEAK}, [vf, vc, vr], timed,
            ("restrict_us", "interpolate_us", "interpolate_add_us", "solve_ms"), ("restrict_bytes", "interpolate_bytes", "interpolate_add_bytes"))


def intermediate(ctx, q, args, rng):
    V1, n = ctx.volume(1), ctx.ndof(1)
    nt = (n + 7) // 8
    coupling_bytes = {32: V1 * 5 * nt * nt * 64 * 8, 16: V1 * 5 * nt * nt * 64 * 4}
    cycles = int(q.post_smooth_iter[1])
    vi = ctx.vector(1, 32).upload(rng.standard_normal((V1, n, 2))); vo = ctx.vector(1, 32)
    start = rng.standard_normal((V1, n, 2)); ph = ctx.vector(1, 32).upload(start)

    def timed(bits, r):
        med, lo, hi = median_ms(ctx, lambda: ctx.coarse_apply(vo, vi), args.warmup, args.reps, args.inner)
        r["apply_us"] = med * 1e3; r["apply_us_min_max"] = [lo * 1e3, hi * 1e3]; r["apply_GBps"] = coupling_bytes[bits] / (med * 1e-3) / 1e9
        med, lo, hi = median_ms(ctx, lambda: ctx.smoother(ph, vi, cycles, initial_guess_zero=False), args.warmup, args.reps, args.inner)
        r["smoother_us"] = med * 1e3; r["smoother_us_min_max"] = [lo * 1e3, hi * 1e3]
        ph.upload(start)
        its = []
        med, lo, hi = median_ms(ctx, lambda: its.append(ctx.kcycle(vo, vi)), 2, max(5, args.reps // 3), 1)
        r["kcycle_us"] = med * 1e3; r["kcycle_us_min_max"] = [lo * 1e3, hi * 1e3]; r["kcycle_iterations"] = its[-1]
    return ({"intermediate_lattice": [args.lattice // 4] * 4, "n": n, "smoother_cycles": cycles}, {"coupling_bytes": coupling_bytes}, [vi, vo, ph], timed,
            ("apply_us", "smoother_us", "kcycle_us", "solve_ms"), ())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", required=True, choices=sorted(DEFAULTS))
    for name in ("lattice", "warmup", "reps", "inner", "solves"):
        ap.add_argument("--" + name, type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    levels, *defaults = DEFAULTS[args.which]
    for name, value in zip(("lattice", "warmup", "reps", "inner", "solves"), defaults):
        if getattr(args, name) is None:
            setattr(args, name, value)
    for k in ("DDAMG_INTERMEDIATE_HALF", "DDAMG_COARSE_HALF", "DDAMG_TRANSFER_HALF"):
        os.environ.pop(k, None)
    import synth
    import ddalphaamg_amd as dd
    from ddalphaamg_amd import api
    from bench import amg_params, GAUGE_EPS, GAUGE_SEED
    L = [args.lattice] * 4
    q = amg_params(api, L, levels, 0)
    ctx = dd.Context(q)
    ctx.set_gauge(synth.synth_gauge(L, GAUGE_EPS, GAUGE_SEED, [1, 1, 1, 1], [0, 0, 0, 0]), anti_pbc=True)
    t0 = time.perf_counter(); ctx.setup(q.setup_iter[0]); ctx.sync()
    print(f"setup {time.perf_counter() - t0:.2f} s", flush=True)
    V = ctx.volume(0)
    head, head_end, vectors, timed, ratio_keys, byte_keys = {"coarse": coarse, "transfer": transfer, "intermediate": intermediate}[args.which](
        ctx, q, args, np.random.default_rng(7))
    set_storage = getattr(ctx, f"set_{args.which}_storage")
    bv = ctx.vector(0, 64).upload(np.stack([np.ones((V, 12)), np.zeros((V, 12))], axis=-1)); xv = ctx.vector(0, 64)
    res = {"lattice": L, **head, "warmup": args.warmup, "reps": args.reps, "inner": args.inner, **head_end}
    for bits in (32, 16, 32, 16):
        set_storage(bits)
        r = {}
        timed(bits, r)
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
    res["ratio_16_over_32"] = {k: b[k] / a[k] for k in ratio_keys}
    if byte_keys:
        res["byte_model_ratio"] = {k: b[k] / a[k] for k in byte_keys}
        print("measured 16/32:", json.dumps(res["ratio_16_over_32"]), "byte model:", json.dumps(res["byte_model_ratio"]), flush=True)
    else:
        print(json.dumps(res["ratio_16_over_32"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    for v in vectors + [bv, xv]:
        v.free()
    ctx.close()


if __name__ == "__main__":
    main()
