#!/usr/bin/env python3
"""tools/dagger_bench.py -- the fine operator D, the fused D^dagger and the composed gamma5, D, gamma5 through the entry points, ONE
process, ONE seeded field, 4^4 blocks, fp32 and fp64.  Run it under a time limit:

  timeout -k 10 300 python tools/dagger_bench.py [--lattice 32] [--calls 200] [--reps 7] [--out FILE.json]

Per precision and form: microseconds per call, the median over --reps repeats of --calls back-to-back calls between the context's
timer events (ddamg_hip_timer_begin / _end) after --warmup untimed repeats, the three forms in alternation inside every repeat, and
the spread (min, max) over the repeats.  `fused_no_slower` is the condition docs/design/04_kernels.md records: the median of the fused
D^dagger is not above the median of D by more than D's own spread (max - min) in this run."""
import argparse, json, os, statistics, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=32)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    import synth
    import ddalphaamg_amd as dd
    from ddalphaamg_amd import api
    n = a.lattice; L = [n] * 4; V = n ** 4
    p = api.default_params(); p.num_levels = 1
    for mu in range(4):
        p.local_lattice[0][mu] = n; p.block_lattice[0][mu] = 4
    p.m0, p.csw = -0.1, 1.0
    ctx = dd.Context(p)
    ctx.set_gauge(synth.synth_gauge(L, 0.35, 20260101), anti_pbc=True)
    res = {"lattice": L, "calls": a.calls, "reps": a.reps, "link_reals_fp32": ctx.link_reals()}
    phi = np.random.default_rng(1).uniform(-0.5, 0.5, (V, 12, 2))
    for prec in (32, 64):
        x = ctx.vector(0, prec).upload(phi); y = ctx.vector(0, prec); t = ctx.vector(0, prec)

        def composed():
            ctx.gamma5(t, x); ctx.dirac_apply(y, t); ctx.gamma5(y, y)
        forms = {"D": lambda: ctx.dirac_apply(y, x), "D_dagger_fused": lambda: ctx.dirac_apply_dagger(y, x), "D_dagger_composed": composed}
        us = {k: [] for k in forms}
        for r in range(a.warmup + a.reps):
            for k, fn in forms.items():
                ctx.timer_begin()
                for _ in range(a.calls):
                    fn()
                ms = ctx.timer_end()
                if r >= a.warmup:
                    us[k].append(ms * 1e3 / a.calls)
        out = {k: {"us": statistics.median(v), "min": min(v), "max": max(v)} for k, v in us.items()}
        spread = out["D"]["max"] - out["D"]["min"]
        out["fused_minus_D_us"] = out["D_dagger_fused"]["us"] - out["D"]["us"]
        out["spread_of_D_us"] = spread
        out["fused_no_slower"] = out["fused_minus_D_us"] <= spread
        res[f"fp{prec}"] = out
        for v in (x, y, t):
            v.free()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
