#!/usr/bin/env python3
"""tools/chrono_bench.py -- what the chronological guess costs: ddamg_hip_chrono_guess_vec from a full store of --depth vectors next to
--depth calls of ddamg_hip_dirac_apply at precision 64 (the operator applications the guess cannot do without), ONE process, ONE seeded
field, 4^4 blocks; and the pair-projection kernel next to its yardstick, vec_multi_axpy_dev, at --columns columns on the same vectors
(tools/chrono_kernel_bench.hip, built on first use).  Run it under a time limit:

  timeout -k 10 300 python tools/chrono_bench.py [--lattice 32] [--depth 4] [--columns 4] [--calls 10] [--reps 7] [--out FILE.json]

Milliseconds are medians over --reps repeats of --calls back-to-back calls between the context's timer events (ddamg_hip_timer_begin /
_end) after --warmup untimed repeats, the two forms in alternation inside every repeat, with the spread (min, max) over the repeats."""
import argparse, json, os, statistics, subprocess, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tools"))
SRC = os.path.join(REPO, "tools", "chrono_kernel_bench.hip")
EXE = os.path.join(REPO, "tools", "chrono_kernel_bench")


def build():
    """the kernel program, linked to the library next to the package"""
    csrc = os.path.join(REPO, "ddalphaamg_amd", "csrc")
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < os.path.getmtime(SRC):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O3", "--offload-arch=gfx950", "-I" + csrc,
                               "-I" + os.path.join(REPO, "include"), "-o", EXE, SRC, "-L" + os.path.join(REPO, "ddalphaamg_amd"), "-lddamg_hip",
                               "-Wl,--enable-new-dtags", "-Wl,-rpath,$ORIGIN/../ddalphaamg_amd"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=32)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--columns", type=int, default=4)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    build()
    if a.build_only:
        return
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
    rng = np.random.default_rng(1)
    x = ctx.vector(0, 64); y = ctx.vector(0, 64); b = ctx.vector(0, 64).upload(rng.uniform(-0.5, 0.5, (V, 12, 2)))
    store = ctx.chrono_create(a.depth)
    for _ in range(a.depth):
        store.push(x.upload(rng.uniform(-0.5, 0.5, (V, 12, 2))))
    kept = []

    def guess():
        kept.append(store.guess(y, b)[0])

    def applies():
        for _ in range(a.depth):
            ctx.dirac_apply(y, x)
    forms = {"chrono_guess": guess, "dirac_applies": applies}
    ms = {k: [] for k in forms}
    for r in range(a.warmup + a.reps):
        for k, fn in forms.items():
            ctx.timer_begin()
            for _ in range(a.calls):
                fn()
            t = ctx.timer_end()
            if r >= a.warmup:
                ms[k].append(t / a.calls)
    res = {"lattice": L, "depth": a.depth, "kept": sorted(set(kept)), "calls": a.calls, "reps": a.reps}
    res.update({k: {"ms": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()})
    res["guess_over_applies"] = res["chrono_guess"]["ms"] / res["dirac_applies"]["ms"]
    for v in (x, y, b):
        v.free()
    store.free()
    ctx.close()
    # the kernels by themselves, in a process of their own (started after this one has given its memory back)
    out = subprocess.run([EXE, str(n), str(a.columns), "20", str(a.reps)], capture_output=True, text=True, timeout=240)
    if out.returncode != 0:
        sys.exit(f"chrono_kernel_bench failed ({out.returncode}): {out.stderr[-2000:]}")
    res["kernels"] = json.loads(out.stdout)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
