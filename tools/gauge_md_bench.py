#!/usr/bin/env python3
"""tools/gauge_md_bench.py -- the gauge sector of the molecular dynamics through its entry points, ONE process, ONE seeded field.
Run it under a time limit:

  timeout -k 10 300 python tools/gauge_md_bench.py [--lattice 32] [--calls 10] [--reps 5] [--grid -1,-1,-1,-1] [--out FILE.json]

Per call: milliseconds, the median over --reps repeats of --calls back-to-back calls between the context's timer events
(ddamg_hip_timer_begin / _end) after one untimed repeat, and the spread (min, max) over the repeats.  Every call waits for its result,
so the time between the events holds the host's wait of each call too: tens of microseconds against milliseconds at 32^4.
`links_TBps` sets the time of the force and of the loops against the links' own 72 V doubles read once per plane a link lies in
(three): the least a plane-tiled kernel reads; the other calls against the fields they must read and write once.
--grid takes process-grid entries of 1 and -1 (-1: the direction is split and the process its own neighbour over RCCL, so the shell of
the links travels through pack -> send/recv -> unpack for real): the same field through the collective _grid calls of a second
context, under "grid", each next to the plain call of the same build ("extra_ms"), with the messages and bytes of one call."""
import argparse, json, os, statistics, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=32)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--grid", help="process-grid entries, 1 or -1 (self-exchange), e.g. -1,-1,-1,-1")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import synth
    import ddalphaamg_amd as dd
    from ddalphaamg_amd import api
    n = a.lattice; L = [n] * 4; V = n ** 4
    p = api.default_params(); p.num_levels = 1
    for mu in range(4):
        p.local_lattice[0][mu] = n; p.block_lattice[0][mu] = 4
    ctx = dd.Context(p)
    U = torch.from_numpy(np.ascontiguousarray(synth.synth_gauge(L, 0.35, 20260101), dtype=np.float64).reshape(V, 4, 9, 2)).cuda()
    m = np.random.default_rng(1).standard_normal((V, 4, 3, 3)) + 1j * np.random.default_rng(2).standard_normal((V, 4, 3, 3))
    m = 0.5 * (m - np.conj(np.swapaxes(m, -1, -2)))
    m -= np.trace(m, axis1=-2, axis2=-1)[..., None, None] * np.eye(3) / 3.0
    P = torch.from_numpy(np.stack([m.real, m.imag], axis=-1).reshape(V, 4, 9, 2)).cuda()
    F = torch.empty_like(U)
    beta, eps = 5.6, 1e-3
    calls = {"gauge_force_c1_0": lambda: ctx.gauge_force_device(F, U, beta, 0.0),
             "gauge_force_c1_-1/12": lambda: ctx.gauge_force_device(F, U, beta, -1.0 / 12.0),
             "links_update": lambda: ctx.links_update_device(U, P, eps),
             "gauge_loops": lambda: ctx.gauge_loops_device(U),
             "gauge_loops_plaquette_only": lambda: ctx.gauge_loops_device(U, rectangles=False),
             "links_reunitarize": lambda: ctx.links_reunitarize_device(U),
             "momentum_update": lambda: ctx.momentum_update_device(P, F, eps),
             "momentum_kinetic": lambda: ctx.momentum_kinetic_device(P)}
    least = {k: 3 * 576 * V for k in calls}
    least.update({"links_update": 3 * 576 * V, "links_reunitarize": 2 * 576 * V, "momentum_update": 3 * 576 * V, "momentum_kinetic": 576 * V})
    res = {"lattice": L, "calls": a.calls, "reps": a.reps, "plaquette_sum_per_6V": ctx.gauge_loops_device(U)[0] / (6 * V)}

    def timed(c, fn):
        ms = []
        for r in range(1 + a.reps):
            c.timer_begin()
            for _ in range(a.calls if r else 1):
                fn()
            t = c.timer_end()
            if r:
                ms.append(t / a.calls)
        return statistics.median(ms), min(ms), max(ms)
    for k, fn in calls.items():
        med, lo, hi = timed(ctx, fn)
        res[k] = {"ms": med, "min": lo, "max": hi, "least_bytes": least[k], "links_TBps": least[k] / (med * 1e-3) / 1e12}
    ctx.close()
    if a.grid:
        entries = [int(e) for e in a.grid.split(",")]
        assert len(entries) == 4 and all(e in (1, -1) for e in entries), "--grid takes four entries of 1 or -1"
        for mu in range(4):
            p.process_grid[mu] = entries[mu]; p.process_coords[mu] = 0
        ctx = dd.Context(p)
        if min(entries) < 0:
            ctx.comm_init_rccl(api.rccl_unique_id())
        twins = {"gauge_force_c1_0": lambda: ctx.gauge_force_device_grid(F, U, beta, 0.0),
                 "gauge_force_c1_-1/12": lambda: ctx.gauge_force_device_grid(F, U, beta, -1.0 / 12.0),
                 "gauge_loops": lambda: ctx.gauge_loops_device_grid(U),
                 "gauge_loops_plaquette_only": lambda: ctx.gauge_loops_device_grid(U, rectangles=False),
                 "links_reunitarize": lambda: ctx.links_reunitarize_device_grid(U),
                 "momentum_kinetic": lambda: ctx.momentum_kinetic_device_grid(P)}
        res["grid"] = {"entries": entries}
        for k, fn in twins.items():
            med, lo, hi = timed(ctx, fn)
            ctx.comm_stats(reset=True)
            fn()
            sent = ctx.comm_stats().get("device_sendrecv", {})
            res["grid"][k] = {"ms": med, "min": lo, "max": hi, "extra_ms": med - res[k]["ms"], "messages": sent.get("messages", 0),
                              "bytes_sent": sent.get("bytes_sent", 0)}
        ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
