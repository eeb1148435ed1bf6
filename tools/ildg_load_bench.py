#!/usr/bin/env python3
"""tools/ildg_load_bench.py -- an ILDG configuration into the operator: the device pipeline of ddamg_hip_load_ildg_conf (file ->
pinned staging -> conversion kernel -> links on the device -> operator) against the host path (ddamg_hip_read_ildg_conf, which
swaps and reorders on the host, then ddamg_hip_set_gauge).  ONE process, ONE seeded synthetic field written into a temporary
directory, warm page cache (the file has just been written, and one untimed call of each form comes first).  Run it under a time
limit:

  timeout -k 10 600 python tools/ildg_load_bench.py [--lattice 32] [--precision 64] [--reps 3] [--out FILE.json]

  load_ildg_conf     seconds per call, host clock around the call (it ends in a synchronise)
  read + set_gauge   seconds per read_ildg_conf into a reused array followed by set_gauge, and the two parts
  kernel             milliseconds per ildg_to_links_kernel launch over the whole record in device memory between the context's
                     timer events, after one untimed launch; GB/s = (file bytes read + 576 bytes of links written per site) / time
Every figure is the median over --reps calls, the two forms in alternation; no figure is a pass criterion."""
import argparse, ctypes, json, os, statistics, sys, tempfile, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=32)
    ap.add_argument("--precision", type=int, default=64, choices=(32, 64))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    import synth
    import ddalphaamg_amd as dd
    from ddalphaamg_amd import api
    from device_interface_bench import hip_runtime, to_device
    n = a.lattice; L = [n] * 4; V = n ** 4
    p = api.default_params(); p.num_levels = 1
    for mu in range(4):
        p.local_lattice[0][mu] = n; p.block_lattice[0][mu] = 4
    p.m0, p.csw = -0.1, 1.0
    U = synth.synth_gauge(L, 0.35, 11)
    res = {"lattice": L, "precision": a.precision}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "conf.ildg")
        ctx = dd.Context(p)
        plaq = ctx.set_gauge(U, anti_pbc=True)
        api.write_ildg_conf(path, L, U, plaq, precision=a.precision)
        res["file_bytes"] = os.path.getsize(path)
        buf = np.empty((V, 4, 9, 2))
        t = {"load_ildg_conf": [], "read_ildg_conf": [], "set_gauge": []}
        plaqs = {}
        for r in range(1 + a.reps):
            t0 = time.perf_counter(); plaqs["device"] = ctx.load_ildg_conf(path, anti_pbc=True)[0]; t1 = time.perf_counter()
            api.read_ildg_conf(path, L, out=buf); t2 = time.perf_counter()
            plaqs["host"] = ctx.set_gauge(buf, anti_pbc=True); t3 = time.perf_counter()
            if r:
                t["load_ildg_conf"].append(t1 - t0); t["read_ildg_conf"].append(t2 - t1); t["set_gauge"].append(t3 - t2)
        res["load_ildg_conf_s"] = statistics.median(t["load_ildg_conf"])
        res["read_ildg_conf_s"] = statistics.median(t["read_ildg_conf"])
        res["set_gauge_s"] = statistics.median(t["set_gauge"])
        res["read_plus_set_gauge_s"] = statistics.median([x + y for x, y in zip(t["read_ildg_conf"], t["set_gauge"])])
        res["spread_s"] = {k: (min(v), max(v)) for k, v in t.items()}
        res["plaquette"] = plaqs
        # the conversion kernel alone, on the whole record in device memory
        info = api.lime_info(path)
        raw = np.fromfile(path, dtype=np.uint8, count=info["data_length"], offset=info["data_offset"])
        hip = hip_runtime()
        d_raw = to_device(hip, raw); d_links = to_device(hip, buf)
        ctx.ildg_to_links_device(d_raw, a.precision, V, d_links)
        ms = []
        for _ in range(a.kernel_reps):
            ctx.timer_begin(); ctx.ildg_to_links_device(d_raw, a.precision, V, d_links); ms.append(ctx.timer_end())
        res["ildg_to_links_kernel_ms"] = statistics.median(ms)
        res["ildg_to_links_GBps"] = (info["data_length"] + V * 576) / (res["ildg_to_links_kernel_ms"] * 1e-3) / 1e9
        hip.hipFree(d_raw); hip.hipFree(d_links)
        ctx.close()
    line = json.dumps(res)
    print(f"load_ildg_conf {res['load_ildg_conf_s']:.4f} s   read_ildg_conf + set_gauge {res['read_plus_set_gauge_s']:.4f} s "
          f"({res['read_ildg_conf_s']:.4f} + {res['set_gauge_s']:.4f})   ildg_to_links_kernel {res['ildg_to_links_kernel_ms']:.3f} ms, "
          f"{res['ildg_to_links_GBps']:.0f} GB/s")
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
