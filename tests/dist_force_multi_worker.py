"""Worker of the two-process test of the many-pair fermion force (started through torch.distributed.run, gloo backend, host
transport; both ranks share the one test GPU).  The lattice is 8x4x4x4 split in T, one level.  Every rank first computes
force_bilinear_multi_vec and force_rational_device of the whole lattice on an undivided context of its own, then its part through
force_bilinear_multi_vec_grid, force_bilinear_multi_device_grid and force_rational_device_grid: each rank's part must equal the
corresponding rows of the undivided result to 1e-13 of the norm, the two entry points must give the same bits, and the bilinear call
must send 4 + ceil(n / G) messages per split direction (link shell, tensor shell, the faces of every group in one message)."""
import argparse, os, sys
import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tools"))
from ddalphaamg_amd import api, dist as ddist  # noqa: E402
import eo_reference as eo  # noqa: E402
from dist_gauge_device_worker import Hip, relerr  # noqa: E402
from dist_multishift_worker import G, params  # noqa: E402

N = api.FORCE_GROUP + 1
WEIGHTS = [0.3, -1.1, 2.5, -0.04, 7.0, 1.0, -3.2, 0.6, 1.7]
RHO = [0.3, 1.1, 2.5]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="2,1,1,1")
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    P = [int(x) for x in a.grid.split(",")]
    assert int(np.prod(P)) == world == 2
    import ddalphaamg_amd as dd
    import synth
    from conftest import splitmix_uniform
    V = int(np.prod(G))
    U = synth.synth_gauge(list(G), 0.35, 4).reshape(V, 4, 9, 2)
    Y = [splitmix_uniform(V * 24, 100 + 2 * s).reshape(V, 12, 2) for s in range(N)]
    X = [splitmix_uniform(V * 24, 101 + 2 * s).reshape(V, 12, 2) for s in range(N)]
    even = eo.parity(G) == 0
    xe = [np.ascontiguousarray(splitmix_uniform(V * 24, 200 + s).reshape(V, 12, 2)[even]) for s in range(len(RHO))]
    w = WEIGHTS[:N]
    L = [G[mu] // P[mu] for mu in range(4)]
    C = ddist.coords_of(rank, P)
    lp = lambda x: np.ascontiguousarray(ddist.local_part(x.reshape(V, -1), G, P, C))
    hip = Hip()

    whole = dd.Context(params(G, [1] * 4, [0] * 4))
    whole.set_gauge(U, anti_pbc=True)
    out = hip.upload(np.zeros(V * 72))
    ys = [whole.vector(0, 64).upload(y) for y in Y]; xs = [whole.vector(0, 64).upload(x) for x in X]
    whole.force_bilinear_multi_vec(out, ys, xs, w, -2.0)
    want_multi = hip.download(out, (V, 72))
    dxe = [hip.upload(h) for h in xe]
    whole.force_rational_device(out, RHO, dxe, None, -2.0)
    want_rational = hip.download(out, (V, 72))
    for v in ys + xs:
        v.free()
    whole.close()

    ctx = dd.Context(params(L, P, C))
    ddist.attach_host(ctx)
    ctx.set_gauge(lp(U), anti_pbc=True)
    Vl = V // world
    mine = hip.upload(np.zeros(Vl * 72))
    ys = [ctx.vector(0, 64).upload(lp(y).reshape(Vl, 12, 2)) for y in Y]; xs = [ctx.vector(0, 64).upload(lp(x).reshape(Vl, 12, 2)) for x in X]
    ctx.comm_stats(reset=True)
    ctx.force_bilinear_multi_vec_grid(mine, ys, xs, w, -2.0)
    shell = ctx.comm_stats()["device_sendrecv"]
    got = hip.download(mine, (Vl, 72))
    err = relerr(got, lp(want_multi))
    print(f"rank {rank}: many pairs: relerr of its part {err:.2e}, {shell}", flush=True)
    assert err < 1e-13, err
    assert shell["messages"] == 4 + -(-N // api.FORCE_GROUP), shell
    dy = [hip.upload(lp(y)) for y in Y]; dx = [hip.upload(lp(x)) for x in X]
    ctx.force_bilinear_multi_device_grid(mine, dy, dx, w, -2.0)
    assert np.array_equal(hip.download(mine, (Vl, 72)).view(np.uint64), got.view(np.uint64)), "_vec_grid and _device_grid differ in their bits"
    # split in T: rank r owns the lexicographic sites [r Vl, (r + 1) Vl), so its even sites are a contiguous range of the even sites
    half = len(xe[0]) // world
    lxe = [hip.upload(np.ascontiguousarray(h[rank * half:(rank + 1) * half])) for h in xe]
    ctx.force_rational_device_grid(mine, RHO, lxe, None, -2.0)
    err = relerr(hip.download(mine, (Vl, 72)), lp(want_rational))
    print(f"rank {rank}: rational force: relerr of its part {err:.2e}", flush=True)
    assert err < 1e-13, err
    for v in ys + xs:
        v.free()
    dist.barrier()
    ctx.close()
    ok = torch.tensor([1.0], dtype=torch.float64)
    dist.all_reduce(ok)
    if rank == 0 and ok.item() == world:
        print("DIST_FORCE_MULTI_OK", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
