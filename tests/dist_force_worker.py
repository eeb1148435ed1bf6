"""Worker of the multi-process test of the fermion force on a process grid (started through torch.distributed.run, gloo backend,
host transport; all ranks share the one test GPU).

Every rank uploads its part of the golden 8^4 links, calls set_gauge_device_grid and then force_bilinear_device_grid,
force_bilinear_vec_grid and force_logdet_grid for both parities.  Its expectation is its part (ddalphaamg_amd.dist.local_part) of
tests/force_reference.py on the whole periodic lattice, which every rank computes for itself; the bar is 1e-13 of the norm of its part,
and the all-reduced relative error over the whole lattice is printed.  On the grid 2,1,1,1 a second context with m0 = -4 and csw = 0
must return the singular-block error of force_logdet_grid on every rank -- an agreed refusal, after which the worker still ends.
"""
import argparse, os, sys
import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
from ddalphaamg_amd import api, dist as ddist  # noqa: E402
import force_reference as fr  # noqa: E402
from conftest import splitmix_uniform  # noqa: E402
from dist_gauge_device_worker import Hip, params, relerr, G  # noqa: E402

V = int(np.prod(G))


def whole_lattice(sq):
    t = torch.tensor(sq, dtype=torch.float64)
    dist.all_reduce(t)
    return float(np.sqrt(t[0].item() / t[1].item()))


def run(rank, P):
    import ddalphaamg_amd as dd
    g = np.load(os.path.join(HERE, "golden", "ref_8x8_dirac.npz"))
    m0, csw = float(g["meta_f64"][0]), float(g["meta_f64"][1])
    L = [G[mu] // P[mu] for mu in range(4)]
    C = ddist.coords_of(rank, P)
    lp = lambda a: ddist.local_part(a, G, P, C)
    U = g["gauge"].reshape(V, 4, 9, 2)
    X = splitmix_uniform(V * 24, 9).reshape(V, 12, 2); Y = splitmix_uniform(V * 24, 10).reshape(V, 12, 2)
    hip = Hip()
    mine = np.ascontiguousarray(lp(U.reshape(V, -1)))
    dU = hip.upload(mine)
    ctx = dd.Context(params(g, L, P, C))
    ddist.attach_host(ctx)
    ctx.set_gauge_device_grid(dU, anti_pbc=True)
    Vl = int(np.prod(L))
    out = hip.upload(np.zeros(Vl * 72))
    x, y = lp(X.reshape(V, -1)), lp(Y.reshape(V, -1))
    dx, dy = hip.upload(x), hip.upload(y)
    nsplit = sum(1 for e in P if e > 1)

    def check(name, want, messages):
        got = hip.download(out, (Vl, 72))
        want = lp(want.reshape(V, -1))
        err = relerr(got, want)
        total = whole_lattice([float(np.sum((got - want) ** 2)), float(np.sum(want ** 2))])
        shell = ctx.comm_stats()["device_sendrecv"]
        ctx.comm_stats(reset=True)
        print(f"rank {rank}: {name}: relerr of its part {err:.2e}" + (f", over the whole lattice {total:.2e}" if rank == 0 else ""), flush=True)
        assert err < 1e-13, (name, err)
        assert shell["messages"] == messages, (name, shell)
        return got

    ctx.comm_stats(reset=True)
    ctx.force_bilinear_device_grid(out, dy, dx)
    first = check("bilinear force", fr.force_bilinear(G, U, 1, m0, csw, Y, X), 5 * nsplit)
    vx = ctx.vector(0, 64).upload(x.reshape(Vl, 12, 2)); vy = ctx.vector(0, 64).upload(y.reshape(Vl, 12, 2))
    ctx.force_bilinear_vec_grid(out, vy, vx)
    assert np.array_equal(hip.download(out, (Vl, 72)).view(np.uint64), first.view(np.uint64)), "_vec_grid and _device_grid differ in their bits"
    ctx.comm_stats(reset=True)
    for par in (0, 1):
        ctx.force_logdet_grid(out, par)
        check(f"determinant force, parity {par}", fr.force_logdet(G, U, 1, m0, csw, par), 4 * nsplit)
    assert np.array_equal(hip.download(dU, mine.shape).view(np.uint64), mine.view(np.uint64)), "the caller's links were written"
    vx.free(); vy.free()
    dist.barrier()
    ctx.close()

    if P == [2, 1, 1, 1]:     # every clover block is zero: all ranks return the same error, nobody waits for a shell
        p = params(g, L, P, C); p.m0, p.csw = -4.0, 0.0
        ctx = dd.Context(p)
        ddist.attach_host(ctx)
        ctx.set_gauge_device_grid(dU, anti_pbc=True)
        try:
            ctx.force_logdet_grid(out, 1)
            raise AssertionError("a singular block was not refused")
        except api.DDAMGError as e:
            assert "singular" in str(e) and "parity 1" in str(e), str(e)
            print(f"rank {rank}: refused: {e}", flush=True)
        dist.barrier()
        ctx.close()
    for p in (dU, out, dx, dy):
        hip.free(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="2,1,1,1")
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    P = [int(x) for x in a.grid.split(",")]
    assert int(np.prod(P)) == world and world <= 4
    run(rank, P)
    ok = torch.tensor([1.0], dtype=torch.float64)
    dist.all_reduce(ok)
    if rank == 0 and ok.item() == world:
        print(f"DIST_FORCE_OK grid={a.grid}", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
