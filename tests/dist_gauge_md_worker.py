"""Worker of the multi-process test of the gauge sector on a process grid (started through torch.distributed.run, gloo backend, host
transport; all ranks share the one test GPU).

Every rank uploads its part of the golden 8^4 links and calls the six ddamg_hip_*_device_grid entry points of the gauge sector.  Its
expectation is its part (ddalphaamg_amd.dist.local_part) of tests/gauge_reference.py on the whole periodic lattice, which every rank
computes for itself: the force within 1e-13 of the norm of its part for c1 = 0 and -1/12; the all-reduced loop sums and the kinetic
energy within 1e-13 of numpy's global values (the bar of test_gpu_gauge_md.py) and identical on every rank; max_deviation of links of
which ONE rank perturbed ONE link is the global maximum on every rank, so it must have travelled; and the messages of every call
(two per split direction for the loops and the force, none for the others).  On the grid 1,1,1,2 a second context on a global
4x4x4x2 lattice (local X = 1) must refuse the two-deep shell on every rank -- an agreed refusal, after which the worker still ends.
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
import gauge_reference as gr  # noqa: E402
from dist_gauge_device_worker import Hip, params, relerr, G  # noqa: E402

V = int(np.prod(G))
BETA = 5.6


def same_on_every_rank(values):
    """the values of this rank, after checking that every rank holds the same bits"""
    mine = torch.tensor(values, dtype=torch.float64)
    lo, hi = mine.clone(), mine.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    assert torch.equal(lo, hi) and torch.equal(lo, mine), (values, lo, hi)
    return values


def run(rank, P):
    import ddalphaamg_amd as dd
    g = np.load(os.path.join(HERE, "golden", "ref_8x8_dirac.npz"))
    L = [G[mu] // P[mu] for mu in range(4)]
    C = ddist.coords_of(rank, P)
    lp = lambda a: ddist.local_part(a, G, P, C)
    U = g["gauge"].reshape(V, 4, 9, 2)
    Vl = int(np.prod(L))
    hip = Hip()
    mine = np.ascontiguousarray(lp(U.reshape(V, -1)))
    dU = hip.upload(mine)
    ctx = dd.Context(params(g, L, P, C))
    ddist.attach_host(ctx)
    out = hip.upload(np.zeros(Vl * 72))
    nsplit = sum(1 for e in P if e > 1)

    def sent(depth):
        """bytes of the shell of the links at this depth: two slabs per split direction (docs/design/06_multi_gpu.md)"""
        total = 0
        for mu in range(4):
            if P[mu] > 1:
                n = 72 * 8 * depth
                for d in range(4):
                    if d != mu:
                        n *= L[d] + 2 * depth if (d < mu and P[d] > 1) else L[d]
                total += 2 * n
        return total

    def messages(name, count, nbytes):
        shell = ctx.comm_stats()["device_sendrecv"]
        ctx.comm_stats(reset=True)
        assert shell["messages"] == count and shell["bytes_sent"] == nbytes, (name, shell, count, nbytes)

    # the loops: the global sums on every rank
    plaq, rect = gr.loops(G, U)
    ctx.comm_stats(reset=True)
    p, r = same_on_every_rank(ctx.gauge_loops_device_grid(dU))
    messages("gauge_loops", 2 * nsplit, sent(2))
    p1, none = ctx.gauge_loops_device_grid(dU, rectangles=False)
    messages("gauge_loops without rectangles", 2 * nsplit, sent(1))
    same_on_every_rank([p1])
    print(f"rank {rank}: plaquette sum {p:.12e} ({abs(p - plaq) / abs(plaq):.1e}), rectangle sum {r:.12e} ({abs(r - rect) / abs(rect):.1e})", flush=True)
    assert none is None
    assert abs(p - plaq) <= 1e-13 * abs(plaq) and abs(p1 - plaq) <= 1e-13 * abs(plaq) and abs(r - rect) <= 1e-13 * abs(rect)

    # the force: this rank's part of the reference of the whole lattice
    parts = gr.force(G, U, BETA, 0.0, "plaquette"), gr.force(G, U, BETA, 0.0, "rectangle")
    for c1 in (gr.WILSON, gr.SYMANZIK):
        ctx.gauge_force_device_grid(out, dU, BETA, c1)
        messages(f"gauge_force c1 {c1}", 2 * nsplit, sent(1 if c1 == 0.0 else 2))
        want = lp(((1.0 - 8.0 * c1) * parts[0] + c1 * parts[1]).reshape(V, -1))
        got = hip.download(out, (Vl, 72))
        err = relerr(got, want)
        t = torch.tensor([float(np.sum((got - want) ** 2)), float(np.sum(want ** 2))], dtype=torch.float64)
        dist.all_reduce(t)
        print(f"rank {rank}: force c1 {c1:+.4f}: relerr of its part {err:.2e}, over the whole lattice {float(np.sqrt(t[0] / t[1])):.2e}", flush=True)
        assert err < 1e-13, (c1, err)
    assert np.array_equal(hip.download(dU, mine.shape).view(np.uint64), mine.view(np.uint64)), "the caller's links were written"

    # the kinetic energy of a global field of momenta
    Pg = fr.as_reals(fr.random_algebra(np.random.default_rng(17), (V, 4)))
    dP = hip.upload(lp(Pg.reshape(V, -1)))
    kin = same_on_every_rank([ctx.momentum_kinetic_device_grid(dP)])[0]
    messages("momentum_kinetic", 0, 0)
    assert abs(kin - gr.kinetic(Pg)) <= 1e-13 * kin, (kin, gr.kinetic(Pg))

    # the two that send nothing: the local kernels, against numpy on this rank's part
    ctx.momentum_update_device_grid(dP, out, -0.3)
    mom = lp(Pg.reshape(V, -1)) - 0.3 * hip.download(out, (Vl, 72))
    assert np.abs(hip.download(dP, (Vl, 72)) - mom).max() <= 4 * np.finfo(np.float64).eps * np.abs(mom).max()
    dW = hip.upload(mine)
    ctx.links_update_device_grid(dW, dP, 0.05)
    assert relerr(hip.download(dW, (Vl, 4, 9, 2)), gr.update_links(mine.reshape(Vl, 4, 9, 2), hip.download(dP, (Vl, 4, 9, 2)), 0.05)) < 1e-13
    messages("momentum_update and links_update", 0, 0)

    # reunitarisation: every rank's links slightly off, and on the last rank one link far more: the maximum must travel
    off = mine.reshape(Vl, 4, 9, 2) + 1e-9 * np.random.default_rng(3 + rank).standard_normal((Vl, 4, 9, 2))
    if rank == dist.get_world_size() - 1:
        off[Vl // 2, 1] *= 1.0 + 1e-4
    local = torch.tensor([gr.unitarity_deviation(off)], dtype=torch.float64)
    worst = local.clone()
    dist.all_reduce(worst, op=dist.ReduceOp.MAX)
    dO = hip.upload(off)
    dev = same_on_every_rank([ctx.links_reunitarize_device_grid(dO)])[0]
    messages("links_reunitarize", 0, 0)
    print(f"rank {rank}: deviation of its part {local.item():.3e}, returned {dev:.3e}, global maximum {worst.item():.3e}", flush=True)
    assert abs(dev - worst.item()) <= 1e-6 * worst.item() and (rank == dist.get_world_size() - 1 or local.item() < 0.01 * dev)
    # 8 eps: test_gpu_gauge_md.py finds the projection of 4096 sites at 4.002 eps, past the 4 eps that hold for 256
    assert gr.unitarity_deviation(hip.download(dO, off.shape)) <= 8 * np.finfo(np.float64).eps
    assert ctx.links_reunitarize_device_grid(dO, deviation=False) is None
    dist.barrier()
    ctx.close()

    if P == [1, 1, 1, 2]:     # local X = 1 is below the two-deep shell: every rank refuses by itself, nobody waits for a slab
        q = params(g, [4, 4, 4, 1], P, C)
        q.block_lattice[0][3] = 1
        ctx = dd.Context(q)
        ddist.attach_host(ctx)
        for call in (lambda: ctx.gauge_force_device_grid(out, dU, BETA, gr.SYMANZIK), lambda: ctx.gauge_loops_device_grid(dU)):
            try:
                call()
                raise AssertionError("a shell deeper than the local lattice was not refused")
            except api.DDAMGError as e:
                assert "below the depth 2" in str(e), str(e)
                print(f"rank {rank}: refused: {e}", flush=True)
        assert ctx.comm_stats()["device_sendrecv"]["messages"] == 0
        dist.barrier()
        ctx.close()
    for p in (dU, out, dP, dW, dO):
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
        print(f"DIST_GAUGE_MD_OK grid={a.grid}", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
