"""Worker of the two-process test of the multi-shift solve (started through torch.distributed.run, gloo backend, host transport; both
ranks share the one test GPU).  The lattice is 8x4x4x4 split in T, one level.  Three shifts: every rank must see the same iteration
counts and relres <= 2 tol (the loop stops on the recursed residual), and the residual recomputed in numpy from the parts of x_s on
both ranks must agree with the reported one."""
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

G = [8, 4, 4, 4]
M0, CSW, TOL = 0.3, 1.0, 1e-10
SHIFTS = [0.0, 0.1, 10.0]


def params(lat, grid, coords):
    p = api.default_params(); p.num_levels = 1
    for mu in range(4):
        p.local_lattice[0][mu] = lat[mu]; p.block_lattice[0][mu] = 2
        p.process_grid[mu] = grid[mu]; p.process_coords[mu] = coords[mu]
    p.tol, p.m0, p.csw = TOL, M0, CSW
    return p


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
    b = splitmix_uniform(V * 24, 23).reshape(V, 12, 2)
    b[eo.parity(G) == 1] = np.nan                     # the odd sites of the right-hand side are not read
    L = [G[mu] // P[mu] for mu in range(4)]
    C = ddist.coords_of(rank, P)
    lp = lambda x: np.ascontiguousarray(ddist.local_part(x.reshape(V, -1), G, P, C))

    whole = dd.Context(params(G, [1] * 4, [0] * 4))
    whole.set_gauge(U, anti_pbc=True)
    D, cl = whole.get_operator()
    whole.close()

    ctx = dd.Context(params(L, P, C))
    ddist.attach_host(ctx)
    ctx.set_gauge(lp(U), anti_pbc=True)
    vb = ctx.vector(0, 64).upload(lp(b)); xs = [ctx.vector(0, 64) for _ in SHIFTS]
    its, rr, ritz = ctx.solve_schur_multishift_vec(SHIFTS, xs, vb)
    x = [v.download() for v in xs]
    for v in xs + [vb]:
        v.free()
    print(f"rank {rank}: iterations {its}, relres {rr}, ritz {ritz}", flush=True)
    mine = torch.tensor([float(i) for i in its] + list(rr), dtype=torch.float64)
    both = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(both, mine)
    assert torch.equal(both[0], both[1]), both                  # the scalars come out of all-reduces: the same on every rank
    assert min(its) > 0 and max(rr) <= 2 * TOL and its[0] >= its[1] >= its[2] and 0 < ritz[0] < ritz[1], (its, rr, ritz)
    odd = eo.parity(G)[:, None, None] == 1
    be = np.where(odd, 0.0, b)
    Vl = V // world
    for s, sigma in enumerate(SHIFTS):
        parts = [torch.zeros(x[s].size, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(parts, torch.from_numpy(x[s].reshape(-1).copy()))
        full = np.zeros((V, 12, 2))
        for r, part in enumerate(parts):                 # split in T: rank r owns the lexicographic sites [r Vl, (r + 1) Vl)
            full[r * Vl:(r + 1) * Vl] = part.numpy().reshape(Vl, 12, 2)
        xe = np.where(odd, 0.0, full)
        Sx, _, psi = eo.schur(G, D, cl, xe)
        Qx = eo.schur(G, D, cl, Sx, True)[0]
        true = float(np.linalg.norm(be - Qx - sigma * xe) / np.linalg.norm(be))
        err_odd = float(np.linalg.norm(np.where(odd, full, 0.0) - psi) / np.linalg.norm(psi))
        print(f"rank {rank}: shift {sigma}: relres {rr[s]:.3e} (numpy {true:.3e}), odd part relerr {err_odd:.2e}", flush=True)
        # the device's and numpy's residual differ by the rounding of the products: 5e-12, as in test_gpu_eo_system.py
        assert abs(true - rr[s]) <= 0.05 * TOL and err_odd < 1e-13, (sigma, rr[s], true, err_odd)
    dist.barrier()
    ctx.close()
    ok = torch.tensor([1.0], dtype=torch.float64)
    dist.all_reduce(ok)
    if rank == 0 and ok.item() == world:
        print("DIST_MULTISHIFT_OK", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
