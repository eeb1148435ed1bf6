"""Worker of the two-process test of the even-odd preconditioned system (started through torch.distributed.run, gloo backend, host
transport; both ranks share the one test GPU).  The lattice is 8x4x4x4 split in T.  ddamg_hip_clover_logdet on both ranks must give
the value of the undivided lattice (one all-reduce of the partial sums), and one Schur solve on a two-level hierarchy must reach
its tolerance, with the residual of the Schur system recomputed from the parts of x_e on both ranks."""
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


def params(lat, grid, coords, levels):
    p = api.default_params(); p.num_levels = levels
    for mu in range(4):
        p.local_lattice[0][mu] = lat[mu]; p.block_lattice[0][mu] = 2; p.local_lattice[1][mu] = lat[mu] // 2
        p.process_grid[mu] = grid[mu]; p.process_coords[mu] = coords[mu]
    p.num_vect[0] = 8; p.post_smooth_iter[0] = 2; p.block_iter[0] = 4; p.setup_iter[0] = 2
    p.restart, p.max_restart, p.tol = 30, 20, TOL
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 100, 5, 5e-2
    p.mixed_precision, p.method, p.m0, p.csw = 1, 2, M0, CSW
    p.test_vector_rng, p.rng_seed = 1, 11
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

    whole = dd.Context(params(G, [1] * 4, [0] * 4, 1))
    whole.set_gauge(U, anti_pbc=True)
    D, cl = whole.get_operator()
    want = [whole.clover_logdet(par) for par in (0, 1)]
    whole.close()
    B = eo.clover_blocks(cl)
    bar = [1e-13 * float(np.sum(np.abs(np.linalg.slogdet(B[eo.parity(G) == par])[1]))) for par in (0, 1)]

    ctx = dd.Context(params(L, P, C, 2))
    ddist.attach_host(ctx)
    ctx.set_gauge(lp(U), anti_pbc=True)
    for par in (0, 1):
        got = ctx.clover_logdet(par)
        print(f"rank {rank}: parity {par} log|det| {got[0]!r} sign {got[1]} (undivided {want[par][0]!r}), bar {bar[par]:.2e}", flush=True)
        assert got[1] == want[par][1] == 1 and abs(got[0] - want[par][0]) <= bar[par], (got, want[par])
    ctx.setup(2)
    vb = ctx.vector(0, 64).upload(lp(b)); vx = ctx.vector(0, 64)
    it, cit, rr = ctx.solve_schur_vec(vx, vb, TOL)
    x = vx.download()
    vb.free(); vx.free()
    # the whole x_e from both ranks, and the Schur residual of it in numpy
    parts = [torch.zeros(x.size, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(parts, torch.from_numpy(x.reshape(-1).copy()))
    full = np.zeros((V, 12, 2))
    Vl = V // world
    for r, part in enumerate(parts):                 # split in T: rank r owns the lexicographic sites [r Vl, (r + 1) Vl)
        full[r * Vl:(r + 1) * Vl] = part.numpy().reshape(Vl, 12, 2)
    odd = eo.parity(G)[:, None, None] == 1
    be = np.where(odd, 0.0, b)
    xe = np.where(odd, 0.0, full)
    Sx, rest, psi = eo.schur(G, D, cl, xe)
    true = float(np.linalg.norm(be - Sx) / np.linalg.norm(be))
    err_odd = float(np.linalg.norm(np.where(odd, full, 0.0) - psi) / np.linalg.norm(psi))
    print(f"rank {rank}: {it} iterations, relres {rr:.3e} (numpy {true:.3e}), odd part relerr {err_odd:.2e}", flush=True)
    # the device's and numpy's residual differ by the rounding of the products, 2 * 64 eps || |Dhat| |x| || / ||b||: 3e-14 times a
    # ratio that is below 30 at this mass
    assert it > 0 and rr <= TOL and abs(true - rr) <= 1e-12 and err_odd < 1e-13, (it, rr, true, err_odd)
    dist.barrier()
    ctx.close()
    ok = torch.tensor([1.0], dtype=torch.float64)
    dist.all_reduce(ok)
    if rank == 0 and ok.item() == world:
        print("DIST_EO_OK", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
