"""Worker of the multi-process tests of links in device memory (started through torch.distributed.run, gloo backend, host
transport; all ranks share the one test GPU).

mode gauge: every rank uploads its part of the golden 8^4 links to the device and calls set_gauge_device_grid; the operator must be
    its part of the one built on the undivided lattice (D bit for bit, clover term to 1e-14), the plaquette the global one, and one
    dirac_apply per precision the golden output.
mode ildg: rank 0 writes the links as an ILDG file, every rank loads its own part with load_ildg_conf in chunks that end inside rows,
    against set_gauge of the same part.
"""
import argparse, ctypes, os, sys
import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
from ddalphaamg_amd import api, dist as ddist  # noqa: E402

G = [8, 8, 8, 8]


def relerr(a, b):
    a = np.asarray(a, dtype=np.float64).ravel(); b = np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


class Hip:
    """hipMalloc / hipMemcpy / hipFree of the libamdhip64 that libddamg_hip.so is linked to"""

    def __init__(self):
        api.load_library()
        path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
        self.lib = ctypes.CDLL(path)
        self.lib.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.lib.hipFree.argtypes = [ctypes.c_void_p]

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = ctypes.c_void_p()
        assert self.lib.hipMalloc(ctypes.byref(p), a.nbytes) == 0
        assert self.lib.hipMemcpy(p.value, a.ctypes.data, a.nbytes, 1) == 0
        return p.value

    def download(self, p, shape):
        out = np.empty(shape, dtype=np.float64)
        assert self.lib.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0
        return out

    def free(self, p):
        self.lib.hipFree(p)


def params(g, lat, grid, coords):
    p = api.default_params(); p.num_levels = 1
    for mu in range(4):
        p.local_lattice[0][mu] = lat[mu]; p.block_lattice[0][mu] = 2
        p.process_grid[mu] = grid[mu]; p.process_coords[mu] = coords[mu]
    p.m0, p.csw = float(g["meta_f64"][0]), float(g["meta_f64"][1])
    return p


def undivided(g):
    import ddalphaamg_amd as dd
    whole = dd.Context(params(g, G, [1] * 4, [0] * 4))
    plaq = whole.set_gauge(g["gauge"], anti_pbc=True)
    D, cl = whole.get_operator()
    whole.close()
    return D, cl, plaq


def run_gauge(rank, P):
    import ddalphaamg_amd as dd
    g = np.load(os.path.join(HERE, "golden", "ref_8x8_dirac.npz"))
    L = [G[mu] // P[mu] for mu in range(4)]
    C = ddist.coords_of(rank, P)
    lp = lambda a: ddist.local_part(a, G, P, C)
    D, cl, plaq = undivided(g)
    assert abs(plaq - float(g["meta_f64"][2])) < 1e-12, plaq
    hip = Hip()
    mine = np.ascontiguousarray(lp(g["gauge"].reshape(4096, -1)))
    dU = hip.upload(mine)
    ctx = dd.Context(params(g, L, P, C))
    ddist.attach_host(ctx)
    plaq_d = ctx.set_gauge_device_grid(dU, anti_pbc=True)
    assert np.array_equal(hip.download(dU, mine.shape).view(np.uint64), mine.view(np.uint64)), "the caller's links were written"
    Dl, cll = ctx.get_operator()
    err_cl = relerr(cll, lp(cl))
    print(f"rank {rank}: plaquette {plaq_d!r} (undivided {plaq!r}), clover relerr {err_cl:.2e}", flush=True)
    assert abs(plaq_d - plaq) < 1e-12, (plaq_d, plaq)
    assert np.array_equal(Dl.reshape(-1), lp(D).reshape(-1)), "D differs from the part of the undivided operator"
    assert err_cl < 1e-14, err_cl
    for prec, ref, tol in ((64, "dirac_out_f64", 1e-13), (32, "dirac_out_f32_as_f64", 2e-6)):
        x = ctx.vector(0, prec).upload(lp(g["dirac_in"])); y = ctx.vector(0, prec)
        ctx.dirac_apply(y, x)
        want = lp(g[ref]).reshape(-1, 12, 2)
        sq = torch.tensor([float(np.sum((y.download() - want) ** 2)), float(np.sum(want ** 2))], dtype=torch.float64)
        dist.all_reduce(sq)
        err = float(np.sqrt(sq[0].item() / sq[1].item()))
        if rank == 0:
            print(f"dirac_apply fp{prec}: relerr {err:.2e} over the whole lattice", flush=True)
        assert err < tol, (prec, err)
        x.free(); y.free()
    shell = ctx.comm_stats()["device_sendrecv"]
    assert shell["messages"] == 2 * sum(1 for e in P if e > 1), shell
    dist.barrier()
    ctx.close()
    hip.free(dU)


def run_ildg(rank, P, directory):
    import ddalphaamg_amd as dd
    import lime_format as lf
    g = np.load(os.path.join(HERE, "golden", "ref_8x8_dirac.npz"))
    L = [G[mu] // P[mu] for mu in range(4)]
    C = ddist.coords_of(rank, P)
    path = os.path.join(directory, "conf.ildg")
    if rank == 0:
        lf.write_ildg(path, G, g["gauge"].reshape(4096, 4, 9, 2), 64)
    dist.barrier()
    os.environ["DDAMG_ILDG_CHUNK_SITES"] = "1001"     # the local lattice has rows of 4 sites: every chunk ends inside one, the last is short
    ctx = dd.Context(params(g, L, P, C))
    ddist.attach_host(ctx)
    plaq_h = ctx.set_gauge(ddist.local_part(g["gauge"].reshape(4096, -1), G, P, C), anti_pbc=True)
    Dh, clh = ctx.get_operator()
    plaq, _ = ctx.load_ildg_conf(path, anti_pbc=True)
    D, cl = ctx.get_operator()
    print(f"rank {rank}: plaquette {plaq!r} (set_gauge {plaq_h!r}), clover relerr {relerr(cl, clh):.2e}", flush=True)
    assert np.array_equal(D, Dh) and relerr(cl, clh) < 1e-14 and abs(plaq - plaq_h) < 1e-12
    dist.barrier()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="gauge")
    ap.add_argument("--grid", default="2,1,1,1")
    ap.add_argument("--dir", default=".")
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    P = [int(x) for x in a.grid.split(",")]
    assert int(np.prod(P)) == world and world <= 4
    if a.mode == "gauge":
        run_gauge(rank, P)
    else:
        run_ildg(rank, P, a.dir)
    ok = torch.tensor([1.0], dtype=torch.float64)
    dist.all_reduce(ok)
    if rank == 0 and ok.item() == world:
        print(f"DIST_GAUGE_DEVICE_OK mode={a.mode} grid={a.grid}", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
