"""The many-pair fermion force on a process grid (-m gpu): ddamg_hip_force_bilinear_multi_vec_grid / _device_grid and
ddamg_hip_force_rational_device_grid.  One process: a process-grid entry of -1 makes the process its own neighbour over RCCL, so the
link shell, the tensor shell and the face spinors of a whole group travel through pack -> send/recv -> unpack for real (contexts as in
test_gpu_force_grid.py).  The sums and their order are those of the undivided kernel, so every form must equal the undivided context
BIT FOR BIT, as the single-pair grid forms do.  Lattices: 8^4 and 4x4x6x6 (a half-filled last workgroup), all four directions split
and two of them (a wrapped and a shell direction in one plane), with G + 1 pairs: a full group and a partial one.
Messages per call and split direction: 2 (link shell) + 2 (tensor shell) with a clover term, and ceil(n / G) for the faces, each of
384 bytes per face site and pair.  Two processes: tests/dist_force_multi_worker.py over the host transport, 1e-13 of the norm.
Measured on the MI355X: no real differs in its bits on any grid; two processes: both ranks' parts equal the undivided rows exactly."""
import os
import numpy as np
import pytest
from conftest import splitmix_uniform
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
import eo_reference as eo
from test_gpu_force_grid import context, fields, nbytes, different_bits, shell_sites, refused, CSW, ALL, Hip

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = api.FORCE_GROUP
N = G + 1
WEIGHTS = [0.3, -1.1, 2.5, -0.04, 7.0, 1.0, -3.2, 0.6, 1.7]
RHO = [0.3, -1.1, 2.5, 0.04, 7.0, 1.0, 3.2, 0.6, 1.7]
LATS = [(8, 8, 8, 8), (4, 4, 6, 6)]
GRIDS = [ALL, (1, 1, -1, -1)]
_pairs = {}


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.free_all()


def pairs(L):
    """N pairs (Y_s, X_s) and N even half fields of a lattice, made once and never changed"""
    L = tuple(L)
    if L not in _pairs:
        V = int(np.prod(L))
        even = eo.parity(list(L)) == 0
        p = ([splitmix_uniform(V * 24, 100 + 2 * s).reshape(V, 12, 2) for s in range(N)], [splitmix_uniform(V * 24, 101 + 2 * s).reshape(V, 12, 2) for s in range(N)],
             [np.ascontiguousarray(splitmix_uniform(V * 24, 200 + s).reshape(V, 12, 2)[even]) for s in range(N)])
        for group in p:
            for a in group:
                a.setflags(write=False)
        _pairs[L] = p
    return _pairs[L]


def all_forms(ctx, hip, L, grid_forms):
    """(multi_vec, multi_device, rational) of the context, through the _grid forms or the plain ones"""
    Y, X, xe = pairs(L)
    V = len(Y[0])
    sfx = "_grid" if grid_forms else ""
    out = hip.alloc(nbytes(L))
    ys = [ctx.vector(0, 64).upload(y) for y in Y]; xs = [ctx.vector(0, 64).upload(x) for x in X]
    getattr(ctx, "force_bilinear_multi_vec" + sfx)(out, ys, xs, WEIGHTS[:N], -2.0)
    res = [hip.download(out, (V, 4, 9, 2))]
    for v in ys + xs:
        v.free()
    getattr(ctx, "force_bilinear_multi_device" + sfx)(out, [hip.upload(y) for y in Y], [hip.upload(x) for x in X], WEIGHTS[:N], -2.0)
    res.append(hip.download(out, (V, 4, 9, 2)))
    getattr(ctx, "force_rational_device" + sfx)(out, RHO[:N], [hip.upload(h) for h in xe], None, -2.0)
    res.append(hip.download(out, (V, 4, 9, 2)))
    return res


_undivided = {}


def undivided(L, hip):
    if tuple(L) not in _undivided:
        ctx, _ = context(L, (1, 1, 1, 1), hip)
        _undivided[tuple(L)] = all_forms(ctx, hip, L, False)
        # on an undivided context the _grid forms are the plain ones
        for a, b in zip(all_forms(ctx, hip, L, True), _undivided[tuple(L)]):
            assert different_bits(a, b) == 0
        ctx.close()
    return _undivided[tuple(L)]


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS, ids=["all", "YX"])
@pytest.mark.parametrize("L", LATS, ids=["8^4", "4x4x6x6"])
def test_every_form_equals_the_undivided_context_bit_for_bit(L, grid, hip):
    want = undivided(L, hip)
    ctx, _ = context(L, grid, hip)
    got = all_forms(ctx, hip, L, True)
    ctx.close()
    report = [different_bits(a, b) for a, b in zip(got, want)]
    print(L, grid, "norms", [float(np.linalg.norm(a)) for a in want], "reals that differ in their bits (multi_vec, multi_device, rational):", report)
    assert all(np.linalg.norm(a) > 1.0 for a in want) and report == [0, 0, 0]


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS, ids=["all", "YX"])
def test_messages_per_call(grid, hip):
    L = (4, 4, 6, 6)
    Y, X, xe = pairs(L)
    V = int(np.prod(L))
    nsplit = sum(1 for e in grid if e == -1)
    faces = sum(V // L[mu] for mu in range(4) if grid[mu] == -1)
    sh = shell_sites(L, grid)
    for csw in (CSW, 0.0):
        ctx, _ = context(L, grid, hip, csw)
        out = hip.alloc(nbytes(L))
        ys = [ctx.vector(0, 64).upload(y) for y in Y]; xs = [ctx.vector(0, 64).upload(x) for x in X]
        dy = [hip.upload(y) for y in Y]; dx = [hip.upload(x) for x in X]
        for n in (1, G, N):
            messages = nsplit * ((4 if csw else 0) + -(-n // G))
            sent = 384 * n * faces + (126 * 8 * sh if csw else 0)
            for call in (lambda: ctx.force_bilinear_multi_vec_grid(out, ys[:n], xs[:n], WEIGHTS[:n]),
                         lambda: ctx.force_bilinear_multi_device_grid(out, dy[:n], dx[:n], WEIGHTS[:n])):
                ctx.comm_stats(reset=True)
                call()
                shell = ctx.comm_stats()["device_sendrecv"]
                print(grid, "csw", csw, "pairs", n, shell)
                assert shell["messages"] == messages and shell["bytes_sent"] == sent
        for v in ys + xs:
            v.free()
        ctx.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_divided_context_come_before_any_message(hip):
    L = (4, 4, 6, 6)
    Y, X, xe = pairs(L)
    V = int(np.prod(L))
    ctx, _ = context(L, ALL, hip)
    out = hip.alloc(nbytes(L)); dy = hip.upload(Y[0]); dx = hip.upload(X[0]); half = hip.upload(xe[0])
    vy = ctx.vector(0, 64).upload(Y[0]); vx = ctx.vector(0, 64).upload(X[0]); v32 = ctx.vector(0, 32)
    ctx.comm_stats(reset=True)
    nan = float("nan")
    refused(lambda: ctx.force_bilinear_multi_vec_grid(out, [], [], []), "npairs = 0")
    refused(lambda: ctx.force_bilinear_multi_device_grid(out, [dy] * 33, [dx] * 33, [1.0] * 33), "npairs = 33")
    refused(lambda: ctx.force_rational_device_grid(out, [], []), "nshift = 0")
    refused(lambda: ctx.force_bilinear_multi_vec_grid(out, [vy, None], [vx, vx], [1.0, 1.0]), "null argument")
    refused(lambda: ctx.force_bilinear_multi_device_grid(out, [dy, dy], [dx, dx], [1.0, nan]), "weight 1 is not finite")
    refused(lambda: ctx.force_rational_device_grid(out, [nan], [half]), "weight 0 is not finite")
    refused(lambda: ctx.force_bilinear_multi_vec_grid(out, [vy, v32], [vx, vx], [1.0, 1.0]), "fp32")
    host = np.zeros(V * 72)
    refused(lambda: ctx.force_bilinear_multi_device_grid(out, [dy], [int(host.ctypes.data)], [1.0]), "not a pointer into device memory")
    refused(lambda: ctx.force_bilinear_multi_device_grid(out, [dy, dy], [dx, out + 8 * 24], [1.0, 1.0]), "overlap")
    refused(lambda: ctx.force_rational_device_grid(out, [1.0, 1.0], [half, out + 64]), "overlap")
    # the forms without _grid refuse, and name the ones that work here
    refused(lambda: ctx.force_bilinear_multi_vec(out, [vy], [vx], [1.0]), "process grid", "ddamg_hip_force_bilinear_multi_vec_grid")
    refused(lambda: ctx.force_bilinear_multi_device(out, [dy], [dx], [1.0]), "process grid", "ddamg_hip_force_bilinear_multi_device_grid")
    refused(lambda: ctx.force_rational_device(out, [1.0], [half]), "process grid", "ddamg_hip_force_rational_device_grid")
    ctx.set_operator(*ctx.get_operator())
    refused(lambda: ctx.force_bilinear_multi_vec_grid(out, [vy], [vx], [1.0]), "did not come from one link field")
    refused(lambda: ctx.force_rational_device_grid(out, [1.0], [half]), "did not come from one link field")
    assert ctx.comm_stats()["device_sendrecv"]["messages"] == 0      # no refusal sent anything
    for v in (vy, vx, v32):
        v.free()
    ctx.close()
    # a grid without a transport
    bare = dd.Context(api_params(L))
    refused(lambda: bare.force_bilinear_multi_device_grid(out, [dy], [dx], [1.0]), "install a transport first")
    bare.close()


def api_params(L):
    from test_gpu_device_interface import params
    from test_gpu_force_grid import M0
    return params(list(L), [2] * 4, M0, CSW, grid=ALL)


# several processes --------------------------------------------------------------------------------------------------------
def test_two_processes():
    """8x4x4x4 split in T over the host transport: each rank's part against the rows of the undivided result"""
    from launcher import torchrun
    r = torchrun(2, os.path.join(HERE, "dist_force_multi_worker.py"), "--grid", "2,1,1,1", timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DIST_FORCE_MULTI_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
