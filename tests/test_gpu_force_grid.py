"""The fermion force on a process grid (-m gpu): ddamg_hip_force_bilinear_vec_grid / _device_grid and ddamg_hip_force_logdet_grid.
One process: a process-grid entry of -1 makes the process its own neighbour over RCCL, so the shell of W = 2 D, the shell of the site
tensor and the face spinors travel through pack -> send/recv -> unpack for real (contexts as in test_gpu_gauge_device_grid.py), and the
result must be the force of the undivided periodic lattice.  Several processes: tests/dist_force_worker.py over the host transport.

Bars.  Against tests/force_reference.py (pinned to finite differences of the oracle by test_force_reference.py): 1e-13 of the field's
norm, the project's fp64 bar, as in test_gpu_force.py.  Finite differences of the operator the grid context itself applies: the central
difference extrapolated once at h = 2^-8, within ten times its spread between h and 2h, the rule and the reason of test_gpu_force.py
test 6.  Lattices: 4x6x8x10 (tile tails of 6 and 10; a second tile only at the extended extents 10 and 12) with one split direction,
with a wrapped and a shell direction in one plane, and with all four; 2x4x6x4 with all four, where both neighbours of a site in T are
shell sites.
Measured on the MI355X: against the reference 2.1e-16 to 2.6e-16 (bilinear) and 9.0e-16 to 9.3e-16 (determinant) on every grid, and no
real differs in its bits from the same call on an undivided context; the grid context's own operator: derivative -21.05, spread
3.8e-6, difference 2.6e-7; several processes (8^4, host transport): 2.5e-16 and 1.0e-15 over the whole lattice.  Times:
docs/design/04_kernels.md, "Fermion force"."""
import os
import numpy as np
import pytest
from conftest import relerr, splitmix_uniform
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
import force_reference as fr
from test_gpu_device_interface import Hip, params, synth_field

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RAGGED = (4, 6, 8, 10)
SMALL = (2, 4, 6, 4)
ALL = (-1, -1, -1, -1)
CASES = [(RAGGED, (-1, 1, 1, 1)), (RAGGED, (1, -1, 1, -1)), (RAGGED, ALL), (SMALL, ALL)]
IDS = ["4x6x8x10-T", "4x6x8x10-ZX", "4x6x8x10-all", "2x4x6x4-all"]
M0, CSW = -0.3, 1.25
EPS = np.finfo(np.float64).eps
H = 2.0 ** -8
_fields, _reference = {}, {}


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.free_all()


def fields(L):
    """(links, X, Y) of a lattice, made once and never changed"""
    L = tuple(L)
    if L not in _fields:
        V = int(np.prod(L))
        f = (synth_field(L, 5), splitmix_uniform(V * 24, 9).reshape(V, 12, 2), splitmix_uniform(V * 24, 10).reshape(V, 12, 2))
        for a in f:
            a.setflags(write=False)
        _fields[L] = f
    return _fields[L]


def reference(L, csw, scale=(1.0, 1.0), m0=M0, par=None):
    """the reference force of the whole periodic lattice, computed once: bilinear (par None) or determinant"""
    key = (tuple(L), csw, scale, m0, par)
    if key not in _reference:
        U, X, Y = fields(L)
        f = fr.force_bilinear(list(L), U, 1, m0, csw, Y, X, scale) if par is None else fr.force_logdet(list(L), U, 1, m0, csw, par, scale)
        f.setflags(write=False)
        _reference[key] = f
    return _reference[key]


def context(L, grid, hip, csw=CSW, m0=M0):
    """a one-level context on the grid (RCCL where it is divided), the links through set_gauge_device_grid; returns (ctx, links on the device)"""
    ctx = dd.Context(params(list(L), [2] * 4, m0, csw, grid=grid))
    if min(grid) < 0:
        ctx.comm_init_rccl(api.rccl_unique_id())
    dU = hip.upload(fields(L)[0])
    ctx.set_gauge_device_grid(dU, anti_pbc=True)
    return ctx, dU


def nbytes(L):
    return int(np.prod(L)) * 72 * 8


def by_vec(ctx, hip, L, y, x, coeff=1.0, accumulate=False, out=None):
    """the force through the _vec_grid entry point, downloaded; the vectors are checked to be unchanged"""
    vy = ctx.vector(0, 64).upload(y); vx = ctx.vector(0, 64).upload(x)
    out = hip.alloc(nbytes(L)) if out is None else out
    assert ctx.force_bilinear_vec_grid(out, vy, vx, coeff, accumulate) == out
    assert np.array_equal(vy.download(), y) and np.array_equal(vx.download(), x)
    vy.free(); vx.free()
    return hip.download(out, (len(x), 4, 9, 2))


def by_device(ctx, hip, L, y, x, coeff=1.0, accumulate=False, out=None):
    dy = hip.upload(y); dx = hip.upload(x)
    out = hip.alloc(nbytes(L)) if out is None else out
    ctx.force_bilinear_device_grid(out, dy, dx, coeff, accumulate)
    assert np.array_equal(hip.download(dy, y.shape), y) and np.array_equal(hip.download(dx, x.shape), x)
    return hip.download(out, (len(x), 4, 9, 2))


def logdet_force(ctx, hip, L, par, coeff=1.0):
    out = hip.alloc(nbytes(L))
    ctx.force_logdet_grid(out, par, coeff)
    return hip.download(out, (int(np.prod(L)), 4, 9, 2))


def different_bits(a, b):
    return int(np.count_nonzero(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)))


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("csw", [CSW, 0.0])
@pytest.mark.parametrize("L,grid", CASES, ids=IDS)
def test_forces_against_the_reference(L, grid, csw, hip):
    _, X, Y = fields(L)
    ctx, _ = context(L, grid, hip, csw)
    got = by_vec(ctx, hip, L, Y, X)
    err = relerr(got, reference(L, csw))
    print(L, grid, "csw", csw, "bilinear: norm", np.linalg.norm(got), "relerr", err)
    assert err < 1e-13
    assert np.array_equal(by_device(ctx, hip, L, Y, X), got)          # the same bits from both entry points
    assert np.array_equal(by_vec(ctx, hip, L, Y, X), got)             # ... and from two calls
    ld = {}
    for par in (0, 1):
        ld[par] = logdet_force(ctx, hip, L, par)
        if csw == 0.0:                                                # C is a constant: the force is zero, exactly
            assert not ld[par].any()
            continue
        ref = reference(L, csw, par=par)
        err = relerr(ld[par], ref)
        print(L, grid, "determinant, parity", par, "norm", np.linalg.norm(ref), "relerr", err)
        assert err < 1e-13
        assert np.array_equal(logdet_force(ctx, hip, L, par), ld[par])
    ctx.close()
    # the difference to the same calls on an undivided context (reported; nothing is required of it)
    plain = dd.Context(params(list(L), [2] * 4, M0, csw))
    plain.set_gauge_device(hip.upload(fields(L)[0]), anti_pbc=True)
    vy = plain.vector(0, 64).upload(Y); vx = plain.vector(0, 64).upload(X); out = hip.alloc(nbytes(L))
    plain.force_bilinear_vec(out, vy, vx)
    report = [different_bits(hip.download(out, got.shape), got)]
    for par in (0, 1):
        plain.force_logdet(out, par)
        report.append(different_bits(hip.download(out, got.shape), ld[par]))
    print(L, grid, "csw", csw, "reals that differ in their bits from the undivided context's (bilinear, even, odd):", report, "of", got.size)
    vy.free(); vx.free(); plain.close()


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,grid", [CASES[1], CASES[3]], ids=[IDS[1], IDS[3]])
def test_the_force_is_in_the_algebra_and_nothing_else_is_written(L, grid, hip):
    """every matrix anti-Hermitian (exactly: it is unpacked from nine reals) and traceless to the rounding of the three-term sum; the
    operator and the caller's links unchanged (the caller's vectors: by_vec / by_device)"""
    U, X, Y = fields(L)
    ctx, dU = context(L, grid, hip)
    D0, cl0 = ctx.get_operator()
    forces = [by_vec(ctx, hip, L, Y, X), by_device(ctx, hip, L, Y, X), logdet_force(ctx, hip, L, 0), logdet_force(ctx, hip, L, 1)]
    for f in forces:
        g = fr.as_matrices(f)
        assert np.array_equal(g, -fr.dag(g)) and np.abs(np.trace(g, axis1=-2, axis2=-1)).max() <= 4 * EPS * np.abs(g).max()
    D1, cl1 = ctx.get_operator()
    assert np.array_equal(D0, D1) and np.array_equal(cl0, cl1) and np.array_equal(hip.download(dU, U.shape), U)
    ctx.close()


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_coeff_and_accumulate(hip):
    L = RAGGED
    _, X, Y = fields(L)
    X2 = splitmix_uniform(X.size, 11).reshape(X.shape)
    ctx, _ = context(L, ALL, hip)
    f1 = by_vec(ctx, hip, L, Y, X)
    f2 = by_vec(ctx, hip, L, Y, X2)
    assert relerr(by_vec(ctx, hip, L, Y, X, coeff=-2.0), -2.0 * f1) <= EPS          # coeff scales the result
    assert relerr(by_device(ctx, hip, L, Y, X, coeff=0.7), 0.7 * f1) <= EPS
    # accumulate: what the array held plus coeff times the force, from both entry points and from the determinant's
    start = splitmix_uniform(f1.size, 12).reshape(f1.shape)
    out = hip.upload(start)
    assert relerr(by_vec(ctx, hip, L, Y, X, coeff=0.7, accumulate=True, out=out), start + 0.7 * f1) <= 2 * EPS
    assert relerr(by_device(ctx, hip, L, Y, X2, coeff=-1.5, accumulate=True, out=out), start + 0.7 * f1 - 1.5 * f2) <= 4 * EPS
    ld = logdet_force(ctx, hip, L, 1)
    ctx.force_logdet_grid(out, 1, -2.0, True)
    assert relerr(hip.download(out, f1.shape), start + 0.7 * f1 - 1.5 * f2 - 2.0 * ld) <= 6 * EPS
    ctx.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_scale_and_mass(hip):
    """the expectations of test_gpu_force.py test 5, on the grid"""
    L = SMALL
    _, X, Y = fields(L)
    ctx, _ = context(L, ALL, hip)
    plain = {par: logdet_force(ctx, hip, L, par) for par in (0, 1)}
    bilinear = by_vec(ctx, hip, L, Y, X)
    # scale_clover: the factor cancels in log det up to a constant; the clover part of the bilinear force carries s(x)
    ctx.scale_clover(1.1, 0.9)
    for par in (0, 1):
        assert relerr(logdet_force(ctx, hip, L, par), plain[par]) < 1e-13
    scaled = by_vec(ctx, hip, L, Y, X)
    assert relerr(scaled, reference(L, CSW, scale=(1.1, 0.9))) < 1e-13 and relerr(scaled, bilinear) > 1e-3
    ctx.scale_clover(1.0, 1.0)
    assert np.array_equal(by_vec(ctx, hip, L, Y, X), bilinear)
    # shift_mass: neither the hopping nor the clover term holds the mass: the same bits; the determinant follows the new mass
    ctx.shift_mass(0.05)
    assert np.array_equal(by_vec(ctx, hip, L, Y, X), bilinear)
    for par in (0, 1):
        shifted = logdet_force(ctx, hip, L, par)
        assert relerr(shifted, reference(L, CSW, m0=0.05, par=par)) < 1e-13 and relerr(shifted, plain[par]) > 1e-3
    ctx.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_derivative_of_the_operator_the_grid_context_applies(hip):
    """no reference code: S(eps) = Re <Y, D X> through set_gauge_device_grid on exp(eps Omega) U, dirac_apply in fp64 and vec_dot"""
    L = (4, 4, 4, 4)
    U, X, Y = fields(L)
    omega = fr.random_algebra(np.random.default_rng(31), (len(X), 4))
    ctx, _ = context(L, ALL, hip)
    vy = ctx.vector(0, 64).upload(Y); vx = ctx.vector(0, 64).upload(X); vz = ctx.vector(0, 64)

    def S(eps):
        ctx.set_gauge_device_grid(hip.upload(fr.perturbed(U, omega, eps)), anti_pbc=True)
        ctx.dirac_apply(vz, vx)
        return ctx.vec_dot(vy, vz)[0].real
    fine, coarse = fr.richardson(S, H), fr.richardson(S, 2 * H)
    ctx.set_gauge_device_grid(hip.upload(U), anti_pbc=True)
    out = hip.alloc(nbytes(L))
    ctx.force_bilinear_vec_grid(out, vy, vx)
    mine = fr.pairing(omega, hip.download(out, (len(X), 4, 9, 2)))
    spread = abs(fine - coarse)
    print(f"derivative {fine:+.12e} force {mine:+.12e} spread {spread:.2e} difference {abs(mine - fine):.2e}")
    assert abs(fine) > 1.0 and abs(mine - fine) <= 10 * spread
    for v in (vy, vx, vz):
        v.free()
    ctx.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(1, -1, 1, -1), ALL], ids=["ZX", "all"])
def test_messages_per_call(grid, hip):
    """what docs/design/06_multi_gpu.md states: per split direction 2 messages for the shell of the links, 2 for that of the site
    tensor (clover term only) and 1 for the face spinors (bilinear only)"""
    L = SMALL
    _, X, Y = fields(L)
    nsplit = sum(1 for e in grid if e == -1)
    V = int(np.prod(L))
    sh = shell_sites(L, grid)
    for csw, bilinear, logdet in ((CSW, 5 * nsplit, 4 * nsplit), (0.0, nsplit, 0)):
        ctx, _ = context(L, grid, hip, csw)
        vy = ctx.vector(0, 64).upload(Y); vx = ctx.vector(0, 64).upload(X); out = hip.alloc(nbytes(L))
        dy = hip.upload(Y); dx = hip.upload(X)
        faces = sum(V // L[mu] for mu in range(4) if grid[mu] == -1)
        for call, messages, sent in ((lambda: ctx.force_bilinear_vec_grid(out, vy, vx), bilinear, 384 * faces + (126 * 8 * sh if csw else 0)),
                                     (lambda: ctx.force_bilinear_device_grid(out, dy, dx), bilinear, 384 * faces + (126 * 8 * sh if csw else 0)),
                                     (lambda: ctx.force_logdet_grid(out, 1), logdet, 126 * 8 * sh if csw else 0)):
            ctx.comm_stats(reset=True)
            call()
            shell = ctx.comm_stats()["device_sendrecv"]
            print(grid, "csw", csw, shell)
            assert shell["messages"] == messages and shell["bytes_sent"] == sent
        vy.free(); vx.free(); ctx.close()


def shell_sites(L, grid):
    """slab sites sent per call and field: both sides of every split direction, each slab spanning the extended range of the split
    directions before it and the own range of those after it (field_strength.h, make_slab)"""
    total = 0
    for mu in range(4):
        if grid[mu] != -1:
            continue
        n = 1
        for d in range(4):
            if d != mu:
                n *= L[d] + 2 if (d < mu and grid[d] == -1) else L[d]
        total += 2 * n
    return total


# 7 ------------------------------------------------------------------------------------------------------------------------
def refused(call, *words):
    with pytest.raises(api.DDAMGError) as e:
        call()
    assert all(w in str(e.value) for w in words), str(e.value)


def reference_operator(L):
    """(D, clover) of the lattice's links from an undivided context: something to give set_operator"""
    ctx = dd.Context(params(list(L), [2] * 4, M0, CSW))
    ctx.set_gauge(fields(L)[0], anti_pbc=True)
    op = ctx.get_operator()
    ctx.close()
    return op


def test_refusals_on_a_divided_context(hip):
    L = SMALL
    U, X, Y = fields(L)
    V = len(X)
    ctx, dU = context(L, ALL, hip)
    out = hip.alloc(nbytes(L)); dx = hip.upload(X); dy = hip.upload(Y)
    y64 = ctx.vector(0, 64).upload(Y); x64 = ctx.vector(0, 64).upload(X); y32 = ctx.vector(0, 32); x32 = ctx.vector(0, 32)
    good = by_vec(ctx, hip, L, Y, X)
    ctx.comm_stats(reset=True)
    refused(lambda: ctx.force_bilinear_vec_grid(out, y32, x32), "fp32")
    refused(lambda: ctx.force_bilinear_vec_grid(out, y64, x32), "fp32")
    host = np.zeros(V * 72)
    refused(lambda: ctx.force_bilinear_vec_grid(int(host.ctypes.data), y64, x64), "not a pointer into device memory")
    refused(lambda: ctx.force_bilinear_device_grid(out, int(host.ctypes.data), dx), "not a pointer into device memory")
    refused(lambda: ctx.force_logdet_grid(int(host.ctypes.data), 0), "not a pointer into device memory")
    refused(lambda: ctx.force_bilinear_device_grid(out, dy, out + 8 * 24), "overlap")
    refused(lambda: ctx.force_logdet_grid(out, 2), "parity")
    refused(lambda: ctx.force_logdet_grid(out, -1), "parity")
    # the forms without _grid keep refusing, and name the ones that work here
    refused(lambda: ctx.force_bilinear_vec(out, y64, x64), "process grid", "not built yet", "ddamg_hip_force_bilinear_vec_grid")
    refused(lambda: ctx.force_bilinear_device(out, dy, dx), "process grid", "ddamg_hip_force_bilinear_device_grid")
    refused(lambda: ctx.force_logdet(out, 1), "process grid", "ddamg_hip_force_logdet_grid")
    # operators with no single link field behind them
    ctx.set_operator(*ctx.get_operator())
    refused(lambda: ctx.force_bilinear_vec_grid(out, y64, x64), "did not come from one link field")
    refused(lambda: ctx.force_logdet_grid(out, 1), "did not come from one link field")
    ctx.set_gauge2_device_grid(dU, hip.upload(synth_field(L, 6)), anti_pbc=True)
    refused(lambda: ctx.force_bilinear_device_grid(out, dy, dx), "did not come from one link field")
    assert ctx.comm_stats()["device_sendrecv"]["messages"] == 2 * 4      # the two-field links' shell and nothing else: no refusal sent anything
    # ... and the context serves again once it has one
    ctx.set_gauge_device_grid(dU, anti_pbc=True)
    assert np.array_equal(by_vec(ctx, hip, L, Y, X), good)
    for v in (y64, x64, y32, x32):
        v.free()
    ctx.close()
    # a grid without a transport
    bare = dd.Context(params(list(L), [2] * 4, M0, CSW, grid=ALL))
    bare.set_operator(*reference_operator(L))
    for call in (lambda: bare.force_logdet_grid(out, 1), lambda: bare.force_bilinear_device_grid(out, dy, dx)):
        refused(call, "install a transport first")
    bare.close()
    # csw = 0 and m0 = -4: every clover block is zero
    ctx, _ = context(L, ALL, hip, csw=0.0, m0=-4.0)
    refused(lambda: ctx.force_logdet_grid(out, 1), "singular", "parity 1")
    refused(lambda: ctx.force_logdet_grid(out, 0), "singular", "parity 0")
    ctx.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_undivided_context_runs_the_plain_calls(hip):
    L = RAGGED
    U, X, Y = fields(L)
    ctx, _ = context(L, (1, 1, 1, 1), hip)
    vy = ctx.vector(0, 64).upload(Y); vx = ctx.vector(0, 64).upload(X); dy = hip.upload(Y); dx = hip.upload(X)
    a, b = hip.alloc(nbytes(L)), hip.alloc(nbytes(L))
    shape = (len(X), 4, 9, 2)
    ctx.force_bilinear_vec(a, vy, vx, 0.7); ctx.force_bilinear_vec_grid(b, vy, vx, 0.7)
    assert different_bits(hip.download(a, shape), hip.download(b, shape)) == 0
    ctx.force_bilinear_device(a, dy, dx, -1.5, True); ctx.force_bilinear_device_grid(b, dy, dx, -1.5, True)
    assert different_bits(hip.download(a, shape), hip.download(b, shape)) == 0
    for par in (0, 1):
        ctx.force_logdet(a, par, 2.0, True); ctx.force_logdet_grid(b, par, 2.0, True)
        assert different_bits(hip.download(a, shape), hip.download(b, shape)) == 0
    assert relerr(hip.download(a, shape), 0.7 * reference(L, CSW) - 1.5 * reference(L, CSW) + 2.0 * (reference(L, CSW, par=0) + reference(L, CSW, par=1))) < 1e-12
    vy.free(); vx.free(); ctx.close()


# several processes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nproc,grid", [(2, "2,1,1,1"), (2, "1,1,1,2"), (4, "2,2,1,1")])
def test_forces_on_a_process_grid(nproc, grid):
    """every rank computes its part of the bilinear force and of both determinant forces of the golden 8^4 links over the host
    transport, against its part of the reference of the whole lattice; 2,2,1,1: corners from a diagonal process.  2,1,1,1 also runs
    the singular-block refusal, which every rank must return"""
    from launcher import torchrun
    r = torchrun(nproc, os.path.join(HERE, "dist_force_worker.py"), "--grid", grid, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DIST_FORCE_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout[-1500:])
