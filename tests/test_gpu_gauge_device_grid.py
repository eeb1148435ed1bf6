"""Links in device memory on a process grid (-m gpu): ddamg_hip_set_gauge_device_grid / _set_gauge2_device_grid and the device path
of ddamg_hip_load_ildg_conf on a grid.  One process: a process-grid entry of -1 makes the process its own neighbour, so the shell of
links travels through pack -> RCCL send/recv -> unpack for real (contexts as in test_gpu_self_exchange.py), and the result must be
the operator of the undivided lattice.  Several processes: tests/dist_gauge_device_worker.py over the host transport."""
import os
import numpy as np
import pytest
from conftest import relerr
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
import lime_format as lf
import test_gpu_self_exchange as sx
from test_gpu_device_interface import Hip, params, check_dirac, synth_field

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RAGGED = [4, 6, 8, 10]     # tile tails, a second tile at the extended extents 10 and 12
SMALL = [2, 4, 6, 4]       # extent 2: both neighbours of a site are shell sites
ALL = [-1, -1, -1, -1]
M0, CSW = -0.3, 1.25
SENTINELS = 64


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.free_all()


def grid_context(p):
    ctx = dd.Context(p)
    ctx.comm_init_rccl(api.rccl_unique_id())
    return ctx


_UNDIVIDED = {}


def undivided(L, seed, anti_pbc):
    """(links, D, clover, plaquette) of ddamg_hip_set_gauge on the undivided lattice; computed once, never changed"""
    key = (tuple(L), seed, anti_pbc)
    if key not in _UNDIVIDED:
        U = synth_field(L, seed)
        ctx = dd.Context(params(L, [2] * 4, M0, CSW))
        plaq = ctx.set_gauge(U, anti_pbc=bool(anti_pbc))
        D, cl = ctx.get_operator()
        ctx.close()
        for a in (U, D, cl):
            a.setflags(write=False)
        _UNDIVIDED[key] = (U, D, cl, plaq)
    return _UNDIVIDED[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).ravel()


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [[-1, 1, 1, 1], [1, -1, 1, -1], ALL])
def test_grids_on_the_golden_case(gold8, hip, grid):
    ctx = grid_context(sx.params(gold8, grid))
    plaq = ctx.set_gauge_device_grid(hip.upload(gold8["gauge"]), anti_pbc=True)
    D, cl = ctx.get_operator()
    print("plaquette", plaq, "clover relerr", relerr(cl[::97], gold8["clover_sample"]))
    assert np.array_equal(D[::97], gold8["D_sample"])
    assert relerr(cl[::97], gold8["clover_sample"]) < 1e-14
    assert abs(plaq - float(gold8["meta_f64"][2])) < 1e-12
    check_dirac(ctx, gold8)
    shell = ctx.comm_stats()["device_sendrecv"]
    nsplit = sum(1 for e in grid if e == -1)
    assert shell["messages"] == 2 * nsplit and shell["bytes_sent"] > 0
    ctx.close()


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("anti_pbc", [0, 1])
@pytest.mark.parametrize("L", [RAGGED, SMALL], ids=["4x6x8x10", "2x4x6x4"])
def test_ragged_lattice_against_the_undivided_host_path(hip, L, anti_pbc):
    U, D0, cl0, plaq0 = undivided(L, 7, anti_pbc)
    ctx = grid_context(params(L, [2] * 4, M0, CSW, grid=ALL))
    plaq = ctx.set_gauge_device_grid(hip.upload(U), anti_pbc=bool(anti_pbc))
    D, cl = ctx.get_operator()
    ctx.close()
    print("clover relerr", relerr(cl, cl0), "plaquette", plaq, plaq0)
    assert np.array_equal(D, D0)
    assert relerr(cl, cl0) < 1e-14
    assert abs(plaq - plaq0) < 1e-12


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_two_fields(hip):
    U1, U2 = synth_field(SMALL, 7), synth_field(SMALL, 8)
    host = grid_context(params(SMALL, [2] * 4, M0, CSW, grid=ALL))
    plaq_h = host.set_gauge2(U1, U2, anti_pbc=True)
    Dh, clh = host.get_operator()
    host.close()
    ctx = grid_context(params(SMALL, [2] * 4, M0, CSW, grid=ALL))
    plaq = ctx.set_gauge2_device_grid(hip.upload(U1), hip.upload(U2), anti_pbc=True)
    D, cl = ctx.get_operator()
    ctx.close()
    print("clover relerr", relerr(cl, clh), "plaquette", plaq, plaq_h)
    assert np.array_equal(D, Dh) and relerr(cl, clh) < 1e-14 and abs(plaq - plaq_h) < 1e-12
    # D is the first field's, the clover term and the plaquette are the second's
    _, D2, cl2, plaq2 = undivided(SMALL, 8, 1)
    assert not np.array_equal(D, D2) and relerr(cl, cl2) < 1e-14 and abs(plaq - plaq2) < 1e-12


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_the_callers_arrays_are_not_written(hip):
    n = int(np.prod(SMALL)) * 72
    fields = []
    for seed in (7, 8):
        a = np.concatenate([synth_field(SMALL, seed).ravel(), np.full(SENTINELS, -123.456 - seed)])   # a sentinel region behind the links
        fields.append((a, hip.upload(a)))
    ctx = grid_context(params(SMALL, [2] * 4, M0, CSW, grid=ALL))
    ctx.set_gauge_device_grid(fields[0][1], anti_pbc=True)
    ctx.set_gauge2_device_grid(fields[0][1], fields[1][1], anti_pbc=True)
    ctx.close()
    for a, d in fields:
        assert np.array_equal(bits(hip.download(d, a.shape)), bits(a))
    assert a.size == n + SENTINELS


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_memory(gold8, hip):
    before = api.memory_in_use()
    ctx = grid_context(sx.params(gold8, ALL))
    ctx.set_gauge(gold8["gauge"], anti_pbc=True)
    with_host = api.memory_in_use()
    dU = hip.upload(gold8["gauge"])        # not the library's memory: not counted
    ctx.set_gauge_device_grid(dU, anti_pbc=True)
    with_device = api.memory_in_use()
    print("device, pinned bytes: after set_gauge", with_host, "after set_gauge_device_grid", with_device)
    assert with_device[0] <= with_host[0] and with_device[1] <= with_host[1]   # the extended array, F, the slab buffers, the staging: released
    ctx.close()
    assert api.memory_in_use() == before


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_undivided_context_runs_set_gauge_device(hip):
    U = synth_field(RAGGED, 7)
    dU, dU2 = hip.upload(U), hip.upload(synth_field(RAGGED, 8))
    ctx = dd.Context(params(RAGGED, [2] * 4, M0, CSW))
    plaq_a = ctx.set_gauge_device(dU, anti_pbc=True)
    Da, cla = ctx.get_operator()
    plaq_b = ctx.set_gauge_device_grid(dU, anti_pbc=True)
    Db, clb = ctx.get_operator()
    assert plaq_a == plaq_b and np.array_equal(bits(Da), bits(Db)) and np.array_equal(bits(cla), bits(clb))
    plaq_a = ctx.set_gauge2_device(dU, dU2, anti_pbc=False)
    Da, cla = ctx.get_operator()
    plaq_b = ctx.set_gauge2_device_grid(dU, dU2, anti_pbc=False)
    Db, clb = ctx.get_operator()
    ctx.close()
    assert plaq_a == plaq_b and np.array_equal(bits(Da), bits(Db)) and np.array_equal(bits(cla), bits(clb))


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_solve(gold8, hip):
    """the bars of test_amg_solve_through_rccl_self_exchange, set_gauge against set_gauge_device_grid on the same grid; then another
    field and back on the hierarchy that is set up (the coarse operators are rebuilt: operator_changed)"""
    b = np.zeros((4096, 12, 2)); b[..., 0] = 1.0
    host = grid_context(sx.params(gold8, ALL, levels=2))
    host.set_gauge(gold8["gauge"], anti_pbc=True)
    host.setup(2)
    x0, it0, _, rr0 = host.solve(b, 1e-10)
    host.close()
    ctx = grid_context(sx.params(gold8, ALL, levels=2))
    dU = hip.upload(gold8["gauge"]); dother = hip.upload(np.ascontiguousarray(gold8["gauge"][::-1]))
    ctx.set_gauge_device_grid(dU, anti_pbc=True)
    ctx.setup(2)
    x1, it1, _, rr1 = ctx.solve(b, 1e-10)
    print("iterations", it0, it1, "relres", rr0, rr1, "x relerr", relerr(x1, x0))
    assert rr1 < 1e-10 and abs(it1 - it0) <= 1
    assert relerr(x1, x0) < 1e-7
    ctx.set_gauge_device_grid(dother, anti_pbc=True)
    ctx.set_gauge_device_grid(dU, anti_pbc=True)
    x2, it2, _, rr2 = ctx.solve(b, 1e-10)
    print("after another field and back: iterations", it2, "relres", rr2, "x relerr", relerr(x2, x0))
    assert rr2 < 1e-10 and abs(it2 - it0) <= 1
    assert relerr(x2, x0) < 1e-7
    ctx.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_refusals(gold4, hip):
    m0, csw = float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])
    dU = hip.upload(gold4["gauge"])
    ctx = grid_context(params([4] * 4, [2] * 4, m0, csw, grid=(-1, 1, 1, -1)))
    ctx.set_gauge(gold4["gauge"], anti_pbc=True)
    host_array = np.ascontiguousarray(gold4["gauge"], dtype=np.float64)
    for bad in (int(host_array.ctypes.data), 0):
        with pytest.raises(api.DDAMGError) as e:
            ctx.set_gauge_device_grid(bad, anti_pbc=True)
        assert str(e.value)
        check_dirac(ctx, gold4)
        with pytest.raises(api.DDAMGError) as e:
            ctx.set_gauge2_device_grid(dU, bad, anti_pbc=True)
        assert str(e.value)
        check_dirac(ctx, gold4)
    ctx.close()
    # a process grid without a transport: refused with the calls that install one; the context is usable afterwards
    bare = dd.Context(params([4] * 4, [2] * 4, m0, csw, grid=(-1, 1, 1, -1)))
    for call in (lambda: bare.set_gauge_device_grid(dU, anti_pbc=True), lambda: bare.set_gauge2_device_grid(dU, dU, anti_pbc=True)):
        with pytest.raises(api.DDAMGError, match="ddamg_hip_comm_init_rccl / ddamg_hip_comm_init_host"):
            call()
    bare.comm_init_rccl(api.rccl_unique_id())
    bare.set_gauge_device_grid(dU, anti_pbc=True)
    check_dirac(bare, gold4)
    # the entry points without _grid keep refusing a grid, and name the ones that work there
    with pytest.raises(api.DDAMGError, match="ddamg_hip_set_gauge_device_grid"):
        bare.set_gauge_device(dU, anti_pbc=True)
    check_dirac(bare, gold4)
    bare.close()


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_ildg_load_on_a_grid_in_ragged_chunks(gold4, hip, tmp_path, monkeypatch):
    m0, csw = float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])
    path = tmp_path / "conf.ildg"
    lf.write_ildg(path, [4] * 4, gold4["gauge"], 64)
    monkeypatch.setenv("DDAMG_ILDG_CHUNK_SITES", "90")     # 256 sites: chunks of 90, 90 and 76, the boundaries inside rows of 4 sites
    ctx = grid_context(params([4] * 4, [2] * 4, m0, csw, grid=(1, -1, 1, -1)))
    plaq_h = ctx.set_gauge(gold4["gauge"], anti_pbc=True)
    Dh, clh = ctx.get_operator()
    ctx.set_gauge(np.ascontiguousarray(gold4["gauge"][::-1]), anti_pbc=True)        # another operator in between
    plaq, _ = ctx.load_ildg_conf(path, anti_pbc=True)
    D, cl = ctx.get_operator()
    print("clover relerr", relerr(cl, clh), "plaquette", plaq, plaq_h)
    assert np.array_equal(D, Dh) and relerr(cl, clh) < 1e-14 and abs(plaq - plaq_h) < 1e-12
    check_dirac(ctx, gold4)
    ctx.close()


# several processes --------------------------------------------------------------------------------------------------------
def launch(nproc, *args, timeout=300):
    from launcher import torchrun
    r = torchrun(nproc, os.path.join(HERE, "dist_gauge_device_worker.py"), *args, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DIST_GAUGE_DEVICE_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("nproc,grid", [(2, "2,1,1,1"), (2, "1,1,1,2"), (4, "2,2,1,1")])
def test_links_in_device_memory_on_a_process_grid(nproc, grid):
    """every rank uploads its part of the golden 8^4 links and calls set_gauge_device_grid (host transport): its part of the undivided
    operator, the global plaquette, the golden Dirac outputs.  2,1,1,1: the signed links of the last time slice arrive at rank 0's
    t = -1 from rank 1; 2,2,1,1: corners from a diagonal process"""
    print(launch(nproc, "--mode", "gauge", "--grid", grid)[-1500:])


def test_ildg_load_on_a_process_grid(tmp_path):
    """every rank reads its own rows of the file (X split: a row of the file holds two ranks' runs), in chunks that end inside rows"""
    print(launch(2, "--mode", "ildg", "--grid", "1,1,1,2", "--dir", str(tmp_path))[-1500:])
