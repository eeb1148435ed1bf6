"""Gauge field, sources and solutions taken from device memory (-m gpu): ddamg_hip_set_gauge_device, _set_gauge2_device,
_vec_upload_device, _vec_download_device, _solve_device and _preconditioner_device against the reference's dumps and against
their host-pointer twins.  Device arrays come from the HIP runtime the library itself has mapped (no second runtime in the
process); the torch case runs in a fresh interpreter."""
import ctypes, os, subprocess, sys
import numpy as np
import pytest
from conftest import load_golden, relerr
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "tools"))


class Hip:
    """hipMalloc / hipMemcpy / hipFree of the libamdhip64 that libddamg_hip.so is linked to"""

    def __init__(self):
        api.load_library()
        path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
        self.lib = ctypes.CDLL(path)
        self.lib.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.lib.hipFree.argtypes = [ctypes.c_void_p]
        self.held = []

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        assert self.lib.hipMalloc(ctypes.byref(p), nbytes) == 0
        self.held.append(p.value)
        return p.value

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = self.alloc(a.nbytes)
        assert self.lib.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p

    def download(self, p, shape):
        out = np.empty(shape, dtype=np.float64)
        assert self.lib.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0
        return out

    def free_all(self):
        for p in self.held:
            self.lib.hipFree(p)
        self.held = []


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.free_all()


def params(L, B, m0, csw, levels=1, grid=(1, 1, 1, 1)):
    p = api.default_params(); p.num_levels = levels
    for mu in range(4):
        p.local_lattice[0][mu] = L[mu]; p.block_lattice[0][mu] = B[mu]
        p.local_lattice[1][mu] = L[mu] // B[mu]
        p.process_grid[mu] = grid[mu]
    p.m0, p.csw = m0, csw
    return p


def two_level_4():
    q = api.default_params(); q.num_levels = 2
    for mu in range(4):
        q.local_lattice[0][mu] = 4; q.block_lattice[0][mu] = 2; q.local_lattice[1][mu] = 2
    q.num_vect[0] = 8; q.setup_iter[0] = 2
    q.mixed_precision, q.method, q.m0, q.csw = 1, 2, 0.3, 1.0
    return q


def params_8_b4(gb):
    """the parameters of test_256_site_blocks_through_rccl_self_exchange, undivided"""
    p = api.default_params(); p.num_levels = 2
    for mu in range(4):
        p.local_lattice[0][mu] = 8; p.block_lattice[0][mu] = 4; p.local_lattice[1][mu] = 2
    p.num_vect[0] = 20; p.post_smooth_iter[0] = 2; p.block_iter[0] = 4; p.setup_iter[0] = 3
    p.restart, p.max_restart, p.tol = 50, 20, 1e-10
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 100, 5, 5e-2
    p.mixed_precision, p.method, p.odd_even = 1, 2, 1
    p.m0, p.csw = float(gb["meta_f64"][0]), float(gb["meta_f64"][1])
    return p


def check_dirac(ctx, g):
    for prec, ref, tol in ((64, "dirac_out_f64", 1e-13), (32, "dirac_out_f32_as_f64", 2e-6)):
        x = ctx.vector(0, prec).upload(g["dirac_in"]); y = ctx.vector(0, prec)
        ctx.dirac_apply(y, x)
        err = relerr(y.download(), g[ref])
        x.free(); y.free()
        assert err < tol, (prec, err)


def synth_field(L, seed):
    import synth
    return synth.synth_gauge(list(L), 0.35, seed).reshape(int(np.prod(L)), 4, 9, 2)


# 1 ------------------------------------------------------------------------------------------------------------------------
def test_reference_dumps_4(gold4, hip):
    ctx = dd.Context(params([4] * 4, [2] * 4, float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])))
    plaq = ctx.set_gauge_device(hip.upload(gold4["gauge"]), anti_pbc=True)
    assert abs(plaq - float(gold4["meta_f64"][2])) < 1e-12
    D, cl = ctx.get_operator()
    assert np.array_equal(D, gold4["D"])
    assert relerr(cl, gold4["clover"]) < 1e-14
    check_dirac(ctx, gold4)
    ctx.close()


@pytest.mark.parametrize("block", [2, 4])
def test_reference_dumps_8(gold8, hip, block):
    ctx = dd.Context(params([8] * 4, [block] * 4, float(gold8["meta_f64"][0]), float(gold8["meta_f64"][1])))
    plaq = ctx.set_gauge_device(hip.upload(gold8["gauge"]), anti_pbc=True)
    assert abs(plaq - float(gold8["meta_f64"][2])) < 1e-12
    D, cl = ctx.get_operator()
    assert np.array_equal(D[::97], gold8["D_sample"])
    assert relerr(cl[::97], gold8["clover_sample"]) < 1e-14
    check_dirac(ctx, gold8)
    ctx.close()


# 2 ------------------------------------------------------------------------------------------------------------------------
RAGGED = [4, 6, 8, 10]   # four different extents; 6 and 10 leave a tile tail


@pytest.mark.parametrize("anti_pbc", [0, 1])
def test_host_path_on_a_lattice_no_tile_divides(hip, anti_pbc):
    U = synth_field(RAGGED, 7)
    host = dd.Context(params(RAGGED, [2] * 4, -0.3, 1.25))
    plaq_h = host.set_gauge(U, anti_pbc=bool(anti_pbc))
    Dh, clh = host.get_operator()
    host.close()
    ctx = dd.Context(params(RAGGED, [2] * 4, -0.3, 1.25))
    plaq_d = ctx.set_gauge_device(hip.upload(U), anti_pbc=bool(anti_pbc))
    Dd, cld = ctx.get_operator()
    ctx.close()
    print("clover relerr", relerr(cld, clh), "plaquette", plaq_d, plaq_h)
    assert np.array_equal(Dd, Dh)
    assert relerr(cld, clh) < 1e-14
    assert abs(plaq_d - plaq_h) < 1e-12


def test_csw_zero(hip):
    U = synth_field(RAGGED, 7)
    ctx = dd.Context(params(RAGGED, [2] * 4, -0.3, 0.0))
    ctx.set_gauge_device(hip.upload(U), anti_pbc=True)
    _, cl = ctx.get_operator()
    ctx.close()
    assert np.all(cl[:, :12, 0] == 4.0 - 0.3)
    assert np.all(cl[:, :12, 1] == 0.0) and np.all(cl[:, 12:] == 0.0)


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_the_callers_arrays_are_not_written(gold8, hip):
    gb = load_golden("ref_8x8_b4.npz")
    ctx = dd.Context(params_8_b4(gb))
    dU = hip.upload(gold8["gauge"])
    ctx.set_gauge_device(dU, anti_pbc=True)
    assert np.array_equal(hip.download(dU, gold8["gauge"].shape), gold8["gauge"])
    ctx.setup(3)
    b = np.zeros((4096, 12, 2)); b[..., 0] = 1.0
    db = hip.upload(b); dx = hip.alloc(b.nbytes)
    ctx.solve_device(dx, db, 1e-10)
    assert np.array_equal(hip.download(db, b.shape), b)
    assert np.array_equal(hip.download(dU, gold8["gauge"].shape), gold8["gauge"])
    ctx.close()


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_two_fields(hip):
    U1, U2 = synth_field(RAGGED, 7), synth_field(RAGGED, 8)
    host = dd.Context(params(RAGGED, [2] * 4, -0.3, 1.25))
    plaq_h = host.set_gauge2(U1, U2, anti_pbc=True)
    Dh, clh = host.get_operator()
    host.close()
    d1, d2 = hip.upload(U1), hip.upload(U2)
    ctx = dd.Context(params(RAGGED, [2] * 4, -0.3, 1.25))
    plaq_d = ctx.set_gauge2_device(d1, d2, anti_pbc=True)
    Dd, cld = ctx.get_operator()
    assert np.array_equal(Dd, Dh) and relerr(cld, clh) < 1e-14 and abs(plaq_d - plaq_h) < 1e-12
    # equal pointers: set_gauge_device
    plaq_2 = ctx.set_gauge2_device(d2, d2, anti_pbc=True)
    D2, cl2 = ctx.get_operator()
    plaq_1 = ctx.set_gauge_device(d2, anti_pbc=True)
    D1, cl1 = ctx.get_operator()
    ctx.close()
    assert plaq_2 == plaq_1 and np.array_equal(D2, D1) and np.array_equal(cl2, cl1)
    assert not np.array_equal(D2, Dd)


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_the_host_mirror_is_rebuilt_on_demand(gold4, hip):
    m0, csw = float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])
    host = dd.Context(params([4] * 4, [2] * 4, m0, csw))
    host.set_gauge(gold4["gauge"], anti_pbc=True)
    host.shift_mass(m0 + 0.01)
    Dh, clh = host.get_operator()
    host.close()
    ctx = dd.Context(params([4] * 4, [2] * 4, m0, csw))
    ctx.set_gauge_device(hip.upload(gold4["gauge"]), anti_pbc=True)
    ctx.shift_mass(m0 + 0.01)          # on a stale mirror: no host update, the export below reads the shifted device field
    Dd, cld = ctx.get_operator()
    assert np.array_equal(Dd, Dh) and relerr(cld, clh) < 1e-14
    ctx.shift_mass(m0)                 # on a valid mirror now
    D0, cl0 = ctx.get_operator()
    assert np.array_equal(D0, gold4["D"]) and relerr(cl0, gold4["clover"]) < 1e-14
    ctx.set_operator(D0, cl0)
    check_dirac(ctx, gold4)
    ctx.close()


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("precision", [32, 64])
def test_vectors(hip, level, precision):
    ctx = dd.Context(two_level_4())
    n = ctx.volume(level) * ctx.ndof(level) * 2
    a = np.random.default_rng(3).standard_normal(n).reshape(ctx.volume(level), ctx.ndof(level), 2)
    v = ctx.vector(level, precision).upload(a); w = ctx.vector(level, precision).upload_device(hip.upload(a))
    ref = v.download()
    assert np.array_equal(w.download(), ref)
    out = hip.alloc(a.nbytes)
    v.download_device(out)
    assert np.array_equal(hip.download(out, a.shape), ref)
    v.free(); w.free(); ctx.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_solve_and_preconditioner(gold8, hip):
    gb = load_golden("ref_8x8_b4.npz")
    b = np.zeros((4096, 12, 2)); b[..., 0] = 1.0
    host = dd.Context(params_8_b4(gb))
    host.set_gauge(gold8["gauge"], anti_pbc=True)
    host.setup(3)
    xh, ith, _, rrh = host.solve(b, 1e-10)
    host.close()
    ctx = dd.Context(params_8_b4(gb))
    ctx.set_gauge_device(hip.upload(gold8["gauge"]), anti_pbc=True)
    ctx.setup(3)
    db = hip.upload(b); dx = hip.alloc(b.nbytes)
    it, cit, rr = ctx.solve_device(dx, db, 1e-10)
    xd = hip.download(dx, b.shape)
    print("iterations", it, ith, "relres", rr, "x relerr", relerr(xd, xh))
    assert it == int(gb["ones_solve_iters"][0]) and rr < 1e-10
    assert relerr(xd, xh) < 1e-7
    src = gold8["dirac_in"]
    ph = ctx.preconditioner(src)
    dout = hip.alloc(src.nbytes)
    ctx.preconditioner_device(dout, hip.upload(src))
    assert np.array_equal(hip.download(dout, src.shape), ph)
    ctx.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_refusals(gold4, hip):
    m0, csw = float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1])
    ctx = dd.Context(params([4] * 4, [2] * 4, m0, csw))
    ctx.set_gauge(gold4["gauge"], anti_pbc=True)
    host_array = np.ascontiguousarray(gold4["gauge"], dtype=np.float64)
    for bad in (int(host_array.ctypes.data), 0):
        with pytest.raises(api.DDAMGError) as e:
            ctx.set_gauge_device(bad, anti_pbc=True)
        assert str(e.value)
        check_dirac(ctx, gold4)
    x = ctx.vector(0, 64)
    hb = np.zeros((256, 12, 2))
    for call in (lambda: x.upload_device(int(hb.ctypes.data)), lambda: x.download_device(0),
                 lambda: ctx.solve_device(int(hb.ctypes.data), hip.upload(hb)), lambda: ctx.preconditioner_device(0, hip.upload(hb))):
        with pytest.raises(api.DDAMGError) as e:
            call()
        assert str(e.value)
    d = hip.upload(hb)
    with pytest.raises(api.DDAMGError, match="overlap"):
        ctx.solve_device(d, d)
    x.free(); ctx.close()
    # a process grid, the self-exchange entry included: refused with the name of the entry point that works there
    grid = dd.Context(params([4] * 4, [2] * 4, m0, csw, grid=(-1, 1, 1, 1)))
    grid.comm_init_rccl(api.rccl_unique_id())
    grid.set_gauge(gold4["gauge"], anti_pbc=True)
    with pytest.raises(api.DDAMGError, match="ddamg_hip_set_gauge"):
        grid.set_gauge_device(hip.upload(gold4["gauge"]), anti_pbc=True)
    check_dirac(grid, gold4)
    grid.close()


def test_null_and_mismatched_vectors_are_refused_and_the_context_still_solves():
    """a null vector in any slot, a null column, a vector of the wrong level or precision, and a null context next to valid vectors:
    each an error with a message from the host-side checks, none reaches a kernel, and the solve afterwards is the one before"""
    q = two_level_4()
    q.post_smooth_iter[0] = 2; q.block_iter[0] = 4
    q.restart, q.max_restart, q.tol = 30, 20, 1e-10
    q.coarse_iter, q.coarse_restart, q.coarse_tol = 100, 5, 5e-2
    ctx = dd.Context(q)
    ctx.set_gauge(synth_field([4] * 4, 2), anti_pbc=True)
    ctx.setup(2)
    b = np.zeros((256, 12, 2)); b[..., 0] = 1.0
    x0, it0, cit0, rr0 = ctx.solve(b, 1e-10)
    assert rr0 < 1e-10
    lib, c = ctx._lib, ctx._h
    v = {(l, p): ctx.vector(l, p) for l in (0, 1) for p in (32, 64)}
    f32, c32, f64 = v[0, 32]._h, v[1, 32]._h, v[0, 64]._h   # fine and coarse in the V-cycle's precision, fine in the outer solver's

    def refused(status):
        assert status != 0 and lib.ddamg_hip_last_error()

    # (entry point, valid vector arguments, the arguments after them)
    calls = [(lib.ddamg_hip_vec_copy, [f32, f32], []), (lib.ddamg_hip_vec_axpy, [f32, f32, f32], [1.0, 0.0]),
             (lib.ddamg_hip_vec_dot, [f32, f32], [None, None, None]), (lib.ddamg_hip_dirac_apply, [f32, f32], []),
             (lib.ddamg_hip_smoother, [f32, f32], [1, 1]), (lib.ddamg_hip_restrict, [c32, f32], []),
             (lib.ddamg_hip_interpolate, [f32, c32], [0]), (lib.ddamg_hip_coarse_apply, [c32, c32], []),
             (lib.ddamg_hip_coarse_hop, [c32, c32], [0, 1.0, 0]), (lib.ddamg_hip_coarse_self_mul, [c32, c32], [0, 0]),
             (lib.ddamg_hip_coarse_solve, [c32, c32], [None]), (lib.ddamg_hip_vcycle, [f32, f32], []),
             (lib.ddamg_hip_solve_vec, [f64, f64], [1e-10, None, None, None])]
    for entry, vecs, rest in calls:
        for slot in range(len(vecs)):
            refused(entry(c, *[None if k == slot else h for k, h in enumerate(vecs)], *rest))
    cols = (ctypes.c_void_p * 2)
    refused(lib.ddamg_hip_coarse_apply_many(c, 2, cols(c32.value, None), cols(c32.value, c32.value)))
    refused(lib.ddamg_hip_coarse_apply_many(c, 2, cols(c32.value, c32.value), cols(None, c32.value)))
    refused(lib.ddamg_hip_smoother(c, f32, c32, 1, 1))   # the wrong level
    refused(lib.ddamg_hip_smoother(c, f32, f64, 1, 1))   # the wrong precision
    refused(lib.ddamg_hip_smoother(c, f64, f64, 1, 1))
    # no context: refused before anything is done with the vectors
    refused(lib.ddamg_hip_vec_copy(None, f32, f32))
    refused(lib.ddamg_hip_vec_axpy(None, f32, f32, f32, 1.0, 0.0))
    refused(lib.ddamg_hip_vec_dot(None, f32, f32, None, None, None))
    refused(lib.ddamg_hip_vec_destroy(None, f32))
    assert lib.ddamg_hip_vec_destroy(c, None) == 0
    x1, it1, cit1, rr1 = ctx.solve(b, 1e-10)
    assert (it1, cit1, rr1) == (it0, cit0, rr0) and np.array_equal(x1, x0)
    for w in v.values():
        w.free()
    ctx.close()


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_memory(gold8, hip):
    gb = load_golden("ref_8x8_b4.npz")
    before = api.memory_in_use()
    host = dd.Context(params_8_b4(gb))
    host.set_gauge(gold8["gauge"], anti_pbc=True)
    with_host = api.memory_in_use()
    host.close()
    assert api.memory_in_use() == before
    dU = hip.upload(gold8["gauge"])    # not the library's memory: not counted
    ctx = dd.Context(params_8_b4(gb))
    ctx.set_gauge_device(dU, anti_pbc=True)
    assert api.memory_in_use() == with_host
    ctx.get_operator()                 # the export's staging arrays are released as well
    assert api.memory_in_use() == with_host
    ctx.close()
    assert api.memory_in_use() == before


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_torch_tensors_in_a_fresh_interpreter():
    """torch imported first, as in test_rccl_self_exchange_inside_a_torch_process: links, source and solution are torch tensors"""
    code = f"""
import sys, numpy as np, torch
sys.path.insert(0, {REPO!r}); sys.path.insert(0, {HERE!r})
from conftest import load_golden, relerr
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
import test_gpu_device_interface as t
g = load_golden("ref_8x8_dirac.npz"); gb = load_golden("ref_8x8_b4.npz")
b = np.zeros((4096, 12, 2)); b[..., 0] = 1.0
host = dd.Context(t.params_8_b4(gb))
host.set_gauge(g["gauge"], anti_pbc=True); host.setup(3)
xh = host.solve(b, 1e-10)[0]
host.close()
ctx = dd.Context(t.params_8_b4(gb))
U = torch.from_numpy(np.ascontiguousarray(g["gauge"])).cuda()
plaq = ctx.set_gauge_device(U, anti_pbc=True)
assert abs(plaq - float(g["meta_f64"][2])) < 1e-12
assert torch.equal(U.cpu(), torch.from_numpy(np.ascontiguousarray(g["gauge"])))
ctx.setup(3)
src = torch.zeros((4096, 12, 2), dtype=torch.float64, device="cuda"); src[..., 0] = 1.0
x = torch.empty_like(src)
it, cit, rr = ctx.solve_device(x, src, 1e-10)
err = relerr(x.cpu().numpy(), xh)
raised = 0
for bad in (U.float(), U.transpose(0, 1), U.cpu()):
    try:
        ctx.set_gauge_device(bad, anti_pbc=True)
    except api.DDAMGError:
        raised += 1
ok = it == int(gb["ones_solve_iters"][0]) and rr < 1e-10 and err < 1e-7 and raised == 3
print("TORCH_DEVICE_OK" if ok else "MISMATCH", it, rr, err, raised)
ctx.close()
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TORCH_DEVICE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
