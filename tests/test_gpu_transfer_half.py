"""GPU tests (-m gpu) of the fine level's interpolation operator in 16-bit storage (ddamg_hip_set_transfer_storage,
transfer_half.h): the two kernels against a bound derived from the number formats, the copy following P, the setup staying on
the 32-bit P, the whole solve in both storages and with the coarse-storage switch, a process grid, memory accounting and the
refusals.

The bound.  An element of P is stored as fp16(p / s), s = s[a][j][h] the largest |re| or |im| of its block (aggregate a, vector
j, chirality h): a normal fp16 result is within 2^-11 relative, a subnormal one within 2^-25 s absolute.  Products are
accumulated in fp32 in either storage, over at most 256 sites * 24 reals = 6144 terms per sum at the shapes used here
(6144 * 2^-24 < 2^-11), which the factor 2 on both terms covers.  With p the fp32 entries from get_interpolation(), f a fine
vector, c a coarse one, component by component (the same for the real and the imaginary part):
    restriction    B[a,h,j] = 2^-10 sum_{x in a, d in h} (|Re p|+|Im p|)(|Re f|+|Im f|) + 2^-23 s[a][j][h] sum_{x in a, d in h} (|Re f|+|Im f|)
    interpolation  B[x,d]   = 2^-10 sum_j (|Re p_j|+|Im p_j|)(|Re c_hj|+|Im c_hj|) + 2^-23 sum_j s[a][j][h] (|Re c_hj|+|Im c_hj|)
                              (+ 2^-22 |result| in the `add` form: the fp32 sum with the vector that was there)

The outer iteration count in 16-bit storage is held to the 32-bit count + 1.  oracle/mg_oracle.py, a two-level cycle on the 4^4
golden hierarchy (rhs = ones, tol 1e-10) with P rounded to this format in numpy: 11 outer iterations with the fp32 P and 11 with
the rounded one (72 / 72 coarse iterations)."""
import numpy as np
import pytest
from conftest import load_golden, splitmix_uniform
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

pytestmark = pytest.mark.gpu

COARSE_TOL = 5e-2


def f32(a):
    """what the device holds of an uploaded array"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def two_level_params(L, Lc, num_vect, m0, csw, block=2, mixed_precision=1, setup_iter=4, grid=(1, 1, 1, 1)):
    p = api.default_params()
    p.num_levels = 2
    for mu in range(4):
        p.local_lattice[0][mu] = L; p.block_lattice[0][mu] = block; p.local_lattice[1][mu] = Lc[mu]
        p.process_grid[mu] = grid[mu]
    p.num_vect[0] = num_vect
    p.post_smooth_iter[0] = 2; p.block_iter[0] = 4; p.setup_iter[0] = setup_iter
    p.restart, p.max_restart, p.tol = 50, 20, 1e-10
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 100, 5, COARSE_TOL
    p.mixed_precision, p.method, p.odd_even = mixed_precision, 2, 1
    p.m0, p.csw = m0, csw
    return p


def params4(gold4, **kw):
    return two_level_params(4, [2] * 4, 20, float(gold4["meta_f64"][0]), float(gold4["meta_f64"][1]), **kw)


# ---- the transfers in numpy -------------------------------------------------------------------------------------------------
class Transfers:
    """restriction and interpolation with the downloaded P in fp64, and the bounds of the module docstring.  Fine vectors
    [V][12][2] and coarse vectors [Vc][2N][2] with lexicographic sites, coarse dof h * N + j."""

    def __init__(self, ctx):
        P = ctx.get_interpolation()
        self.P = P[..., 0] + 1j * P[..., 1]                                   # [N][V][12]
        self.aP = np.abs(P[..., 0]) + np.abs(P[..., 1])
        self.N, self.V = self.P.shape[:2]
        L = [int(v) for v in ctx.params.local_lattice[0]]; Lc = [int(v) for v in ctx.params.local_lattice[1]]
        self.Vc = int(np.prod(Lc))
        c = np.stack(np.unravel_index(np.arange(self.V), L), axis=1) // (np.array(L) // np.array(Lc))
        self.agg = np.ravel_multi_index(c.T, Lc)                              # coarse site of every fine site
        m = np.maximum(np.abs(P[..., 0]), np.abs(P[..., 1])).reshape(self.N, self.V, 2, 6).max(axis=3)     # [N][V][h]
        self.s = np.zeros((self.Vc, 2, self.N))                               # s[a][h][j]
        np.maximum.at(self.s, self.agg, m.transpose(1, 2, 0))

    def _agg_sum(self, per_site):                                             # [V][2][N] -> [Vc][2N]
        out = np.zeros((self.Vc, 2, self.N), dtype=per_site.dtype)
        np.add.at(out, self.agg, per_site)
        return out.reshape(self.Vc, 2 * self.N)

    def restrict(self, f):
        fc = f[..., 0] + 1j * f[..., 1]
        y = self._agg_sum((np.conj(self.P) * fc[None]).reshape(self.N, self.V, 2, 6).sum(axis=3).transpose(1, 2, 0))
        return np.stack([y.real, y.imag], axis=-1)

    def restrict_bound(self, f):
        af = np.abs(f[..., 0]) + np.abs(f[..., 1])                            # [V][12]
        B = 2.0 ** -10 * self._agg_sum((self.aP * af[None]).reshape(self.N, self.V, 2, 6).sum(axis=3).transpose(1, 2, 0))
        fsum = np.zeros((self.Vc, 2)); np.add.at(fsum, self.agg, af.reshape(self.V, 2, 6).sum(axis=2))
        return B + 2.0 ** -23 * (self.s * fsum[:, :, None]).reshape(self.Vc, 2 * self.N)

    def interpolate(self, c):
        cc = (c[..., 0] + 1j * c[..., 1]).reshape(self.Vc, 2, self.N)[self.agg]                            # [V][h][j]
        y = np.einsum("jxhd,xhj->xhd", self.P.reshape(self.N, self.V, 2, 6), cc).reshape(self.V, 12)
        return np.stack([y.real, y.imag], axis=-1)

    def interpolate_bound(self, c):
        ac = (np.abs(c[..., 0]) + np.abs(c[..., 1])).reshape(self.Vc, 2, self.N)
        B = 2.0 ** -10 * np.einsum("jxhd,xhj->xhd", self.aP.reshape(self.N, self.V, 2, 6), ac[self.agg])
        B = B + 2.0 ** -23 * ((self.s * ac).sum(axis=2)[self.agg])[:, :, None]
        return B.reshape(self.V, 12)


def inputs(ctx):
    V, Vc, n = ctx.volume(0), ctx.volume(1), ctx.ndof(1)
    fu = np.zeros((V, 12, 2)); fu[V - 1, 11, 0] = 1.0
    cu = np.zeros((Vc, n, 2)); cu[Vc - 1, n - 1, 1] = 1.0
    return {"random": (f32(splitmix_uniform(V * 24, 4242).reshape(V, 12, 2)), f32(splitmix_uniform(Vc * n * 2, 4243).reshape(Vc, n, 2))),
            "unit": (fu, cu)}


def transfers(ctx, xs, bits=None):
    """restriction, interpolation and interpolation on top of the fine input, of every input pair, with the storage set to
    `bits` (None: left as it is)"""
    if bits is not None:
        ctx.set_transfer_storage(bits)
    vf = ctx.vector(0, 32); vc = ctx.vector(1, 32)
    out = {}
    for k, (f, c) in xs.items():
        vf.upload(f); ctx.restrict(vc, vf); r = vc.download()
        vc.upload(c); ctx.interpolate(vf, vc, add=False); i0 = vf.download()
        vf.upload(f); ctx.interpolate(vf, vc, add=True); i1 = vf.download()
        out[k] = (r, i0, i1)
    vf.free(); vc.free()
    return out


def doctored_vectors(gold4):
    """(a'): vector 3 zero in chirality 0 on aggregate 0 (s = 0); a handful of entries of vector 5, chirality 1, aggregate 1
    scaled by 1e-6: the largest entry of a block is at most 1, so what is stored of them is below 2^-14, an fp16 subnormal"""
    P = np.array(gold4["interp_vectors"], dtype=np.float64)
    c = np.stack(np.unravel_index(np.arange(256), [4] * 4), axis=1) // 2
    agg = np.ravel_multi_index(c.T, [2] * 4)
    P[3, agg == 0, :6, :] = 0.0
    sites = np.flatnonzero(agg == 1)[[0, 3, 7, 12]]
    P[5, sites[:, None], [6, 8, 9, 11], :] *= 1e-6
    return P


@pytest.fixture(scope="module")
def hier_a(gold4):
    """(a) 4^4 golden lattice, 2^4 aggregates (16 sites: a quarter of a wavefront), the reference's 20 interpolation vectors"""
    ctx = dd.Context(params4(gold4))
    ctx.set_operator(gold4["D"], gold4["clover"])
    ctx.set_test_vectors(gold4["interp_vectors"], orthonormalised=True)
    yield ctx, transfers(ctx, inputs(ctx))
    ctx.close()


@pytest.fixture(scope="module")
def hier_a_doctored(gold4):
    ctx = dd.Context(params4(gold4))
    ctx.set_operator(gold4["D"], gold4["clover"])
    ctx.set_test_vectors(doctored_vectors(gold4), orthonormalised=True)
    yield ctx, transfers(ctx, inputs(ctx))
    ctx.close()


@pytest.fixture(scope="module")
def hier_b(gold8):
    """(b) 8^4 golden configuration, 4^4 aggregates (256 sites: four wavefronts, the sums cross wavefronts), 20 vectors"""
    ctx = dd.Context(two_level_params(8, [2] * 4, 20, float(gold8["meta_f64"][0]), float(gold8["meta_f64"][1]), block=4))
    ctx.set_gauge(gold8["gauge"], anti_pbc=True)
    ctx.setup(1)
    yield ctx, transfers(ctx, inputs(ctx))
    ctx.close()


@pytest.fixture(scope="module")
def hier_c(gold8):
    """(c) 8^4, aggregates 4 x 4 x 2 x 2 (64 sites: exactly one wavefront; coarse lattice 2 x 2 x 4 x 4), 10 vectors: the last
    tile of eight vectors of the restriction is not full"""
    ctx = dd.Context(two_level_params(8, [2, 2, 4, 4], 10, float(gold8["meta_f64"][0]), float(gold8["meta_f64"][1])))
    ctx.set_gauge(gold8["gauge"], anti_pbc=True)
    ctx.setup(1)
    yield ctx, transfers(ctx, inputs(ctx))
    ctx.close()


def assert_within_bound(y16, y32, B, what):
    d = np.abs(y16 - y32).max(axis=-1)
    worst = float((d / np.where(B > 0, B, 1.0)).max())
    print(f"{what}: max |y16 - y32| = {d.max():.3e}, largest |y16 - y32| / B = {worst:.3f}")
    assert np.all(d <= B), what


# ---- 1. the kernels against the bound ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "a_doctored", "b", "c"])
def test_transfers_in_16_bit_storage_are_within_the_format_bound(which, request):
    ctx, y32 = request.getfixturevalue("hier_" + which)          # y32: from before any switch
    xs = inputs(ctx)
    y16 = transfers(ctx, xs, 16)
    y32_again = transfers(ctx, xs, 32)
    tr = Transfers(ctx)
    for k, (f, c) in xs.items():
        refs = (tr.restrict(f), tr.interpolate(c), f + tr.interpolate(c))
        Bi = tr.interpolate_bound(c)
        bounds = (tr.restrict_bound(f), Bi, Bi + 2.0 ** -22 * np.abs(refs[2]).max(axis=-1))
        for form, ref, B, a16, a32, again in zip(("restrict", "interpolate", "interpolate add"), refs, bounds, y16[k], y32[k], y32_again[k]):
            assert np.abs(a32 - ref).max() <= 1e-5 * np.abs(ref).max(), (form, k)     # the numpy P is the one on the device
            assert_within_bound(a16, a32, B, f"({which}) {form}, {k}")
            assert not np.array_equal(a16, a32), (form, k)                            # the 16-bit path was taken
            assert np.array_equal(again, a32), (form, k)                              # 32 bits again: the fp32 kernel, bit for bit
            assert np.all(np.isfinite(a16)), (form, k)
    if which == "a_doctored":
        N = tr.N
        assert tr.s[0, 0, 3] == 0.0 and np.all(tr.s.reshape(-1)[np.arange(tr.s.size) != 3] > 0)
        # the stored values of the scaled-down entries are fp16 subnormals
        assert 0 < np.abs(ctx.get_interpolation()[5][np.abs(ctx.get_interpolation()[5]) > 0]).min() / tr.s[1, 1, 5] < 2.0 ** -14
        for k in xs:
            assert np.all(y16[k][0][0, 3] == 0.0)                                     # restriction onto the zero block
        cu = np.zeros((tr.Vc, 2 * N, 2)); cu[0, 3, 0] = 1.0                           # interpolation of that coefficient alone
        out = transfers(ctx, {"zero block": (xs["random"][0], cu)}, 16)["zero block"]
        ctx.set_transfer_storage(32)
        assert np.all(out[1] == 0.0) and np.array_equal(out[2], xs["random"][0])


# ---- 2. the copy follows P ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change", ["set_test_vectors", "setup_update"])
def test_the_16_bit_copy_follows_the_interpolation_operator(gold4, change):
    ctx = dd.Context(params4(gold4))
    ctx.set_operator(gold4["D"], gold4["clover"])
    # setup_update iterates on the test vectors: there the golden vectors are handed over as test vectors, not as P as it is
    ctx.set_test_vectors(gold4["interp_vectors"], orthonormalised=(change == "set_test_vectors"))
    f = inputs(ctx)["random"][0]
    vf = ctx.vector(0, 32).upload(f); vc = ctx.vector(1, 32)
    B0 = Transfers(ctx).restrict_bound(f)
    ctx.restrict(vc, vf); old32 = vc.download()
    ctx.set_transfer_storage(16)
    ctx.restrict(vc, vf); old16 = vc.download()
    assert_within_bound(old16, old32, B0, "before the change")
    if change == "set_test_vectors":
        ctx.set_test_vectors(np.asarray(gold4["interp_vectors"])[::-1], orthonormalised=True)      # the same vectors in reverse order
    else:
        ctx.setup_update(1)
    ctx.restrict(vc, vf); new16 = vc.download()
    ctx.set_transfer_storage(32)
    ctx.restrict(vc, vf); new32 = vc.download()
    B1 = Transfers(ctx).restrict_bound(f)
    assert_within_bound(new16, new32, B1, "after " + change)
    # a stale copy would have left the 16-bit result within B0 of old32: where the fp32 results moved by more than 2 (B0 + B1)
    # the new 16-bit result must have left the old one by more than B1
    moved = np.abs(new32 - old32).max(axis=-1) > 2 * (B0 + B1)
    print(f"{change}: fp32 restriction moved by more than 2 (B0 + B1) in {int(moved.sum())} of {moved.size} components")
    assert moved.any()
    assert np.all(np.abs(new16 - old16).max(axis=-1)[moved] > B1[moved])
    vf.free(); vc.free()
    ctx.close()


# ---- 3. the setup never sees the setting ----------------------------------------------------------------------------------
@pytest.mark.parametrize("bootstrap", ["batched", "one-at-a-time"])
def test_setup_runs_on_the_32_bit_interpolation_whatever_the_setting(gold4, monkeypatch, bootstrap):
    """A setup under DDAMG_TRANSFER_HALF=1 against one without the switch, on the same rand() stream: the same coarse iteration
    count, the same interpolation and coarse operator bit for bit.  The default bootstrap transfers all test vectors at once
    (restrict_batch, interpolate_batch), which never read the 16-bit copy; with DDAMG_BOOTSTRAP_UNBATCHED every V-cycle of the
    bootstrap goes through restrict_to(0, ...) and interpolate(0, ...), the calls the storage switches, so that case holds only
    through the setup's own guard.  Then the golden run of tests/golden/ref_4x4.npz (11 outer, 72 coarse iterations for rhs = ones)
    on the hierarchy that was set up under the switch, in 32-bit storage."""
    if bootstrap == "one-at-a-time":
        monkeypatch.setenv("DDAMG_BOOTSTRAP_UNBATCHED", "1")
    res = []
    for half in (None, "1"):
        if half:
            monkeypatch.setenv("DDAMG_TRANSFER_HALF", half)       # a context's switches are the environment at its creation
        ctx = dd.Context(params4(gold4))
        ctx.set_operator(gold4["D"], gold4["clover"])
        ci = ctx.setup(4)
        vf = ctx.vector(0, 32).upload(inputs(ctx)["random"][0]); vc = ctx.vector(1, 32)
        ctx.restrict(vc, vf)
        res.append((ci, ctx.get_interpolation(), ctx.get_coarse_operator(), vc.download(), ctx))
        vf.free(); vc.free()
    monkeypatch.delenv("DDAMG_TRANSFER_HALF")
    (ci0, P0, (D0, cl0), y0, c0), (ci1, P1, (D1, cl1), y1, c1) = res
    print(f"{bootstrap}: {ci0} coarse iterations of the setup without the switch, {ci1} with it")
    assert ci1 == ci0 and ci0 > 0
    assert np.array_equal(P1, P0)
    assert np.array_equal(D1, D0) and np.array_equal(cl1, cl0)
    assert not np.array_equal(y1, y0)            # the same hierarchy, but the second context does restrict in 16-bit storage
    c1.set_transfer_storage(32)
    b = np.zeros((c1.volume(0), 12, 2)); b[..., 0] = 1.0
    x, it, cit, rr = c1.solve(b, 1e-10)
    print(f"{bootstrap}: solve after the setup under the switch, 32-bit storage: {it} outer, {cit} coarse iterations, relres {rr:.3e}")
    assert it == int(gold4["ones_solve_iters"][0]) and abs(cit - int(gold4["ones_solve_iters"][1])) <= 8 and rr < 1e-10
    # a further setup_update in 16-bit storage leaves the setting as it was, and gives the same vectors as in c0
    c1.set_transfer_storage(16)
    c0.setup_update(1); c1.setup_update(1)
    assert np.array_equal(c1.get_interpolation(), c0.get_interpolation())
    vf = c1.vector(0, 32).upload(inputs(c1)["random"][0]); vc = c1.vector(1, 32)
    c1.restrict(vc, vf); y16 = vc.download()
    c1.set_transfer_storage(32); c1.restrict(vc, vf)
    assert not np.array_equal(y16, vc.download())
    vf.free(); vc.free()
    c0.close(); c1.close()


# ---- 4. the whole solve ----------------------------------------------------------------------------------------------
def three_level_ctx(gold8):
    g3 = load_golden("ref_8x8_3lvl.npz")
    p = api.default_params()
    p.num_levels = 3
    for mu in range(4):
        p.local_lattice[0][mu] = 8; p.block_lattice[0][mu] = 2
        p.local_lattice[1][mu] = 4; p.block_lattice[1][mu] = 2
        p.local_lattice[2][mu] = 2
    p.num_vect[0] = 28; p.num_vect[1] = 28
    p.post_smooth_iter[0] = p.post_smooth_iter[1] = 2; p.block_iter[0] = p.block_iter[1] = 4
    p.setup_iter[0] = 4; p.setup_iter[1] = 3
    p.restart, p.max_restart, p.tol = 50, 20, 1e-10
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 100, 5, COARSE_TOL
    p.kcycle, p.kcycle_restart, p.kcycle_max_restart, p.kcycle_tol = 1, 5, 2, 1e-1
    p.mixed_precision, p.method, p.odd_even = 1, 2, 1
    p.m0, p.csw = float(g3["meta_f64"][0]), float(g3["meta_f64"][1])
    ctx = dd.Context(p)
    ctx.set_gauge(gold8["gauge"], anti_pbc=True)
    return ctx


def true_relres(ctx, x, b):
    """|b - D x| / |b| with the fp64 operator"""
    vx = ctx.vector(0, 64).upload(x); vy = ctx.vector(0, 64)
    ctx.dirac_apply(vy, vx)
    r = np.linalg.norm(b - vy.download()) / np.linalg.norm(b)
    vx.free(); vy.free()
    return float(r)


def runs_of(ctx, settings):
    b = np.zeros((ctx.volume(0), 12, 2)); b[..., 0] = 1.0
    runs = []
    for coarse_bits, transfer_bits in settings:
        ctx.set_coarse_storage(coarse_bits); ctx.set_transfer_storage(transfer_bits)
        x, it, cit, rr = ctx.solve(b, 1e-10)
        runs.append((x.copy(), it, cit, rr, ctx.residual_history(), true_relres(ctx, x, b)))
    return runs


@pytest.mark.parametrize("hierarchy", ["ref_4x4", "ref_8x8_3lvl"])
def test_solve_in_32_16_32_bit_storage(hierarchy, gold4, gold8):
    if hierarchy == "ref_4x4":
        ctx = dd.Context(params4(gold4))
        ctx.set_operator(gold4["D"], gold4["clover"])
    else:
        ctx = three_level_ctx(gold8)
    ctx.setup(4)
    (x1, it1, cit1, rr1, h1, t1), (x2, it2, cit2, rr2, h2, t2), (x3, it3, cit3, rr3, h3, t3) = runs_of(ctx, [(32, 32), (32, 16), (32, 32)])
    ctx.close()
    print(f"{hierarchy}: outer iterations {it1} (32-bit) / {it2} (16-bit), coarse iterations {cit1} / {cit2}, true relres {t1:.3e} / {t2:.3e}")
    assert t2 <= 1e-10 and rr2 <= 1e-10
    assert it2 <= it1 + 1
    assert not np.array_equal(x2, x1)
    assert np.array_equal(x3, x1) and (it3, cit3, rr3) == (it1, cit1, rr1) and np.array_equal(h3, h1)


# ---- 5. both switches together -------------------------------------------------------------------------------------------
def test_solve_with_coarse_and_transfer_storage_in_16_bits(gold4):
    ctx = dd.Context(params4(gold4))
    ctx.set_operator(gold4["D"], gold4["clover"])
    ctx.setup(4)
    (x1, it1, cit1, rr1, h1, t1), (x2, it2, cit2, rr2, h2, t2), (x3, it3, cit3, rr3, h3, t3) = runs_of(ctx, [(32, 32), (16, 16), (32, 32)])
    ctx.close()
    print(f"both in 16 bits: outer iterations {it1} / {it2}, coarse iterations {cit1} / {cit2}, true relres {t1:.3e} / {t2:.3e}")
    assert t2 <= 1e-10 and rr2 <= 1e-10
    assert not np.array_equal(x2, x1)
    assert np.array_equal(x3, x1) and (it3, cit3, rr3) == (it1, cit1, rr1) and np.array_equal(h3, h1)


# ---- 6. one process with a self-exchange -----------------------------------------------------------------------------------
def test_restriction_on_a_process_grid_equals_the_undivided_one(gold8):
    """8^4, the process its own neighbour in the T direction: aggregates never cross a process boundary and the kernels are local,
    so the 16-bit restriction and interpolation equal those of the undivided context bit for bit.  One hierarchy is set up (on the
    process grid); the undivided context takes its interpolation vectors as they are."""
    m0, csw = float(gold8["meta_f64"][0]), float(gold8["meta_f64"][1])
    out = []
    P = None
    for grid in ((-1, 1, 1, 1), (1, 1, 1, 1)):
        ctx = dd.Context(two_level_params(8, [2] * 4, 20, m0, csw, block=4, grid=grid))
        if grid[0] == -1:
            ctx.comm_init_rccl(api.rccl_unique_id())
        ctx.set_gauge(gold8["gauge"], anti_pbc=True)
        if P is None:
            ctx.setup(0)
            P = ctx.get_interpolation()
        else:
            ctx.set_interpolation(P)
            assert np.array_equal(ctx.get_interpolation(), P)
        xs = {"random": inputs(ctx)["random"]}
        out.append((transfers(ctx, xs, 32)["random"], transfers(ctx, xs, 16)["random"]))
        ctx.close()
    (g32, g16), (u32, u16) = out
    for a, b, c in zip(g16, u16, g32):
        assert np.array_equal(a, b) and not np.array_equal(a, c)
    for a, b in zip(g32, u32):
        assert np.array_equal(a, b)


# ---- 7. memory and refusals ---------------------------------------------------------------------------------------------
def test_memory_of_the_copy_and_refusals(gold4):
    before = api.memory_in_use()[0]
    ctx = dd.Context(params4(gold4))
    ctx.set_operator(gold4["D"], gold4["clover"])
    ctx.set_test_vectors(gold4["interp_vectors"], orthonormalised=True)
    f = inputs(ctx)["random"][0]
    vf = ctx.vector(0, 32).upload(f); vc = ctx.vector(1, 32)
    ctx.restrict(vc, vf); y32 = vc.download()
    m32 = api.memory_in_use()[0]
    ctx.set_transfer_storage(16)
    assert api.memory_in_use()[0] == m32                     # nothing before the first use
    ctx.restrict(vc, vf)
    assert not np.array_equal(vc.download(), y32)
    fp32_bytes = ctx.params.num_vect[0] * ctx.volume(0) * 24 * 4
    rise = api.memory_in_use()[0] - m32
    print(f"16-bit copy: {rise} bytes, fp32 interpolation operator {fp32_bytes}")
    assert 0.5 * fp32_bytes <= rise <= 0.51 * fp32_bytes
    ctx.set_transfer_storage(32)
    assert api.memory_in_use()[0] == m32
    with pytest.raises(dd.DDAMGError, match="16 or 32"):
        ctx.set_transfer_storage(8)
    ctx.restrict(vc, vf)
    assert np.array_equal(vc.download(), y32) and api.memory_in_use()[0] == m32
    ctx.set_transfer_storage(16); ctx.restrict(vc, vf)      # closed with the copy alive
    vf.free(); vc.free()
    ctx.close()
    assert api.memory_in_use()[0] == before
    # the fp64 V-cycle
    c = dd.Context(params4(gold4, mixed_precision=0))
    c.set_operator(gold4["D"], gold4["clover"])
    c.set_test_vectors(gold4["interp_vectors"], orthonormalised=True)
    vf = c.vector(0, 64).upload(f); vc = c.vector(1, 64)
    c.restrict(vc, vf); y = vc.download()
    m = api.memory_in_use()[0]
    with pytest.raises(dd.DDAMGError, match="mixed_precision"):
        c.set_transfer_storage(16)
    c.restrict(vc, vf)
    assert np.array_equal(vc.download(), y) and api.memory_in_use()[0] == m
    vf.free(); vc.free()
    c.close()
    # no hierarchy
    p = params4(gold4); p.num_levels = 1
    c = dd.Context(p)
    c.set_operator(gold4["D"], gold4["clover"])
    vf = c.vector(0, 32).upload(f); vo = c.vector(0, 32)
    c.dirac_apply(vo, vf); y = vo.download()
    m = api.memory_in_use()[0]
    with pytest.raises(dd.DDAMGError, match="two levels"):
        c.set_transfer_storage(16)
    c.dirac_apply(vo, vf)
    assert np.array_equal(vo.download(), y) and api.memory_in_use()[0] == m
    vf.free(); vo.free()
    c.close()
    assert api.memory_in_use()[0] == before
