"""GPU parity (-m gpu) against the pinned numpy/scipy restatement (oracle/mg_oracle.py) on lattices that are in no
golden set, seeded random links: 4x8x4x4 (T,Z,Y,X) with Schwarz blocks 2x4x2x2 = aggregates; 4x4x4x8 with blocks
2x2x2x4; and 4x4x8x8 with 2^4 blocks inside 2x2x4x4 aggregates (several blocks per aggregate).  The hierarchy comes from
the GPU setup (device generator); the oracle receives the same interpolation vectors and coarse operator, and the fine
operator from the pinned C oracle (not from the library).

The production shape: 8x8x16x16 with 4^4 blocks = aggregates and 24 test vectors, a 2x2x4x4 coarse lattice.  Y and X have
4 blocks each, so the +mu and -mu neighbour blocks there are different blocks (on an 8^4 lattice they coincide, and a mix-up
between them cannot show), and the production kernels run: sap_pair_kernel (fp32, mixed_precision 1) or the fp64 kernels of
sap.hip (mixed_precision 0), the tiled Galerkin stencil and the matrix-core restriction -- for the additive (1), red-black
(2) and sixteen-colour (3) Schwarz methods."""
import numpy as np
import pytest
from conftest import relerr, random_su3, splitmix_uniform
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

pytestmark = pytest.mark.gpu

# name: (lattice, blocks = aggregates' divisor, coarse lattice, test vectors, mixed_precision, method)
SHAPES = {"blocks=aggregates": ([4, 8, 4, 4], [2, 4, 2, 2], [2, 2, 2, 2], 10, 1, 2),
          "long-x": ([4, 4, 4, 8], [2, 2, 2, 4], [2, 2, 2, 2], 10, 1, 2),
          "blocks-in-aggregates": ([4, 4, 8, 8], [2, 2, 2, 2], [2, 2, 2, 2], 10, 1, 2)}
for _mp in (1, 0):
    for _method in (1, 2, 3):
        SHAPES[f"8x8x16x16-b4-mp{_mp}-m{_method}"] = ([8, 8, 16, 16], [4, 4, 4, 4], [2, 2, 4, 4], 24, _mp, _method)
M0, CSW = 0.3, 1.0
_FINE = {}


def fine_matrix(L, U):
    """the fine operator as an fp64 sparse matrix from the pinned C oracle, once per lattice"""
    from oracle import mg_oracle as mo, orc
    key = tuple(L)
    if key not in _FINE:
        D, cl, _ = orc.gauge_to_operator(L, U, 1, M0, CSW)
        _FINE[key] = (D, cl, mo.fine_matrix(L, D, cl))
    return _FINE[key]


def tol(mp, fp32, fp64):
    return fp32 if mp == 1 else fp64


@pytest.fixture(scope="module", params=list(SHAPES), ids=list(SHAPES))
def pair(request):
    global L, B, LC, V, MP
    L, B, LC, nvec, MP, method = SHAPES[request.param]
    V = int(np.prod(L))
    from oracle import mg_oracle as mo
    p = api.default_params(); p.num_levels = 2
    for mu in range(4):
        p.local_lattice[0][mu] = L[mu]; p.block_lattice[0][mu] = B[mu]; p.local_lattice[1][mu] = LC[mu]
    p.num_vect[0] = nvec; p.post_smooth_iter[0] = 2; p.block_iter[0] = 4; p.setup_iter[0] = 2
    p.restart, p.max_restart, p.tol = 30, 20, 1e-10
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 100, 5, 5e-2
    p.mixed_precision, p.method, p.odd_even = MP, method, 1
    p.m0, p.csw = M0, CSW
    p.test_vector_rng, p.rng_seed = 1, 99
    ctx = dd.Context(p)
    U = random_su3(V * 4, 31).reshape(V, 4, 9, 2)
    ctx.set_gauge(U, anti_pbc=True)
    ctx.setup(2)
    D, cl, A = fine_matrix(L, U)
    Dc, clc = ctx.get_coarse_operator()
    tl = mo.TwoLevel(L, LC, B, D, cl, ctx.get_interpolation(), Dc, clc, method=method, A=A)
    yield ctx, tl, mo
    ctx.close()


def vec(a, mo):
    return mo.cplx(np.asarray(a, dtype=np.float64)).ravel()


def test_galerkin_operator_vs_oracle(pair):
    ctx, tl, mo = pair
    G = (tl.P.conj().T @ tl.A @ tl.P).toarray()
    err = np.abs(G - tl.Mc.toarray()).max() / np.abs(G).max()
    print(f"Galerkin operator vs P^H A P: {err:.2e}")
    assert err < tol(MP, 2e-5, 1e-13)


@pytest.mark.parametrize("cycles", [1, 3])
def test_smoother_vs_oracle(pair, cycles):
    ctx, tl, mo = pair
    prec = ctx.vprec()
    eta = splitmix_uniform(V * 24, 3).reshape(V, 12, 2)
    e = ctx.vector(0, prec).upload(eta); phi = ctx.vector(0, prec)
    ctx.smoother(phi, e, cycles, initial_guess_zero=True)
    err0 = relerr(phi.download().reshape(-1, 2), mo.reim(tl.sap.smooth(vec(eta, mo), cycles)))
    phi0 = splitmix_uniform(V * 24, 4).reshape(V, 12, 2)
    phi.upload(phi0)
    ctx.smoother(phi, e, cycles, initial_guess_zero=False)
    err1 = relerr(phi.download().reshape(-1, 2), mo.reim(tl.sap.smooth(vec(eta, mo), cycles, phi0=vec(phi0, mo))))
    print(f"smoother, {cycles} cycles: {err0:.2e} from zero, {err1:.2e} with an initial guess")
    assert err0 < tol(MP, 5e-5, 1e-11) and err1 < tol(MP, 5e-5, 1e-11)
    e.free(); phi.free()


def test_transfer_and_coarse_apply_vs_oracle(pair):
    ctx, tl, mo = pair
    prec = ctx.vprec()
    Vc, nc = ctx.volume(1), ctx.ndof(1)
    f = splitmix_uniform(V * 24, 5).reshape(V, 12, 2)
    c = splitmix_uniform(Vc * nc * 2, 6).reshape(Vc, nc, 2)
    fv = ctx.vector(0, prec).upload(f); cv = ctx.vector(1, prec); cw = ctx.vector(1, prec)
    ctx.restrict(cv, fv)
    errs = [relerr(cv.download().reshape(-1, 2), mo.reim(tl.restrict(vec(f, mo))))]
    cv.upload(c)
    ctx.interpolate(fv, cv, add=False)
    errs.append(relerr(fv.download().reshape(-1, 2), mo.reim(tl.interpolate(vec(c, mo)))))
    ctx.coarse_apply(cw, cv)
    errs.append(relerr(cw.download().reshape(-1, 2), mo.reim(tl.Mc @ vec(c, mo))))
    print("restrict, interpolate, coarse apply:", " ".join(f"{x:.2e}" for x in errs))
    assert max(errs) < tol(MP, 5e-6, 1e-13), errs
    for v in (fv, cv, cw):
        v.free()


def test_vcycle_and_solve_vs_oracle(pair):
    ctx, tl, mo = pair
    prec = ctx.vprec()
    eta = splitmix_uniform(V * 24, 8).reshape(V, 12, 2)
    e = ctx.vector(0, prec).upload(eta); phi = ctx.vector(0, prec)
    ctx.vcycle(phi, e)
    err = relerr(phi.download().reshape(-1, 2), mo.reim(tl.vcycle(vec(eta, mo))))
    print(f"V-cycle: {err:.2e}")
    assert err < tol(MP, 2e-4, 1e-9)
    b = np.zeros((V, 12, 2)); b[..., 0] = 1.0
    x, it, cit, rr = ctx.solve(b, 1e-10)
    xo, ito, hist = tl.solve(vec(b, mo), 1e-10, restart=30)
    print(f"solve: {it} iterations ({ito} oracle), coarse {cit} ({tl.coarse_its} oracle)")
    assert it == ito and abs(cit - tl.coarse_its) <= 3
    assert relerr(x.reshape(-1, 2), mo.reim(xo)) < 1e-8
    ratio = ctx.residual_history() / np.array(hist)   # fp32 V-cycle against the fp64 restatement: the curves drift apart slowly
    print("residual history / oracle's:", np.array2string(ratio, precision=4))
    # (the production shape converges a hundredfold per iteration, and the fp32 V-cycle's rounding shows in the residual from
    # the second iteration on: 1.005, 1.061, 1.104 with mixed_precision 1 and red-black Schwarz)
    first = 3 if V < 4096 else 1
    assert np.all(np.abs(ratio[:first] - 1.0) < 0.05) and np.all(np.abs(ratio - 1.0) < 0.3)
    e.free(); phi.free()


@pytest.mark.parametrize("mp", [1, 0])
def test_gram_schmidt_on_every_aggregate_vs_numpy(mp):
    """gram_schmidt_on_aggregates on seeded raw test vectors of the 8x8x16x16 lattice (4^4 aggregates: the one-wavefront
    kernel in fp32, the workgroup kernel in fp64): the interpolation operator against a modified Gram-Schmidt in fp64 in the
    reference's order (vector k projected on 0..k-1 one after the other, then normalised), on every aggregate and chirality"""
    L, Lc, N = [8, 8, 16, 16], [2, 2, 4, 4], 24
    V = int(np.prod(L))
    p = api.default_params(); p.num_levels = 2
    for mu in range(4):
        p.local_lattice[0][mu] = L[mu]; p.block_lattice[0][mu] = 4; p.local_lattice[1][mu] = Lc[mu]
    p.num_vect[0] = N; p.mixed_precision, p.method, p.odd_even = mp, 2, 1
    p.m0, p.csw = M0, CSW
    ctx = dd.Context(p)
    ctx.set_gauge(random_su3(V * 4, 32).reshape(V, 4, 9, 2), anti_pbc=True)
    raw = splitmix_uniform(N * V * 24, 12).reshape(N, V, 12, 2)
    if mp == 1:
        raw = raw.astype(np.float32).astype(np.float64)       # what the fp32 kernel starts from
    ctx.set_test_vectors(raw, orthonormalised=False)
    P = ctx.get_interpolation()
    ctx.close()
    # [vec][site][dof] -> [aggregate][chirality][vec][256 sites x 6 dof]
    to_blocks = lambda a: (a[..., 0] + 1j * a[..., 1]).reshape(N, 2, 4, 2, 4, 4, 4, 4, 4, 2, 6) \
        .transpose(1, 3, 5, 7, 9, 0, 2, 4, 6, 8, 10).reshape(2 * 2 * 4 * 4, 2, N, 256 * 6)
    got, v = to_blocks(P), to_blocks(raw)
    for k in range(N):
        for j in range(k):
            v[:, :, k] -= np.einsum("abi,abi->ab", v[:, :, j].conj(), v[:, :, k])[..., None] * v[:, :, j]
        v[:, :, k] /= np.linalg.norm(v[:, :, k], axis=-1, keepdims=True)
    err = np.abs(got - v).max(axis=(2, 3)) / np.abs(v).max(axis=(2, 3))       # per aggregate and chirality
    print(f"Gram-Schmidt, mixed_precision {mp}: worst aggregate {err.max():.2e}")
    assert err.max() < (1e-6 if mp == 1 else 1e-13), np.unravel_index(np.argmax(err), err.shape)
