"""GPU tests (-m gpu) of the three-level hierarchy bench.py builds (bench.amg_params: 32^4, 4^4 then 2^4 aggregates, 24 and 28
test vectors), with the batched setup paths that only production shapes take (matrix-core restriction, one-wavefront
Gram-Schmidt, batched coarse construction), against fp64 values computed here and not by the library:

- P^H P = 1 on every aggregate and both chiralities;
- restrict / interpolate of seeded vectors on the whole lattice against P^H f and P c;
- the level-1 operator entry by entry (self coupling and all eight hops) at 64 coarse sites against P_X^H D P_Y, D applied to
  the columns of P through oracle/site_ops.py (straight from the gauge field);
- the level-2 operator entry by entry against oracle/mg_oracle.galerkin_coarse_operator of the downloaded level-1 operator and
  the level-1 interpolation, read column by column as the interpolation of unit vectors.

mixed_precision 1 (fp32 hierarchy) and 0 (fp64).  Host memory: about 15 GB (the interpolation operator, 4.8 GB, and one copy)."""
import os, sys
import numpy as np
import pytest
from conftest import splitmix_uniform
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tools"))
pytestmark = pytest.mark.gpu

L, L1, L2 = [32] * 4, [8] * 4, [4] * 4
V, V1, V2 = 32 ** 4, 8 ** 4, 4 ** 4
N0, N1 = 24, 28
GAUGE_EPS, GAUGE_SEED = 0.35, 20260101


@pytest.fixture(scope="module", params=[1, 0], ids=["mixed_precision 1", "mixed_precision 0"])
def hier(request):
    import bench, synth
    p = bench.amg_params(api, L, 3, 0)
    p.mixed_precision = request.param
    ctx = dd.Context(p)
    U = synth.synth_gauge(L, GAUGE_EPS, GAUGE_SEED)
    ctx.set_gauge(U, anti_pbc=True)
    ctx.setup(p.setup_iter[0])
    P = ctx.get_interpolation()
    Pc = P[..., 0] + 1j * P[..., 1]         # [vec][site][12]
    del P
    yield ctx, U, Pc, request.param, p
    ctx.close()


def cx(a):
    return a[..., 0] + 1j * a[..., 1]


def agg_blocks(a, t):
    """[vec][site][12] of the aggregates with T-block index t -> [8^3 aggregates][chirality][vec][256 sites x 6 dof]"""
    n = a.shape[0]
    s = a.reshape(n, 8, 4, 8, 4, 8, 4, 8, 4, 2, 6)[:, t]
    return s.transpose(2, 4, 6, 8, 0, 1, 3, 5, 7, 9).reshape(512, 2, n, 1536)


def test_interpolation_is_orthonormal_on_every_aggregate(hier):
    ctx, U, Pc, mp, p = hier
    worst = 0.0
    for t in range(8):
        b = agg_blocks(Pc, t)
        g = b.conj() @ b.transpose(0, 1, 3, 2)
        worst = max(worst, float(np.abs(g - np.eye(N0)).max()))
    print(f"mixed_precision {mp}: max |P^H P - 1| over every aggregate and chirality {worst:.2e}")
    assert worst < (1e-6 if mp == 1 else 1e-13)      # measured 3.5e-7 and 1.2e-15


def test_restrict_and_interpolate_on_the_whole_lattice(hier):
    ctx, U, Pc, mp, p = hier
    prec = ctx.vprec(); n1 = 2 * N0
    f = splitmix_uniform(V * 24, 41).reshape(V, 12, 2)
    c = splitmix_uniform(V1 * n1 * 2, 42).reshape(V1, n1, 2)
    fv = ctx.vector(0, prec).upload(f); cv = ctx.vector(1, prec)
    ctx.restrict(cv, fv)
    r = cx(cv.download())
    cv.upload(c)
    ctx.interpolate(fv, cv, add=False)
    y = cx(fv.download()).reshape(8, 4, 8, 4, 8, 4, 8, 4, 2, 6)
    fv.free(); cv.free()
    # P^H f: coarse dof h*N0 + k of aggregate a = <column k of P on a, chirality h | f>
    fb = cx(f)[None]
    rerr = ierr = 0.0
    cc = cx(c).reshape(8, 8, 8, 8, 2, N0)
    for t in range(8):
        Pb = agg_blocks(Pc, t)                                      # [512][2][N0][1536]
        ref = np.einsum("ahki,ahi->ahk", Pb.conj(), agg_blocks(fb, t)[:, :, 0])
        got = r.reshape(8, 512, 2, N0)[t]
        rerr = max(rerr, float(np.abs(got - ref).max() / np.abs(ref).max()))
        ref = np.einsum("ahki,ahk->ahi", Pb, cc[t].reshape(512, 2, N0))
        got = y[t].transpose(1, 3, 5, 7, 0, 2, 4, 6, 8).reshape(512, 2, 1536)
        ierr = max(ierr, float(np.abs(got - ref).max() / np.abs(ref).max()))
    print(f"mixed_precision {mp}: restrict {rerr:.2e}, interpolate {ierr:.2e}")
    bound = 5e-7 if mp == 1 else 1e-13           # measured 2.4e-7 and 3.1e-15
    assert rerr < bound and ierr < bound, (rerr, ierr)


def coarse_blocks(D, cl, X, n):
    """the self coupling and the forward links of coarse site X as n x n matrices, from the library's storage (the reference's:
    packed Hermitian self coupling + the chirality-mixing block, links in four column-major blocks A, C, B, D)"""
    N = n // 2; tri = N * (N + 1) // 2
    c = cx(cl[X]); M = np.zeros((n, n), dtype=complex)
    for b in range(2):
        k = 0
        for j in range(N):
            for i in range(j + 1):
                M[b * N + i, b * N + j] = c[b * tri + k]
                M[b * N + j, b * N + i] = np.conj(c[b * tri + k])
                k += 1
    B = c[2 * tri:].reshape(N, N).T
    M[:N, N:] = B; M[N:, :N] = -B.conj().T
    fw = []
    for mu in range(4):
        q = cx(D[X, mu]).reshape(4, N, N)
        A_, C_, B_, D_ = (q[i].T for i in range(4))
        fw.append(np.block([[A_, B_], [C_, D_]]))
    return M, fw


def test_level1_operator_entry_by_entry_at_sampled_coarse_sites(hier):
    """(D_c)_XY = P_X^H D P_Y: self coupling (Y = X), forward link (Y = X + mu: -U_mu(X)) and backward coupling
    (Y = X - mu: -g5 U_mu(X-mu)^H g5), D applied to the 48 columns of P_Y at the 256 sites of X by oracle/site_ops.py"""
    from oracle import site_ops
    ctx, U, Pc, mp, p = hier
    n = 2 * N0
    D1, cl1 = ctx.get_coarse_operator(1)
    rng = np.random.default_rng(3)
    Xs = np.unique(np.concatenate([[0, V1 - 1], rng.integers(0, V1, 62)]))
    agg = site_ops.coords_of(L, np.arange(V)) // 4
    agg = site_ops.lex_of(L1, agg)
    g5 = np.concatenate([np.ones(N0), -np.ones(N0)])
    worst = 0.0
    for X in Xs:
        sx = np.nonzero(agg == X)[0]
        cX = site_ops.coords_of(L1, X)

        def cols(Y):
            """the 48 columns of P on aggregate Y as a spinor field: idx -> [m][12][48]"""
            def phi(idx):
                out = np.zeros((len(idx), 12, n), dtype=complex)
                on = agg[idx] == Y
                v = Pc[:, idx[on]].transpose(1, 2, 0)                 # [m][12][N0]
                out[on, :6, :N0] = v[:, :6]; out[on, 6:, N0:] = v[:, 6:]
                return out
            return phi

        def block(Y):
            DP = site_ops.dirac_sites(L, U, cols(Y), sx, p.m0, p.csw)     # [256][12][48]
            PX = cols(X)(sx)
            return np.einsum("sda,sdb->ab", PX.conj(), DP)
        M, fw = coarse_blocks(D1, cl1, X, n)
        refs = [(block(X), M)]
        for mu in range(4):
            up = cX.copy(); up[mu] = (up[mu] + 1) % L1[mu]
            dn = cX.copy(); dn[mu] = (dn[mu] - 1) % L1[mu]
            Xd = int(site_ops.lex_of(L1, dn))
            _, fwd = coarse_blocks(D1, cl1, Xd, n)
            refs.append((block(int(site_ops.lex_of(L1, up))), -fw[mu]))
            refs.append((block(Xd), -(g5[:, None] * fwd[mu].conj().T * g5[None, :])))
        scale = max(np.abs(r).max() for r, _ in refs)
        worst = max(worst, max(float(np.abs(r - g).max()) for r, g in refs) / scale)
    print(f"mixed_precision {mp}: level-1 operator at {len(Xs)} coarse sites, worst entry error / largest entry {worst:.2e}")
    assert worst < (3e-6 if mp == 1 else 1e-13), worst      # measured 1.5e-6 and 3.3e-15


def test_level2_operator_entry_by_entry(hier):
    from oracle import mg_oracle as mo
    ctx, U, Pc, mp, p = hier
    prec = ctx.vprec(); n1, n2 = 2 * N0, 2 * N1
    D1, cl1 = ctx.get_coarse_operator(1)
    D2, cl2 = ctx.get_coarse_operator(2)
    # the level-1 interpolation: unit vector j on every coarse site at once (aggregates do not overlap)
    iv = np.zeros((N1, V1, n1), dtype=complex)
    e2 = ctx.vector(2, prec); f1 = ctx.vector(1, prec)
    for j in range(n2):
        e = np.zeros((V2, n2, 2)); e[:, j, 0] = 1.0
        e2.upload(e)
        ctx.interpolate(f1, e2, add=False)
        col = cx(f1.download())
        h, k = divmod(j, N1)
        iv[k, :, h * N0:(h + 1) * N0] = col[:, h * N0:(h + 1) * N0]
        assert np.abs(col[:, (1 - h) * N0:(2 - h) * N0]).max() == 0.0      # a chirality stays in its half
    e2.free(); f1.free()
    parts = mo.coarse_matrix(L1, D1, cl1, n1, parts=True)
    P1 = mo.coarse_interpolation_matrix(L1, L2, np.stack([iv.real, iv.imag], axis=-1), n1)
    Dref, clref = mo.galerkin_coarse_operator(L1, L2, parts, P1, n2)
    errD = np.abs(cx(D2) - Dref).max() / np.abs(Dref).max()
    errc = np.abs(cx(cl2) - clref).max() / np.abs(clref).max()
    print(f"mixed_precision {mp}: level-2 operator vs galerkin_coarse_operator: links {errD:.2e}, self couplings {errc:.2e}")
    bound = 3e-6 if mp == 1 else 1e-13           # measured 1.5e-6 and 2.3e-15
    assert errD < bound and errc < bound, (errD, errc)
