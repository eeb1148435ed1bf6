"""dirac_apply_lds_kernel walks the directions in the order of one list (fine_op.hip, kDirOrder: X, Y, T, Z), alternates its two
backward-product buffers with the position in that list, takes the tile's eight neighbour tiles from scalars read once and the
pivot bytes of a site from one word.  4^4 blocks, anti-periodic T, csw = 1, random SU(3) links.

The four cyclic rotations of 12x8x4x8 (T, Z, Y, X) give every direction extent 12 once (three tiles: the +mu and -mu neighbour
tiles differ), extent 4 once (the tile is its own neighbour through the face path) and extent 8 twice (both neighbours are the same
other tile).  Bounds: those of tests/test_gpu_dirac.py (relative 2-norm error against the fp64 oracle: fp32 2e-6, fp64 1e-13).

The fp64 operator on an fp32 input (FineOp<double>::apply_f32in) has no entry point of its own: it is the operator of the outer
FGMRES of a mixed-precision solve, so it is checked through one: a wrong hop term there gives Arnoldi vectors of another matrix, and
the solution then misses the oracle's residual."""
import numpy as np
import pytest
from conftest import relerr, splitmix_uniform, random_su3
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

pytestmark = pytest.mark.gpu
TOL32, TOL64 = 2e-6, 1e-13          # tests/test_gpu_dirac.py
BASE = [12, 8, 4, 8]
ROTATIONS = [BASE[k:] + BASE[:k] for k in range(4)]
RIDS = ["x".join(map(str, L)) for L in ROTATIONS]
M0, CSW = -0.1, 1.0
# (DDAMG_LINK_PIVOT, DDAMG_LINK_COMPRESSION, DDAMG_CLOVER_COMPRESSION) -> reals per link the fp32 operator reads
FORMS = {"pivot10_clover56": ((None, None, None), 10), "tworow12": (("0", None, None), 12), "full18": ((None, "0", None), 18),
         "pivot10_clover72": ((None, None, "0"), 10)}


def switches(monkeypatch, form):
    for name, v in zip(("DDAMG_LINK_PIVOT", "DDAMG_LINK_COMPRESSION", "DDAMG_CLOVER_COMPRESSION"), FORMS[form][0]):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def context(L, monkeypatch, form="pivot10_clover56"):
    switches(monkeypatch, form)            # read once when the context is created
    p = api.default_params(); p.num_levels = 1
    for mu in range(4):
        p.local_lattice[0][mu] = L[mu]; p.block_lattice[0][mu] = 4
    p.m0, p.csw = M0, CSW
    ctx = dd.Context(p)
    ctx.set_gauge(gauge(L), anti_pbc=True)
    assert ctx.link_reals() == FORMS[form][1]
    return ctx


def apply(ctx, phi, prec):
    x = ctx.vector(0, prec).upload(phi); y = ctx.vector(0, prec)
    ctx.dirac_apply(y, x)
    out = y.download()
    x.free(); y.free()
    return out


_cases = {}


def gauge(L):
    return case(L)[0]


def case(L):
    """links, operator, random source and the fp64 oracle's result on L; computed once per shape and left unchanged"""
    from oracle import orc
    key = tuple(L)
    if key not in _cases:
        V = int(np.prod(L))
        U = random_su3(V * 4, 100 + L[0] + 2 * L[1]).reshape(V, 4, 9, 2)
        D, cl, _ = orc.gauge_to_operator(L, U, 1, M0, CSW)
        phi = splitmix_uniform(V * 24, 200 + L[0]).reshape(V, 12, 2)
        _cases[key] = (U, D, cl, phi, orc.dirac_apply(L, D, cl, phi, 64))
    return _cases[key]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("L", ROTATIONS, ids=RIDS)
def test_rotations_against_the_oracle(L, form, monkeypatch):
    """fp32 and fp64 applies on every rotation and every link / clover form against the fp64 oracle"""
    _, _, _, phi, ref = case(L)
    ctx = context(L, monkeypatch, form)
    for prec, tol in ((32, TOL32), (64, TOL64)):
        err = relerr(apply(ctx, phi, prec), ref)
        print(f"{L} {form} fp{prec}: rel.err {err:.3e}")
        assert err < tol, (L, form, prec, err)
    ctx.close()


SOLVE_BASE = [16, 8, 8, 8]
SOLVE_ROTATIONS = [SOLVE_BASE[k:] + SOLVE_BASE[:k] for k in range(4)]


@pytest.mark.parametrize("L", SOLVE_ROTATIONS, ids=["x".join(map(str, L)) for L in SOLVE_ROTATIONS])
def test_fp64_operator_on_fp32_input_through_a_mixed_precision_solve(L, monkeypatch):
    """two-level FGMRES + AMG with mixed_precision = 1: the outer solver applies the fp64 operator to the fp32 iterates of the
    V-cycle (apply_f32in).  The Schwarz smoother needs an even number of blocks per direction, so the extents 12 and 4 of the
    rotations above cannot be solved on; the rotations of 16x8x8x8 give every direction four tiles once (distinct +mu and -mu
    neighbour tiles) and two tiles three times.  The solver stops at 1e-10 on its own residual; the oracle's residual of the
    solution differs from it by fp64 rounding of one apply (1e-13 of |D||x|, a few 1e-13 of |b| here), so 1.1e-10 bounds it."""
    from oracle import orc
    U, D, cl, _, _ = case(L)
    V = int(np.prod(L))
    switches(monkeypatch, "pivot10_clover56")
    p = api.default_params(); p.num_levels = 2
    for mu in range(4):
        p.local_lattice[0][mu] = L[mu]; p.block_lattice[0][mu] = 4; p.local_lattice[1][mu] = L[mu] // 4
    p.num_vect[0] = 8; p.post_smooth_iter[0] = 2; p.block_iter[0] = 4; p.setup_iter[0] = 1
    p.restart, p.max_restart, p.tol = 30, 20, 1e-10
    p.coarse_iter, p.coarse_restart, p.coarse_tol = 100, 5, 5e-2
    p.mixed_precision, p.method, p.m0, p.csw = 1, 2, M0, CSW
    ctx = dd.Context(p)
    ctx.set_gauge(U, anti_pbc=True)
    ctx.setup(1)
    b = splitmix_uniform(V * 24, 300 + L[0]).reshape(V, 12, 2)
    x, it, _, rr = ctx.solve(b, 1e-10)
    ctx.close()
    res = np.linalg.norm(b - orc.dirac_apply(L, D, cl, x.reshape(V, 12, 2), 64)) / np.linalg.norm(b)
    print(f"{L}: {it} iterations, reported relres {rr:.3e}, oracle relres {res:.3e}")
    assert rr < 1e-10 and res < 1.1e-10


def face_sites(L):
    """for each mu, a site with x_mu = 3 and one with x_mu = 0 (both on a face of their 4^4 tile), the other coordinates inside a
    tile that has distinct +-mu neighbour tiles where the extent allows (block coordinate 1 of 3 in T)"""
    out = []
    for mu in range(4):
        for xmu in (3, 0):
            c = np.array([5, 1, 2, 6])          # tile (1, 0, 0, 1), an interior site of it
            c[mu] = (c[mu] // 4) * 4 + xmu
            out.append((mu, xmu, c))
    return out


@pytest.mark.parametrize("prec,tol", [(32, TOL32), (64, TOL64)])
def test_point_sources_on_tile_faces(prec, tol, monkeypatch):
    """a source on one site: the output is non-zero exactly on the site and its eight neighbours, and equals the oracle's there.
    Each of the eight hop terms of the source's neighbours is seen alone: a neighbour-tile scalar of another direction, or a
    backward product taken from the other buffer, changes or moves one of them.  (Two consecutive directions writing the SAME
    buffer is a race between wavefronts of one workgroup and shows only by timing: a seeded one passed here.)"""
    from oracle import orc, site_ops
    L = BASE; V = int(np.prod(L))
    _, D, cl, _, _ = case(L)
    ctx = context(L, monkeypatch)
    rng = np.random.default_rng(17)
    for mu, xmu, c in face_sites(L):
        s0 = int(site_ops.lex_of(L, c))
        phi = np.zeros((V, 12, 2)); phi[s0] = rng.uniform(-1, 1, (12, 2))
        ref = orc.dirac_apply(L, D, cl, phi, 64)
        want = {s0}
        for nu in range(4):
            for d in (1, -1):
                want.add(int(site_ops.lex_of(L, site_ops._shift(L, c, {nu: d}))))
        assert len(want) == 9
        out = apply(ctx, phi, prec)
        got = set(np.flatnonzero(np.abs(out).reshape(V, -1).max(1) > 0).tolist())
        assert got == want, (mu, xmu, sorted(got ^ want))
        idx = sorted(want)
        assert set(np.flatnonzero(np.abs(ref).reshape(V, -1).max(1) > 0).tolist()) == want
        for s in idx:                           # every hop term on its own, at the bound of the whole-vector comparison
            err = relerr(out[s], ref[s])
            assert err < tol, (mu, xmu, s, err)
    ctx.close()


@pytest.mark.parametrize("prec", [32, 64])
def test_two_applies_give_identical_bits(prec, monkeypatch):
    L = BASE
    phi = case(L)[3]
    ctx = context(L, monkeypatch)
    a = apply(ctx, phi, prec); b = apply(ctx, phi, prec)
    ctx.close()
    assert np.abs(a).max() > 0.1 and np.array_equal(a, b)
