"""The fp32 fine operator on the 10-real pivot form of the links (FineOpDev::Dp, fine_op.h; DDAMG_LINK_PIVOT=0 keeps the two-row
form): fp32, anti-periodic T, 4^4 blocks.  The two shapes (T, Z, Y, X) put every class of direction in front of the kernel: one
block (the wrap stays inside the tile), two blocks (+mu and -mu are the same neighbour tile) and three blocks (distinct neighbour
tiles); T has two and three blocks, so the links with the -1 sign are read through the backward-face global path; 24 tiles take
the XCD order of dirac_apply_lds_kernel, 6 tiles do not."""
import numpy as np
import pytest
from conftest import splitmix_uniform, random_su3
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
import link_pivot_form as lp

pytestmark = pytest.mark.gpu
SHAPES = [[8, 8, 8, 12], [12, 4, 8, 8]]
IDS = ["8x8x8x12", "12x4x8x8"]
M0, CSW = -0.1, 1.0


def params(L, B=(4, 4, 4, 4), grid=None):
    p = api.default_params(); p.num_levels = 1
    for mu in range(4):
        p.local_lattice[0][mu] = L[mu]; p.block_lattice[0][mu] = B[mu]
        if grid:
            p.process_grid[mu] = grid[mu]
    p.m0, p.csw = M0, CSW
    return p


def apply32(ctx, phi):
    x = ctx.vector(0, 32).upload(phi); y = ctx.vector(0, 32)
    ctx.dirac_apply(y, x)
    out = y.download()
    x.free(); y.free()
    return out


def switches(monkeypatch, pivot=None, compression=None):
    for name, v in (("DDAMG_LINK_PIVOT", pivot), ("DDAMG_LINK_COMPRESSION", compression)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def monomial_gauge(V, seed):
    """[V][4][9][2]: every link one of the 96 monomial SU(3) matrices, drawn uniformly"""
    M = lp.monomial_su3()
    pick = np.random.default_rng(seed).integers(0, len(M), V * 4)
    U = M[pick].reshape(V, 4, 9)
    return np.ascontiguousarray(np.stack([U.real, U.imag], -1))


def run(monkeypatch, L, U, phi, pivot, want, grid=None):
    switches(monkeypatch, pivot=pivot)
    ctx = dd.Context(params(L, grid=grid))
    if grid:
        ctx.comm_init_rccl(api.rccl_unique_id())
    ctx.set_gauge(U, anti_pbc=True)
    assert ctx.link_reals() == want
    out = apply32(ctx, phi)
    op = ctx.get_operator()
    ctx.close()
    return out, op


@pytest.mark.parametrize("L", SHAPES, ids=IDS)
def test_monomial_links_give_the_two_row_result_bit_for_bit(L, monkeypatch):
    """links with entries 0, +-1, +-i only: the reconstruction of row1[p] is exact, so any wrong select, sign, tail-row address or
    neighbour-link load of the 10-real path shows as a difference from the two-row path, without a tolerance"""
    V = int(np.prod(L))
    U = monomial_gauge(V, 5)
    phi = splitmix_uniform(V * 24, 21).reshape(V, 12, 2)
    out10, (D, _) = run(monkeypatch, L, U, phi, None, 10)
    _, b = lp.compress((D[..., 0] + 1j * D[..., 1]).reshape(V * 4, 3, 3))
    assert set(np.unique(b)) == {-3, -2, -1, 1, 2, 3}            # all three pivots and both signs are in the field
    out12, _ = run(monkeypatch, L, U, phi, "0", 12)
    assert np.abs(out12).max() > 0.1
    assert np.array_equal(out10, out12)


_random_case = {}


def random_case(monkeypatch, L):
    """random SU(3) links and a spinor on L, the fp64 oracle's result and the two-row form's worst per-site error against it
    (measured through DDAMG_LINK_PIVOT=0: the path of before, not the code under test); computed once per shape"""
    from oracle import orc, site_ops
    key = tuple(L)
    if key not in _random_case:
        V = int(np.prod(L))
        U = random_su3(V * 4, 7).reshape(V, 4, 9, 2)
        phi = splitmix_uniform(V * 24, 8).reshape(V, 12, 2)
        out12, (D, cl) = run(monkeypatch, L, U, phi, "0", 12)
        ref = orc.dirac_apply(L, D, cl, phi, 64)
        _random_case[key] = (U, phi, ref, out12, float(site_ops.per_site_error(out12, ref).max()))
    return _random_case[key]


@pytest.mark.parametrize("L", SHAPES, ids=IDS)
def test_random_links_against_the_oracle_and_the_two_row_form(L, monkeypatch):
    """random SU(3): worst site of the 10-real form within 1.5 x the worst site of the two-row form (the parent's path, measured
    here through the switch) against the fp64 oracle: the link part of the error grows by a quarter, it is only part of the
    total, and a maximum over a few thousand sites scatters by about a tenth.  The outputs are not bit-equal: the 10-real path ran.
    Measured on MI355X (worst per-site error, 10-real / two-row): 8x8x8x12 3.46e-7 / 3.20e-7; 12x4x8x8 3.89e-7 / 3.89e-7."""
    from oracle import site_ops
    U, phi, ref, out12, w12 = random_case(monkeypatch, L)
    out10, _ = run(monkeypatch, L, U, phi, None, 10)
    w10 = float(site_ops.per_site_error(out10, ref).max())
    print(f"{L}: worst per-site error 10-real {w10:.3e}, two-row {w12:.3e}, ratio {w10 / w12:.3f}")
    assert w10 <= 1.5 * w12
    assert not np.array_equal(out10, out12)


def test_fallbacks(monkeypatch):
    """a link that is no multiple of a unitary matrix: full links (18), bit-equal to DDAMG_LINK_COMPRESSION=0 on the same
    operator; DDAMG_LINK_COMPRESSION=0 with the pivot switch on: 18; 2^4 blocks: 18, never 10"""
    from oracle import orc
    L = SHAPES[1]; V = int(np.prod(L))
    U = random_su3(V * 4, 9).reshape(V, 4, 9, 2)
    phi = splitmix_uniform(V * 24, 10).reshape(V, 12, 2)
    D, cl, _ = orc.gauge_to_operator(L, U, 1, M0, CSW)
    D = D.copy(); D[V // 3, 18:27] *= 1.001                      # one link (direction 2) scaled
    outs = []
    for pivot, comp in (("1", None), ("1", "0")):
        switches(monkeypatch, pivot=pivot, compression=comp)
        ctx = dd.Context(params(L))
        ctx.set_operator(D, cl)
        assert ctx.link_reals() == 18
        outs.append(apply32(ctx, phi))
        ctx.close()
    assert np.array_equal(outs[0], outs[1])
    switches(monkeypatch, pivot="1", compression="0")
    ctx = dd.Context(params(L)); ctx.set_gauge(U, anti_pbc=True)
    assert ctx.link_reals() == 18
    ctx.close()
    switches(monkeypatch)
    ctx = dd.Context(params(L, B=(2, 2, 2, 2))); ctx.set_gauge(U, anti_pbc=True)
    assert ctx.link_reals() == 18
    ctx.close()
    ctx = dd.Context(params(L)); ctx.set_gauge(U, anti_pbc=True)
    assert ctx.link_reals() == 10
    ctx.close()


def test_second_upload_refills_the_field(monkeypatch):
    """set_gauge with A, then with B, on one context: the result of a fresh context on B, bit for bit"""
    L = SHAPES[1]; V = int(np.prod(L))
    A = random_su3(V * 4, 31).reshape(V, 4, 9, 2); B = random_su3(V * 4, 32).reshape(V, 4, 9, 2)
    phi = splitmix_uniform(V * 24, 33).reshape(V, 12, 2)
    switches(monkeypatch)
    ctx = dd.Context(params(L))
    ctx.set_gauge(A, anti_pbc=True)
    outA = apply32(ctx, phi)
    ctx.set_gauge(B, anti_pbc=True)
    assert ctx.link_reals() == 10
    outB = apply32(ctx, phi)
    ctx.close()
    fresh, _ = run(monkeypatch, L, B, phi, None, 10)
    assert np.array_equal(outB, fresh) and not np.array_equal(outA, outB)


def test_self_exchange_in_t(monkeypatch):
    """8x8x8x12 with the process its own neighbour in T (RCCL on one GPU): the boundary tiles run the same kernel through the tile
    list; within the bound of the random-links case against the oracle (1.5 x the two-row form's worst site, undivided).
    Measured on MI355X: 3.46e-7 against 3.20e-7."""
    from oracle import site_ops
    L = SHAPES[0]
    U, phi, ref, _, w12 = random_case(monkeypatch, L)
    out10, _ = run(monkeypatch, L, U, phi, None, 10, grid=[-1, 1, 1, 1])
    w10 = float(site_ops.per_site_error(out10, ref).max())
    print(f"self-exchange in T: worst per-site error 10-real {w10:.3e}, two-row undivided {w12:.3e}")
    assert w10 <= 1.5 * w12
