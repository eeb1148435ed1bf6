"""The inverted self couplings of the coarsest level (-m gpu): invert_self_kernel (coarse_op.hip), a batched Gauss-Jordan
elimination in fp64 in LDS without pivoting, and coarse_site_kernel<T, NT, MODE_SELFINV> that applies its result, through
coarse_self_mul(..., inverse=True), against numpy.linalg.solve of the matrix as the device stores it (row a13 of
docs/design/01a_coverage.md).

Two-level contexts on a 2x4x4x4 coarsest lattice, fp32 and fp64, n = 4, 8, ..., 64 and 6, 10, the operator installed by
set_coarse_operator.  Self couplings [[A, B], [-B^H, D]] (the Hermitian part is diag(A, D)):
  easy  the well-conditioned one of coarse_schwarz_reference.random_couplings (4 + 0.3 H);
  hard  A = Q diag(lambda) Q^H, D likewise, with random unitary Q and lambda spaced geometrically in [8 / kappa, 8], kappa spread
        over the sites from 10 to 1000, and B = 0.3 / sqrt(kappa n / 2) x random, small enough to leave the condition number of the
        site near kappa: the Hermitian part is positive definite throughout (every pivot of the
        elimination has a positive real part, so it needs no pivoting), its smallest eigenvalue goes down to 0.008 -- a diagonal of
        4 + m with m = -3.5 would leave 0.5 -- and the condition numbers spread up to about 10^3 (printed).

The bound, per real component, with u = 2^-24 (fp32) or 2^-53 (fp64), gamma_k(u) = k u / (1 - k u), G = M^-1:
      | out - G y |  <=  gamma_{n+2}(u) (|G| |y|)  +  10 E sum_j |y_j|.
The first term covers the rounding of the stored inverse to the vectors' precision (one u) and the product (a complex
multiplication is two roundings deep, the sum over the tiles of a row and the butterfly over its eight lanes at most n / 8 + 2).
E is the elimination's own error in fp64, measured here on the CPU: `gauss_jordan` restates the kernel's pivot-free elimination
in its order, and E is the largest entry of |gauss_jordan(M) - G| of the site, with G = numpy.linalg.inv(M) refined by one residual
step in longdouble.  It is one number per site and not a matrix: the error of a single entry in one order of the arithmetic says
nothing about that entry in another order (a unit input reads one entry of the inverse; against ten times numpy's error of that
very entry the device's fp64 elimination lay at 2.2 at n = 6), the size of the errors of a site does.  The factor ten is for the
differences between numpy's and the device's fp64 arithmetic (fused multiply-adds).  The largest E over the sites, and relative to
the largest entry of |G|, is printed per n.

The way back: out = M (G y) returns y within 2 |M| (bound above): |M| times the error of the first product, plus the error
gamma (|M| |G y|) of the second, which the first term of the bound propagated through |M| covers once more.

After shift_mass the diagonal of the stored self coupling moves by the difference of the masses (shift_self_diagonal_kernel: the
stored diagonal plus the difference, rounded to the vectors' precision) and the inverse is recomputed: the same bound against a
reference rebuilt from the shifted matrix.  The mass shift reaches a coarse level only once a setup has run, so these contexts run
setup(0) first."""
import numpy as np
import pytest
from conftest import splitmix_uniform
from coarse_reference import pack
from coarse_schwarz_reference import random_couplings
from test_gpu_many_rhs_kernels import two_level_ctx

pytestmark = pytest.mark.gpu

LC = [2, 4, 4, 4]
V = int(np.prod(LC))
NS = sorted(set(range(4, 65, 4)) | {6, 10})
SHIFT_NS = [6, 24, 64]
SENTINEL = 30000.5
ODD = np.stack(np.unravel_index(np.arange(V), LC), axis=1).sum(axis=1) % 2 == 1


def hard_couplings(n, seed):
    rng = np.random.default_rng(seed)
    N = n // 2

    def unit(*shape):
        return rng.uniform(-1, 1, size=shape) + 1j * rng.uniform(-1, 1, size=shape)

    kappa = 10.0 ** (1 + 2 * rng.permutation(V) / (V - 1))

    def pd_block():
        Q, _ = np.linalg.qr(unit(V, N, N))
        lam = 8.0 / kappa[:, None] ** (np.arange(N)[None, :] / max(N - 1, 1))
        H = (Q * lam[:, None, :]) @ Q.conj().transpose(0, 2, 1)
        H = (H + H.conj().transpose(0, 2, 1)) / 2
        idx = np.arange(N); H[:, idx, idx] = H[:, idx, idx].real
        return H

    M0 = np.zeros((V, n, n), dtype=complex)
    B = (0.3 / np.sqrt(kappa * N))[:, None, None] * unit(V, N, N)
    M0[:, :N, :N] = pd_block(); M0[:, N:, N:] = pd_block()
    M0[:, :N, N:] = B; M0[:, N:, :N] = -B.conj().transpose(0, 2, 1)
    return M0, 0.5 / np.sqrt(n) * unit(V, 4, n, n)


def stored(a, prec):
    """a complex or real array as the device holds it"""
    if prec == 64:
        return a
    return a.astype(np.complex64).astype(np.complex128) if np.iscomplexobj(a) else a.astype(np.float32).astype(np.float64)


def gauss_jordan(M):
    """invert_self_kernel in numpy, for all sites at once: in place, column k of the identity replaces column k of A as it is
    eliminated, no pivoting; complex products as (ar br - ai bi, ar bi + ai br) in fp64"""
    A = M.astype(np.complex128).copy()
    n = A.shape[1]
    for k in range(n):
        p = A[:, k, k]
        d = p.real * p.real + p.imag * p.imag
        piv = p.real / d + 1j * (-p.imag / d)
        col = A[:, :, k].copy()
        row = A[:, k, :] * piv[:, None]
        row[:, k] = piv
        upd = col[:, :, None] * row[:, None, :]
        new = A - upd
        new[:, :, k] = -upd[:, :, k]
        new[:, k, :] = row
        A = new
    return A


def refined_inverse(M):
    """numpy.linalg.inv and one step G <- G + G (1 - M G) with the residual and the update in longdouble"""
    G = np.linalg.inv(M).astype(np.clongdouble)
    Ml = M.astype(np.clongdouble)
    R = np.eye(M.shape[1], dtype=np.clongdouble)[None] - np.einsum("xij,xjk->xik", Ml, G)
    return G + np.einsum("xij,xjk->xik", G, R)


def gamma(k, prec):
    u = 2.0 ** -24 if prec == 32 else 2.0 ** -53
    return k * u / (1 - k * u)


class Reference:
    """the stored matrix M of every site, G = M^-1 refined, E the elimination's error, and the bound of an input"""

    def __init__(self, M0, prec):
        self.n, self.prec = M0.shape[1], prec
        self.M = stored(M0, prec)
        Gl = refined_inverse(self.M)
        self.G = Gl.astype(np.complex128)
        self.absG = np.abs(self.G)
        self.E = np.abs((gauss_jordan(self.M).astype(np.clongdouble) - Gl)).astype(np.float64).max(axis=(1, 2))
        self.cond = np.linalg.cond(self.M)

    def solve(self, y):
        """numpy.linalg.solve, and one residual step in longdouble: in fp64 the error of the plain solve reaches 0.7 of the bound
        below (measured on the CPU at n = 4), which would leave the device too little of it"""
        x = np.linalg.solve(self.M, y[..., None])[..., 0]
        r = (y.astype(np.clongdouble) - np.einsum("xij,xj->xi", self.M.astype(np.clongdouble), x.astype(np.clongdouble))).astype(np.complex128)
        return x + np.linalg.solve(self.M, r[..., None])[..., 0]

    def bound(self, y):
        ay = np.abs(y)
        return gamma(self.n + 2, self.prec) * np.einsum("xij,xj->xi", self.absG, ay) + 10 * (self.E * ay.sum(axis=1))[:, None]


def cplx(a):
    return a[..., 0] + 1j * a[..., 1]


def worst(got, ref, bound):
    """largest |component error| / bound over the real and imaginary parts"""
    err = np.maximum(np.abs(got.real - ref.real), np.abs(got.imag - ref.imag))
    return float((err / bound).max())


def inputs(n, prec):
    unit = np.zeros((V, n, 2)); unit[np.arange(V), np.arange(V) % n, 0] = 1.0
    rnd = splitmix_uniform(V * n * 2, 77 + n).reshape(V, n, 2)
    return {"random": rnd, "unit": unit}


def self_mul(ctx, prec, y, parity, inverse):
    """one coarse_self_mul; the sites of the other parity must keep the sentinel"""
    vi = ctx.vector(1, prec).upload(y); vo = ctx.vector(1, prec).upload(np.full(y.shape, SENTINEL))
    ctx.coarse_self_mul(vo, vi, parity, inverse)
    out = vo.download()
    vi.free(); vo.free()
    mine = ODD if parity else ~ODD
    assert np.all(out[~mine] == SENTINEL), f"parity {parity}: the other parity was touched"
    return out, mine


def check_inverse(ctx, ref, prec, what):
    n = ref.n
    ratios = {}
    for name, y in inputs(n, prec).items():
        yc = stored(cplx(y), prec)
        x, b = ref.solve(yc), ref.bound(yc)
        for parity in (0, 1):
            out, mine = self_mul(ctx, prec, y, parity, True)
            got = cplx(out)
            assert np.all(np.isfinite(out[mine]))
            ratios[(name, parity, "inverse")] = worst(got[mine], x[mine], b[mine])
            # and back: M (G y) = y within 2 |M| bound
            back, _ = self_mul(ctx, prec, out * mine[:, None, None], parity, False)
            b2 = 2 * np.einsum("xij,xj->xi", np.abs(ref.M), b)
            ratios[(name, parity, "round trip")] = worst(cplx(back)[mine], yc[mine], b2[mine])
    print(f"self inverse n {n} fp{prec} {what}: cond {ref.cond.min():.1f} .. {ref.cond.max():.1f}; elimination error {ref.E.max():.2e} = {ref.E.max() / ref.absG.max():.2e} of the "
          f"largest entry; largest error / bound: " + ", ".join(f"{k[0]} p{k[1]} {k[2]} {r:.3f}" for k, r in ratios.items()))
    bad = {k: r for k, r in ratios.items() if not r <= 1}
    assert not bad, bad


@pytest.fixture(scope="module", params=[(n, mp) for n in NS for mp in (1, 0)], ids=lambda p: f"n{p[0]}-mp{p[1]}")
def level(request):
    n, mp = request.param
    ctx = two_level_ctx(LC, n // 2, mixed_precision=mp)
    prec = ctx.vprec()
    assert prec == (32 if mp else 64) and ctx.ndof(1) == n
    if n in SHIFT_NS:
        ctx.setup(0)
    yield ctx, n, prec
    ctx.close()


@pytest.mark.parametrize("kind", ["easy", "hard"])
def test_inverse_of_the_self_coupling(level, kind):
    ctx, n, prec = level
    M0, U = random_couplings(n, LC, 8100 + n) if kind == "easy" else hard_couplings(n, 8200 + n)
    ctx.set_coarse_operator(*pack(M0, U, LC), level=1)
    check_inverse(ctx, Reference(M0, prec), prec, kind)


def test_inverse_follows_a_mass_shift(level):
    ctx, n, prec = level
    if n not in SHIFT_NS:
        return
    M0, U = hard_couplings(n, 8300 + n)
    ctx.set_coarse_operator(*pack(M0, U, LC), level=1)
    m0 = float(ctx.params.m0)
    cur, total = m0, 0.0
    try:
        for shift in (0.25, -0.004):          # the second leaves the smallest eigenvalue of the Hermitian part at 0.004
            ctx.shift_mass(m0 + shift)
            total += (m0 + shift) - cur; cur = m0 + shift          # the library adds up the differences it is given, in fp64
            Ms = stored(M0, prec).copy()
            idx = np.arange(n)
            Ms[:, idx, idx] = stored(Ms[:, idx, idx].real + stored(np.array([total]), prec)[0], prec) + 1j * Ms[:, idx, idx].imag
            check_inverse(ctx, Reference(Ms, prec), prec, f"hard, mass shifted by {shift}")
    finally:
        ctx.shift_mass(m0)
