"""References for the Schwarz smoother of an intermediate level (CoarseSap<T>::smooth, coarse_mg.hip) at every block shape and dof
count: the shapes and cases of tests/test_gpu_coarse_schwarz_shapes.py, the operator, the fp64 reference (oracle/mg_oracle.py
`Schwarz` with plain-block MinRes on `coarse_matrix` of the operator), a Python restatement of the launch rule of the fused block
solver (`path`), and a second, vectorised restatement of the sweep (`CoarseSweep`, the schedule of schwarz_reference.Sweep around the
coarse block solver) which

  * in complex128 must agree with `mg_oracle.Schwarz` to rounding (tests/test_coarse_schwarz_reference.py), and then carries the
    wrong smoothers ("mutants") that the bar of the GPU test has to tell from the right one;
  * in complex64 rounds the operator, eta, phi0, every vector after every operation and the MinRes coefficient to fp32, every
    product and sum a rounded fp32 operation of its own (no fused multiply-add), in a stated order: the fused kernel's
    (coarse_block_minres_kernel, coarse_op.hip) or one of two permuted ones.

The kernel's order.  A product of a coupling with a site vector (wave_mv / wave_mv2): the matrix lies in 8x8 tiles, lane (a, b)
of the wavefront holds the entry (a, b) of every tile and sums its products over the tiles of its tile row one after the other;
the eight lanes of a row are then summed by a butterfly, ((0+1)+(2+3))+((4+5)+(6+7)).  The backward coupling G5 L^H G5 of the same
link: lane (a, b) sums conj(L_ab) (G5 v)_a over the tiles of its tile column, the butterfly runs over a, the sign G5 of the
result row comes last.  (D_block r)(i): the self coupling first, then the hopping terms subtracted in the order in which
make_block_plan made them (`contrib`: by the block-local index of the link's owner, then by direction).  The three block sums
<Dr,r> (two reals) and <Dr,Dr> run in fp64 over the fp32 values -- their order is immaterial at fp32 and they are summed by
numpy here --, alpha = <Dr,r> / <Dr,Dr> is rounded to fp32.  The residual updates between the block solves are those of
coarse_site_kernel: the nine products of a site in the order self, +T, +Z, +Y, +X, -T, -Z, -Y, -X.
The permuted orders shuffle the tiles, the lanes (the second sums them one after the other instead of by a butterfly) and the
hopping terms of a site.

The distance of the complex64 restatements from the fp64 reference is the *spread*: what correct fp32 code may differ by.  The
kernel's order runs at every shape, dof count, method and start, the permuted orders at the start from a guess, where the spread
is five to six times that of the starts from zero at every case.  Ten times
the largest spread over all cases is the fp32 bar of the GPU test (the factor ten for the orders not enumerated here: fused
multiply-adds, the step-by-step form of the block solver, the 16-bit kernel's register layout).  LARGEST_SPREAD records it;
tests/test_coarse_schwarz_reference.py recomputes it.  LARGEST_SPREAD_FP64 is the same for the two permuted orders in complex128
(red-black, from a guess): ten times it lies far below the fp64 bar of 1e-11, which therefore stands.

A MinRes step whose <Dr,Dr> lies below EPS_float = 1e-6 (fp64: EPS_double = 1e-14) is skipped by the reference, by the kernels and
by every restatement here; the fp64 reference of an fp32 run carries EPS_float.

Mutants (CoarseSweep(mutant=...)), and where each cannot differ from the right smoother:
  "iter3"  3 MinRes steps instead of 4.  Differs everywhere.
  "no45"   no list-4/5 rule in the first red-black sweep from zero.  Red-black only, and only where a block of the second colour
           has no face on the upper lattice boundary (lists 4 and 5), which needs a direction with more than two blocks: not on
           4^4, 4x4x4x8, 8x4x4x4, 4x4x8x8 and 4x8x8x8.
  "stale"  the residual update of the last colour reads `latest` as the colour before saw it.  Differs everywhere from the second
           cycle on.
  "nog5"   the backward coupling taken as L^H, without the signs G5 on either side (the factor sg of wave_mv2).  Differs wherever
           a backward coupling is applied: everywhere.
  "drop"   the last hopping item of make_block_plan (last owner site, its last direction inside the block) left out of the block
           solver, with both of its products.  Every shape has at least one hopping item per block, so it differs everywhere.

Vectors are complex [n V] in lexicographic site order (T,Z,Y,X; X fastest), index n site + dof."""
import numpy as np
from conftest import splitmix_uniform
from coarse_reference import pack
import schwarz_reference as sr
from schwarz_reference import STARTS, EPS, relerr, cvec      # the starts, thresholds and helpers of the fine twin

BLOCK_ITER = 4
METHODS = (1, 2, 3)
TOL_SWEEP = 1e-4        # the bar of test_gpu_three_levels.py for this kernel
# name: level-1 block (T,Z,Y,X), level-1 lattice, dof counts; "A": aggregates where they are not the blocks; "big": the lattice
# of the largest dof counts.  Every direction holds an even number of blocks; "2" .. "32-t" have one direction with more than two
# (blocks in list 5, a partial last launch), except on their "big" lattice.
SHAPES = {
    "2": dict(B=[2, 1, 1, 1], L=[12, 2, 2, 2], n=[48, 64]),
    "4": dict(B=[1, 1, 2, 2], L=[2, 2, 4, 12], n=[20]),
    "8": dict(B=[1, 2, 2, 2], L=[2, 4, 4, 12], n=[8, 48, 56]),
    "16": dict(B=[2, 2, 2, 2], L=[4, 4, 4, 12], n=[4, 6, 8, 12, 16, 20, 24, 32, 36, 40, 48, 52], big=([4, 4, 4, 4], [56, 64])),
    "24": dict(B=[2, 2, 2, 3], L=[4, 4, 4, 12], A=[2, 2, 2, 6], n=[20, 40, 48, 64]),
    "32-x": dict(B=[2, 2, 2, 4], L=[4, 4, 4, 24], n=[16, 32, 40], big=([4, 4, 4, 8], [64])),
    "32-t": dict(B=[4, 2, 2, 2], L=[24, 4, 4, 4], n=[16, 32], big=([8, 4, 4, 4], [64])),
    "64": dict(B=[2, 2, 4, 4], L=[4, 4, 8, 8], n=[16, 24, 32, 34]),
    "128": dict(B=[2, 4, 4, 4], L=[4, 8, 8, 8], n=[8, 16]),
}
CASES = [(name, n) for name, s in SHAPES.items() for n in s["n"] + s.get("big", ([], []))[1]]
# largest distance of a complex64 restatement (three orders) from the fp64 reference over CASES x METHODS x STARTS, and of a
# complex128 restatement in the two permuted orders, as test_coarse_schwarz_reference.py measures them
LARGEST_SPREAD = 7.3072e-07
LARGEST_SPREAD_FP64 = 5.6806e-15


def geometry(name, n):
    """(block, level-1 lattice, aggregate) of a case"""
    s = SHAPES[name]
    L = s["big"][0] if n in s.get("big", ([], []))[1] else s["L"]
    return list(s["B"]), list(L), list(s.get("A", s["B"]))


def block_sites(name):
    return int(np.prod(SHAPES[name]["B"]))


def fp32_bar():
    return 10 * LARGEST_SPREAD


def fp64_bar():
    return max(1e-11, 10 * LARGEST_SPREAD_FP64)


# ---- the launch rule of the fused block solver ---------------------------------------------------------------------------------
def path(B, n, prec):
    """CoarseOp<T>::block_minres and coarse_block_minres_kernel restated: which form of the block solver a shape is expected to
    take (it cannot be asked of the device) and which branches of the fused kernel it runs.  `half`: the number of self couplings
    a wavefront of coarse_half_block_minres_kernel keeps in registers, `nres` how many of the block are resident there"""
    BS = int(np.prod(B)); NT = (n + 7) // 8
    nitems = BS + sum(BS * (b - 1) // b for b in B)
    lds = 384 + (4 if prec == 32 else 8) * 16 * NT * (2 * BS + 2 * nitems)
    by_size, by_lds = BS * n > 2048, lds > 150 * 1024
    half = 2 if NT <= 5 else 1 if NT == 6 else 0
    return dict(fused=not (by_size or by_lds), by_size=by_size, by_lds=by_lds, NT=NT, nitems=nitems, lds=lds,
                resident=NT <= 6 and BS >= 8, items_in_lds=nitems <= 128, trips=-(-BS * n // 512), padded=n % 8 != 0,
                half=half, nres=min(BS, 8 * half))


def path_name(B, n, prec):
    p = path(B, n, prec)
    if not p["fused"]:
        return "step by step (" + ("BS n > 2048" if p["by_size"] else f"LDS {p['lds']} B") + ")"
    return (f"fused NT {p['NT']}, {'resident' if p['resident'] else 'streamed'} self couplings, items in {'LDS' if p['items_in_lds'] else 'global memory'}, "
            f"{p['trips']} trips, LDS {p['lds']} B")


# ---- operator and vectors -------------------------------------------------------------------------------------------------------
def random_couplings(n, Lc, seed):
    """(M0 [V][n][n], U [V][4][n][n]) well conditioned, so that MinRes on a Schwarz block never meets its eps guard by accident: self
    coupling [[A, B], [-B^H, D]] with A, D = 4 + 0.3 H, H Hermitian of unit-size entries, B = 0.3 x random, links 0.5 / sqrt(n) x
    random"""
    rng = np.random.default_rng(seed)
    V = int(np.prod(Lc)); N = n // 2

    def unit(*shape):
        return rng.uniform(-1, 1, size=shape) + 1j * rng.uniform(-1, 1, size=shape)

    def hermitian():
        up = np.triu(unit(V, N, N), 1)
        return up + up.conj().transpose(0, 2, 1) + np.eye(N) * rng.uniform(-1, 1, size=(V, N, 1))

    M0 = np.zeros((V, n, n), dtype=complex)
    B = 0.3 * unit(V, N, N)
    M0[:, :N, :N] = 4 * np.eye(N) + 0.3 * hermitian(); M0[:, N:, N:] = 4 * np.eye(N) + 0.3 * hermitian()
    M0[:, :N, N:] = B; M0[:, N:, :N] = -B.conj().transpose(0, 2, 1)
    return M0, 0.5 / np.sqrt(n) * unit(V, 4, n, n)


def random_operator(n, Lc, seed):
    """random_couplings in the storage of set_coarse_operator"""
    M0, U = random_couplings(n, Lc, seed)
    return pack(M0, U, Lc)


# cases whose first operator puts a <Dr,Dr> of the third cycle within 3 % of EPS_float (test_coarse_schwarz_reference.py measures
# it): they take the next seed
RESEED = {("8", 8): 2}
# 48 blocks of 16 sites at n = 12: in the third cycle the <Dr,Dr> of one MinRes step scatter around EPS_float whatever the seed
# (twelve seeds tried); eta and phi0 times this factor put the threshold between the values of two successive steps
SCALE = {("16", 12): 2.0}


def seed_of(name, n):
    return 7000 + 100 * list(SHAPES).index(name) + n + 10000 * RESEED.get((name, n), 0)


_COUPLINGS, _LEVEL, _MATRIX, _SCHWARZ, _OUT = {}, {}, {}, {}, {}


def forget(name, n):
    """drop what is cached for a case (the matrices of the larger ones take hundreds of megabytes)"""
    for cache in (_COUPLINGS, _LEVEL, _MATRIX):
        cache.pop((name, n), None)
    for cache in (_SCHWARZ, _OUT):
        for key in [k for k in cache if k[:2] == (name, n)]:
            del cache[key]


def couplings(name, n):
    if (name, n) not in _COUPLINGS:
        _COUPLINGS[(name, n)] = random_couplings(n, geometry(name, n)[1], seed_of(name, n))
    return _COUPLINGS[(name, n)]


def operator(name, n):
    """(D, clover) of the case for set_coarse_operator(level=1)"""
    return pack(*couplings(name, n), geometry(name, n)[1])


def vectors(name, n):
    """(eta, phi0) as [V][n][2] reals"""
    V = int(np.prod(geometry(name, n)[1])); f = SCALE.get((name, n), 1.0)
    return f * splitmix_uniform(V * n * 2, 3).reshape(V, n, 2), f * splitmix_uniform(V * n * 2, 4).reshape(V, n, 2)


def matrix(name, n):
    """the operator as an fp64 sparse matrix: oracle.mg_oracle.coarse_matrix on the storage that the library gets"""
    from oracle import mg_oracle as mo
    if (name, n) not in _MATRIX:
        D, cl = operator(name, n)
        _MATRIX[(name, n)] = mo.coarse_matrix(geometry(name, n)[1], D, cl, n)
    return _MATRIX[(name, n)]


def schwarz(name, n, method, prec):
    """the fp64 restatement of the smoother the library runs in precision `prec` (32 or 64): plain-block MinRes, the arithmetic fp64
    in both, the threshold below which a MinRes step is skipped that precision's"""
    from oracle import mg_oracle as mo
    key = (name, n, method, prec)
    if key not in _SCHWARZ:
        B, L, _ = geometry(name, n)
        _SCHWARZ[key] = mo.Schwarz(L, B, matrix(name, n), BLOCK_ITER, method, ndof=n, odd_even=False, eps=EPS[prec])
    return _SCHWARZ[key]


def reference(name, n, method, start, prec):
    """phi of the fp64 reference as complex [n V]; computed once"""
    key = (name, n, method, start, prec)
    if key not in _OUT:
        cycles, guess = STARTS[start]
        eta, phi0 = vectors(name, n)
        _OUT[key] = schwarz(name, n, method, prec).smooth(cvec(eta), cycles, phi0=cvec(phi0) if guess else None)
        _OUT[key].setflags(write=False)
    return _OUT[key]


def guard_blocks(name, n):
    """the two blocks on which eta vanishes in the eps-guard case: the first of colour 0 and, of colour 1, the first of lists 4 / 5
    where there is one (it gets no residual update in the first red-black sweep from zero, so that its residual is exactly zero),
    else the first; as indices into mg_oracle.Schwarz.blocks (lexicographic over the block lattice)"""
    S = schwarz(name, n, 2, 32)
    c0 = next(i for i, b in enumerate(S.blocks) if b["colour"] == 0)
    c1 = [i for i, b in enumerate(S.blocks) if b["colour"] == 1]
    late = [i for i in c1 if S.blocks[i]["list"] in (4, 5)]
    return c0, (late or c1)[0]


def guard_eta(name, n):
    """eta [V][n][2] of the eps-guard case"""
    eta = vectors(name, n)[0].copy()
    S = schwarz(name, n, 2, 32)
    for b in guard_blocks(name, n):
        eta.reshape(-1, 2)[S.blocks[b]["I"]] = 0.0
    return eta


def guard_reference(name, n, prec):
    key = (name, n, 2, "guard", prec)
    if key not in _OUT:
        _OUT[key] = schwarz(name, n, 2, prec).smooth(cvec(guard_eta(name, n)), 1)
        _OUT[key].setflags(write=False)
    return _OUT[key]


# ---- the level site by site -----------------------------------------------------------------------------------------------------
class Level:
    """geometry of a case as Geometry::build and make_block_plan lay it out: `sites` [blocks][BS] the lexicographic sites of every
    block in block-local order (even r_T + r_Z + r_Y + r_X first, lexicographic inside); `nbs` [V][8] the neighbour in +T,+Z,+Y,+X,
    -T,-Z,-Y,-X; `inb` [V][8] it lies in the same block; `nbl` [BS][8] its block-local index or -1; `contrib` [BS][8] the
    directions whose products enter (D_block r)(i), in the order of make_block_plan, padded with -1; `last_item` (i, mu, j)"""

    def __init__(self, name, n):
        from oracle import mg_oracle as mo
        B, L, _ = geometry(name, n)
        self.B, self.L, self.n = np.array(B), np.array(L), n
        V = int(np.prod(L)); self.V = V
        c = mo.coords(L)
        nblk = [L[mu] // B[mu] for mu in range(4)]
        assert all(k % 2 == 0 for k in nblk)
        self.block_of = mo.lex(c // self.B, nblk)
        self.BS = int(np.prod(B)); self.nb = V // self.BS
        par = (c % self.B).sum(axis=1) % 2
        self.sites = np.lexsort((np.arange(V), par, self.block_of)).reshape(self.nb, self.BS)
        assert np.all(self.block_of[self.sites] == np.arange(self.nb)[:, None])
        loc = np.empty(V, dtype=np.int64); loc[self.sites] = np.arange(self.BS)[None, :]
        self.nbs = np.empty((V, 8), dtype=np.int64)
        for mu in range(4):
            for d, sgn in ((mu, 1), (4 + mu, -1)):
                cc = c.copy(); cc[:, mu] = (cc[:, mu] + sgn) % L[mu]
                self.nbs[:, d] = mo.lex(cc, L)
        self.inb = self.block_of[self.nbs] == self.block_of[:, None]
        s0 = self.sites[0]
        self.nbl = np.where(self.inb[s0], loc[self.nbs[s0]], -1)
        for b in range(self.nb):       # the table is the same for every block
            assert np.array_equal(np.where(self.inb[self.sites[b]], loc[self.nbs[self.sites[b]]], -1), self.nbl)
        entries = [[] for _ in range(self.BS)]
        for i in range(self.BS):
            for mu in range(4):
                j = self.nbl[i, mu]
                if j >= 0:
                    entries[i].append(((i, mu), mu)); entries[j].append(((i, mu), 4 + mu))
                    self.last_item = (i, mu, int(j))
        self.contrib = np.full((self.BS, 8), -1, dtype=np.int64)
        for i in range(self.BS):
            for q, (_, d) in enumerate(sorted(entries[i])):
                self.contrib[i, q] = d
        assert sum(len(e) for e in entries) // 2 + self.BS == path(B, n, 32)["nitems"]
        self.g5 = np.concatenate([np.ones(n // 2), -np.ones(n // 2)])


def level(name, n):
    if (name, n) not in _LEVEL:
        _LEVEL[(name, n)] = Level(name, n)
    return _LEVEL[(name, n)]


class Order:
    """in which order the sums run: `seed` None the kernel's, else tiles, lanes and the hopping terms of a site shuffled; `tree`
    the eight lanes by a butterfly (as the kernel does) or one after the other"""

    def __init__(self, seed=None, tree=True):
        self.seed, self.tree = seed, tree
        self.lanes = np.arange(8) if seed is None else np.random.default_rng(seed).permutation(8)

    def tiles(self, NT):
        return np.arange(NT) if self.seed is None else np.random.default_rng(self.seed + NT).permutation(NT)

    def slots(self, k):
        return np.arange(k) if self.seed is None else np.random.default_rng(self.seed + 100 + k).permutation(k)


KERNEL_ORDER = Order()
ORDERS = (KERNEL_ORDER, Order(1, tree=True), Order(2, tree=False))


class _Rows:
    def __init__(self, lv, blocks):
        self.blocks = list(blocks)
        self.sites = lv.sites[self.blocks]                                        # [nb][BS]
        self.rows = (lv.n * self.sites[:, :, None] + np.arange(lv.n)).ravel()


class Products:
    """One coupling times one site vector, for many sites at once (M [S][n][n] as real and imaginary part, v [S][n] complex), in the
    type `ct` and the summation order `order` of a wavefront; blas = True: by numpy's matrix product instead (complex128 only, where
    the order of a sum is far below what is asserted; tests/test_coarse_schwarz_reference.py holds the ordered form to it)"""

    def __init__(self, n, ct, order, g5_signs=True, blas=False):
        self.n, self.ct, self.order, self.blas = n, ct, order, blas
        self.rt = np.float32 if ct == np.complex64 else np.float64
        assert not blas or ct == np.complex128
        self.g5 = np.concatenate([np.ones(n // 2), -np.ones(n // 2)]).astype(self.rt) if g5_signs else np.ones(n, dtype=self.rt)

    def _reduce(self, pr, pi):
        """the sum over the last axis in the order of a wavefront: tile after tile in every lane, then across the eight lanes"""
        n = pr.shape[-1]; NT = (n + 7) // 8
        out = []
        for p in (pr, pi):
            acc = None
            for q in self.order.tiles(NT):
                t = p[..., 8 * q:8 * q + 8]
                if t.shape[-1] < 8:                                               # the padding columns hold zeros
                    t = np.concatenate([t, np.zeros(t.shape[:-1] + (8 - t.shape[-1],), dtype=p.dtype)], axis=-1)
                acc = t if acc is None else acc + t
            acc = acc[..., self.order.lanes]
            if self.order.tree:
                while acc.shape[-1] > 1:
                    acc = acc[..., 0::2] + acc[..., 1::2]
                out.append(acc[..., 0])
            else:
                tot = acc[..., 0]
                for k in range(1, 8):
                    tot = tot + acc[..., k]
                out.append(tot)
        res = np.empty(out[0].shape, dtype=self.ct)
        res.real, res.imag = out
        return res

    def mv(self, Mr, Mi, v):
        """M v as wave_mv<DAG = false> / the forward half of wave_mv2"""
        if self.blas:
            return np.matmul(Mr + 1j * Mi, v[:, :, None])[:, :, 0]
        vr, vi = v.real[:, None, :], v.imag[:, None, :]
        return self._reduce(Mr * vr - Mi * vi, Mr * vi + Mi * vr)

    def mv_dag(self, Mr, Mi, v):
        """G5 M^H G5 v as wave_mv<DAG = true> / the backward half of wave_mv2"""
        if self.blas:
            return self.g5 * np.matmul((Mr - 1j * Mi).swapaxes(1, 2), (self.g5 * v)[:, :, None])[:, :, 0]
        Mr, Mi = Mr.swapaxes(1, 2), Mi.swapaxes(1, 2)                              # [S][column][row]
        wr, wi = (self.g5 * v.real)[:, None, :], (self.g5 * v.imag)[:, None, :]
        return self.g5 * self._reduce(Mr * wr + Mi * wi, Mr * wi - Mi * wr)


class CoarseSweep(sr.Sweep):
    """The sweep of `mg_oracle.Schwarz` S (its colours, block lists and method; the schedule is schwarz_reference.Sweep.smooth)
    around the plain-block MinRes of an intermediate level, over all blocks of a colour at once, in the type `ct` and the
    summation order `order`.  mutant: see the module docstring.  In complex128 and the kernel's order the products of a coupling
    with a site vector run through numpy's matrix product (Products.blas): the mutants and the comparison with the oracle do not
    depend on the order of a sum"""

    def __init__(self, name, n, S, ct=np.complex128, order=KERNEL_ORDER, mutant=None):
        lv = level(name, n)
        self.lv, self.S, self.ct, self.order, self.mutant = lv, S, ct, order, mutant
        self.rt = np.float32 if ct == np.complex64 else np.float64
        self.eps, self.margin = S.eps, np.inf
        self.block_iter = S.block_iter - 1 if mutant == "iter3" else S.block_iter
        assert np.array_equal(S.block_of, lv.block_of) and not S.odd_even
        self.colour = np.array([b["colour"] for b in S.blocks]); self.list = np.array([b["list"] for b in S.blocks])
        self.ncol = int(self.colour.max()) + 1
        M0, U = couplings(name, n)
        self.M0r, self.M0i = M0.real.astype(self.rt), M0.imag.astype(self.rt)
        self.Ur, self.Ui = U.real.astype(self.rt), U.imag.astype(self.rt)
        self.P = Products(n, ct, order, g5_signs=mutant != "nog5", blas=ct == np.complex128 and order is KERNEL_ORDER)
        self.contrib, self.nbl = lv.contrib.copy(), lv.nbl
        if mutant == "drop":
            i, mu, j = lv.last_item
            for site, d in ((i, mu), (j, 4 + mu)):
                row = [s for s in self.contrib[site] if s != d]
                assert len(row) == 7
                self.contrib[site] = row + [-1]
        self._rows = {}

    def rows(self, blocks, part="all"):
        assert part == "all"
        if blocks not in self._rows:
            self._rows[blocks] = _Rows(self.lv, blocks)
        return self._rows[blocks]

    def self_product(self, s, v):
        return self.P.mv(self.M0r[s], self.M0i[s], v)

    def hop_product(self, s, d, v):
        """the hopping term of direction d of the sites s, v the vectors of their neighbours in that direction"""
        if d < 4:
            return self.P.mv(self.Ur[s, d], self.Ui[s, d], v)
        y = self.lv.nbs[s, d]
        return self.P.mv_dag(self.Ur[y, d - 4], self.Ui[y, d - 4], v)

    def products(self, sites, x, which):
        """the products of the eight hopping terms of `sites` [S] with the full vector x [V][n] where which [S][8] says so, zero
        elsewhere: [S][8][n]"""
        lv = self.lv
        out = np.zeros((len(sites), 8, lv.n), dtype=self.ct)
        for d in range(8):
            k = np.nonzero(which[:, d])[0]
            if len(k):
                out[k, d] = self.hop_product(sites[k], d, x[lv.nbs[sites[k], d]])
        return out

    def full(self, R, x):
        """D x on the rows of R as coarse_site_kernel<T, NT, MODE_FULL> sums it"""
        s = R.sites.ravel(); x = x.reshape(self.lv.V, self.lv.n)
        acc = self.self_product(s, x[s])
        P = self.products(s, x, np.ones((len(s), 8), dtype=bool))
        for d in self.order.slots(8):
            acc = acc - P[:, d]
        return acc.ravel()

    def hop_out(self, R, x):
        """minus the hopping terms that leave the block (coarse_site_kernel<T, NT, MODE_HOP> under the block-face mask adds them
        up, the masked ones as zeros, and adds the sum to r)"""
        s = R.sites.ravel(); x = x.reshape(self.lv.V, self.lv.n)
        P = self.products(s, x, ~self.lv.inb[s])
        acc = None
        for d in self.order.slots(8):
            acc = P[:, d] if acc is None else acc + P[:, d]
        return -acc.ravel()

    def block_op(self, R, rb):
        """D_block r for the blocks of R, rb [nb][BS][n]"""
        nb, BS, n = rb.shape
        acc = self.self_product(R.sites.ravel(), rb.reshape(nb * BS, n)).reshape(nb, BS, n)
        P = np.zeros((nb, BS, 8, n), dtype=self.ct)
        for d in range(8):
            k = np.nonzero(self.nbl[:, d] >= 0)[0]
            if len(k):
                P[:, k, d] = self.hop_product(R.sites[:, k].ravel(), d, rb[:, self.nbl[k, d]].reshape(-1, n)).reshape(nb, len(k), n)
        for q in self.order.slots(8):
            d = self.contrib[:, q]
            term = P[:, np.arange(BS), np.maximum(d, 0)]
            acc = acc - np.where((d >= 0)[None, :, None], term, 0)
        return acc

    def minres_step(self, Dr, rb, d, nb):
        f8 = np.float64
        dr, di, rr, ri = (a.astype(f8) for a in (Dr.real, Dr.imag, rb.real, rb.imag))
        ax = (1, 2)
        s0 = (dr * rr + di * ri).sum(axis=ax); s1 = (dr * ri - di * rr).sum(axis=ax); s2 = (dr * dr + di * di).sum(axis=ax)
        ok = np.abs(s2) >= self.eps
        self.margin = min(self.margin, float(np.abs(s2 / self.eps - 1).min()))
        s2 = np.where(ok, s2, 1)
        ar = np.where(ok, s0 / s2, 0).astype(self.rt)[:, None, None]; ai = np.where(ok, s1 / s2, 0).astype(self.rt)[:, None, None]
        dn = np.empty_like(d); rn = np.empty_like(rb)
        dn.real = d.real + (ar * rb.real - ai * rb.imag); dn.imag = d.imag + (ar * rb.imag + ai * rb.real)
        rn.real = rb.real - (ar * Dr.real - ai * Dr.imag); rn.imag = rb.imag - (ar * Dr.imag + ai * Dr.real)
        return dn, rn

    def solve(self, blocks, x, r, out, w):
        R = self.rows(blocks)
        nb, BS, n = len(blocks), self.lv.BS, self.lv.n
        rb = r[R.rows].reshape(nb, BS, n); d = np.zeros_like(rb)
        for _ in range(self.block_iter):
            d, rb = self.minres_step(self.block_op(R, rb), rb, d, nb)
        x[R.rows] += d.ravel(); out[R.rows] = d.ravel(); r[R.rows] = rb.ravel()


PERMUTED_START = "2 from a guess"       # where the spread is largest (five to six times that of the starts from zero) at every case


def restatements(name, n, method, start, ct=np.complex64, orders=ORDERS):
    cycles, guess = STARTS[start]
    eta, phi0 = (cvec(v) for v in vectors(name, n))
    S = schwarz(name, n, method, 32 if ct == np.complex64 else 64)
    return [CoarseSweep(name, n, S, ct, o).smooth(eta, cycles, phi0 if guess else None) for o in orders]


def spread(name, n, method, start):
    """the kernel's order at every start, the permuted ones at PERMUTED_START"""
    ref = reference(name, n, method, start, 32)
    return max(relerr(x, ref) for x in restatements(name, n, method, start, orders=ORDERS if start == PERMUTED_START else ORDERS[:1]))


def spread_fp64(name, n, method, start):
    ref = reference(name, n, method, start, 64)
    return max(relerr(x, ref) for x in restatements(name, n, method, start, np.complex128, ORDERS[1:]))
