"""References for the fine Schwarz smoother (sap.hip) at every block volume: the shapes and cases of tests/test_gpu_schwarz_shapes.py,
the fp64 reference (oracle/mg_oracle.py `Schwarz` on the fine matrix of the pinned C oracle), and a second, vectorised restatement
of the same sweep (`Sweep`) which

  * in complex128 must agree with `mg_oracle.Schwarz` to rounding (tests/test_schwarz_reference.py), and then carries the wrong
    smoothers ("mutants") that the bar of the GPU test has to tell from the right one;
  * in complex64 rounds the operator, eta, phi0, every vector after every operation (residual update, D r, the two MinRes updates,
    the odd-site back-substitution) and the MinRes scalars to fp32, with every sum running in fp32 in a stated order: the kernels'
    (clover term first, then the directions T, Z, Y, X, forward before backward, the six products of a direction one after the
    other; the twelve components of a site one after the other and then a binary tree over the sites of a block, across wavefronts
    of 64 one after the other) or one of two permuted ones (slots, components and sites shuffled; the second sums the sites one
    after the other instead of by a tree).

The distance of the complex64 restatements from the fp64 reference is the *spread*: what correct fp32 code may differ by.  Ten times
the largest spread over all shapes and cases is the bar of the GPU test (the factor ten for the orders not enumerated here: fused
multiply-adds, the projection before the link product, ...).  The largest spread is a property of this file's inputs; it is recorded
in LARGEST_SPREAD so that the GPU test does not have to run the restatements, and tests/test_schwarz_reference.py recomputes it.

A MinRes step whose <Dr,Dr> lies below EPS_float = 1e-6 (fp64: EPS_double = 1e-14) is skipped by the reference, by the kernels and
by every restatement here; the fp64 reference of an fp32 run therefore carries EPS_float (`schwarz(..., prec)`).  That is a rule of
the algorithm, not rounding: at 16-site blocks it decides the last step of the third red-black cycle from zero.

Vectors are complex [12 V] in lexicographic order (T,Z,Y,X; X fastest), index 12 site + dof."""
import numpy as np
from conftest import random_su3, splitmix_uniform

M0, CSW, BLOCK_ITER = 0.3, 1.0, 4
# name: (block (T,Z,Y,X), lattice).  Every direction holds an even number of blocks; all but the last have one direction with more
# than two, once the first and once the last direction; up to 64 sites a colour of the sixteen-colour schedule holds 3 blocks
SHAPES = {
    "16": ([2, 2, 2, 2], [4, 4, 4, 12]),
    "32-x": ([2, 2, 2, 4], [4, 4, 4, 24]), "32-t": ([4, 2, 2, 2], [24, 4, 4, 4]),
    "64-x": ([2, 2, 4, 4], [4, 4, 8, 24]), "64-t": ([4, 4, 2, 2], [24, 8, 4, 4]),
    "128-x": ([2, 4, 4, 4], [4, 8, 8, 16]), "128-t": ([4, 4, 4, 2], [16, 8, 8, 4]),
    "256": ([2, 4, 4, 8], [8, 8, 8, 16]),
    "512": ([4, 4, 4, 8], [8, 8, 8, 16]),
}
METHODS = (1, 2, 3)
STARTS = {"1 from zero": (1, False), "3 from zero": (3, False), "2 from a guess": (2, True)}
# largest distance of a complex64 restatement (three orders) from the fp64 reference over SHAPES x {odd-even, plain} x METHODS x
# STARTS, as test_schwarz_reference.py::test_spread measures it
LARGEST_SPREAD = 1.1427e-06
TOL_SWEEP = 5e-5
EPS = {32: 1e-6, 64: 1e-14}     # EPS_float, EPS_double of the reference: a MinRes step with <Dr,Dr> below it is skipped


def block_sites(name):
    return int(np.prod(SHAPES[name][0]))


def forms(name):
    """odd_even values the library offers at this block volume (the plain kernel stops at 256 sites)"""
    return (True, False) if block_sites(name) <= 256 else (True,)


def fp32_bar():
    return 10 * LARGEST_SPREAD


def relerr(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


_LATTICE, _SCHWARZ, _ELL, _OUT = {}, {}, {}, {}
_ROWS = {}          # the row sets of the shape in work: (shape, type, mutant columns, blocks, part) -> _Rows


def gauge(L):
    V = int(np.prod(L))
    return random_su3(V * 4, 31 + V).reshape(V, 4, 9, 2)


def fine_matrix(L):
    """the fine operator as an fp64 sparse matrix from the pinned C oracle, once per lattice"""
    from oracle import mg_oracle as mo, orc
    key = tuple(L)
    if key not in _LATTICE:
        D, cl, _ = orc.gauge_to_operator(list(L), gauge(L), 1, M0, CSW)
        _LATTICE[key] = mo.fine_matrix(list(L), D, cl)
    return _LATTICE[key]


def vectors(L):
    """(eta, phi0) as [V][12][2] reals"""
    V = int(np.prod(L))
    return splitmix_uniform(V * 24, 3).reshape(V, 12, 2), splitmix_uniform(V * 24, 4).reshape(V, 12, 2)


def cvec(a):
    a = np.asarray(a, dtype=np.float64)
    return (a[..., 0] + 1j * a[..., 1]).ravel()


def schwarz(name, method, odd_even, prec):
    """the fp64 restatement of the smoother the library runs in precision `prec` (32 or 64): the arithmetic is fp64 in both, the
    threshold below which a MinRes step is skipped is that precision's"""
    from oracle import mg_oracle as mo
    key = (name, method, odd_even, prec)
    if key not in _SCHWARZ:
        B, L = SHAPES[name]
        _SCHWARZ[key] = mo.Schwarz(L, B, fine_matrix(L), BLOCK_ITER, method, odd_even=odd_even, eps=EPS[prec])
    return _SCHWARZ[key]


def reference(name, method, odd_even, start, prec):
    """phi of the fp64 reference as complex [12 V]; computed once"""
    key = (name, method, odd_even, start, prec)
    if key not in _OUT:
        cycles, guess = STARTS[start]
        eta, phi0 = vectors(SHAPES[name][1])
        _OUT[key] = schwarz(name, method, odd_even, prec).smooth(cvec(eta), cycles, phi0=cvec(phi0) if guess else None)
        _OUT[key].setflags(write=False)
    return _OUT[key]


# ---- the operator slot by slot ---------------------------------------------------------------------------------------------------
class Ell:
    """The fine matrix with the 54 entries of every row in fixed slots: 0..5 the clover block, 6 + 6 d .. 11 + 6 d the hop in
    direction d = 2 mu (to x + mu) or 2 mu + 1 (to x - mu); `inblk`: the column lies in the row's block; `cinv`: the inverses of the
    clover blocks in the slots 0..5"""

    def __init__(self, A, L, B):
        from oracle import mg_oracle as mo
        L = np.array(L); B = np.array(B)
        V = int(np.prod(L)); n = 12 * V
        c = mo.coords(list(L))
        self.L, self.B, self.c = L, B, c
        self.block_of = mo.lex(c // B, list(L // B))
        A = A.tocoo()
        rs, cs = A.row // 12, A.col // 12
        d = (c[cs] - c[rs]) % L
        cls = np.zeros(len(rs), dtype=np.int64)
        for mu in range(4):
            assert L[mu] >= 3
            cls[d[:, mu] == 1] = 1 + 2 * mu
            cls[d[:, mu] == L[mu] - 1] = 2 + 2 * mu
        assert np.all((cls > 0) == (rs != cs))
        o = np.lexsort((A.col, cls, A.row))
        assert len(o) == 54 * n and np.array_equal(A.row[o].reshape(n, 54), np.repeat(np.arange(n), 54).reshape(n, 54))
        assert np.array_equal(cls[o].reshape(n, 54), np.broadcast_to(np.repeat(np.arange(9), 6), (n, 54)))
        self.cols = A.col[o].reshape(n, 54).astype(np.int64)
        self.vals = A.data[o].reshape(n, 54)
        self.inblk = self.block_of[self.cols // 12] == self.block_of[np.arange(n) // 12][:, None]
        Cb = self.vals[:, :6].reshape(V, 2, 6, 6)
        assert np.array_equal(self.cols[:, :6].reshape(V, 2, 6, 6)[:, :, 0], 12 * np.arange(V)[:, None, None] + 6 * np.arange(2)[None, :, None] + np.arange(6))
        self.cinv = np.linalg.inv(Cb).reshape(n, 6)
        # mutant: across a block face of the direction with more than two blocks, read the block on the other side
        nblk = L // B
        mu = int(np.argmax(nblk))
        self.cols_swapped = None
        if nblk[mu] > 2:
            cs_ = self.cols.copy()
            site = np.arange(n) // 12
            for d_, shift in ((2 * mu, 1 - 2 * B[mu]), (2 * mu + 1, 2 * B[mu] - 1)):
                cc = c[site].copy(); cc[:, mu] = (cc[:, mu] + shift) % L[mu]
                other = mo.lex(cc, list(L))
                sl = slice(6 + 6 * d_, 12 + 6 * d_)
                cs_[:, sl] = np.where(self.inblk[:, sl], self.cols[:, sl], 12 * other[:, None] + self.cols[:, sl] % 12)
            self.cols_swapped = cs_


def ell(name):
    B, L = SHAPES[name]
    key = (tuple(B), tuple(L))
    if key not in _ELL:
        _ELL[key] = Ell(fine_matrix(L), L, B)
    return _ELL[key]


class Order:
    """in which order the sums run: `hop` a permutation of the 48 hop slots, `self` of the 6 clover slots, `comp` of the 12
    components of a site, `sites` a seed for the permutation of the sites of a block (None: as they are), `tree` binary tree over
    the sites (as the kernels do) or one after the other"""

    def __init__(self, seed=None, tree=True):
        rng = np.random.default_rng(seed)
        self.hop = np.arange(48) if seed is None else rng.permutation(48)
        self.self_ = np.arange(6) if seed is None else rng.permutation(6)
        self.comp = np.arange(12) if seed is None else rng.permutation(12)
        self.seed, self.tree = seed, tree

    def sites(self, S):
        return None if self.seed is None else np.random.default_rng(self.seed + S).permutation(S)


KERNEL_ORDER = Order()
ORDERS = (KERNEL_ORDER, Order(1, tree=True), Order(2, tree=False))


def _acc(vals, cols, x, order, init=None):
    acc = init
    for k in order:
        t = vals[k] * x[cols[k]]
        acc = t if acc is None else acc + t
    return acc


class _Rows:
    """the slots of a set of rows, slot-major, cast to the working type"""

    def __init__(self, e, rows, ct, swapped):
        self.rows = rows
        self.cl_c = np.ascontiguousarray(e.cols[rows, :6].T.astype(np.int32))
        self.cl_v = np.ascontiguousarray(e.vals[rows, :6].T).astype(ct)
        self.ci_v = np.ascontiguousarray(e.cinv[rows].T).astype(ct)
        self.h_c = np.ascontiguousarray(e.cols[rows, 6:].T.astype(np.int32))
        self.h_c_out = np.ascontiguousarray(e.cols_swapped[rows, 6:].T.astype(np.int32)) if swapped else self.h_c
        hv = np.ascontiguousarray(e.vals[rows, 6:].T).astype(ct)
        inb = np.ascontiguousarray(e.inblk[rows, 6:].T)
        self.h_in = np.where(inb, hv, 0).astype(ct)      # a product with an exact zero adds nothing to a sum
        self.h_out = np.where(inb, 0, hv).astype(ct)


class Sweep:
    """The sweep of `mg_oracle.Schwarz` S (its colours, block lists, method, block solver and matrix) over all blocks of a colour
    at once, in the type `ct` and the summation order `order`.  mutant: None, "iter3" (one MinRes step fewer), "no45" (red-black
    from zero without the list-4/5 rule), "stale" (the residual update of the last colour reads `latest` as the colour before saw
    it), "swap" (the +mu and -mu neighbour blocks exchanged in the direction with more than two blocks)"""

    def __init__(self, name, S, ct=np.complex128, order=KERNEL_ORDER, mutant=None):
        e = ell(name)
        self.e, self.S, self.ct, self.order, self.mutant = e, S, ct, order, mutant
        self.rt = np.float32 if ct == np.complex64 else np.float64
        self.eps = S.eps
        self.margin = np.inf     # closest any <Dr,Dr> came to the threshold, as |<Dr,Dr> / eps - 1|
        self.block_iter = S.block_iter - 1 if mutant == "iter3" else S.block_iter
        assert np.array_equal(S.block_of, e.block_of)
        if mutant == "swap":
            assert e.cols_swapped is not None
        nb = len(S.blocks)
        self.colour = np.array([b["colour"] for b in S.blocks]); self.list = np.array([b["list"] for b in S.blocks])
        self.ncol = int(self.colour.max()) + 1
        self.BS = int(np.prod(e.B))
        par = e.c.sum(axis=1) % 2
        # sites block by block, even sites first, lexicographic inside: [blocks][BS]
        o = np.lexsort((np.arange(len(par)), par, e.block_of))
        self.sites = o.reshape(nb, self.BS)
        assert np.all(e.block_of[self.sites] == np.arange(nb)[:, None]) and np.all(par[self.sites[:, :self.BS // 2]] == 0)
        self.name = name
        if _ROWS and next(iter(_ROWS))[0] != name:
            _ROWS.clear()

    def rows(self, blocks, part):
        """rows of the blocks in `blocks` (a tuple of block indices): part "e", "o" or "all"; [blocks][sites][12] flattened"""
        key = (self.name, self.ct, self.mutant == "swap", blocks, part)
        if key not in _ROWS:
            H = self.BS // 2
            s = self.sites[list(blocks)]
            s = s[:, :H] if part == "e" else s[:, H:] if part == "o" else s
            r = (12 * s[:, :, None] + np.arange(12)).ravel()
            _ROWS[key] = _Rows(self.e, r, self.ct, self.mutant == "swap")
        return _ROWS[key]

    # ---- pieces of the operator on a row set, x a full vector ----
    def clover(self, R, x):
        return _acc(R.cl_v, R.cl_c, x, self.order.self_)

    def clover_inv(self, R, x):
        return _acc(R.ci_v, R.cl_c, x, self.order.self_)

    def hop_in(self, R, x, init=None):
        return _acc(R.h_in, R.h_c, x, self.order.hop, init)

    def hop_out(self, R, x):
        return _acc(R.h_out, R.h_c_out, x, self.order.hop)

    def full(self, R, x):
        # the couplings to other blocks go through h_c_out, so that the mutant "swap" reaches the full residual too
        e = self.clover(R, x)
        for k in self.order.hop:
            e = e + R.h_in[k] * x[R.h_c[k]] + R.h_out[k] * x[R.h_c_out[k]]
        return e

    def block_sum(self, p, nb):
        """sum of p [nb * S * 12] over the sites and components of every block: [nb]"""
        p = p.reshape(nb, -1, 12)
        S = p.shape[1]
        acc = None
        for k in self.order.comp:
            acc = p[:, :, k] if acc is None else acc + p[:, :, k]
        perm = self.order.sites(S)
        if perm is not None:
            acc = acc[:, perm]
        if self.order.tree:
            W = min(S, 64)
            q = acc.reshape(nb, S // W, W)
            while W > 1:
                W //= 2
                q = q[..., :W] + q[..., W:]
            acc = q[..., 0]
        tot = acc[:, 0]
        for k in range(1, acc.shape[1]):
            tot = tot + acc[:, k]
        return tot

    def minres_step(self, Dr, rm, d, nb):
        num = self.block_sum(np.conj(Dr) * rm, nb)
        dn = self.block_sum((Dr.real * Dr.real + Dr.imag * Dr.imag), nb)
        ok = np.abs(dn) >= self.eps
        self.margin = min(self.margin, float(np.abs(dn / self.eps - 1).min()))
        dn = np.where(ok, dn, 1)
        alpha = np.where(ok, num.real / dn, 0).astype(self.rt) + 1j * np.where(ok, num.imag / dn, 0).astype(self.rt)
        alpha = np.repeat(alpha.astype(self.ct), len(rm) // nb)
        return d + alpha * rm, rm - alpha * Dr

    def solve(self, blocks, x, r, out, w):
        """the block solves of `blocks`; w: scratch full vector"""
        nb = len(blocks)
        if not self.S.odd_even:
            R = self.rows(blocks, "all")
            rb = r[R.rows]; d = np.zeros_like(rb)
            for _ in range(self.block_iter):
                w[R.rows] = rb
                Dr = self.hop_in(R, w, init=self.clover(R, w))
                d, rb = self.minres_step(Dr, rb, d, nb)
            x[R.rows] += d; out[R.rows] = d; r[R.rows] = rb
            return
        E, O = self.rows(blocks, "e"), self.rows(blocks, "o")
        ro = r[O.rows]
        w[O.rows] = ro
        w[O.rows] = self.clover_inv(O, w)
        re = r[E.rows] - self.hop_in(E, w)
        de = np.zeros_like(re)
        for _ in range(self.block_iter):
            w[E.rows] = re
            w[O.rows] = self.hop_in(O, w)
            w[O.rows] = self.clover_inv(O, w)
            Dr = self.clover(E, w) - self.hop_in(E, w)
            de, re = self.minres_step(Dr, re, de, nb)
        w[E.rows] = de
        w[O.rows] = ro - self.hop_in(O, w)
        do = self.clover_inv(O, w)
        x[E.rows] += de; x[O.rows] += do
        out[E.rows] = de; out[O.rows] = do
        r[E.rows] = re; r[O.rows] = 0

    def smooth(self, eta, cycles, phi0=None):
        ct, S = self.ct, self.S
        eta = eta.astype(ct)
        x = np.zeros_like(eta) if phi0 is None else phi0.astype(ct)
        r = eta.copy(); w = np.zeros_like(eta)
        additive = S.method == 1
        latest = x.copy() if (additive and phi0 is not None) else np.zeros_like(eta)
        seen = []                                          # `latest` as the residual updates saw it, one entry per colour step
        of_colour = [tuple(np.nonzero(self.colour == c)[0]) for c in range(self.ncol)]
        late = tuple(b for b in of_colour[-1] if self.list[b] not in (4, 5)) if S.method == 2 else None
        have_res = phi0 is not None
        for k in range(cycles):
            new = np.zeros_like(eta) if additive else latest
            for c in range(self.ncol):
                blocks = of_colour[c]
                # which residual update (the rules of mg_oracle.Schwarz.smooth and _smooth_generic)
                if S.method == 2:
                    if k == 0 and phi0 is not None:
                        mode = "full"
                    elif k == 0:
                        mode = None if c == 0 else "boundary"
                        if c == 1 and self.mutant != "no45":
                            blocks = late
                    else:
                        mode = "boundary"
                elif not have_res:
                    mode = None
                else:
                    first = k == 0 if (additive or S.sixteen) else (k == 0 and phi0 is not None)
                    mode = "full" if first else "boundary"
                seen.append(latest.copy() if self.mutant == "stale" else None)
                if mode == "full":
                    R = self.rows(blocks, "all")
                    r[R.rows] = eta[R.rows] - self.full(R, latest if additive else x)
                elif mode == "boundary" and len(blocks):
                    R = self.rows(blocks, "all")
                    src = latest
                    if self.mutant == "stale" and c == self.ncol - 1:
                        src = seen[-2] if len(seen) > 1 else np.zeros_like(eta)
                    r[R.rows] = r[R.rows] - self.hop_out(R, src)
                self.solve(of_colour[c], x, r, new, w)
                have_res = True
            latest = new
        return x.astype(np.complex128)


def restatements(name, method, odd_even, start):
    """the complex64 restatements of a case in the three orders"""
    cycles, guess = STARTS[start]
    eta, phi0 = (cvec(v) for v in vectors(SHAPES[name][1]))
    S = schwarz(name, method, odd_even, 32)
    return [Sweep(name, S, np.complex64, o).smooth(eta, cycles, phi0 if guess else None) for o in ORDERS]


def spread(name, method, odd_even, start):
    ref = reference(name, method, odd_even, start, 32)
    return max(relerr(x, ref) for x in restatements(name, method, odd_even, start))
