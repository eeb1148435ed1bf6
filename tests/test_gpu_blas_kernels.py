"""The kernels of blas.hip, one operation per process of tests/native/blas_driver, against plain numpy (-m gpu).

Two kinds of input.

EXACT.  Every entry is a small integer: basis vectors X_i in {-1, +1}, w and the panel's columns in {-2, .., 2}, coefficients
Gaussian integers.  Then every product is an integer of magnitude <= 2, every fp32 group sum of panel_dot_kernel (32 products)
one of magnitude <= 64, every fp64 partial sum an integer far below 2^53 in whatever order it is formed, and every partial sum
of an updated entry  w + sum_i c_i X_i  is an integer bounded by |w| + sum_i (|re c_i| + |im c_i|).  Each test asserts in numpy,
before the driver starts, that this last bound, the dots that become fp32 coefficients and the group sums stay below 2^22
(< 2^24, where fp32 stops holding every integer).  So the device result is exact in both precisions and must EQUAL numpy's
int64 arithmetic: one missed, doubled or misplaced chunk changes it, at any length, where a relative tolerance would not see one
chunk in 2^21.

RANDOM (splitmix_uniform in (-0.5, 0.5), rounded to fp32 for the float cases; the reference is fp64 numpy on those values).
u = 2^-24 (float) or 2^-53 (double).
* elementwise: every real operation of the type rounds once, so an expression of k operations on magnitudes M is off by at
  most gamma_k M, gamma_k = k u / (1 - k u)  [Higham, Accuracy and Stability, Lemma 3.1; contraction to fma only removes
  roundings].  axpy  x + ar*yr - ai*yi: k = 4, M = |x| + |ar||yr| + |ai||yi|; scale: k = 3; plus / minus: k = 2 (the factor
  +-1 and the sum); scale_inv  x * (T)(1.0 / s): k = 3 (reciprocal, conversion, product); multi_axpy: k = 4m,
  M = |w| + sum_i (|cr_i||x| + |ci_i||y|) with the coefficients rounded to T as the kernel rounds them.
* reductions accumulated in fp64 (multi_dot, norm, dot_and_norm2, panel_dot for double): products of fp32 numbers are exact in
  fp64, the sum of n terms in any order is off by at most gamma_n(fp64) S, S = sum |x_k||w_k|; for the n <= 4.2e6 terms here
  that is 4.7e-10 S in the worst case and ~sqrt(n) u = 2e-13 S for a serial sum; the two-stage tree sum (<= 2 terms per
  thread and pass, 8 shuffle levels, 4 waves, <= 1024 blocks) has depth < 40, so 40 u = 4.4e-15 S; the issue's bound
  1e-13 S is used.  Errors are measured against S, never against the dot (which is ~0 for random vectors).
* fp32 panel_dot_kernel: a group of 8 chunks (32 products) is summed in fp32: rounded products and 31 additions, at most
  gamma_33(fp32) <= 33 * 2^-24 S per group, then fp64 as above: 33 * 2^-24 S + 1e-13 S.

Every reduction runs twice inside the driver; the two results must be bit-identical (blas.h: deterministic, no atomics).
Elements outside a view carry a sentinel and must come back bit-identical.
"""
import zlib
import numpy as np
import pytest
from conftest import splitmix_uniform
import native_driver as nd

pytestmark = pytest.mark.gpu

TYPES = ["float", "double"]
CH = {"float": 4, "double": 2}
DT = {"float": np.float32, "double": np.float64}
UBITS = {"float": np.uint32, "double": np.uint64}
U = {"float": 2.0 ** -24, "double": 2.0 ** -53}
SENTINEL = -12345.6875          # exactly representable in fp32
LIMIT = 2 ** 22
CB = 4                          # PANEL_COLUMNS
BIG = (32 << 20)                # bytes per vector at which stream_sized switches to the non-temporal kernels (above it)

LENGTHS = [1, 255, 256, 257, 773, 2305, 262403]       # chunks; reductions: 1024-block cap passed at 262403
LENGTHS_EW = LENGTHS + [524547]                        # elementwise: 2048-block cap
VIEWS = [(part, nb) for part in ("even", "odd") for nb in (1, 3, 40)]


def gamma(k, ty):
    return k * U[ty] / (1 - k * U[ty])


def pad64(n):
    return (n + 63) // 64 * 64


# ---- views ------------------------------------------------------------------------------------------------------------------
def whole(nchunks, ty):
    n = nchunks * CH[ty]
    return dict(rows=1, stride=0, off=0, len=n), n


def block_view(part, nb, ty):
    """the even / odd sites of every 2^4 Schwarz block of a 24-real field over nb blocks (mg.cpp, bicgstab.h)"""
    ch = CH[ty]
    return dict(rows=(24 // ch) * nb, stride=16 * ch, off=0 if part == "even" else 8 * ch, len=8 * ch), 24 * 16 * nb


def make_view(spec, ty):
    return whole(spec, ty) if isinstance(spec, int) else block_view(spec[0], spec[1], ty)


def addresses(v):
    """the reals a view addresses, in the order of its chunks (numpy restatement of chunk_addr)"""
    return (v["off"] + np.arange(v["rows"], dtype=np.int64)[:, None] * v["stride"] + np.arange(v["len"], dtype=np.int64)[None, :]).ravel()


def spec_id(s):
    return str(s) if isinstance(s, int) else f"{s[0]}{s[1]}"


def cplx(a):
    return a[..., 0::2] + 1j * a[..., 1::2]


def bits(a, ty):
    return np.ascontiguousarray(a).view(UBITS[ty])


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape, dtype=np.int8).astype(np.int64)


def signs(rng, shape):
    return ints(rng, shape, 0, 1) * 2 - 1


def uniform(n, seed, ty):
    u = splitmix_uniform(n, seed)
    return u.astype(np.float32).astype(np.float64) if ty == "float" else u


def embed(logical, idx, nalloc, ty):
    """a buffer of sentinels with `logical` at the view's addresses"""
    buf = np.full(nalloc, SENTINEL, dtype=DT[ty])
    buf[idx] = logical
    return buf


def embed_many(logical, idx, stride, ty, extra=0):
    """vectors logical[i] at i*stride + the view's addresses"""
    buf = np.full(stride * (len(logical) + extra), SENTINEL, dtype=DT[ty])
    for i, l in enumerate(logical):
        buf[i * stride + idx] = l
    return buf


def check_outside(got, before, idx_list, ty):
    mask = np.ones(len(before), bool)
    for idx in idx_list:
        mask[idx] = False
    assert np.array_equal(bits(got, ty)[mask], bits(before, ty)[mask]), "elements outside the view changed"


def int_cdot(Xl, wl):
    """<X_i, w> for integer arrays with interleaved (re, im): conjugate on X"""
    xr, xi, wr, wi = Xl[..., 0::2], Xl[..., 1::2], wl[..., 0::2], wl[..., 1::2]
    return (xr * wr + xi * wi).sum(-1), (xr * wi - xi * wr).sum(-1)


def int_caxpy(wl, cr, ci, xl):
    """w + (cr + i ci) x on interleaved integer arrays"""
    out = wl.copy()
    out[0::2] += cr * xl[0::2] - ci * xl[1::2]
    out[1::2] += cr * xl[1::2] + ci * xl[0::2]
    return out


def abs_cdot(Xl, wl):
    """the sums of |products| behind the real and the imaginary part of <X_i, w>"""
    xr, xi, wr, wi = np.abs(Xl[..., 0::2]), np.abs(Xl[..., 1::2]), np.abs(wl[..., 0::2]), np.abs(wl[..., 1::2])
    return (xr * wr + xi * wi).sum(-1), (xr * wi + xi * wr).sum(-1)


def timeout_for(nreal_total):
    return 40 + nreal_total // (1 << 21)


# ---- multi_dot --------------------------------------------------------------------------------------------------------------
DOT_CASES = [(l, 5) for l in LENGTHS] + [(773, m) for m in (1, 3, 4, 8, 9, 12)] + [(v, 5) for v in (("even", 1), ("odd", 3), ("even", 40))]


def run_multi_dot(tmp_path, ty, spec, m, Xl, wl, max_m=12, **kw):
    v, nalloc = make_view(spec, ty)
    idx = addresses(v)
    xstride = pad64(nalloc) + 64                      # Gmres::alloc pads to 64; larger than the vector
    r = nd.run(tmp_path, dict(op="multi_dot", type=ty, m=m, xstride=xstride, max_m=max_m, **v),
               dict(x=embed_many(Xl, idx, xstride, ty), y=embed(wl, idx, nalloc, ty)), timeout=timeout_for(m * nalloc), **kw)
    if kw:
        return None
    res = r.read("res", np.float64).reshape(2, 2 * m)
    assert np.array_equal(res[0].view(np.uint64), res[1].view(np.uint64)), "two runs of the reduction differ"
    return res[0]


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("spec,m", DOT_CASES, ids=[f"{spec_id(s)}-m{m}" for s, m in DOT_CASES])
def test_multi_dot_exact(tmp_path, ty, spec, m):
    """multi_dot_kernel + final_sum_kernel on integer inputs: equal to int64 arithmetic (tile tail m % 4, capped grid, views)"""
    v, _ = make_view(spec, ty)
    n = v["rows"] * v["len"]
    rng = rng_for("dot", spec, m)
    Xl, wl = signs(rng, (m, n)), ints(rng, n, -2, 2)
    re, im = int_cdot(Xl, wl)
    assert 2 * n * 2 < 2 ** 53
    got = run_multi_dot(tmp_path, ty, spec, m, Xl, wl)
    print("multi_dot exact", ty, spec, m, "max |got - ref|", np.abs(got[0::2] - re).max(), np.abs(got[1::2] - im).max())
    assert np.array_equal(got[0::2], re.astype(np.float64)) and np.array_equal(got[1::2], im.astype(np.float64))


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("spec,m", [(257, 5), (2305, 5), (262403, 5), (773, 12), (("odd", 3), 5)], ids=["257", "2305", "262403", "773-m12", "odd3"])
def test_multi_dot_random(tmp_path, ty, spec, m):
    """fp64-accumulated: |got - ref| <= 1e-13 sum |x||w| (module docstring)"""
    v, _ = make_view(spec, ty)
    n = v["rows"] * v["len"]
    Xl, wl = uniform(m * n, 3, ty).reshape(m, n), uniform(n, 4, ty)
    ref = np.array([np.vdot(cplx(Xl[i]), cplx(wl)) for i in range(m)])
    sre, sim = abs_cdot(Xl, wl)
    got = run_multi_dot(tmp_path, ty, spec, m, Xl, wl)
    ere, eim = np.abs(got[0::2] - ref.real) / sre, np.abs(got[1::2] - ref.imag) / sim
    print("multi_dot random", ty, spec, m, "error / sum|x||w|", ere.max(), eim.max())
    assert ere.max() <= 1e-13 and eim.max() <= 1e-13


@pytest.mark.parametrize("ty", TYPES)
def test_multi_dot_refuses_more_vectors_than_the_workspace(tmp_path, ty):
    Xl, wl = np.ones((13, 8 * CH[ty])), np.ones(8 * CH[ty])
    run_multi_dot(tmp_path, ty, 8, 13, Xl, wl, max_m=12, expect_error="multi_dot: too many vectors for the reduction workspace")


# ---- multi_axpy -------------------------------------------------------------------------------------------------------------
AXPY_CASES = [(l, 5) for l in LENGTHS_EW] + [(773, m) for m in (1, 3, 4, 8, 9, 12)] + [(v, 5) for v in (("odd", 1), ("even", 3), ("odd", 40))]


def run_multi_axpy(tmp_path, ty, spec, m, wl, Xl, coef, sign):
    v, nalloc = make_view(spec, ty)
    idx = addresses(v)
    xstride = pad64(nalloc) + 64
    before = embed(wl, idx, nalloc, ty)
    r = nd.run(tmp_path, dict(op="multi_axpy", type=ty, m=m, xstride=xstride, sign=float(sign), **v),
               dict(w=before, X=embed_many(Xl, idx, xstride, ty), coef=np.asarray(coef, np.float64)), timeout=timeout_for(m * nalloc))
    got = r.read("w", DT[ty])
    check_outside(got, before, [idx], ty)
    return got[idx].astype(np.float64)


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("spec,m", AXPY_CASES, ids=[f"{spec_id(s)}-m{m}" for s, m in AXPY_CASES])
def test_multi_axpy_exact(tmp_path, ty, spec, m):
    """multi_axpy_kernel on integer inputs and Gaussian-integer coefficients: equal to int64 arithmetic"""
    v, _ = make_view(spec, ty)
    n = v["rows"] * v["len"]
    rng = rng_for("axpy", spec, m)
    Xl, wl, coef = signs(rng, (m, n)), ints(rng, n, -2, 2), ints(rng, 2 * m, -3, 3)
    sign = -1 if m % 2 else 1
    assert 2 + np.abs(coef).sum() < LIMIT
    ref = wl
    for i in range(m):
        ref = int_caxpy(ref, sign * coef[2 * i], sign * coef[2 * i + 1], Xl[i])
    got = run_multi_axpy(tmp_path, ty, spec, m, wl, Xl, coef, sign)
    print("multi_axpy exact", ty, spec, m, "max |got - ref|", np.abs(got - ref).max())
    assert np.array_equal(got, ref.astype(np.float64))


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("spec,m", [(257, 5), (524547, 5), (("even", 40), 3)], ids=["257", "524547", "even40"])
def test_multi_axpy_random(tmp_path, ty, spec, m):
    """k = 4m operations per entry on M = |w| + sum_i (|cr||x| + |ci||y|), coefficients rounded to T as the kernel does"""
    v, _ = make_view(spec, ty)
    n = v["rows"] * v["len"]
    Xl, wl = uniform(m * n, 5, ty).reshape(m, n), uniform(n, 6, ty)
    coef = 3.0 * splitmix_uniform(2 * m, 7)
    ct = coef.astype(DT[ty]).astype(np.float64)
    c = ct[0::2] + 1j * ct[1::2]
    ref = cplx(wl) - (c[:, None] * cplx(Xl)).sum(0)
    mre = np.abs(wl[0::2]) + (np.abs(ct[0::2])[:, None] * np.abs(Xl[:, 0::2]) + np.abs(ct[1::2])[:, None] * np.abs(Xl[:, 1::2])).sum(0)
    mim = np.abs(wl[1::2]) + (np.abs(ct[0::2])[:, None] * np.abs(Xl[:, 1::2]) + np.abs(ct[1::2])[:, None] * np.abs(Xl[:, 0::2])).sum(0)
    got = cplx(run_multi_axpy(tmp_path, ty, spec, m, wl, Xl, coef, -1.0))
    ere, eim = np.abs(got.real - ref.real) / mre, np.abs(got.imag - ref.imag) / mim
    print("multi_axpy random", ty, spec, m, "error / M in units of u", ere.max() / U[ty], eim.max() / U[ty])
    assert ere.max() <= gamma(4 * m, ty) and eim.max() <= gamma(4 * m, ty)


# ---- panel projection -------------------------------------------------------------------------------------------------------
PANEL_CASES = ([(773, nb, m) for nb in (1, 2, 3, 4) for m in (1, 4, 5, 9)] + [(l, 3, 5) for l in LENGTHS if l != 773]
               + [(v, 2, 5) for v in (("even", 1), ("odd", 3), ("even", 40))])


def run_panel(tmp_path, ty, spec, nb, m, Wl, Xl, max_m=36, wcols=CB, second_w=1, **kw):
    v, nalloc = make_view(spec, ty)
    idx = addresses(v)
    xstride, wstride = pad64(nalloc) + 64, pad64(nalloc) + 192      # wstride != xstride
    before = embed_many(Wl, idx, wstride, ty, extra=wcols - len(Wl))   # the columns after nb: sentinels throughout
    r = nd.run(tmp_path, dict(op="panel", type=ty, m=m, nb=nb, xstride=xstride, wstride=wstride, max_m=max_m, second_w=second_w, **v),
               dict(W=before, X=embed_many(Xl, idx, xstride, ty)), timeout=timeout_for((m + nb) * nalloc), **kw)
    if kw:
        return None
    coef = r.read("coef", np.float64).reshape(2, m, CB, 2)
    assert np.array_equal(coef[0].view(np.uint64), coef[1].view(np.uint64)), "two runs of the panel's reduction differ"
    got = r.read("W", DT[ty])
    if second_w:
        assert np.array_equal(bits(got, ty), bits(r.read("W2", DT[ty]), ty)), "two runs of the panel's update differ"
    check_outside(got, before, [q * wstride + idx for q in range(nb)], ty)
    return coef[0], np.stack([got[q * wstride + idx] for q in range(nb)]).astype(np.float64)


def panel_exact(tmp_path, ty, spec, nb, m, **kw):
    v, _ = make_view(spec, ty)
    n = v["rows"] * v["len"]
    rng = rng_for("panel", spec, nb, m)
    Xl, Wl = signs(rng, (m, n)), ints(rng, (nb, n), -2, 2)
    cre = np.empty((m, nb), np.int64); cim = np.empty((m, nb), np.int64)
    ref = []
    for q in range(nb):
        cre[:, q], cim[:, q] = int_cdot(Xl, Wl[q])
        out = Wl[q]
        for i in range(m):
            out = int_caxpy(out, -cre[i, q], -cim[i, q], Xl[i])
        ref.append(out)
    # fp32 group sums (32 products of magnitude <= 2), the coefficients as fp32 numbers, every partial sum of an updated entry
    assert 32 * 2 < LIMIT and max(np.abs(cre).max(), np.abs(cim).max()) < LIMIT
    assert 2 + (np.abs(cre) + np.abs(cim)).sum(0).max() < LIMIT
    coef, got = run_panel(tmp_path, ty, spec, nb, m, Wl, Xl, **kw)
    print("panel exact", ty, spec, nb, m, "max |coef - ref|", np.abs(coef[:, :nb, 0] - cre).max(), np.abs(coef[:, :nb, 1] - cim).max(),
          "max |W - ref|", np.abs(got - np.stack(ref)).max())
    assert np.array_equal(coef[:, :nb, 0], cre.astype(np.float64)) and np.array_equal(coef[:, :nb, 1], cim.astype(np.float64))
    assert np.array_equal(got, np.stack(ref).astype(np.float64))


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("spec,nb,m", PANEL_CASES, ids=[f"{spec_id(s)}-nb{nb}-m{m}" for s, nb, m in PANEL_CASES])
def test_panel_project_exact(tmp_path, ty, spec, nb, m):
    """panel_dot_kernel (padded one-dimensional grid, early return, fp32 groups and their remainder) + panel_axpy_kernel
    (columns >= nb not written: they hold sentinels) on integer inputs: equal to int64 arithmetic.  m = 9 fills max_m = 36."""
    panel_exact(tmp_path, ty, spec, nb, m)


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("spec,nb,m", [(773, 4, 9), (2305, 3, 5), (262403, 2, 4), (("odd", 3), 3, 5)], ids=["773", "2305", "262403", "odd3"])
def test_panel_project_random(tmp_path, ty, spec, nb, m):
    """dots: 33 * 2^-24 S + 1e-13 S (float), 1e-13 S (double); update: 4m operations with the coefficients the device returned"""
    v, _ = make_view(spec, ty)
    n = v["rows"] * v["len"]
    Xl, Wl = uniform(m * n, 8, ty).reshape(m, n), uniform(nb * n, 9, ty).reshape(nb, n)
    coef, got = run_panel(tmp_path, ty, spec, nb, m, Wl, Xl)
    bound = 1e-13 + (33 * U["float"] if ty == "float" else 0.0)
    for q in range(nb):
        ref = np.array([np.vdot(cplx(Xl[i]), cplx(Wl[q])) for i in range(m)])
        sre, sim = abs_cdot(Xl, Wl[q])
        ere, eim = np.abs(coef[:, q, 0] - ref.real) / sre, np.abs(coef[:, q, 1] - ref.imag) / sim
        ct = coef[:, q, :].astype(DT[ty]).astype(np.float64)
        c = ct[:, 0] + 1j * ct[:, 1]
        upd = cplx(Wl[q]) - (c[:, None] * cplx(Xl)).sum(0)
        mre = np.abs(Wl[q, 0::2]) + (np.abs(ct[:, :1]) * np.abs(Xl[:, 0::2]) + np.abs(ct[:, 1:]) * np.abs(Xl[:, 1::2])).sum(0)
        mim = np.abs(Wl[q, 1::2]) + (np.abs(ct[:, :1]) * np.abs(Xl[:, 1::2]) + np.abs(ct[:, 1:]) * np.abs(Xl[:, 0::2])).sum(0)
        g = cplx(got[q])
        ure, uim = np.abs(g.real - upd.real) / mre, np.abs(g.imag - upd.imag) / mim
        print("panel random", ty, spec, nb, m, "column", q, "dot error / S", ere.max(), eim.max(), "bound", bound,
              "update error / M in u", ure.max() / U[ty], uim.max() / U[ty])
        assert ere.max() <= bound and eim.max() <= bound
        assert ure.max() <= gamma(4 * m, ty) and uim.max() <= gamma(4 * m, ty)


@pytest.mark.parametrize("ty", TYPES)
def test_panel_project_refuses_more_vectors_than_the_workspace(tmp_path, ty):
    Xl, Wl = np.ones((10, 8 * CH[ty])), np.ones((2, 8 * CH[ty]))
    run_panel(tmp_path, ty, 8, 2, 10, Wl, Xl, max_m=36, expect_error="panel projection: too many vectors for the reduction workspace")


# ---- each side of stream_sized: 32 MiB per vector (cached kernels) and one chunk more (non-temporal kernels) -------------------
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("extra", [0, 1], ids=["32MiB", "32MiB+1chunk"])
@pytest.mark.parametrize("op", ["multi_dot", "multi_axpy", "panel"])
def test_stream_sized_threshold_exact(tmp_path, ty, extra, op):
    nch = BIG // 16 + extra
    m = 5
    if op == "panel":
        return panel_exact(tmp_path, ty, nch, 2, m, max_m=20, wcols=2, second_w=0)
    n = nch * CH[ty]
    rng = rng_for("big", op)
    Xl, wl = signs(rng, (m, n)), ints(rng, n, -2, 2)
    if op == "multi_dot":
        re, im = int_cdot(Xl, wl)
        got = run_multi_dot(tmp_path, ty, nch, m, Xl, wl)
        assert np.array_equal(got[0::2], re.astype(np.float64)) and np.array_equal(got[1::2], im.astype(np.float64))
    else:
        coef = ints(rng, 2 * m, -3, 3)
        assert 2 + np.abs(coef).sum() < LIMIT
        ref = wl
        for i in range(m):
            ref = int_caxpy(ref, -coef[2 * i], -coef[2 * i + 1], Xl[i])
        got = run_multi_axpy(tmp_path, ty, nch, m, wl, Xl, coef, -1)
        assert np.array_equal(got, ref.astype(np.float64))


# ---- elementwise ------------------------------------------------------------------------------------------------------------
A_RE, A_IM = 0.75, -1.25      # exact in fp32: (T)a is a

EW_CASES = ([("axpy", l, 0) for l in LENGTHS_EW] + [(f, 257, 0) for f in ("zero", "copy", "scale", "minus", "plus")] + [("axpy", 257, 1)]
            + [(f, s, 0) for f, s in zip(("zero", "copy", "scale", "minus", "plus", "axpy"), VIEWS)] + [("axpy", ("odd", 3), 1)])


def ew_reference(f, x, y, ty):
    """(reference, magnitudes, operation count) on interleaved real arrays"""
    if f == "zero":
        return np.zeros_like(x), None, 0
    if f == "copy":
        return x, None, 0
    if f in ("minus", "plus"):
        return (x - y if f == "minus" else x + y), np.abs(x) + np.abs(y), 2
    xc, yc, a = cplx(x), cplx(y), A_RE + 1j * A_IM
    ref = np.empty_like(x); mag = np.empty_like(x)
    if f == "scale":
        z = a * xc
        mag[0::2] = abs(A_RE) * np.abs(x[0::2]) + abs(A_IM) * np.abs(x[1::2]); mag[1::2] = abs(A_RE) * np.abs(x[1::2]) + abs(A_IM) * np.abs(x[0::2])
        k = 3
    else:
        z = xc + a * yc
        mag[0::2] = np.abs(x[0::2]) + abs(A_RE) * np.abs(y[0::2]) + abs(A_IM) * np.abs(y[1::2])
        mag[1::2] = np.abs(x[1::2]) + abs(A_RE) * np.abs(y[1::2]) + abs(A_IM) * np.abs(y[0::2])
        k = 4
    ref[0::2], ref[1::2] = z.real, z.imag
    return ref, mag, k


def check_ew(got, ref, mag, k, ty, label):
    if k == 0:
        assert np.array_equal(bits(got.astype(DT[ty]), ty), bits(ref.astype(DT[ty]), ty)), label
        return
    err = np.abs(got - ref)
    bound = gamma(k, ty) * mag + float(np.finfo(DT[ty]).tiny)
    print(label, "max error / M in units of u", (err / np.maximum(mag, 1e-300)).max() / U[ty], "k", k)
    assert np.all(err <= bound), label


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("f,spec,inplace", EW_CASES, ids=[f"{f}-{spec_id(s)}" + ("-inplace" if ip else "") for f, s, ip in EW_CASES])
def test_elementwise(tmp_path, ty, f, spec, inplace):
    """vec_zero / copy / scale / minus / plus / axpy (also z == x): one rounding per operation, sentinels outside the view"""
    v, nalloc = make_view(spec, ty)
    idx = addresses(v)
    n = len(idx)
    x, y = uniform(n, 21, ty), uniform(n, 22, ty)
    ref, mag, k = ew_reference(f, x, y, ty)
    before = embed(x if inplace else np.full(n, 0.5), idx, nalloc, ty)
    arrays = dict(z=before, y=embed(y, idx, nalloc, ty))
    if not inplace:
        arrays["x"] = embed(x, idx, nalloc, ty)
    r = nd.run(tmp_path, dict(op="ew", type=ty, ew=f, inplace=inplace, are=A_RE, aim=A_IM, **v), arrays, timeout=timeout_for(nalloc))
    got = r.read("z", DT[ty])
    check_outside(got, before, [idx], ty)
    check_ew(got[idx].astype(np.float64), ref, mag, k, ty, f"{f} {ty} {spec}")


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("scalar,spec,inplace", [(2.0, 257, 0), (-0.5, ("even", 3), 1), (3.0, 2305, 1), (1e-16, 257, 0), (0.0, 257, 1)],
                         ids=["2", "-0.5-even3-inplace", "3-inplace", "1e-16-copies", "0-copies-inplace"])
def test_scale_inv_dev(tmp_path, ty, scalar, spec, inplace):
    """z = x * (T)(1 / s) (k = 3; exact for s = 2, -0.5), a copy for |s| <= 1e-15; Gmres calls it with z == x"""
    v, nalloc = make_view(spec, ty)
    idx = addresses(v)
    x = uniform(len(idx), 23, ty)
    before = embed(x if inplace else np.full(len(idx), 0.5), idx, nalloc, ty)
    arrays = dict(z=before) if inplace else dict(z=before, x=embed(x, idx, nalloc, ty))
    r = nd.run(tmp_path, dict(op="ew", type=ty, ew="scale_inv", inplace=inplace, scalar=scalar, **v), arrays)
    got = r.read("z", DT[ty])
    check_outside(got, before, [idx], ty)
    if abs(scalar) <= 1e-15:
        check_ew(got[idx].astype(np.float64), x, None, 0, ty, "scale_inv copy")
    elif scalar in (2.0, -0.5):
        assert np.array_equal(got[idx].astype(np.float64), x / scalar)
    else:
        check_ew(got[idx].astype(np.float64), x / scalar, np.abs(x / scalar), 3, ty, f"scale_inv {scalar}")


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("V,s0,s1", [(48, 16, 32), (48, 40, 48), (48, 0, 48)], ids=["middle", "end", "all"])
def test_site_range_addresses(tmp_path, ty, V, s0, s1):
    """site_range<T> of sites [s0, s1) of a 24-real field: vec_copy through it moves exactly the reals soa_index names"""
    nreal, ch = 24, CH[ty]
    n = nreal * V
    site, r = np.meshgrid(np.arange(s0, s1), np.arange(nreal), indexing="ij")
    idx = np.unique(((r // ch) * V + site) * ch + r % ch)       # common.h soa_index
    x = uniform(n, 24, ty).astype(DT[ty])
    before = np.full(n, SENTINEL, DT[ty])
    r_ = nd.run(tmp_path, dict(op="ew", type=ty, ew="copy", site_range=1, nreal=nreal, V=V, s0=s0, s1=s1), dict(z=before, x=x))
    view = r_.read("view", np.int64)
    expect = [1, 0, 0, n] if (s0, s1) == (0, V) else [nreal // ch, V * ch, s0 * ch, (s1 - s0) * ch]
    assert list(view) == expect
    assert np.array_equal(np.sort(addresses(dict(rows=view[0], stride=view[1], off=view[2], len=view[3]))), idx)
    got = r_.read("z", DT[ty])
    ref = before.copy(); ref[idx] = x[idx]
    assert np.array_equal(bits(got, ty), bits(ref, ty))


# ---- single reductions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("spec", [1, 257, 2305, 262403, ("even", 3)], ids=spec_id)
def test_norm(tmp_path, ty, spec):
    """sqrt of an fp64-accumulated sum of squares: the sum within 1e-13 of itself (S = the sum), the root of (1 + e) is
    1 + e/2, plus the root's own rounding: |got - ref| <= 1e-13 ref"""
    v, nalloc = make_view(spec, ty)
    idx = addresses(v)
    x = uniform(len(idx), 31, ty)
    r = nd.run(tmp_path, dict(op="norm", type=ty, **v), dict(x=embed(x, idx, nalloc, ty)))
    res = r.read("res", np.float64)
    ref = float(np.sqrt(np.sum(x * x)))
    print("norm", ty, spec, "relative error", abs(res[0] - ref) / ref)
    assert res[0].tobytes() == res[1].tobytes()
    assert abs(res[0] - ref) <= 1e-13 * ref


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("spec", [257, 262403, ("odd", 40)], ids=spec_id)
def test_dot_and_norm2_exact(tmp_path, ty, spec):
    """<x, y> with the conjugate on x (the imaginary part keeps its sign) and <x, x>, integer inputs: equal to int64 arithmetic"""
    v, nalloc = make_view(spec, ty)
    idx = addresses(v)
    for attempt in range(8):           # deterministic; almost always the first
        rng = rng_for("dn2", spec, attempt)
        x, y = ints(rng, len(idx), -2, 2), ints(rng, len(idx), -2, 2)
        re, im = int_cdot(x, y)
        if im != 0:
            break
    assert im != 0, "the case must tell <x,y> from <y,x>"
    r = nd.run(tmp_path, dict(op="dot_norm2", type=ty, **v), dict(x=embed(x, idx, nalloc, ty), y=embed(y, idx, nalloc, ty)))
    res = r.read("res", np.float64).reshape(2, 3)
    assert res[0].tobytes() == res[1].tobytes()
    assert list(res[0]) == [float(re), float(im), float((x * x).sum())]


@pytest.mark.parametrize("ty", TYPES)
def test_dot_and_norm2_random(tmp_path, ty):
    v, nalloc = make_view(2305, ty)
    x, y = uniform(nalloc, 32, ty), uniform(nalloc, 33, ty)
    r = nd.run(tmp_path, dict(op="dot_norm2", type=ty, **v), dict(x=x.astype(DT[ty]), y=y.astype(DT[ty])))
    res = r.read("res", np.float64).reshape(2, 3)
    ref = np.vdot(cplx(x), cplx(y))
    sre, sim = abs_cdot(x, y)
    assert res[0].tobytes() == res[1].tobytes()
    assert abs(res[0, 0] - ref.real) <= 1e-13 * sre and abs(res[0, 1] - ref.imag) <= 1e-13 * sim
    assert abs(res[0, 2] - np.sum(x * x)) <= 1e-13 * np.sum(x * x)


@pytest.mark.parametrize("case", ["positive", "zero", "negative"])
def test_arnoldi_norm_from_dots(tmp_path, case):
    """h[2m] <- sqrt(<w,w> - sum |h_i|^2), -1 for a negative difference; the slot after it is zeroed"""
    m = 3
    h = np.array([3.0, 4.0, 1.0, -2.0, 0.0, 6.0, 0.0, 7.5, 99.0])          # sum |h_i|^2 = 25 + 5 + 36 = 66
    h[2 * m] = {"positive": 66.0 + 2.25, "zero": 66.0, "negative": 65.0}[case]
    r = nd.run(tmp_path, dict(op="arnoldi_norm", m=m), dict(h=h))
    got = r.read("h", np.float64)
    assert np.array_equal(got[:2 * m], h[:2 * m]) and got[2 * m + 2] == 99.0
    assert got[2 * m] == {"positive": 1.5, "zero": 0.0, "negative": -1.0}[case]
    assert got[2 * m + 1] == 0.0


# ---- precision conversion and the mixed-precision update ------------------------------------------------------------------------
def float_layout_of_double(nreal, V):
    """index into the double chunk layout for every element of the float chunk layout of the same field"""
    i = np.arange(nreal * V)
    c, e = i // 4, i % 4                 # float chunk c = q*V + s holds reals 4q .. 4q+3 of site s
    q, s = c // V, c % V
    return ((2 * q + e // 2) * V + s) * 2 + e % 2


@pytest.mark.parametrize("nreal", [24, 4, 96])
@pytest.mark.parametrize("to", ["double", "float"])
def test_convert(tmp_path, to, nreal):
    """float -> double is exact and double -> float is numpy's astype(float32), each through the layout permutation; together:
    the round trip float -> double -> float returns the input"""
    V = 301
    perm = float_layout_of_double(nreal, V)
    assert np.array_equal(np.sort(perm), np.arange(nreal * V))
    if to == "double":
        x = splitmix_uniform(nreal * V, 41).astype(np.float32)
        r = nd.run(tmp_path, dict(op="convert", to=to, V=V, nreal=nreal), dict(x=x, y=np.full(nreal * V + 8, SENTINEL, np.float64)))
        got = r.read("y", np.float64)
        assert np.array_equal(got[perm], x.astype(np.float64)) and np.all(got[nreal * V:] == SENTINEL)
    else:
        x = splitmix_uniform(nreal * V, 42)
        r = nd.run(tmp_path, dict(op="convert", to=to, V=V, nreal=nreal), dict(x=x, y=np.full(nreal * V + 8, SENTINEL, np.float32)))
        got = r.read("y", np.float32)
        assert np.array_equal(got[:nreal * V].view(np.uint32), x[perm].astype(np.float32).view(np.uint32)) and np.all(got[nreal * V:] == np.float32(SENTINEL))


@pytest.mark.parametrize("nreal", [24, 96])
@pytest.mark.parametrize("m", [1, 5])
def test_multi_axpy_f32basis(tmp_path, nreal, m):
    """fp64 w (its layout) += sum_i c_i X_i with fp32 X_i (theirs), products and sums in fp64: k = 4m, u = 2^-53"""
    V = 301
    n = nreal * V
    perm = float_layout_of_double(nreal, V)
    xstride = pad64(n) + 64
    Xf = splitmix_uniform(m * n, 43).astype(np.float32).reshape(m, n)
    w = splitmix_uniform(n, 44)
    coef = 3.0 * splitmix_uniform(2 * m, 45)
    X = np.full(m * xstride, SENTINEL, np.float32)
    for i in range(m):
        X[i * xstride:i * xstride + n] = Xf[i]
    r = nd.run(tmp_path, dict(op="axpy_f32basis", V=V, nreal=nreal, m=m, xstride=xstride, sign=1.0), dict(w=np.concatenate([w, [SENTINEL] * 4]), X=X, coef=coef))
    got = r.read("w", np.float64)
    assert np.all(got[n:] == SENTINEL)
    wl, Xl = w[perm], Xf.astype(np.float64)         # both in the float layout's order: (re, im) pairs stay pairs
    c = coef[0::2] + 1j * coef[1::2]
    ref = cplx(wl) + (c[:, None] * cplx(Xl)).sum(0)
    ac = np.abs(coef)
    mre = np.abs(wl[0::2]) + (ac[0::2, None] * np.abs(Xl[:, 0::2]) + ac[1::2, None] * np.abs(Xl[:, 1::2])).sum(0)
    mim = np.abs(wl[1::2]) + (ac[0::2, None] * np.abs(Xl[:, 1::2]) + ac[1::2, None] * np.abs(Xl[:, 0::2])).sum(0)
    g = cplx(got[:n][perm])
    assert np.all(np.abs(g.real - ref.real) <= gamma(4 * m, "double") * mre) and np.all(np.abs(g.imag - ref.imag) <= gamma(4 * m, "double") * mim)


# ---- generator, pinned round trip ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("seed,stream", [(1, 0), (0xDEADBEEFCAFEF00D, 7)])
def test_vec_random(tmp_path, ty, seed, stream):
    """bit equality with random_kernel restated: splitmix64 of seed + golden * (i + 1) + 0xD1B5.. * (stream + 1), 53 bits"""
    n = 256 * 4096 + 1027           # more than the capped grid covers in one pass
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (i + np.uint64(1)) + np.uint64(0xD1B54A32D192ED03) * np.uint64(stream + 1)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    ref = ((z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0) - 0.5).astype(DT[ty])
    r = nd.run(tmp_path, dict(op="random", type=ty, n=n, seed=seed, stream=stream), {})
    assert np.array_equal(bits(r.read("x", DT[ty]), ty), bits(ref, ty))


def test_publish_wait_and_upload(tmp_path):
    """three rounds of publish_to_host -> wait_published: the values arrive, the sequence number advances by one per round;
    upload_coefficients copies h_coef and nothing more"""
    n, max_m = 25, 12
    src = splitmix_uniform(3 * n, 51)
    hcoef = splitmix_uniform(2 * 7, 52)
    r = nd.run(tmp_path, dict(op="pinned", n=n, max_m=max_m), dict(src=src, hcoef=hcoef))
    assert np.array_equal(r.read("pub", np.float64), src)
    assert r.read("seq", np.uint64).tolist() == [1, 1, 2, 2, 3, 3]
    d = r.read("dcoef", np.float64)
    assert np.array_equal(d[:14], hcoef) and np.all(np.isnan(d[14:]))
