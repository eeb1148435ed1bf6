"""The BLAS-1 kernels on batches of 32 columns (coarse_lockstep.h: batch_gather, batch_scatter, batch_dots, batch_axpy,
batch_scale_inv), one call per process of tests/native/blas_driver, against plain numpy (-m gpu).

A batch is W[row][c], c < 32, complex fp32; every column has its own coefficient.  As in test_gpu_blas_kernels.py:

EXACT.  Integer entries: basis vectors and w in {-2, .., 2}, coefficients Gaussian integers in [-3, 3].  Every product of a dot
is an integer of magnitude <= 8 and every fp64 partial sum one far below 2^53 in whatever order it is formed; every updated
entry w + sum_i c_i V_i is an integer bounded by 2 + 17 * 6 * 4 < 2^24.  The device result must EQUAL numpy's integers.

RANDOM (splitmix_uniform, rounded to fp32; the reference is numpy on those values).
* batch_dots accumulates fp64 sums of exact products of fp32 numbers: within 1e-13 * sum |v||w| of a column, the bound derived
  in test_gpu_blas_kernels.py for such sums (the dot itself is ~0 for random vectors and is no measure).
* batch_axpy forms the update in fp64 and rounds once to fp32: |got - ref| <= 2^-24 |ref| + 2^-149, the reference in extended
  precision so that it adds no error of its own.

Gaps between columns and between basis vectors, and everything behind the last element, hold a sentinel (no integer, so a
kernel that read it cannot return an integer result) and must come back bit-identical.  Every batch_dots case runs twice inside
the driver and the two results must be bit-identical (deterministic two-stage sums, no atomics)."""
import numpy as np
import pytest
from conftest import splitmix_uniform
import native_driver as nd

pytestmark = pytest.mark.gpu

NC = 32                         # LOCKSTEP_COLS
SENTINEL = -12345.6875          # exactly representable in fp32
ONES64 = np.uint64(0xFFFFFFFFFFFFFFFF)
ONES32 = np.uint32(0xFFFFFFFF)


def ints(rng, lo, hi, *shape):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- gather / scatter -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncols", [2, 31, 32])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000])
def test_gather_zeroes_the_unused_columns_and_round_trips(rows, ncols, tmp_path):
    """ls_gather_kernel (64 rows per workgroup through LDS): columns >= ncols of every row < rows are zeroed, nothing behind row
    `rows` is written; ls_scatter_kernel on what came out gives the columns back"""
    rng = np.random.default_rng(rows * 100 + ncols)
    sstride = 2 * rows + 6                                            # floats: three complex numbers of sentinel between columns
    src = np.full((NC, sstride), SENTINEL, dtype=np.float32)
    src[:, :2 * rows] = ints(rng, -99, 99, NC, 2 * rows)              # the columns >= ncols hold data too: they must not be read
    Wb = np.full((rows + 3, NC, 2), SENTINEL, dtype=np.float32)
    r = nd.run(tmp_path / "g", dict(op="batch_gather", rows=rows, sstride=sstride, ncols=ncols), dict(Wb=Wb, src=src))
    got = r.read("Wb", np.float32).reshape(rows + 3, NC, 2)
    exp = Wb.copy()
    exp[:rows] = 0.0
    exp[:rows, :ncols] = src[:ncols, :2 * rows].reshape(ncols, rows, 2).transpose(1, 0, 2)
    assert same_bits(got, exp), f"{np.count_nonzero(bits(got) != bits(exp))} reals differ"
    dst = np.full((NC, sstride), SENTINEL, dtype=np.float32)
    r = nd.run(tmp_path / "s", dict(op="batch_scatter", rows=rows, dstride=sstride, ncols=ncols), dict(Wb=got, dst=dst))
    back = r.read("dst", np.float32).reshape(NC, sstride)
    exp = dst.copy(); exp[:ncols, :2 * rows] = src[:ncols, :2 * rows]
    assert same_bits(back, exp)


@pytest.mark.parametrize("ncols", [2, 31, 32])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000])
def test_scatter_leaves_the_other_columns_and_the_gaps_alone(rows, ncols, tmp_path):
    """a batch with data in all 32 columns and behind row `rows`: only the first ncols columns of the rows < rows arrive"""
    rng = np.random.default_rng(rows * 100 + ncols + 7)
    dstride = 2 * rows + 10
    Wb = ints(rng, -99, 99, rows + 3, NC, 2)
    dst = np.full((NC, dstride), SENTINEL, dtype=np.float32)
    r = nd.run(tmp_path, dict(op="batch_scatter", rows=rows, dstride=dstride, ncols=ncols), dict(Wb=Wb, dst=dst))
    got = r.read("dst", np.float32).reshape(NC, dstride)
    exp = dst.copy()
    exp[:ncols, :2 * rows] = Wb[:rows, :ncols].transpose(1, 0, 2).reshape(ncols, 2 * rows)
    assert same_bits(got, exp), f"{np.count_nonzero(bits(got) != bits(exp))} reals differ"


def test_driver_refuses_batches_that_would_address_outside_the_arrays(tmp_path):
    Wb = np.zeros((4, NC, 2), dtype=np.float32); src = np.zeros(2 * 10, dtype=np.float32)
    nd.run(tmp_path / "a", dict(op="batch_gather", rows=5, sstride=10, ncols=2), dict(Wb=Wb, src=src), expect_error="batch exceeds Wb")
    nd.run(tmp_path / "b", dict(op="batch_gather", rows=4, sstride=10, ncols=3), dict(Wb=Wb, src=src), expect_error="columns exceed src")
    nd.run(tmp_path / "c", dict(op="batch_dots", rows=4, vstride=4 * NC, m=2), dict(basis=Wb, w=Wb), expect_error="vectors exceed basis")
    nd.run(tmp_path / "d", dict(op="batch_axpy", elems=4 * NC, vstride=4 * NC, m=1, sign=1.0), dict(w=Wb, basis=Wb, coef=np.zeros(2 * NC - 1)),
           expect_error="arrays too short")


# ---- batch_dots ---------------------------------------------------------------------------------------------------------------
def dots_case(rng, m, rows, make):
    """basis vectors vstride apart with sentinels between them, w; returns the arrays and the vectors as complex [m][rows][32]"""
    vstride = rows * NC + 40                                          # complex numbers
    basis = np.full(((m - 1) * vstride + rows * NC + 40, 2), SENTINEL, dtype=np.float32)
    V = np.empty((m, rows, NC, 2), dtype=np.float32)
    for i in range(m):
        V[i] = make(rng, rows, NC, 2)
        basis[i * vstride:i * vstride + rows * NC] = V[i].reshape(rows * NC, 2)
    w = np.full((rows + 2, NC, 2), SENTINEL, dtype=np.float32)
    w[:rows] = make(rng, rows, NC, 2)
    return vstride, basis, w, V.astype(np.float64), w[:rows].astype(np.float64)


def run_dots(path, m, rows, vstride, basis, w, extra=2):
    r = nd.run(path, dict(op="batch_dots", rows=rows, vstride=vstride, m=m, extra=extra), dict(basis=basis, w=w))
    res = r.read("res", np.float64).reshape(2, m + extra, NC, 2)
    assert same_bits(res[0], res[1]), "two runs of the same reduction differ"
    assert np.all(bits(res[0, m:]) == ONES64), "entries of the result behind m were written"
    return res[0, :m]


@pytest.mark.parametrize("rows", [1, 127, 128, 129, 1027])
@pytest.mark.parametrize("m", [1, 7, 8, 9, 17])
def test_batch_dots_of_integers_are_exact(m, rows, tmp_path):
    """ls_dot_kernel / ls_dot_final_kernel: <V_i, w>_c = sum_row conj(V_i[row][c]) w[row][c]; m around DOT_CHUNK = 8 (a second
    pair of launches from m = 9 on), rows around the 128 workgroups (fewer rows than workgroups, one row each, a ragged last one)"""
    rng = np.random.default_rng(1000 * m + rows)
    vstride, basis, w, V, wv = dots_case(rng, m, rows, lambda g, *s: ints(g, -2, 2, *s))
    got = run_dots(tmp_path, m, rows, vstride, basis, w)
    vr, vi, wr, wi = (a.astype(np.int64) for a in (V[..., 0], V[..., 1], wv[..., 0], wv[..., 1]))
    ref = np.stack([(vr * wr + vi * wi).sum(axis=1), (vr * wi - vi * wr).sum(axis=1)], axis=-1)        # [m][32][2]
    assert np.array_equal(got, ref), f"{np.count_nonzero(got != ref)} of {ref.size} sums differ"
    assert len({ref[i, c].tobytes() for i in range(m) for c in range(NC)}) > 1 or rows == 1                # the columns do differ


@pytest.mark.parametrize("m,rows", [(1, 1), (8, 128), (9, 1027), (17, 129)])
def test_batch_dots_of_random_vectors(m, rows, tmp_path):
    seed = [3 * m + rows]

    def uniform(_, *shape):
        seed[0] += 1
        return splitmix_uniform(int(np.prod(shape)), seed[0]).reshape(shape).astype(np.float32)

    vstride, basis, w, V, wv = dots_case(None, m, rows, uniform)
    got = run_dots(tmp_path, m, rows, vstride, basis, w)
    Vc, wc = V[..., 0] + 1j * V[..., 1], wv[..., 0] + 1j * wv[..., 1]
    ref = (np.conj(Vc) * wc[None]).sum(axis=1)
    S = (np.abs(Vc) * np.abs(wc)[None]).sum(axis=1)
    err = np.maximum(np.abs(got[..., 0] - ref.real), np.abs(got[..., 1] - ref.imag))
    print(f"m = {m}, rows = {rows}: largest error / sum |v||w| = {(err / S).max():.3e}")
    assert np.all(err <= 1e-13 * S)


# ---- batch_axpy ---------------------------------------------------------------------------------------------------------------
def axpy_case(rng, m, rows, make, make_coef):
    elems = rows * NC
    vstride = elems + 24
    basis = np.full(((m - 1) * vstride + elems + 24, 2), SENTINEL, dtype=np.float32)
    V = np.empty((m, rows, NC, 2), dtype=np.float32)
    for i in range(m):
        V[i] = make(rng, rows, NC, 2)
        basis[i * vstride:i * vstride + elems] = V[i].reshape(elems, 2)
    w = np.full((rows + 2, NC, 2), SENTINEL, dtype=np.float32)
    w[:rows] = make(rng, rows, NC, 2)
    coef = make_coef(rng, m, NC, 2).astype(np.float64)               # coef[i][c]: its own for every column
    return elems, vstride, basis, w, coef, V


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("rows", [1, 9, 257])
@pytest.mark.parametrize("m", [1, 3, 17])
def test_batch_axpy_with_integer_coefficients_is_exact(m, rows, sign, tmp_path):
    """ls_axpy_kernel: w[row][c] += sign * sum_i coef[i][c] V_i[row][c]"""
    rng = np.random.default_rng(77 * m + rows + int(sign))
    elems, vstride, basis, w, coef, V = axpy_case(rng, m, rows, lambda g, *s: ints(g, -2, 2, *s), lambda g, *s: ints(g, -3, 3, *s))
    assert len({coef[0, c].tobytes() for c in range(NC)}) > 4         # a column that took its neighbour's coefficient shows
    r = nd.run(tmp_path, dict(op="batch_axpy", elems=elems, vstride=vstride, m=m, sign=sign), dict(w=w, basis=basis, coef=coef))
    got = r.read("w", np.float32).reshape(rows + 2, NC, 2)
    cr, ci = coef[..., 0].astype(np.int64)[:, None], coef[..., 1].astype(np.int64)[:, None]
    vr, vi = V[..., 0].astype(np.int64), V[..., 1].astype(np.int64)
    s = int(sign)
    ref = np.stack([w[:rows, :, 0].astype(np.int64) + s * (cr * vr - ci * vi).sum(axis=0),
                    w[:rows, :, 1].astype(np.int64) + s * (cr * vi + ci * vr).sum(axis=0)], axis=-1)
    assert np.abs(ref).max() < 2 ** 24
    assert np.array_equal(got[:rows], ref), f"{np.count_nonzero(got[:rows] != ref)} of {ref.size} components differ"
    assert same_bits(got[rows:], w[rows:])


@pytest.mark.parametrize("m,rows", [(1, 1), (5, 9), (17, 257)])
def test_batch_axpy_with_random_coefficients_rounds_once(m, rows, tmp_path):
    seed = [11 * m + rows]

    def uniform(_, *shape):
        seed[0] += 1
        return splitmix_uniform(int(np.prod(shape)), seed[0]).reshape(shape).astype(np.float32)

    def coefs(_, *shape):
        seed[0] += 1
        return 4.0 * splitmix_uniform(int(np.prod(shape)), seed[0]).reshape(shape)      # fp64 coefficients, as the solver's are

    elems, vstride, basis, w, coef, V = axpy_case(None, m, rows, uniform, coefs)
    r = nd.run(tmp_path, dict(op="batch_axpy", elems=elems, vstride=vstride, m=m, sign=-1.0), dict(w=w, basis=basis, coef=coef))
    got = r.read("w", np.float32).reshape(rows + 2, NC, 2)
    L = np.longdouble
    cr, ci = coef[..., 0].astype(L)[:, None], coef[..., 1].astype(L)[:, None]
    vr, vi = V[..., 0].astype(L), V[..., 1].astype(L)
    ref = np.stack([w[:rows, :, 0].astype(L) - (cr * vr - ci * vi).sum(axis=0), w[:rows, :, 1].astype(L) - (cr * vi + ci * vr).sum(axis=0)], axis=-1)
    err = np.abs(got[:rows].astype(L) - ref)
    print(f"m = {m}, rows = {rows}: largest |got - ref| / (2^-24 |ref| + 2^-149) = {float((err / (2.0 ** -24 * np.abs(ref) + 2.0 ** -149)).max()):.4f}")
    assert np.all(err <= 2.0 ** -24 * np.abs(ref) + 2.0 ** -149)
    assert same_bits(got[rows:], w[rows:])


# ---- batch_scale_inv ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 9, 257])
def test_batch_scale_inv_by_column(rows, tmp_path):
    """ls_scale_inv_kernel: out[row][c] = w[row][c] / sqrt(n2[c]).  Norms^2 that are powers of four give exact quotients; a column
    of norm^2 1e-31 (norm below 1e-15) is copied, and so is one of negative norm^2, which the kernel clamps to zero"""
    rng = np.random.default_rng(rows)
    elems = rows * NC
    w = np.full((rows + 2, NC, 2), SENTINEL, dtype=np.float32)
    w[:rows] = ints(rng, -99, 99, rows, NC, 2)
    k = np.arange(NC) % 17 - 8                                        # norm = 2^k, k = -8 .. 8
    n2 = np.full((NC, 2), 12345.0)                                    # the imaginary slots are never read
    n2[:, 0] = 4.0 ** k
    n2[5, 0] = 1e-31; n2[21, 0] = -4.0; n2[30, 0] = 0.0
    r = nd.run(tmp_path, dict(op="batch_scale_inv", elems=elems), dict(w=w, n2=n2))
    got = r.read("out", np.float32).reshape(rows + 2, NC, 2)
    scale = 2.0 ** -k.astype(np.float64)
    scale[[5, 21, 30]] = 1.0
    ref = (w[:rows].astype(np.float64) * scale[None, :, None]).astype(np.float32)
    assert np.array_equal(ref.astype(np.float64), w[:rows].astype(np.float64) * scale[None, :, None])       # exact quotients
    assert same_bits(got[:rows], ref), f"{np.count_nonzero(bits(got[:rows]) != bits(ref))} reals differ"
    assert np.all(bits(got[rows:]) == ONES32), "elements behind `elems` were written"
