"""GPU tests (-m gpu) of the kernels that build the interpolation operator and move vectors between levels: everything in
transfer.hip (Interpolation<T>) and the transfer half of coarse_mg.hip (CoarseTransfer<T>), run by tests/native/transfer_driver on
arrays written here -- no operator, no gauge field, no context -- against tests/transfer_reference.py.

1. Exactly.  P with integer parts in [-3, 3], vectors with integer parts in [-4, 4]: every partial sum of a result is an integer
   of magnitude at most 2048 sites x 6 dof x 48 < 2^24 (asserted on the reference, transfer_reference.restrict_bound), so fp32 in
   any summation order, on the matrix cores as on the vector units, must return the integer bit for bit.  Every output buffer is
   filled with a sentinel first, longer than needed and with strides wider than a vector: what the operation does not define
   must come back unchanged.
2. Gram-Schmidt on well-conditioned random columns (condition number below 5, asserted) against the fp64 modified Gram-Schmidt of
   the same input.  The bounds are not constants: they are 10 x the spread, around the fp64 reference, of other correct
   restatements (numpy with fp32 rounding in the kernels' order and in two permuted summation orders; for fp64 kernels the two
   permuted fp64 orders), measured on the input of the case.

The lattices (level / aggregate -> aggregates x sites): see GEO.  One driver process serves one (geometry, Nvec, type) and loops
over the column counts.

Which case runs which branch that no whole-cycle test reaches:
  gs_aggregates_kernel<T, 2, 1> / <T, 4, 1> / the refusal above 1024 sites   test_fine_gram_schmidt[2x512-*] / [2x1024-*] /
                                                                              test_gram_schmidt_refuses_2048_sites
  second trip (i += nt) of restrict_kernel and interpolate_kernel            test_restrict_and_interpolate[2x512-*], [2x1024-7-float], [2x2048-4-float]
  task >= ntasks of gs_aggregates_wave_kernel<3> / aos_gs_wave_kernel<T, 8>  test_fine_gram_schmidt_wave_and_workgroup_forms (6 tasks) /
                                                                              test_coarse_gram_schmidt[c3x16-20-*], [c3x16-64-*] (default form)
  ai >= naggs of the five-part launch                                        test_restrict_batch_compact[3x256-*], [2x512-9-0-2], [16x256-17-5-10]
  restrict_mfma_kernel<2, true>: nct, col < nw, i < nvec                      test_restrict_batch[16x16-{1,15,17,24,31}-*] with 1, 15, 17, 31, 33, 47, 49, 63 fields
  restrict_mfma_kernel<8> at ntile % 4 != 0                                   test_restrict_batch[*] with 65, 96, 160 (3, 3, 5 tiles) and 129, 255 fields
  restrict_mfma_kernel<1> beyond 2 Nvec = 20                                  test_restrict_batch_compact[*] with 1, 16, 17, 31, 32 columns at Nvec 7 ... 24
  Mdirect at col_base != 0                                                   test_restrict_batch_compact_direct_store[*] (bases 8 and 32)
  interpolate_batch_kernel<24> / <32> below their width; 64, 128, 512 sites  test_interpolate_batch[8x64-24], [4x128-17], [2x512-7] with 1, 23 / 25, 31 vectors
  jt < TL of restrict_kernel                                                 test_restrict_and_interpolate[16x16-{1,3,5,7,9,17,31,33}-*]
  the two boundaries of CoarseTransfer<T>::orthonormalize                    test_coarse_gram_schmidt[*-64-*] (512 / 1024: wave, register), [*-66-*] (528 / 1056: global)
  aos_gs_reg_kernel bit-identical to aos_gs_kernel                           test_coarse_gram_schmidt[*-20-*], [*-64-*]: the workgroup switch against the global one"""
import numpy as np
import pytest
import native_driver
import transfer_reference as tr

pytestmark = pytest.mark.gpu

SENT = 7.5
DT = {"float": np.float32, "double": np.float64}

# name: (level lattice, aggregate)
GEO = {
    "16x16": ([4, 4, 4, 4], [2, 2, 2, 2]),          # 16 aggregates of 16 sites: one wavefront with idle lanes
    "16x32": ([4, 4, 4, 8], [2, 2, 2, 4]),          # 32-site aggregates
    "8x64": ([4, 4, 4, 8], [2, 2, 4, 4]),           # 64 sites: batched interpolation available
    "4x128": ([4, 4, 4, 8], [2, 4, 4, 4]),          # 128 sites: 128 threads
    "16x48": ([4, 4, 4, 12], [2, 2, 2, 6]),         # 48 sites: batched restriction yes, batched interpolation no
    "3x256": ([4, 4, 4, 12], [4, 4, 4, 4]),         # 3 aggregates: tails of the wave Gram-Schmidt and of the five-part launch
    "16x256": ([8, 8, 8, 8], [4, 4, 4, 4]),         # coarse site order not lexicographic, two groups of 8 aggregates
    "2x512": ([4, 4, 8, 8], [4, 4, 4, 8]),          # second trip of the site loops, two sites per thread
    "2x1024": ([4, 4, 8, 16], [4, 4, 8, 8]),        # four sites per thread
    "2x2048": ([4, 8, 8, 16], [4, 8, 8, 8]),        # Gram-Schmidt refused, transfers still correct
    "16x24": ([4, 4, 4, 6], [2, 2, 2, 3]),          # 24 sites: no multiple of 16, the batched paths refuse
    # levels of CoarseTransfer
    "c16x16": ([4, 4, 4, 4], [2, 2, 2, 2]),
    "c3x16": ([2, 2, 2, 6], [2, 2, 2, 2]),
    "c16x32": ([4, 4, 4, 8], [2, 2, 2, 4]),
    "c3x32": ([2, 2, 2, 12], [2, 2, 2, 4]),
}


def geo(name):
    L, A = GEO[name]
    return L, A, tr.coarse_lattice(L, A)


def sites(name):
    L, A, Lc = geo(name)
    return int(np.prod(L)), int(np.prod(A)), int(np.prod(Lc))


def scalars(name, cls, type_, nvec, ops, **extra):
    L, A, Lc = geo(name)
    s = {"cls": cls, "type": type_, "nvec": nvec, "ops": ",".join(ops), "sentinel": SENT}
    for mu in range(4):
        s[f"L{mu}"], s[f"A{mu}"] = L[mu], A[mu]
        s[f"B{mu}"] = 2 if A[mu] % 2 == 0 else 1
        s[f"Bc{mu}"] = Lc[mu]                    # one block: even sites first, so the coarse order is not lexicographic
    s.update(extra)
    return s


def run(tmp_path, sc, arrays, **kw):
    return native_driver.run(tmp_path, sc, arrays, driver="transfer_driver", **kw)


def ints(rng, lo, hi, *shape):
    return rng.integers(lo, hi + 1, shape).astype(np.float64) + 1j * rng.integers(lo, hi + 1, shape).astype(np.float64)


def reals(z, dtype):
    """complex [..][sites][dof] -> reals [..][sites][2 dof] of the case's type"""
    return tr.reim(z).reshape(z.shape[:-1] + (2 * z.shape[-1],)).astype(dtype)


def read_c(res, name, dtype, *shape):
    """an output back as complex [shape], and the elements of its buffer outside the vectors"""
    a = res.read(name, dtype).astype(np.float64).reshape(shape + (2,))
    return a[..., 0] + 1j * a[..., 1], res.read(name + "_gaps", dtype)


def assert_exact(got, ref, what):
    bad = int(np.count_nonzero(got != ref))
    assert bad == 0, f"{what}: {bad} of {ref.size} components differ from the integer result, the largest difference {np.abs(got - ref).max()}"


def assert_gaps(gaps, at_least, what):
    assert gaps.size >= at_least and np.all(gaps == SENT), f"{what}: {int(np.count_nonzero(gaps != SENT))} of {gaps.size} elements outside the vectors changed"


def assert_small_integers(bound):
    assert bound + 4 < 2 ** 24, bound


_P = {}


def integer_P(name, nvec, nd=12):
    key = (name, nvec, nd)
    if key not in _P:
        _P[key] = ints(np.random.default_rng(sum(map(ord, name)) + 100 * nvec + nd), -3, 3, nvec, sites(name)[0], nd)
    return _P[key]


# ---- the site order, from coordinates alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["16x16", "16x48", "3x256", "16x256", "2x512", "8x64"])
def test_site_order(tmp_path, name):
    """device site s of aggregate a = s // agg_sites lies in the coarse cell coord // A = a-th lexicographic coarse site, and
    agg_csite is the coarse level's own site of that cell"""
    L, A, Lc = geo(name)
    V, S, Vc = sites(name)
    res = run(tmp_path, scalars(name, "fine", "float", 1, ["none"]), {})
    los, losc, ac = res.read("lex_of_site", np.int32), res.read("lex_of_site_c", np.int32), res.read("agg_csite", np.int32)
    assert np.array_equal(np.sort(los), np.arange(V)) and np.array_equal(np.sort(losc), np.arange(Vc))
    assert np.array_equal(tr.aggregate_of(L, A)[los], np.arange(V) // S)
    site_of_lex_c = np.empty(Vc, dtype=np.int64); site_of_lex_c[losc] = np.arange(Vc)
    assert np.array_equal(ac, site_of_lex_c)
    if name == "16x256":
        assert not np.array_equal(losc, np.arange(Vc)), "this lattice is here for a coarse order that is not lexicographic"


# ---- one vector: restrict_kernel<T, 1>, <T, 5>, interpolate_kernel ---------------------------------------------------------------
NVEC_ALL = [1, 3, 4, 5, 7, 8, 9, 16, 17, 24, 31, 32, 33]
ONE_VECTOR = [("16x16", nv, t) for nv in NVEC_ALL for t in ("float", "double")] + [
    ("2x512", 5, "float"), ("2x512", 9, "double"), ("2x512", 33, "float"), ("2x1024", 7, "float"), ("2x2048", 4, "float"),
    ("3x256", 24, "float"), ("16x256", 8, "float"), ("16x256", 3, "double"), ("16x48", 7, "float"), ("4x128", 3, "float"),
    ("16x32", 17, "double"), ("8x64", 31, "float")]


@pytest.mark.parametrize("name,nvec,type_", ONE_VECTOR)
def test_restrict_and_interpolate(tmp_path, name, nvec, type_):
    L, A, Lc = geo(name)
    V, S, Vc = sites(name)
    dt = DT[type_]
    rng = np.random.default_rng(nvec)
    P = integer_P(name, nvec)
    phi5, phic, phi0 = ints(rng, -4, 4, 5, V, 12), ints(rng, -4, 4, Vc, 2 * nvec), ints(rng, -4, 4, V, 12)
    assert_small_integers(tr.restrict_bound(P, phi5, L, A))
    in_stride, out_stride = 24 * V + 8, 4 * nvec * Vc + 4
    res = run(tmp_path, scalars(name, "fine", type_, nvec, ["restrict", "restrict5", "interp", "interp_add"], have_P=1,
                                in_stride=in_stride, out_stride=out_stride),
              {"P": reals(P, dt), "phi": reals(phi5[2], dt), "phi5": reals(phi5, dt), "phic": reals(phic, dt), "phi0": reals(phi0, dt)})
    ref5 = tr.restrict(P, phi5, L, A)
    got, gaps = read_c(res, "restrict", dt, Vc, 2 * nvec)
    assert_exact(got, ref5[2], "restrict_to"); assert_gaps(gaps, 64, "restrict_to")
    got, gaps = read_c(res, "restrict5", dt, 5, Vc, 2 * nvec)
    assert_exact(got, ref5, "restrict5"); assert_gaps(gaps, 64 + 4 * 4, "restrict5")
    got, gaps = read_c(res, "interp", dt, V, 12)
    assert_exact(got, tr.interpolate(P, phic, L, A), "interpolate"); assert_gaps(gaps, 64, "interpolate")
    got, gaps = read_c(res, "interp_add", dt, V, 12)
    assert_exact(got, tr.interpolate(P, phic, L, A, phi0), "interpolate, add"); assert_gaps(gaps, 64, "interpolate, add")


# ---- set_column / get_column -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nvec,type_", [("16x16", 3, "float"), ("16x16", 3, "double"), ("16x48", 5, "float"), ("2x512", 2, "double")])
def test_columns(tmp_path, name, nvec, type_):
    V, S, Vc = sites(name)
    dt = DT[type_]
    P = np.random.default_rng(3).standard_normal((nvec, V, 24)).astype(dt)
    res = run(tmp_path, scalars(name, "fine", type_, nvec, ["columns"], have_P=1, col_stride=24 * V + 12), {"P": P})
    los = res.read("lex_of_site", np.int32)
    site_of_lex = np.empty(V, dtype=np.int64); site_of_lex[los] = np.arange(V)
    assert np.array_equal(res.read("Praw", dt), tr.fine_device_P(P, site_of_lex, S, 4 if type_ == "float" else 2)), "the layout of P"
    assert np.array_equal(res.read("cols", dt).reshape(P.shape), P), "set_column, then get_column"
    assert_gaps(res.read("cols_gaps", dt), 64 + 12 * (nvec - 1), "get_column")


# ---- batched operations: the calls of one process ---------------------------------------------------------------------------------
def fine_pool(rng, npool, V):
    """npool integer fields, then a zero field and a field with one unit entry (last site, last dof)"""
    pool = np.zeros((npool + 2, V, 12), dtype=complex)
    pool[:npool] = ints(rng, -4, 4, npool, V, 12)
    pool[npool + 1, V - 1, 11] = 1.0
    return pool


def selection(n, npool):
    """n columns of a pool of npool (+ zero + unit): pool columns in turn, a zero field in the middle, the unit entry last"""
    sel = [q % npool for q in range(n)]
    if n >= 3:
        sel[n // 2] = npool
    if n >= 2:
        sel[-1] = npool + 1
    return sel


def sel_array(sels):
    w = max(max((len(s) for s in sels), default=1), 1)
    a = np.zeros((len(sels), 1 + w), dtype=np.int32)
    for k, s in enumerate(sels):
        a[k, 0] = len(s); a[k, 1:1 + len(s)] = s
    return a, w


NW = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 96, 127, 128, 129, 160, 255, 256]
RBATCH = [("16x16", nv, NW) for nv in (1, 15, 16, 17, 24, 31, 32)] + [
    ("16x48", 17, NW), ("8x64", 24, NW), ("3x256", 32, [1, 17, 33, 64, 65, 96, 129, 256]), ("2x512", 15, [16, 31, 65, 160]),
    ("16x256", 16, [17, 48, 65, 100])]


@pytest.mark.parametrize("name,nvec,nws", RBATCH)
def test_restrict_batch(tmp_path, name, nvec, nws):
    """restrict_mfma_kernel<2, true> (up to 64 fields) and <8>: partial tiles of 16 and of 32 columns, nvec not a multiple of 16"""
    L, A, Lc = geo(name)
    V, S, Vc = sites(name)
    npool = 256 if V <= 768 else 13          # 13: prime, so a column displaced by a tile width meets another field
    pool = fine_pool(np.random.default_rng(nvec + V), npool, V)
    P = integer_P(name, nvec)
    assert_small_integers(tr.restrict_bound(P, pool, L, A))
    ref = tr.restrict(P, pool, L, A)
    sels = [selection(nw, npool) for nw in nws]
    sa, w = sel_array(sels)
    os_ = 4 * nvec * Vc + 8
    res = run(tmp_path, scalars(name, "fine", "float", nvec, ["rbatch"], have_P=1, selw_rbatch=w, in_stride_rbatch=24 * V + 16, out_stride_rbatch=os_),
              {"P": reals(P, np.float32), "W": reals(pool, np.float32), "sel_rbatch": sa})
    for k, sel in enumerate(sels):
        got, gaps = read_c(res, f"rbatch_{k}", np.float32, len(sel), Vc, 2 * nvec)
        assert_exact(got, ref[sel], f"restrict_batch, {len(sel)} fields"); assert_gaps(gaps, 64 + 8 * (len(sel) - 1), f"restrict_batch, {len(sel)} fields")


@pytest.mark.parametrize("name,nvec,agg0,naggs", [("3x256", 24, 1, 2), ("16x16", 9, 3, 9), ("16x256", 5, 9, 6)])
def test_restrict_batch_slab(tmp_path, name, nvec, agg0, naggs):
    """restrict_mfma_kernel<8> on the aggregates [agg0, agg0 + naggs): the coarse sites of the others stay untouched"""
    L, A, Lc = geo(name)
    V, S, Vc = sites(name)
    npool = 13
    pool = fine_pool(np.random.default_rng(nvec), npool, V)
    P = integer_P(name, nvec)
    assert_small_integers(tr.restrict_bound(P, pool, L, A))
    ref = tr.restrict(P, pool, L, A)
    ref[:, :agg0] = SENT; ref[:, agg0 + naggs:] = SENT
    ref.imag[:, :agg0] = SENT; ref.imag[:, agg0 + naggs:] = SENT
    sels = [selection(5, npool), selection(240, npool)]
    sa, w = sel_array(sels)
    res = run(tmp_path, scalars(name, "fine", "float", nvec, ["rslab"], have_P=1, selw_rslab=w, agg0=agg0, naggs=naggs,
                                in_stride_rslab=24 * naggs * S + 4, out_stride_rslab=4 * nvec * Vc + 4),
              {"P": reals(P, np.float32), "W": reals(pool, np.float32), "sel_rslab": sa})
    for k, sel in enumerate(sels):
        got, gaps = read_c(res, f"rslab_{k}", np.float32, len(sel), Vc, 2 * nvec)
        assert_exact(got, ref[sel], f"restrict_batch_slab, {len(sel)} fields"); assert_gaps(gaps, 64, "restrict_batch_slab")


NCOLS = [1, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]
COMPACT = [("3x256", 24, 0, 3), ("3x256", 7, 1, 2), ("3x256", 16, 0, 3), ("8x64", 12, 0, 8), ("2x512", 9, 0, 2), ("16x256", 8, 0, 16), ("16x256", 17, 5, 10)]


@pytest.mark.parametrize("name,nvec,agg0,naggs", COMPACT)
def test_restrict_batch_compact(tmp_path, name, nvec, agg0, naggs):
    """the five-part launch of restrict_mfma_kernel<1> (up to 32 columns) and <2, true> into coarse column vectors: 3 or 2 of a
    group of 8 aggregates, two groups, a slab"""
    L, A, Lc = geo(name)
    V, S, Vc = sites(name)
    npool = 11
    rng = np.random.default_rng(nvec + naggs)
    pool = ints(rng, -4, 4, npool + 2, 5, V, 12)
    pool[npool] = 0
    pool[npool + 1] = 0; pool[npool + 1, :, V - 1, 11] = 1.0
    P = integer_P(name, nvec)
    assert_small_integers(tr.restrict_bound(P, pool.reshape(-1, V, 12), L, A))
    ref = tr.restrict5_compact(P, pool, L, A)                        # [pool][5][Vc][2N]
    ref[:, :, :agg0] = SENT * (1 + 1j); ref[:, :, agg0 + naggs:] = SENT * (1 + 1j)
    ncols = NCOLS if V <= 1024 else [1, 17, 33, 64]
    sels = [selection(n, npool) for n in ncols]
    sa, w = sel_array(sels)
    res = run(tmp_path, scalars(name, "fine", "float", nvec, ["rcompact"], have_P=1, selw_rcompact=w, agg0=agg0, naggs=naggs,
                                out_stride_rcompact=4 * nvec * Vc + 4),
              {"P": reals(P, np.float32), "W5": reals(pool, np.float32), "sel_rcompact": sa})
    for k, sel in enumerate(sels):
        got, gaps = read_c(res, f"rcompact_{k}", np.float32, len(sel), 5, Vc, 2 * nvec)
        assert_exact(got, ref[sel], f"restrict_batch_compact, {len(sel)} columns"); assert_gaps(gaps, 64 + 4 * (5 * len(sel) - 1), "restrict_batch_compact")


DIRECT_CALLS = {      # (col_base, ncols): restrict_mfma_kernel<1> up to 32 columns, <2, true> above
    18: [(0, 36), (0, 20), (8, 28), (8, 12), (32, 4), (32, 1), (0, 33), (8, 17)],
    24: [(8, 40), (0, 48), (32, 16), (8, 33), (32, 7)],
}


@pytest.mark.parametrize("name,nvec,agg0,naggs", [("3x256", 18, 0, 3), ("3x256", 18, 1, 2), ("3x256", 24, 0, 3), ("16x256", 18, 0, 16)])
def test_restrict_batch_compact_direct_store(tmp_path, name, nvec, agg0, naggs):
    """the same straight into the next level's coupling matrices at column bases 0, 8 and 32; with nvec = 18, n = 36 is no
    multiple of 8, so the padding of the last tile row and tile column lies between the entries and must keep the sentinel"""
    L, A, Lc = geo(name)
    V, S, Vc = sites(name)
    npool, n2 = 11, 2 * nvec
    nt2 = (n2 + 7) // 8; msize2 = nt2 * nt2 * 64
    pool = ints(np.random.default_rng(nvec + agg0), -4, 4, npool + 2, 5, V, 12)
    pool[npool] = 0
    pool[npool + 1] = 0; pool[npool + 1, :, V - 1, 11] = 1.0
    P = integer_P(name, nvec)
    ref = tr.restrict5_compact(P, pool, L, A)
    calls = DIRECT_CALLS[nvec]
    sels = [selection(n, npool) for _, n in calls]
    sa, w = sel_array(sels)
    res = run(tmp_path, scalars(name, "fine", "float", nvec, ["rcompact"], have_P=1, selw_rcompact=w, agg0=agg0, naggs=naggs, mdirect=1,
                                nt2=nt2, msize2=msize2, col_bases=",".join(str(b) for b, _ in calls)),
              {"P": reals(P, np.float32), "W5": reals(pool, np.float32), "sel_rcompact": sa})
    losc = res.read("lex_of_site_c", np.int32)
    csite = np.empty(Vc, dtype=np.int64); csite[losc] = np.arange(Vc)
    inside = np.arange(agg0, agg0 + naggs)
    for k, ((base, n), sel) in enumerate(zip(calls, sels)):
        exp = np.full((Vc, 5, msize2, 2), SENT)
        exp[csite[inside]] = tr.matrices_with_columns(ref[sel][:, :, inside], np.arange(naggs), nt2, msize2, base, SENT)
        got = res.read(f"mdirect_{k}", np.float32).reshape(exp.shape)
        assert_exact(got, exp, f"direct store of {n} columns at {base}")


NRHS = [1, 23, 24, 25, 31, 32]


@pytest.mark.parametrize("name,nvec", [("8x64", 24), ("4x128", 17), ("3x256", 32), ("2x512", 7), ("16x256", 4)])
def test_interpolate_batch(tmp_path, name, nvec):
    """interpolate_batch_kernel<24> and <32> below and at their width, strides with gaps"""
    L, A, Lc = geo(name)
    V, S, Vc = sites(name)
    npool = 32
    rng = np.random.default_rng(nvec)
    pool = np.zeros((npool + 2, Vc, 2 * nvec), dtype=complex)
    pool[:npool] = ints(rng, -4, 4, npool, Vc, 2 * nvec)
    pool[npool + 1, Vc - 1, 2 * nvec - 1] = 1.0
    P = integer_P(name, nvec)
    ref = tr.interpolate(P, pool, L, A)
    sels = [selection(n, npool) for n in NRHS]
    sa, w = sel_array(sels)
    res = run(tmp_path, scalars(name, "fine", "float", nvec, ["ibatch"], have_P=1, selw_ibatch=w, c_stride=4 * nvec * Vc + 12, out_stride_ibatch=24 * V + 8),
              {"P": reals(P, np.float32), "C": reals(pool, np.float32), "sel_ibatch": sa})
    for k, sel in enumerate(sels):
        got, gaps = read_c(res, f"ibatch_{k}", np.float32, len(sel), V, 12)
        assert_exact(got, ref[sel], f"interpolate_batch, {len(sel)} vectors"); assert_gaps(gaps, 64 + 8 * (len(sel) - 1), "interpolate_batch")


# ---- column independence, bit for bit ---------------------------------------------------------------------------------------------
def independence_calls(n, npool):
    """calls of n columns with pool column 0 at index 3 (index 19 in the last): the other columns from one part of the pool, from
    the same shifted by 7 places, all zero, one of them scaled by 2^10 (pool column npool + 2)"""
    a = [1 + q for q in range(n)]; a[3] = 0
    b = [1 + (q + 7) % n for q in range(n)]; b[3] = 0
    z = [npool] * n; z[3] = 0
    s = list(a); s[4] = npool + 2
    m = list(b); m[3] = 5; m[19] = 0
    return [a, b, z, s, m], [3, 3, 3, 3, 19]


@pytest.mark.parametrize("op,n", [("rbatch", 32), ("rbatch", 96), ("rcompact", 24), ("rcompact", 48), ("ibatch", 24), ("ibatch", 32)])
def test_column_independence(tmp_path, op, n):
    """column w's result is the same whatever the other columns hold, and at index 3 as at index 19 (random data: nothing but
    the column's own arithmetic may enter)"""
    name, nvec = "3x256", 24
    L, A, Lc = geo(name)
    V, S, Vc = sites(name)
    npool = n + 1
    rng = np.random.default_rng(n)
    P = rng.standard_normal((nvec, V, 24)).astype(np.float32)
    sels, where = independence_calls(n, npool)
    sa, w = sel_array(sels)
    if op == "ibatch":
        pool = rng.standard_normal((npool + 3, Vc, 4 * nvec)).astype(np.float32)
        arrays, shape = {"C": pool}, (V, 24)
    elif op == "rbatch":
        pool = rng.standard_normal((npool + 3, V, 24)).astype(np.float32)
        arrays, shape = {"W": pool}, (Vc, 4 * nvec)
    else:
        pool = rng.standard_normal((npool + 3, 5, V, 24)).astype(np.float32)
        arrays, shape = {"W5": pool}, (5, Vc, 4 * nvec)
    pool[npool] = 0; pool[npool + 2] = pool[5] * 1024
    res = run(tmp_path, scalars(name, "fine", "float", nvec, [op], have_P=1, **{f"selw_{op}": w}), dict(arrays, P=P, **{f"sel_{op}": sa}))
    cols = [res.read(f"{op}_{k}", np.float32).reshape((n,) + shape)[i] for k, i in enumerate(where)]
    assert np.all(np.isfinite(cols[0])) and np.abs(cols[0]).max() > 0
    for k in range(1, len(cols)):
        assert np.array_equal(cols[0], cols[k]), f"{op}, {n} columns: call {k} changed the column"


# ---- CoarseTransfer: aos_restrict_kernel, aos_interpolate_kernel -------------------------------------------------------------------
CN, CNVEC = [8, 20, 40, 64], [1, 4, 10, 32]
COARSE = [("c16x16", n, nv, "float") for n in CN for nv in CNVEC] + [("c16x16", n, nv, "double") for n, nv in zip(CN, CNVEC)] + [
    (g, n, nv, t) for g, shift in (("c3x16", 1), ("c16x32", 2), ("c3x32", 3)) for i, n in enumerate(CN)
    for nv, t in [(CNVEC[(i + shift) % 4], "float" if (i + shift) % 2 else "double")]]


@pytest.mark.parametrize("name,n,nvec,type_", COARSE)
def test_coarse_restrict_and_interpolate(tmp_path, name, n, nvec, type_):
    L, A, Lc = geo(name)
    V, S, Vc = sites(name)
    dt = DT[type_]
    rng = np.random.default_rng(n + nvec)
    P = integer_P(name, nvec, n)
    phi, phic, phi0 = ints(rng, -4, 4, V, n), ints(rng, -4, 4, Vc, 2 * nvec), ints(rng, -4, 4, V, n)
    assert_small_integers(tr.restrict_bound(P, phi, L, A))
    res = run(tmp_path, scalars(name, "coarse", type_, nvec, ["c_restrict", "c_interp", "c_interp_add"], have_P=1, n=n),
              {"P": reals(P, dt), "phi": reals(phi, dt), "phic": reals(phic, dt), "phi0": reals(phi0, dt)})
    got, gaps = read_c(res, "c_restrict", dt, Vc, 2 * nvec)
    assert_exact(got, tr.restrict(P, phi, L, A), "restrict_to"); assert_gaps(gaps, 64, "restrict_to")
    got, gaps = read_c(res, "c_interp", dt, V, n)
    assert_exact(got, tr.interpolate(P, phic, L, A), "interpolate"); assert_gaps(gaps, 64, "interpolate")
    got, gaps = read_c(res, "c_interp_add", dt, V, n)
    assert_exact(got, tr.interpolate(P, phic, L, A, phi0), "interpolate, add"); assert_gaps(gaps, 64, "interpolate, add")


# ---- refusals: a DDAMG_REQUIRE before any launch ------------------------------------------------------------------------------------
REFUSALS = {
    "nw=0": ("16x16", "float", 4, "rbatch", [[]], "batched restriction: unsupported shape"),
    "nw=257": ("16x16", "float", 4, "rbatch", [[0] * 257], "batched restriction: unsupported shape"),
    "ncols=65": ("3x256", "float", 4, "rcompact", [[0] * 65], "compact batched restriction: unsupported shape"),
    "nrhs=33": ("8x64", "float", 4, "ibatch", [[0] * 33], "batched interpolation: unsupported shape"),
    "nvec=33, restrict_batch": ("16x16", "float", 33, "rbatch", [[0] * 4], "batched restriction: unsupported shape"),
    "nvec=33, restrict_batch_compact": ("3x256", "float", 33, "rcompact", [[0] * 4], "compact batched restriction: unsupported shape"),
    "nvec=33, interpolate_batch": ("8x64", "float", 33, "ibatch", [[0] * 4], "batched interpolation: unsupported shape"),
    "24 sites, restrict_batch": ("16x24", "float", 4, "rbatch", [[0] * 4], "batched restriction: unsupported shape"),
    "24 sites, interpolate_batch": ("16x24", "float", 4, "ibatch", [[0] * 4], "batched interpolation: unsupported shape"),
    "48 sites, interpolate_batch": ("16x48", "float", 4, "ibatch", [[0] * 4], "batched interpolation: unsupported shape"),
    "16 sites, restrict_batch_compact": ("16x16", "float", 4, "rcompact", [[0] * 4], "compact batched restriction: unsupported shape"),
    "double, restrict_batch": ("16x16", "double", 4, "rbatch", [[0] * 4], "batched restriction is an fp32 path"),
    "double, restrict_batch_slab": ("16x16", "double", 4, "rslab", [[0] * 4], "batched restriction is an fp32 path"),
    "double, restrict_batch_compact": ("3x256", "double", 4, "rcompact", [[0] * 4], "batched restriction is an fp32 path"),
    "double, interpolate_batch": ("8x64", "double", 4, "ibatch", [[0] * 4], "batched interpolation is an fp32 path"),
}


@pytest.mark.parametrize("which", list(REFUSALS))
def test_refusals(tmp_path, which):
    name, type_, nvec, op, sels, text = REFUSALS[which]
    V, S, Vc = sites(name)
    dt = DT[type_]
    sa, w = sel_array(sels)
    arrays = {f"sel_{op}": sa, "W": np.zeros((1, V, 24), dt), "W5": np.zeros((1, 5, V, 24), dt), "C": np.zeros((1, Vc, 4 * nvec), dt)}
    extra = {f"selw_{op}": w}
    if op == "rslab":
        extra.update(agg0=1, naggs=2)
    run(tmp_path, scalars(name, "fine", type_, nvec, [op], **extra), arrays, expect_error=text)


def test_gram_schmidt_refuses_2048_sites(tmp_path):
    V = sites("2x2048")[0]
    run(tmp_path, scalars("2x2048", "fine", "float", 2, ["gs"]), {"tv": np.ones((2, V, 24), np.float32)},
        expect_error="aggregates larger than 1024 sites are not supported by the Gram-Schmidt kernel")


# ---- Gram-Schmidt ------------------------------------------------------------------------------------------------------------------
def gs_bounds(tv, L, A, passes, type_):
    """(fp64 reference, bound on the distance to it, bound on |P^H P - 1|): 10 x the spread of other correct restatements"""
    ref = tr.gram_schmidt(tv, L, A, passes)
    E = tr.blocks(tv, L, A).shape[2]
    rng = np.random.default_rng(E)
    dtype = np.float32 if type_ == "float" else np.float64
    others = [tr.gram_schmidt(tv, L, A, passes, dtype=dtype, order=o) for o in
              ([None] if type_ == "float" else []) + [rng.permutation(E), rng.permutation(E)]]
    dist = max(np.abs(o - ref).max() for o in others)
    orth = max(tr.orthonormality(o, L, A).max() for o in others)
    return ref, dist, orth


def check_gs(got, tv, L, A, passes, type_, what, cap=None):
    assert np.linalg.cond(tr.blocks(tv, L, A)).max() < 5
    ref, dist, orth = gs_bounds(tv, L, A, passes, type_)
    d, o = np.abs(got - ref).max(), tr.orthonormality(got, L, A).max()
    R = tr.coefficients(got, tv, L, A)
    diag = np.diagonal(R, axis1=2, axis2=3)
    low = np.abs(np.tril(R, -1)).max()
    # P^H tv of the reference is upper triangular with a real diagonal; an entry of it moves by at most |got - ref| sum |tv|
    slack = 10 * dist * np.abs(tr.blocks(tv, L, A)).sum(axis=2).max() + 1e-12
    print(f"GS {what}: distance {d:.3e} (spread {dist:.3e}), |P^H P - 1| {o:.3e} (spread {orth:.3e}), below the diagonal {low:.3e}")
    assert d <= 10 * dist, f"{what}: {d:.3e} from the fp64 Gram-Schmidt, 10 x spread = {10 * dist:.3e}"
    assert o <= 10 * orth, f"{what}: |P^H P - 1| = {o:.3e}, 10 x spread = {10 * orth:.3e}"
    if cap is not None:
        assert o <= cap
    assert low <= slack and np.all(diag.real > 0) and np.abs(diag.imag).max() <= slack, f"{what}: P^H tv is not upper triangular with a positive real diagonal"


def random_columns(seed, nvec, V, nd):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nvec, V, nd)) + 1j * rng.standard_normal((nvec, V, nd))


def run_fine_gs(tmp_path, name, nvec, type_, tv, **knobs):
    V = sites(name)[0]
    dt = DT[type_]
    res = run(tmp_path, scalars(name, "fine", type_, nvec, ["gs"], **knobs), {"tv": reals(tv, dt)})
    got, gaps = read_c(res, "gs", dt, nvec, V, 12)
    assert_gaps(gaps, 64, "get_column")
    return got


GS_NVEC = [1, 2, 3, 24, 25, 26]
FINE_GS = ([("16x16", nv, "float") for nv in GS_NVEC] + [("16x16", 25, "double"), ("16x32", 3, "float"), ("8x64", 26, "float"),
           ("4x128", 2, "float"), ("4x128", 24, "double"), ("3x256", 25, "double"), ("3x256", 24, "double"),
           ("2x512", 3, "float"), ("2x512", 25, "float"), ("2x512", 24, "double"),
           ("2x1024", 2, "float"), ("2x1024", 26, "float"), ("2x1024", 24, "double"), ("16x256", 24, "float")])


@pytest.mark.parametrize("name,nvec,type_", FINE_GS)
def test_fine_gram_schmidt(tmp_path, name, nvec, type_):
    """gs_aggregates_kernel<T, 1, 2> (up to 256 sites; the odd tail of its two-column pass at nvec = 1, 3, 25), <T, 2, 1> at 512
    and <T, 4, 1> at 1024 sites; at 256 sites in fp32 the wave kernel"""
    L, A, Lc = geo(name)
    V, S, Vc = sites(name)
    tv = random_columns(nvec + S, nvec, V, 12)
    got = run_fine_gs(tmp_path, name, nvec, type_, tv)
    check_gs(got, tv, L, A, 1, type_, f"{name} nvec {nvec} {type_}", cap=5e-6 if (S == 256 and type_ == "float") else None)


@pytest.mark.parametrize("nvec", GS_NVEC)
def test_fine_gram_schmidt_wave_and_workgroup_forms(tmp_path, nvec):
    """256-site aggregates in fp32: gs_aggregates_wave_kernel<3> (three aggregates = six tasks: the last workgroup is half
    empty; both tails of its three-column pass) and, with gs_workgroup, gs_aggregates_kernel<float, 1, 2> on the same input"""
    name = "3x256"
    L, A, Lc = geo(name)
    tv = random_columns(nvec, nvec, sites(name)[0], 12)
    wave = run_fine_gs(tmp_path / "wave", name, nvec, "float", tv)
    wg = run_fine_gs(tmp_path / "wg", name, nvec, "float", tv, gs_workgroup=1)
    check_gs(wave, tv, L, A, 1, "float", f"wave form nvec {nvec}", cap=5e-6)
    check_gs(wg, tv, L, A, 1, "float", f"workgroup form nvec {nvec}", cap=5e-6)
    ref, dist, orth = gs_bounds(tv, L, A, 1, "float")
    assert np.abs(wave - wg).max() <= 10 * dist, "the wave form against the workgroup form"


COARSE_GS = [(g, n, nv, p, t) for g, p, t in (("c3x16", 2, "float"), ("c16x16", 1, "float"), ("c3x16", 2, "double"))
             for n, nv in ((20, 10), (64, 10), (66, 4))]


@pytest.mark.parametrize("name,n,nvec,passes,type_", COARSE_GS)
def test_coarse_gram_schmidt(tmp_path, name, n, nvec, passes, type_):
    """CoarseTransfer<T>::orthonormalize with 16-site aggregates on both sides of its two dispatch boundaries: n = 64 is 512
    elements per chirality (the wave form's last size) and 1024 per aggregate (the register form's last size), n = 66 is 528 and
    1056 (the global form whatever the switches say).  The three switch settings on the same input; the register form against
    the global form bit for bit."""
    L, A, Lc = geo(name)
    V, S, Vc = sites(name)
    dt = DT[type_]
    tv = random_columns(n + nvec, nvec, V, n)
    out = {}
    for form, knobs in (("default", {}), ("workgroup", {"coarse_gs_workgroup_form": 1}), ("global", {"coarse_gs_global": 1})):
        res = run(tmp_path / form, scalars(name, "coarse", type_, nvec, ["c_gs"], n=n, passes=passes, **knobs), {"tv": reals(tv, dt)})
        out[form], gaps = read_c(res, "c_gs", dt, nvec, V, n)
        assert_gaps(gaps, 64, "orthonormalize")
        check_gs(out[form], tv, L, A, passes, type_, f"{name} n {n} nvec {nvec} passes {passes} {type_} {form}")
    # aos_gs_reg_kernel (n <= 64 with the workgroup switch) claims the results of aos_gs_kernel bit for bit; at n = 66 both are
    # aos_gs_kernel
    assert np.array_equal(out["workgroup"], out["global"]), "the register form against the global form"
    if n == 66:
        assert np.array_equal(out["default"], out["global"])
    else:
        ref, dist, orth = gs_bounds(tv, L, A, passes, type_)
        assert np.abs(out["default"] - out["global"]).max() <= 10 * dist, "the wave form against the global form"
