"""GPU tests (-m gpu) of the fine Wilson-Clover operator at the production volumes against fp64 values that do not come from the
library: the whole 32^4 lattice against the pinned oracle (orc), and sampled sites of 48^4, 64^4 and 36x44x52x60 against the
site-local restatement oracle/site_ops.py (pinned by tests/test_site_ops.py), which reads only the links and spinors around
the sites it is asked for.

The branches that only large or oddly shaped lattices take run here: the XCD-aware tile order of dirac_apply_lds_kernel
(number of 256-site tiles a multiple of 8: every cubic case) and its plain order (36x44x52x60 has 9*11*13*15 = 19305 tiles),
the two-row link storage (default) and the full one (DDAMG_LINK_COMPRESSION=0), each in fp32 and fp64, and 64-bit offsets:
the sampled sites include those whose byte offset into the link, clover or spinor field of either precision crosses 2^31 or
2^32.  The error is bounded site by site (max |error| / max |reference| at the site), so one wrong site cannot hide among
16 M right ones as it would in a global relative error.

Host memory: the library keeps the fp64 operator on the host (72 + 84 doubles a site), the test the field while set_gauge
runs and one full spinor at a time.  Peak at 64^4: 9.7 (U) + 21.0 (operator) during set_gauge, 30.5 GB measured; U is reduced
to the links the sampled sites read before the spinors are made."""
import os, resource, sys
import numpy as np
import pytest
from ddalphaamg_amd import api
import ddalphaamg_amd as dd

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tools"))
pytestmark = pytest.mark.gpu

M0, CSW = -0.3, 1.0
GAUGE_EPS, GAUGE_SEED = 0.35, 20260101
# per-site bounds, measured on MI355X over every case here: fp64 1.7e-15 at most, fp32 4.3e-7 at most (the rounding of the operator
# and spinor to fp32 plus the fp32 sums)
TOL64 = 1e-14
TOL32 = 6e-7
LATTICES = {"32^4": [32] * 4, "48^4": [48] * 4, "64^4": [64] * 4, "36x44x52x60": [36, 44, 52, 60]}
# the device fields, as (sub-arrays, reals per site and sub-array): SoA in 16-byte chunks of the site index (fine_op.hip
# soa_index_dev, vec_from_lex): links [4][18], two-row links [4][12], clover [72], spinor [24]
FIELDS = {"links": (4, 18), "two-row links": (4, 12), "clover": (1, 72), "spinor": (1, 24)}


def field_planes(V, nsub, nreal, size):
    """(byte offset of site 0, bytes per site) of every chunk row of a field in the library's SoA chunk layout"""
    ch = 16 // size
    nf, tl = nreal // ch, nreal % ch
    for m in range(nsub):
        base = m * nreal * V * size
        for k in range(nf):
            yield base + k * V * 16, 16
        if tl:
            yield base + nf * V * 16, tl * size


def offset_crossing_sites(V):
    """device sites whose element in some chunk row of a field starts at or spans a byte offset of 2^31 or 2^32, and the sites
    just before them, for both precisions"""
    out = set()
    for nsub, nreal in FIELDS.values():
        for size in (4, 8):
            for base, stride in field_planes(V, nsub, nreal, size):
                for b in (2 ** 31, 2 ** 32):
                    if base <= b < base + V * stride:
                        s = (b - base) // stride
                        out.update(x for x in (s - 1, s) if 0 <= x < V)
    return np.array(sorted(out), dtype=np.int64)


def sample_sites(L, order, seed=5):
    """lexicographic sites: the first and last, every site of the first and last tile (256 consecutive device sites), 512 on
    each T boundary, the 64-bit offset crossings, 2 000 random ones"""
    V = int(np.prod(L)); slab = V // L[0]
    rng = np.random.default_rng(seed)
    dev = np.concatenate([np.arange(256), np.arange(V - 256, V), offset_crossing_sites(V)])
    lexs = np.concatenate([[0, V - 1], order[dev], rng.integers(0, slab, 512), V - slab + rng.integers(0, slab, 512),
                           rng.integers(0, V, 2000)])
    return np.unique(lexs.astype(np.int64))


def make_ctx(L):
    p = api.default_params(); p.num_levels = 1
    for mu in range(4):
        p.local_lattice[0][mu] = L[mu]; p.block_lattice[0][mu] = 4
    p.m0, p.csw = M0, CSW
    return dd.Context(p)


def peak_rss_gb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20


@pytest.mark.parametrize("compression", ["default", "0"], ids=["two-row links", "full links"])
@pytest.mark.parametrize("name", list(LATTICES))
def test_fine_operator_at_full_volume(name, compression, monkeypatch):
    import synth
    from oracle import orc, site_ops
    if compression == "0":
        monkeypatch.setenv("DDAMG_LINK_COMPRESSION", "0")
    else:
        monkeypatch.delenv("DDAMG_LINK_COMPRESSION", raising=False)
    L = LATTICES[name]; V = int(np.prod(L))
    whole = name == "32^4"
    ntiles = V // 256
    assert (ntiles % 8 == 0) != (name == "36x44x52x60")      # the XCD remap is taken or skipped as intended
    U = synth.synth_gauge(L, GAUGE_EPS, GAUGE_SEED)
    ctx = make_ctx(L)
    ctx.set_gauge(U, anti_pbc=True)
    order = ctx.site_order(0)
    if whole:
        sites = np.arange(V)
        D, cl, _ = orc.gauge_to_operator(L, U, 1, M0, CSW)
        Dg, clg = ctx.get_operator()
        assert np.array_equal(Dg, D)
        assert np.abs(clg - cl).max() / np.abs(cl).max() < 1e-13
        del Dg, clg
    else:
        sites = sample_sites(L, order)
        U = site_ops.Patch(U, site_ops.link_sites(L, sites))
    phi = np.random.default_rng(11).random((V, 12, 2)) - 0.5
    xs = {prec: ctx.vector(0, prec).upload(phi) for prec in (32, 64)}
    if whole:
        ref = orc.dirac_apply(L, D, cl, phi, 64)
        del D, cl
    else:
        ref = site_ops.dirac_sites(L, U, site_ops.Patch(phi, site_ops.spinor_sites(L, sites)), sites, M0, CSW)
    del phi, U
    worst = {}
    for prec, tol in ((64, TOL64), (32, TOL32)):
        y = ctx.vector(0, prec)
        ctx.dirac_apply(y, xs[prec])
        out = y.download()[sites]
        y.free(); xs[prec].free()
        err = site_ops.per_site_error(out, ref)
        worst[prec] = (float(err.max()), int(sites[np.argmax(err)]))
        del out
        assert err.max() < tol, (prec, worst[prec])
    ctx.close()
    print(f"{name} links={compression}: {len(sites)} sites, worst per-site error fp64 {worst[64][0]:.2e} fp32 {worst[32][0]:.2e}, "
          f"peak host memory {peak_rss_gb():.1f} GB")
