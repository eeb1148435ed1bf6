"""The fine Schwarz smoother (sap.hip) at every block volume and kernel form (-m gpu) against the fp64 reference
`mg_oracle.Schwarz` on the fine matrix of the pinned C oracle (tests/schwarz_reference.py; pinned on the CPU in
tests/test_schwarz_reference.py).

Shapes (schwarz_reference.SHAPES): blocks of 16, 32, 64, 128, 256 (2x4x4x8, not 4^4) and 512 sites on the smallest lattices with an
even number of blocks per direction, more than two blocks in one direction (once the first, once the last; not at 512 sites) and,
up to 64 sites, three blocks per colour of the sixteen-colour schedule, which is a partial last workgroup wherever a workgroup
holds 2, 4 or 8 blocks.  Two levels, four test vectors, no setup, blocks = aggregates, m0 0.3, csw 1, four MinRes steps.

Kernel forms: "site" = the default switches (sap_site_kernel<T, 16 .. 256>; at 512 sites sap_block_kernel<float, 256>),
"block" = DDAMG_SAP_VARIANT=1 (sap_block_kernel<T, 8 .. 256>), "plain" = odd_even 0 (sap_plain_kernel<T, 16 .. 256>); each in
fp32 (mixed_precision 1) and fp64 (0), with the additive, red-black and sixteen-colour schedule, 1 and 3 cycles from zero and 2
cycles from a guess.

Bars: fp64 1e-11 of the norm; fp32 ten times the largest spread of the fp32 restatements around the fp64 reference over all
shapes and cases (schwarz_reference.LARGEST_SPREAD, recomputed by the CPU test), which lies below TOL_SWEEP = 5e-5.  The reference
skips a MinRes step whose <Dr,Dr> lies below the EPS of the precision the library runs in, as the kernels and the C reference do.

Isolation: phi (from zero) is filled with NaN and the vectors allocated right before and after it with a sentinel before every
call; eta must come back as it went in.  The smoother's own work vectors (r, latest, x) are not reachable through the interface.

Process boundary: the same lattice through the RCCL self-exchange (the process its own neighbour in the directions of the split),
which runs the DIST = true instantiations and the interior / boundary split of every colour, against the reference with the same
bars, and against the undivided run bit for bit."""
import numpy as np
import pytest
from ddalphaamg_amd import api
import ddalphaamg_amd as dd
import schwarz_reference as sr

pytestmark = pytest.mark.gpu

NVEC = 4
FORMS = {"site": (None, 1), "block": ("1", 1), "plain": (None, 0)}      # DDAMG_SAP_VARIANT, odd_even
SENTINEL = 30000.5
DIST_SHAPES = ["16", "32-t", "64-x", "128-t", "256", "512"]             # one per block volume


def forms_of(name):
    return [f for f in FORMS if FORMS[f][1] or sr.block_sites(name) <= 256]


def precisions_of(name):
    return (1, 0) if sr.block_sites(name) <= 256 else (1,)


def params(L, B, mp, method, odd_even, split=""):
    p = api.default_params(); p.num_levels = 2
    for mu in range(4):
        p.local_lattice[0][mu] = L[mu]; p.block_lattice[0][mu] = B[mu]; p.local_lattice[1][mu] = L[mu] // B[mu]
        if str(mu) in split:
            p.process_grid[mu] = -1
    p.num_vect[0] = NVEC; p.post_smooth_iter[0] = 2; p.block_iter[0] = sr.BLOCK_ITER
    p.mixed_precision, p.method, p.odd_even = mp, method, odd_even
    p.m0, p.csw = sr.M0, sr.CSW
    return p


def context(name, form, mp, method, monkeypatch, split=""):
    variant, odd_even = FORMS[form]
    if variant is None:
        monkeypatch.delenv("DDAMG_SAP_VARIANT", raising=False)
    else:
        monkeypatch.setenv("DDAMG_SAP_VARIANT", variant)
    B, L = sr.SHAPES[name]
    ctx = dd.Context(params(L, B, mp, method, odd_even, split))
    if split:
        ctx.comm_init_rccl(api.rccl_unique_id())
    ctx.set_gauge(sr.gauge(L), anti_pbc=True)
    return ctx


def as_stored(a, prec):
    return a.astype(np.float32).astype(np.float64) if prec == 32 else a


def smooth(ctx, name, cycles, guess):
    """one smoother call, from zero or from the guess, with the isolation checks; returns phi [V][12][2]"""
    prec = ctx.vprec()
    eta, phi0 = sr.vectors(sr.SHAPES[name][1])
    e = ctx.vector(0, prec).upload(eta)
    before = ctx.vector(0, prec); phi = ctx.vector(0, prec); after = ctx.vector(0, prec)
    for g in (before, after):
        g.upload(np.full(eta.shape, SENTINEL))
    phi.upload(phi0 if guess else np.full(eta.shape, np.nan))
    ctx.smoother(phi, e, cycles, initial_guess_zero=not guess)
    out = phi.download()
    assert np.array_equal(e.download(), as_stored(eta, prec)), "eta changed"
    for g in (before, after):
        assert np.all(g.download() == SENTINEL), "a vector next to phi changed"
    for v in (e, before, phi, after):
        v.free()
    return out


CASES = [(name, form, mp, method) for name in sr.SHAPES for form in forms_of(name) for mp in precisions_of(name) for method in sr.METHODS]


@pytest.mark.parametrize("name,form,mp,method", CASES, ids=[f"{n}-{f}-mp{mp}-m{m}" for n, f, mp, m in CASES])
def test_smoother_vs_reference(name, form, mp, method, monkeypatch):
    ctx = context(name, form, mp, method, monkeypatch)
    prec = ctx.vprec()
    bar = sr.fp32_bar() if prec == 32 else 1e-11
    dist = {}
    for start in sr.STARTS:
        out = smooth(ctx, name, *sr.STARTS[start])
        dist[start] = sr.relerr(sr.cvec(out), sr.reference(name, method, bool(FORMS[form][1]), start, prec))
    ctx.close()
    print(f"schwarz {name} {form} fp{prec} method {method}: " + ", ".join(f"{s} {d:.3e}" for s, d in dist.items()) + f" (bar {bar:.2e})")
    assert sr.fp32_bar() <= sr.TOL_SWEEP
    for start, d in dist.items():
        assert d < bar, (start, d, bar)


DIST_CASES = [(name, form, mp) for name in DIST_SHAPES for form in forms_of(name) for mp in precisions_of(name)
              if not (sr.block_sites(name) == 512 and form == "block")]        # at 512 sites both switches run the one kernel


def splits_of(name):
    """"23" and "0123" make every block one of the process boundary (a split direction holds two blocks); the long direction alone
    leaves the blocks away from its ends to the first launch: 4 of 6 or 2 of 4 positions, a partial workgroup again"""
    nblk = np.array(sr.SHAPES[name][1]) // np.array(sr.SHAPES[name][0])
    return ["23", "0123"] + ([str(int(np.argmax(nblk)))] if nblk.max() > 2 else [])


@pytest.fixture(scope="module", params=DIST_CASES, ids=[f"{n}-{f}-mp{mp}" for n, f, mp in DIST_CASES])
def divided(request):
    """red-black, the three starts, undivided (split "") and through the self-exchange: the DIST = true instantiation with the
    colour's blocks in two launches (away from the process boundary while the exchange is in flight, then the others)"""
    name, form, mp = request.param
    out = {}
    with pytest.MonkeyPatch.context() as patch:
        for split in [""] + splits_of(name):
            ctx = context(name, form, mp, 2, patch, split)
            out[split] = {s: smooth(ctx, name, *sr.STARTS[s]) for s in sr.STARTS}
            ctx.close()
    return name, form, mp, out


def test_process_boundary_vs_reference(divided):
    """the divided runs against the fp64 reference, with the bars of the undivided ones"""
    name, form, mp, out = divided
    prec = 64 if mp == 0 else 32
    bar = sr.fp32_bar() if prec == 32 else 1e-11
    dist = {(split, s): sr.relerr(sr.cvec(out[split][s]), sr.reference(name, 2, bool(FORMS[form][1]), s, prec))
            for split in splits_of(name) for s in sr.STARTS}
    print(f"schwarz divided {name} {form} fp{prec}: " + ", ".join(f"{k[0]}/{k[1]} {d:.3e}" for k, d in dist.items()) + f" (bar {bar:.2e})")
    for k, d in dist.items():
        assert d < bar, (k, d, bar)


def test_process_boundary_equals_the_undivided_run(divided):
    """Bit for bit.  A neighbour across a process boundary gets its product U^dagger (1 + gamma_mu) phi in the sender's pack kernel
    (halo.hip, packed fused products) and a local one inside the smoother (sap.hip, scalar form); the scalar SU(3) products of
    dirac_device.h spell out the fused steps of the packed ones, so both round alike in fp32 and fp64.  Before that the divided
    runs lay 1.5e-8 ... 4.4e-7 (fp32) and 1.9e-17 ... 6.8e-16 (fp64) of the norm from the undivided one."""
    name, form, mp, out = divided
    far = {(split, s): (sr.relerr(out[split][s], out[""][s]), int(np.count_nonzero(out[split][s] != out[""][s])))
           for split in splits_of(name) for s in sr.STARTS}
    print(f"schwarz divided {name} {form} mp{mp} from the undivided run: " + ", ".join(f"{k[0]}/{k[1]} {d:.3e} ({n} reals)" for k, (d, n) in far.items()))
    for s in sr.STARTS:
        assert np.all(np.isfinite(out[""][s]))
    for k, (d, n) in far.items():
        assert n == 0, f"split {k[0]}, {k[1]}: {d:.3e} from the undivided run, {n} reals differ"


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
REFUSALS = {
    "512 sites in fp64": ([4, 4, 4, 8], [8, 8, 8, 16], 0, 2, 1, "512-site Schwarz blocks are only supported in fp32"),
    "512 sites without odd-even": ([4, 4, 4, 8], [8, 8, 8, 16], 1, 2, 0, "Schwarz blocks of more than 256 sites need odd_even = 1"),
    "odd number of blocks, red-black": ([2, 2, 2, 2], [4, 4, 4, 6], 1, 2, 1, "multiplicative SAP needs an even number of blocks per direction"),
    "block volume no power of two": ([2, 2, 2, 6], [4, 4, 4, 12], 1, 2, 1, "Schwarz block volume must be 16..512 sites and a power of two"),
}


@pytest.mark.parametrize("which", list(REFUSALS))
def test_refusals(which, monkeypatch):
    B, L, mp, method, odd_even, text = REFUSALS[which]
    monkeypatch.delenv("DDAMG_SAP_VARIANT", raising=False)
    V = int(np.prod(L))
    ctx = dd.Context(params(L, B, mp, method, odd_even))
    vecs = []
    try:
        with pytest.raises(api.DDAMGError, match=text):
            ctx.set_gauge(sr.gauge(L), anti_pbc=True)
            for _ in range(2):
                vecs.append(ctx.vector(0, ctx.vprec()))
            vecs[0].upload(np.ones((V, 12, 2)))
            ctx.smoother(vecs[1], vecs[0], 1, initial_guess_zero=True)
    finally:
        for v in vecs:
            v.free()
        ctx.close()
