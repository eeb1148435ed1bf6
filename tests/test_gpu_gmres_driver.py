"""Gmres<float> and Gmres<double> of krylov.h on an operator of the test driver, against tests/gmres_reference.py (-m gpu).

The operator, the preconditioner and the reference algorithm: gmres_reference.py (pinned by tests/test_gmres_reference.py).
n = 1546 complex numbers (773 float chunks), restart length 10, up to 8 restarts, tol 1e-10 (double) / 1e-5 (float).

What is compared, per case: the iteration count (equal), the true residual (< 2 tol: the recurrence's residual is below tol
and differs from the true one by O(u cond(A)) << tol), the residual history entry by entry (relative difference), the solution
(relative 2-norm difference) and max |V^H V - I| over the basis vectors of the last cycle.

The reference of a case is the fp64 numpy restatement of ITS Arnoldi form.  The three forms are one algorithm in exact
arithmetic only: the single-allreduce and pipelined forms take the new vector's norm from sqrt(<w,w> - sum |h_i|^2), and
numpy alone shows that this moves the residual history by up to 1e-2 (fp64) against the classical form on this problem
(the error grows ~40x per step).  A classical reference cannot judge them.

The bounds on history, solution and orthogonality cannot be derived from the algorithm alone.  They come from the reference,
not from the device code: the SPREAD between two correct restatements of the same algorithm, times 10 (the device sums in
another order than numpy; nothing else may differ).
* double: the restatement with classical against modified Gram-Schmidt (pipelined, which has no such variant: against the
  single-allreduce restatement);
* float: the fp64 restatement against the one with every vector rounded to fp32 after each vector operation, and the scalars
  blas.hip rounds to the vectors' type rounded too (update coefficients, the reciprocal of a norm); inner products in fp64;
* both: seven more restatements whose inner products are plain fp64 sums (np.vdot, which sums serially, and six tree sums over
  permuted orders), the one difference a device reduction is entitled to.  The spread is the largest deviation of any of these from the reference,
  whose own inner products are summed in extended precision (gmres_reference.accurate_dot).
The orthogonality bound is 10 x the larger defect of the two restatements (float: of the fp32 one).  The spreads are recomputed
from the reference when the tests run; this is what they were when the tests were written, with what the device showed on an
MI355X (docs/design/01a_coverage.md has the same table):

    case                  type    iterations   history spread (device)  solution spread (device)  max|V^H V-I| spread (device)
    classical             float     8 ( 8)     4.1e-04 (4.3e-04)   9.3e-08 (1.1e-07)     3.2e-02 (3.2e-02)
    classical             double   15 (15)     1.6e-09 (1.0e-10)   1.6e-16 (1.6e-16)     8.7e-13 (8.0e-13)
    single-allreduce      float     8 ( 8)     3.2e-01 (3.2e-01)   6.6e-07 (6.6e-07)     2.9e-02 (3.4e-02)
    single-allreduce      double   15 (15)     8.6e-02 (1.1e-02)   1.0e-15 (1.7e-16)     2.7e-09 (4.0e-09)
    pipelined             float    11 ( 8)     1.0e+02 (1.0e+02)   2.4e-06 (2.4e-06)     8.0e-07 (9.3e-07)
    pipelined             double   15 (15)     9.1e-03 (1.1e-02)   1.7e-16 (1.8e-16)     2.1e-09 (4.9e-10)
    classical-jacobi      float     7 ( 7)     6.2e-04 (6.3e-04)   8.8e-08 (1.0e-07)     3.5e-02 (3.5e-02)
    classical-jacobi      double   13 (13)     1.9e-09 (2.4e-10)   1.6e-16 (1.7e-16)     8.1e-14 (5.2e-14)
    single-jacobi         float     7 ( 7)     3.8e-01 (3.8e-01)   2.7e-06 (2.7e-06)     1.6e-03 (3.0e-03)
    single-jacobi         double   13 (13)     2.9e-01 (8.8e-02)   4.6e-11 (4.6e-11)     1.3e-09 (1.7e-11)
    classical-jacobi-z32  double   13 (13)     1.8e-08 (3.7e-09)   1.7e-16 (1.8e-16)     7.5e-14 (3.2e-14)
    single-jacobi-guess   float     7 ( 7)     3.7e-01 (3.8e-01)   3.6e-06 (3.6e-06)     3.5e-05 (2.1e-05)
    single-jacobi-guess   double   13 (13)     1.1e+00 (1.1e+00)   9.4e-14 (1.7e-16)     2.9e-11 (8.4e-12)
"iterations": the device (the fp64 restatement).  Each bound is 10 x the spread.  The defect of the basis is large next to u because the last vector of a converging cycle is
what is left after cancellation.  In fp32 the norm-from-a-difference forms are at the edge of what they can do here (history
spreads of 0.3 and more: those history bounds say little, the iteration count, the true residual and the solution still
bind).  pipelined-float: the fp64 restatement needs 8 iterations, the fp32 one 11, because a negative <w,w> - sum |h_i|^2 ends
a cycle early (the negative-norm restart of krylov.h); the device must show the fp32 restatement's count.  The fp32
single-allreduce cases and single-jacobi-double go through that restart as well, in the restatement and on the device (the
driver reports how many steps the last cycle completed; the basis is checked over those).

Which branch a norm-from-a-difference form takes is a matter of one rounding error.  The error of the first step's norm
(a few u, amplified 23x by the difference) grows ~42x per step with its sign kept: basis vectors a little too long make
sum |h_i|^2 overcount, so by step 10 the difference is -0.4 <w,w> and the cycle ends in the negative-norm restart; a little too
short, and the difference stays positive and the cycle keeps its tenth column.  Both give 13 iterations and a true residual
of 5e-11, and solutions 4.6e-11 apart (single-jacobi-double, single-jacobi-guess-double).  The restatements with tree sums
land on either side, the serial np.vdot always on the first (its error at step 1 is -1.8e-14 against an extended-precision
value, the device's +1.5e-15): this is why the reference sums in extended precision and why tree sums belong to the family.
"""
import functools
import numpy as np
import pytest
import gmres_reference as gr
import native_driver as nd

pytestmark = pytest.mark.gpu

N, RESTART, NUM_RESTART = 1546, 10, 8
TOL = {"float": 1e-5, "double": 1e-10}
DT = {"float": np.float32, "double": np.float64}

CASES = {
    "classical":            dict(form="classical", prec="none"),
    "single-allreduce":     dict(form="single", prec="none"),
    "pipelined":            dict(form="pipelined", prec="none"),
    "classical-jacobi":     dict(form="classical", prec="jacobi"),
    "single-jacobi":        dict(form="single", prec="jacobi"),
    "classical-jacobi-z32": dict(form="classical", prec="jacobi", z_fp32=1),
    "single-jacobi-guess":  dict(form="single", prec="jacobi", guess=1),
}
PARAMS = [(c, t) for c in CASES for t in ("float", "double") if not (CASES[c].get("z_fp32") and t == "float")]


def reference_kwargs(case):
    kw = dict(restart=RESTART, num_restart=NUM_RESTART)
    if case.get("guess"):
        kw["x0"] = 0.25 * gr.right_hand_side(N, seed=12)
    return kw


def make_prec(case):
    if case["prec"] == "none":
        return None
    return gr.VariableJacobi(N, post=gr.round_fp32 if case.get("z_fp32") else None)     # prec32 hands over fp32 numbers


def defect(V):
    return float(np.abs(V.conj().T @ V - np.eye(V.shape[1])).max())


REF_FORM = {"classical": "classical", "single": "single", "pipelined": "pipelined"}


def history_spread(a, b):
    k = min(len(a), len(b))
    return float(np.max(np.abs(a[:k] - b[:k]) / b[:k])) if k else 0.0


ORDERS = 6      # restatements that sum their inner products in another order


@functools.lru_cache(maxsize=None)
def reference(name, ty):
    """(the fp64 restatement of the case's Arnoldi form, the spreads (history, solution, orthogonality) of other correct
    restatements around it, the iteration counts those needed)"""
    case, b = CASES[name], gr.right_hand_side(N)
    form = REF_FORM[case["form"]]
    run = lambda **kw: gr.gmres(b, TOL[ty], prec=make_prec(case), **reference_kwargs(case), **kw)
    ref = run(form=form)
    if ty == "float":
        first = dict(form=form, fp32=True)
    elif form == "pipelined":
        first = dict(form="single")          # no Gram-Schmidt variant of this form: its sibling with the same kind of norm
    else:
        first = dict(form=form, gs="mgs")
    family = [first, dict(form=form, fp32=ty == "float", dot=np.vdot)]
    family += [dict(form=form, fp32=ty == "float", dot=gr.permuted_dot(N, seed)) for seed in range(1, ORDERS + 1)]
    alts = [run(**kw) for kw in family]
    spread = (max(history_spread(a["history"], ref["history"]) for a in alts),
              max(float(np.linalg.norm(a["x"] - ref["x"]) / np.linalg.norm(ref["x"])) for a in alts),
              max(defect(a["V"]) for a in alts + ([ref] if ty == "double" else [])))
    return ref, spread, sorted(set(a["iter"] for a in alts))


def run_driver(tmp_path, ty, case, b, x0=None, tol=None, **extra):
    scal = dict(op="gmres", type=ty, n=len(b), restart=RESTART, num_restart=NUM_RESTART, tol=tol or TOL[ty], **case, **extra)
    ri = lambda z: np.stack([z.real, z.imag], axis=1).ravel().astype(DT[ty])
    arrays = dict(b=ri(b))
    if x0 is not None:
        arrays["x0"] = ri(x0)
    r = nd.run(tmp_path, scal, arrays, timeout=60)
    sc = r.read("scalars", np.float64)
    x = r.read("x", DT[ty]).astype(np.float64)
    vstride = int(sc[5])
    Vb = r.read("Vb", DT[ty]).astype(np.float64).reshape(RESTART + 1, vstride)[:, :2 * len(b)]
    return dict(iter=int(sc[0]), last_cycle_steps=int(sc[6]), gamma_jp1=sc[1], norm_r0=sc[2], true_residual=sc[3], history=r.read("history", np.float64),
                x=x[0::2] + 1j * x[1::2], V=(Vb[:, 0::2] + 1j * Vb[:, 1::2]).T)


@pytest.mark.parametrize("name,ty", PARAMS, ids=[f"{c}-{t}" for c, t in PARAMS])
def test_gmres_against_the_reference(tmp_path, name, ty):
    """Arnoldi forms x preconditioning x types of the issue's table.  Bounds: 10 x the spread of the module docstring, computed
    from the reference for this very case (printed below with the device's figures)."""
    case = CASES[name]
    ref, (s_hist, s_x, s_orth), alt_iters = reference(name, ty)
    kw = reference_kwargs(case)
    got = run_driver(tmp_path, ty, case, gr.right_hand_side(N), x0=kw.get("x0"))
    # the basis of the last cycle: V_0 and one vector per completed step (a step that ended in a negative norm left none)
    ncol = got["last_cycle_steps"] + 1
    assert 1 <= ncol <= RESTART + 1
    d_hist = history_spread(got["history"], ref["history"])      # entry by entry (pipelined-float: the entries both have)
    d_x = float(np.linalg.norm(got["x"] - ref["x"]) / np.linalg.norm(ref["x"]))
    d_orth = defect(got["V"][:, :ncol])
    print(f"gmres {name} {ty}: iterations {got['iter']} (reference {ref['iter']}), true residual {got['true_residual']:.3e}, "
          f"history {d_hist:.3e} (spread {s_hist:.3e}), solution {d_x:.3e} (spread {s_x:.3e}), orthogonality {d_orth:.3e} (spread {s_orth:.3e})")
    # the count of the fp64 restatement; where fp32 vectors change the count of the restatement itself, that count
    assert got["iter"] in (alt_iters if ty == "float" else [ref["iter"]]) and len(got["history"]) == got["iter"]
    assert got["true_residual"] < 2 * TOL[ty]
    if not case.get("guess"):        # ||b||: an fp64-accumulated sum of exact squares
        assert abs(got["norm_r0"] - ref["norm_r0"]) <= 1e-13 * ref["norm_r0"]
    assert d_orth <= 10 * s_orth
    assert d_hist <= 10 * s_hist
    assert d_x <= 10 * s_x


@pytest.mark.parametrize("ty", ["float", "double"])
def test_zero_right_hand_side(tmp_path, ty):
    got = run_driver(tmp_path, ty, CASES["classical"], np.zeros(N, complex))
    assert got["iter"] == 0 and got["gamma_jp1"] == 0 and not got["x"].any() and len(got["history"]) == 0


@pytest.mark.parametrize("ty", ["float", "double"])
def test_breakdown_exit_on_an_eigenvector(tmp_path, ty):
    """diagonal A, b = 2 e_17: A V_0 lies in span{V_0}, H(1,0) = 0 <= tol / 10, one iteration, x = b / d_17 (one division and the
    rounding of d and of the coefficient to T: a few u)"""
    b = np.zeros(N, complex); b[17] = 2.0
    got = run_driver(tmp_path, ty, CASES["classical"], b, diag_only=1)
    ref = gr.gmres(b, TOL[ty], diag_only=True)
    u = 2.0 ** -24 if ty == "float" else 2.0 ** -53
    assert got["iter"] == ref["iter"] == 1 and len(got["history"]) == 0
    assert np.count_nonzero(got["x"]) == 1
    assert abs(got["x"][17] - ref["x"][17]) <= 8 * u * abs(ref["x"][17])
    assert got["true_residual"] <= 8 * u
