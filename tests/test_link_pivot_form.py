"""The 10-real pivot form of the fp32 links (fine_op.h: row 0, two entries of row 1 and one byte per link) in a numpy fp32
restatement of the compress kernel and of load_link (tests/link_pivot_form.py).  Rows 0 and 1 of U/2 are orthogonal, so the
entry of row 1 in the column p where row 0 is largest follows from the five stored complex numbers, with a divisor of at least
1/sqrt(3) of the row's norm."""
import numpy as np
import pytest
from conftest import random_su3
import link_pivot_form as lp

EPS32 = float(np.finfo(np.float32).eps)
# a few roundings of a quantity of size at most 0.5 (entries of U/2), the divisor at least 0.577 of the row norm
ENTRY_BOUND = 4 * EPS32 * 0.5


def as_links(u):
    """[n][9][2] float64 -> U/2 as [n][3][3] complex"""
    return 0.5 * (u[..., 0] + 1j * u[..., 1]).reshape(-1, 3, 3)


@pytest.mark.parametrize("which", ["golden 4^4", "random_su3 2^16"])
def test_reconstructed_entry_pivot_size_and_positions(which, gold4):
    U = as_links(gold4["gauge"].reshape(-1, 9, 2)) if which == "golden 4^4" else as_links(random_su3(1 << 16, 777))
    n = U.shape[0]
    # the inputs are what the form is for: U/2 with U in SU(3)
    assert np.abs(np.einsum("nij,nkj->nik", U, U.conj()) - 0.25 * np.eye(3)).max() < 1e-12
    c, b = lp.compress(U)
    R = lp.reconstruct(c, b)
    p = np.abs(b.astype(int)) - 1
    idx = np.arange(n)
    err = np.abs(R[idx, 1, p].astype(complex) - U[idx, 1, p])
    row0 = c[:, :6].astype(np.float64).reshape(n, 3, 2)
    ratio = np.sqrt((row0[idx, p] ** 2).sum(1) / (row0 ** 2).sum((1, 2)))
    print(f"{which}: {n} links, row1[p] max error {err.max():.3e} (bound {ENTRY_BOUND:.3e}), smallest |pivot|/|row| {ratio.min():.4f}, "
          f"pivots {np.bincount(p, minlength=3)}")
    assert err.max() <= ENTRY_BOUND
    assert ratio.min() >= 1 / np.sqrt(3) - 1e-6
    assert (np.bincount(p, minlength=3) > 0).all()
    assert (b > 0).all()                                              # det U = 1: row 2 = +2 conj(row0 x row1)
    # the stored numbers are the rounded entries themselves, and the whole link stays at rounding distance: an entry of row 2 is
    # 2 (a_k1 b_k2 - a_k2 b_k1), so it sees the error of row1[p] times 2 |a| <= 1, and as much again for its own roundings
    assert np.array_equal(R[:, 0], U[:, 0].astype(np.complex64))
    assert np.abs(R.astype(complex) - U).max() <= 2 * ENTRY_BOUND


def test_monomial_links_are_reconstructed_exactly():
    """entries 0, +-1/2, +-i/2: every product, sum and the division are exact in fp32, so the rebuilt link IS the link, for each
    pivot position and both signs of the third row (the anti-periodic boundary negates a link)"""
    M = lp.monomial_su3()
    assert M.shape == (96, 3, 3)
    seen = set()
    for sgn in (1, -1):
        U = 0.5 * sgn * M
        c, b = lp.compress(U)
        assert (np.sign(b) == sgn).all()
        p = np.abs(b.astype(int)) - 1
        assert np.array_equal(p, np.argmax(np.abs(M[:, 0]), axis=1))
        R = lp.reconstruct(c, b)
        assert np.array_equal(R.astype(complex), U)
        seen |= {(sgn, int(k)) for k in p}
    assert seen == {(s, k) for s in (1, -1) for k in range(3)}
