"""The 10-real pivot form of the fp32 links (FineOpDev::Dp, fine_op.h), restated in numpy fp32: what link_compress_kernel stores
and what load_link<..., LinkForm::Pivot> rebuilds, operation by operation (numpy rounds every product and sum, the kernel may
contract some into FMAs: the same model up to those roundings).  Shared by tests/test_link_pivot_form.py and
tests/test_gpu_link_pivot.py; not a test module."""
import itertools
import numpy as np

f32 = np.float32


def compress(U):
    """U: [n][3][3] complex128, links as the operator holds them (U/2, the anti-periodic sign included) -> ([n][10] fp32, [n] int8):
    row 0, the two entries of row 1 outside the pivot column p in ascending column order, and the byte sgn * (1 + p).  p is the
    smallest column that maximises |row0[k]|^2 of the fp32-rounded row 0 (squares and sum in fp64, where they are exact enough
    that no rounding can move the choice); sgn is the sign with which 2 conj(row0 x row1) gives row 2."""
    n = U.shape[0]
    r0 = np.stack([U[:, 0].real.astype(f32), U[:, 0].imag.astype(f32)], -1)          # [n][3][2]
    r1 = np.stack([U[:, 1].real.astype(f32), U[:, 1].imag.astype(f32)], -1)
    n2 = r0[..., 0].astype(np.float64) ** 2 + r0[..., 1].astype(np.float64) ** 2
    p = np.argmax(n2, axis=1)                                                          # first maximum
    ka = np.where(p == 0, 1, 0); kb = np.where(p == 2, 1, 2)
    idx = np.arange(n)
    c = np.concatenate([r0.reshape(n, 6), r1[idx, ka], r1[idx, kb]], axis=1)
    third = 2 * np.conj(np.cross(U[:, 0], U[:, 1]))
    plus = np.abs(U[:, 2] - third).sum(1) <= np.abs(U[:, 2] + third).sum(1)
    return c.astype(f32), (np.where(plus, 1, -1) * (1 + p)).astype(np.int8)


def reconstruct(c, b):
    """([n][10] fp32, [n] int8) -> [n][3][3] complex64, in fp32 arithmetic in the kernel's order of operations"""
    c = [c[:, k] for k in range(10)]
    p = np.abs(b.astype(np.int32)) - 1
    sg = np.where(b < 0, f32(-2), f32(2)).astype(f32)
    ar = np.where(p == 0, c[2], c[0]); ai = np.where(p == 0, c[3], c[1])
    br = np.where(p == 2, c[2], c[4]); bi = np.where(p == 2, c[3], c[5])
    pr = np.where(p == 0, c[0], np.where(p == 1, c[2], c[4])); pi = np.where(p == 0, c[1], np.where(p == 1, c[3], c[5]))
    nr = c[6] * ar + c[7] * ai + (c[8] * br + c[9] * bi)
    ni = c[7] * ar - c[6] * ai + (c[9] * br - c[8] * bi)
    inv = f32(1) / (pr * pr + pi * pi)
    xr = -(nr * pr - ni * pi) * inv; xi = -(nr * pi + ni * pr) * inv
    r = list(c[:6]) + [np.where(p == 0, xr, c[6]), np.where(p == 0, xi, c[7]),
                       np.where(p == 0, c[6], np.where(p == 1, xr, c[8])), np.where(p == 0, c[7], np.where(p == 1, xi, c[9])),
                       np.where(p == 2, xr, c[8]), np.where(p == 2, xi, c[9])]
    assert all(x.dtype == f32 for x in r)
    out = np.zeros((len(b), 3, 3), dtype=np.complex64)
    for k in range(3):
        out[:, 0, k] = r[2 * k] + 1j * r[2 * k + 1]
        out[:, 1, k] = r[6 + 2 * k] + 1j * r[6 + 2 * k + 1]
        k1, k2 = (k + 1) % 3, (k + 2) % 3
        cr = r[2 * k1] * r[6 + 2 * k2] - r[2 * k1 + 1] * r[6 + 2 * k2 + 1] - (r[2 * k2] * r[6 + 2 * k1] - r[2 * k2 + 1] * r[6 + 2 * k1 + 1])
        ci = r[2 * k1] * r[6 + 2 * k2 + 1] + r[2 * k1 + 1] * r[6 + 2 * k2] - (r[2 * k2] * r[6 + 2 * k1 + 1] + r[2 * k2 + 1] * r[6 + 2 * k1])
        out[:, 2, k] = sg * cr + 1j * (-sg * ci)
    return out


def monomial_su3():
    """the 96 SU(3) matrices with one entry from {1, -1, i, -i} in every row and column and determinant 1, [96][3][3] complex128"""
    out = []
    for perm in itertools.permutations(range(3)):
        for ph in itertools.product((1, -1, 1j, -1j), repeat=3):
            M = np.zeros((3, 3), dtype=complex)
            for row in range(3):
                M[row, perm[row]] = ph[row]
            if abs(np.linalg.det(M) - 1) < 1e-12:
                out.append(M)
    return np.array(out)
