"""CPU tests (-m "not gpu"): pin oracle/site_ops.py -- the fine operator at a list of sites, straight from the gauge field --
against the pinned oracle (orc.gauge_to_operator + orc.dirac_apply) on the golden 4^4 and 8^4 fields and on two ragged lattices,
before the full-volume GPU tests (tests/test_gpu_full_volume.py, test_gpu_hierarchy_32.py) rely on it."""
import numpy as np
import pytest
from conftest import splitmix_uniform, random_su3
from oracle import orc, site_ops


def case(name, gold4, gold8):
    if name in ("4", "8"):
        g = gold4 if name == "4" else gold8
        L = [int(x) for x in g["meta_int"][:4]]
        return L, np.asarray(g["gauge"]), float(g["meta_f64"][0]), float(g["meta_f64"][1]), bool(g["meta_int"][10])
    L = {"ragged-a": [4, 6, 8, 2], "ragged-b": [6, 2, 4, 10]}[name]
    V = int(np.prod(L))
    return L, random_su3(V * 4, 17).reshape(V, 4, 9, 2), 0.1, 1.3, True


@pytest.mark.parametrize("name", ["4", "8", "ragged-a", "ragged-b"])
def test_site_operator_matches_the_oracle_on_every_site(name, gold4, gold8):
    L, U, m0, csw, apbc = case(name, gold4, gold8)
    V = int(np.prod(L))
    D, cl, _ = orc.gauge_to_operator(L, U, int(apbc), m0, csw)
    phi = splitmix_uniform(V * 24, 7).reshape(V, 12, 2)
    ref = orc.dirac_apply(L, D, cl, phi, 64)
    got = site_ops.dirac_sites(L, U, phi, np.arange(V), m0, csw, apbc)
    err = site_ops.per_site_error(got, ref)
    assert err.max() <= 1e-13, err.max()
    # the same through patches of the fields that hold only what a handful of sites read
    sites = np.array([0, V - 1, V // 3, 5 * V // 7])
    Up = site_ops.Patch(U, site_ops.link_sites(L, sites)); pp = site_ops.Patch(phi, site_ops.spinor_sites(L, sites))
    assert len(Up.idx) < V or V <= 256
    assert np.array_equal(site_ops.dirac_sites(L, Up, pp, sites, m0, csw, apbc), got[sites])


def test_several_right_hand_sides_at_once(gold4):
    L, U = [4, 4, 4, 4], np.asarray(gold4["gauge"])
    phis = np.stack([splitmix_uniform(256 * 24, s).reshape(256, 12, 2) for s in (1, 2, 3)], axis=-2)   # [V][12][3][2]
    many = site_ops.dirac_sites(L, U, lambda i: phis[i][..., 0] + 1j * phis[i][..., 1], np.arange(256), -0.2, 1.0)
    for k in range(3):
        assert np.array_equal(many[..., k], site_ops.dirac_sites(L, U, phis[:, :, k], np.arange(256), -0.2, 1.0))


def test_a_wrong_link_at_one_sampled_site_is_flagged(gold8):
    """the per-site bound of the GPU tests is sensitive: one link entry changed by 1e-5 moves the result at the sites that read it
    by far more than the fp32 bound, while the other sites stay exact"""
    L, U = [8, 8, 8, 8], np.asarray(gold8["gauge"])
    m0, csw = float(gold8["meta_f64"][0]), float(gold8["meta_f64"][1])
    V = 4096
    D, cl, _ = orc.gauge_to_operator(L, U, 1, m0, csw)
    phi = splitmix_uniform(V * 24, 9).reshape(V, 12, 2)
    x = 1234
    Ubad = U.copy(); Ubad[x, 2, 4, 0] += 1e-5
    sites = np.arange(V)
    err = site_ops.per_site_error(orc.dirac_apply(L, D, cl, phi, 64), site_ops.dirac_sites(L, Ubad, phi, sites, m0, csw))
    assert err[x] > 1e-6 and err.max() > 1e-6            # caught at the site that owns the link (fp32 bound: 1e-6 at most)
    flagged = set(np.nonzero(err > 1e-13)[0])
    assert x in flagged and len(flagged) < 40             # and only inside that link's stencil: hopping and clover leaves
